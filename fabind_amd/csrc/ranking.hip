// FABind+ confidence training on the device: per-sample pose statistics and the pairwise ranking loss over the copies of a complex
// (reference FABind_plus/fabind/utils/training_confidence.py:41-77 -- training -- and :215-252 -- validation: the python double loop
// over the rmsd-sorted scores, S(S-1)/2 iterations of scalar torch ops, plus the optional BCE on "RMSD < 2 A").
//
// pose_stats_kernel: one wave per sample.  Lane l sums atoms l, l + 64, ... in index order, a butterfly adds the lanes: a fixed order.
//   rmsd = sqrt(mean_i |p_i - t_i|^2); centroid distance = |mean_i (p_i - t_i)| -- the reference's difference of two scatter_means
//   (:44-46) without the cancellation of two +-32 A centroids.  A sample without atoms writes 0 / 0 (scatter_mean's empty row).
// rank_loss_kernel: one work-group per ranking group [group_off[g], group_off[g + 1]), 2 <= S <= 1024, scores and rmsds staged in LDS.
//   b is BETTER than a when (rmsd_b, b) < (rmsd_a, a) lexicographically: the reference's rmsd.argsort() made stable (it is undefined
//   on ties).  Ranks come from counting the better samples: no sort network, no data-dependent loop -- thread a walks b = 0 .. S-1.
//   Thread a owns row a: it sums the terms of the pairs in which a is the WORSE sample (every pair is counted once) and the
//   derivative of every pair a takes part in, so no two threads add into one element.  The block sums are wave butterflies followed
//   by the waves in order: bit-reproducible, no float atomics, no counter that outlives the launch.
//   Exact expf / log1pf / IEEE division on purpose: the fast intrinsics (1 ulp of the RESULT of exp, not of the term) are what the
//   loss bound of tests/test_gpu_ranking.py has no room for.
#include "common.h"
#include "fabind_hip.h"

#define RANK_THREADS 256
#define RANK_MAX_S 1024
#define RANK_ROWS (RANK_MAX_S / RANK_THREADS)

__global__ __launch_bounds__(64) void pose_stats_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                        const int* __restrict__ atom_off, float* __restrict__ rmsd,
                                                        float* __restrict__ cdis) {
    const int b = blockIdx.x, ln = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    float sq = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = ln; i < n; i += 64) {
        const size_t o = (size_t)(a0 + i) * 3;
        const float dx = pred[o] - truth[o], dy = pred[o + 1] - truth[o + 1], dz = pred[o + 2] - truth[o + 2];
        sq += dx * dx + dy * dy + dz * dz;
        sx += dx; sy += dy; sz += dz;
    }
    sq = wave_sum(sq); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    if (ln != 0) return;
    if (n <= 0) { rmsd[b] = 0.f; cdis[b] = 0.f; return; }
    const float fn = (float)n;
    const float mx = sx / fn, my = sy / fn, mz = sz / fn;
    rmsd[b] = sqrtf(sq / fn);
    cdis[b] = sqrtf(mx * mx + my * my + mz * mz);
}

// fixed-order block sums: butterfly inside a wave, then the waves in order; every thread gets the total
__device__ __forceinline__ float rank_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                              // (the previous sum's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < RANK_THREADS / 64; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ int rank_block_sum_i(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < RANK_THREADS / 64; ++w) t += red[w];
    return t;
}

// sigmoid(-d) = 1 / (1 + exp(d)) without overflow
__device__ __forceinline__ float rank_sigmoid_neg(float d) {
    const float e = expf(-fabsf(d));
    return d >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
}

__global__ __launch_bounds__(RANK_THREADS) void rank_loss_kernel(const float* __restrict__ scores, const float* __restrict__ rmsd,
                                                                 const int* __restrict__ group_off, int mode, int with_ce,
                                                                 float* __restrict__ terms, float* __restrict__ d_scores,
                                                                 int* __restrict__ counts) {
    __shared__ float s[RANK_MAX_S], r[RANK_MAX_S];
    __shared__ float redf[RANK_THREADS / 64];
    __shared__ int redi[RANK_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int g0 = group_off[g], S = group_off[g + 1] - g0;
    if (S < 2 || S > RANK_MAX_S) {                // the host refuses these; never index past the LDS arrays
        if (tid < 3) terms[g * 3 + tid] = __int_as_float(0x7fc00000);
        if (tid < 4) counts[g * 4 + tid] = 0;
        return;
    }
    for (int i = tid; i < S; i += RANK_THREADS) { s[i] = scores[g0 + i]; r[i] = rmsd[g0 + i]; }
    __syncthreads();
    const float P = 0.5f * (float)S * (float)(S - 1);             // exact: S(S-1)/2 < 2^24
    const float s_first = s[0];
    float term_sum = 0.f, ce_sum = 0.f;
    int n_right = 0, n_hit = 0, n_conf = 0;
#pragma unroll
    for (int k = 0; k < RANK_ROWS; ++k) {
        const int a = tid + k * RANK_THREADS;
        if (a >= S) continue;
        const float sa = s[a], ra = r[a];
        float row = 0.f, grad = 0.f, others = -INFINITY;
        int rank = 0;
        for (int b = 0; b < S; ++b) {
            if (b == a) continue;
            const float sb = s[b], rb = r[b];
            others = fmaxf(others, sb);
            const bool b_better = rb < ra || (rb == ra && b < a);
            const float delta = b_better ? sb - sa : sa - sb;     // score of the better sample minus score of the worse
            float t, dneg;                                        // the pair's term and -d term / d delta
            if (mode == 0) {
                t = fmaxf(-delta, 0.f) + log1pf(expf(-fabsf(delta)));
                dneg = rank_sigmoid_neg(delta);
            } else {
                const float m = (b_better ? ra - rb : rb - ra) - delta;
                t = fmaxf(m, 0.f);
                dneg = m > 0.f ? 1.f : 0.f;                       // relu's gradient is 0 at 0
            }
            if (b_better) { row += t; grad += dneg; ++rank; n_right += sb > sa; }
            else grad -= dneg;
        }
        term_sum += row;
        grad = grad / P;
        const bool lt2 = ra < 2.f;
        if (with_ce) {                                            // BCE with logits against [rmsd < 2]
            const float e = expf(-fabsf(sa));
            ce_sum += fmaxf(sa, 0.f) - (lt2 ? sa : 0.f) + log1pf(e);
            const float sig = sa >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            grad += (sig - (lt2 ? 1.f : 0.f)) / (float)S;
        }
        d_scores[g0 + a] = grad;
        n_hit += rank == 0 && sa > others;
        // training_confidence.py:77 taken literally: `confidence_score_pred[0] > 0` is the group's FIRST sample in batch order,
        // compared with every sample's [rmsd < 2] (the reference does not index the score by a)
        n_conf += (s_first > 0.f) == lt2;
    }
    term_sum = rank_block_sum(term_sum, redf);
    ce_sum = with_ce ? rank_block_sum(ce_sum, redf) : 0.f;
    n_right = rank_block_sum_i(n_right, redi);
    n_hit = rank_block_sum_i(n_hit, redi);
    n_conf = rank_block_sum_i(n_conf, redi);
    if (tid != 0) return;
    const float ranking = term_sum / P, ce = ce_sum / (float)S;
    terms[g * 3] = ranking;
    terms[g * 3 + 1] = ce;
    terms[g * 3 + 2] = ranking + ce;
    counts[g * 4] = n_right;
    counts[g * 4 + 1] = S * (S - 1) / 2;
    counts[g * 4 + 2] = n_hit > 0;
    counts[g * 4 + 3] = n_conf;
}

extern "C" int fabind_pose_stats(const float* pred, const float* truth, const int* atom_off, int B, float* rmsd, float* cdis,
                                 hipStream_t stream) {
    if (B <= 0) return 0;
    FB_REQUIRE(pred && truth && atom_off && rmsd && cdis, "fabind_pose_stats: null pointer");
    hipLaunchKernelGGL(pose_stats_kernel, dim3(B), dim3(64), 0, stream, pred, truth, atom_off, rmsd, cdis);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_rank_loss_fwd(const float* scores, const float* rmsd, const int* group_off, int G, int mode, int with_ce,
                                    float* terms, float* d_scores, int* counts, hipStream_t stream) {
    if (G <= 0) return 0;
    FB_REQUIRE(mode == 0 || mode == 1, "fabind_rank_loss_fwd: mode is 0 (logsigmoid) or 1 (dynamic_hinge)");
    FB_REQUIRE(scores && rmsd && group_off && terms && d_scores && counts, "fabind_rank_loss_fwd: null pointer");
    hipLaunchKernelGGL(rank_loss_kernel, dim3(G), dim3(RANK_THREADS), 0, stream, scores, rmsd, group_off, mode, with_ce, terms, d_scores,
                       counts);
    FB_CHECK_LAUNCH();
    return 0;
}
