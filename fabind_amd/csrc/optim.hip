// Fused Adam / AdamW step over MANY parameter tensors: global-norm clip and non-finite guard folded in, two launches per step.
// Replaces, after backward() of a training step (reference main_fabind.py:257-260, 419-426): torch.nn.utils.clip_grad_norm_ (one norm per
// tensor, a stack, a second norm, one mul_ per tensor), torch.optim.Adam / AdamW.step() and the NaN guard -- ~1,600 ATen launches for the
// 394 tensors of the production model.
//
// One device table of FabindAdamRow (a row per tensor that has a gradient this step).  A tensor is cut into chunks of FB_OPT_CHUNK
// elements; chunk ids run over all rows (row r owns [chunk0[r], chunk0[r + 1])), a block finds the row of a chunk by binary search over
// chunk0 and strides over the chunks with a capped grid.
//   multi_sqnorm: partials[chunk] = sum g^2 of the chunk (fp32, fixed order inside the block); no atomics, no arrival ticket.  The block of a
//                 row's first chunk copies the row's step counter into snap[row].
//   multi_adam:   every block sums ALL partials in one fixed order in double -> the same total_norm in every block and in every run;
//                 coef = min(1, max_norm / (total_norm + 1e-6)); then torch's single-tensor Adam arithmetic per element with
//                 t = snap[row] + 1.  The first-chunk block writes the counter back as snap + 1: it reads the snapshot, never the live
//                 counter, so a block of the same row that starts later cannot see t + 1.
// The element -> thread assignment and the order of every sum are the same in the 16-byte and the scalar access form, so a step on
// misaligned views (ParamPack's gradient views start at arbitrary element offsets of one flat buffer) equals the aligned step bit for bit.
// .grad is read, never written: unlike clip_grad_norm_ the clip does not rescale it.
#include "common.h"
#include "fabind_hip.h"
#include <math.h>

#define FB_OPT_CHUNK 4096          // elements per chunk: 256 threads x 4 rounds x 4 consecutive elements
#define FB_OPT_MAX_GRID 2048       // memory-bound: 256 CUs x 8 blocks, the rest grid-strides

extern "C" int fabind_adam_chunk(void) { return FB_OPT_CHUNK; }

// row of a chunk: the last r with chunk0[r] <= chunk (rows are sorted by chunk0, chunk0[0] = 0; wave-uniform, scalar loads)
__device__ __forceinline__ int opt_find_row(const FabindAdamRow* __restrict__ rows, int n_rows, int chunk) {
    int lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// four consecutive elements e .. e + 3 of a chunk that holds n valid ones; elements past n read as zero
template <bool VEC> __device__ __forceinline__ float4 opt_ld4(const float* __restrict__ p, int e, int n) {
    if (e + 4 <= n) {
        if (VEC) return *(const float4*)(p + e);
        return make_float4(p[e], p[e + 1], p[e + 2], p[e + 3]);
    }
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < n) r.x = p[e];
    if (e + 1 < n) r.y = p[e + 1];
    if (e + 2 < n) r.z = p[e + 2];
    return r;
}
template <bool VEC> __device__ __forceinline__ void opt_st4(float* __restrict__ p, int e, int n, float4 v) {
    if (e + 4 <= n) {
        if (VEC) { *(float4*)(p + e) = v; return; }
        p[e] = v.x; p[e + 1] = v.y; p[e + 2] = v.z; p[e + 3] = v.w;
        return;
    }
    if (e < n) p[e] = v.x;
    if (e + 1 < n) p[e + 1] = v.y;
    if (e + 2 < n) p[e + 2] = v.z;
}

template <bool VEC> __device__ __forceinline__ float opt_chunk_sq(const float* __restrict__ g, int n) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = j * 1024 + 4 * (int)threadIdx.x;
        if (e < n) {                       // (a zero adds nothing: fmaf(0, 0, acc) == acc, so the guard is only a saved load)
            const float4 x = opt_ld4<VEC>(g, e, n);
            acc = fmaf(x.x, x.x, acc); acc = fmaf(x.y, x.y, acc); acc = fmaf(x.z, x.z, acc); acc = fmaf(x.w, x.w, acc);
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void multi_sqnorm_kernel(const FabindAdamRow* __restrict__ rows, int n_rows, int n_chunks,
                                                           const float* __restrict__ steps, float* __restrict__ partials,
                                                           float* __restrict__ snap) {
    __shared__ float red[4];
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int r = opt_find_row(rows, n_rows, chunk);
        const FabindAdamRow row = rows[r];
        const long long off = (long long)(chunk - row.chunk0) * FB_OPT_CHUNK;
        const long long left = row.numel - off;
        const int n = left < FB_OPT_CHUNK ? (int)left : FB_OPT_CHUNK;
        const float* g = row.g + off;
        float acc = (((uintptr_t)row.g & 15) == 0) ? opt_chunk_sq<true>(g, n) : opt_chunk_sq<false>(g, n);
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            partials[chunk] = ((red[0] + red[1]) + red[2]) + red[3];
            if (chunk == row.chunk0) snap[r] = steps[row.step_idx];
        }
        __syncthreads();
    }
}

struct OptCoef {        // per-chunk constants of the update (fp32, rounded once from double)
    float coef, wd, decay, omb1, beta2, omb2, inv_bc2_sqrt, step_size, eps;
    int decoupled;
};

// torch 2.10 _single_tensor_adam on one element.  No contraction beyond the fmaf written here: both access forms must round alike.
__device__ __forceinline__ void opt_update1(float& p, float g, float& m, float& v, const OptCoef& c) {
#pragma clang fp contract(off)
    g = c.coef * g;
    if (c.decoupled) p = p * c.decay;                 // param.mul_(1 - lr * wd)
    else g = fmaf(c.wd, p, g);                        // grad.add(param, alpha = wd)   (wd = 0: g unchanged)
    m = fmaf(g - m, c.omb1, m);                       // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(c.omb2 * g, g, c.beta2 * v);             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) * c.inv_bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);                // param.addcdiv_(exp_avg, denom, value = -step_size)
}

template <bool GVEC, bool PVEC>
__device__ __forceinline__ void opt_chunk_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int n, const OptCoef& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = j * 1024 + 4 * (int)threadIdx.x;
        if (e >= n) continue;
        float4 P = opt_ld4<PVEC>(p, e, n), M = opt_ld4<PVEC>(m, e, n), V = opt_ld4<PVEC>(v, e, n);
        const float4 G = opt_ld4<GVEC>(g, e, n);
        opt_update1(P.x, G.x, M.x, V.x, c);
        opt_update1(P.y, G.y, M.y, V.y, c);
        opt_update1(P.z, G.z, M.z, V.z, c);
        opt_update1(P.w, G.w, M.w, V.w, c);
        opt_st4<PVEC>(p, e, n, P);
        opt_st4<PVEC>(m, e, n, M);
        opt_st4<PVEC>(v, e, n, V);
    }
}

__global__ __launch_bounds__(256) void multi_adam_kernel(const FabindAdamRow* __restrict__ rows, int n_rows, int n_chunks,
                                                         const float* __restrict__ partials, const float* __restrict__ snap,
                                                         float* __restrict__ steps, float max_norm, int flags,
                                                         float* __restrict__ grad_norm, int* __restrict__ skipped) {
    __shared__ double red[256];
    // total norm: the same fixed-order double sum in every block (thread t takes partials t, t + 256, ...; then a binary tree)
    double s = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += 256) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double total = sqrt(red[0]);
    const bool finite = isfinite(total);
    const bool skip = !finite && (flags & 2);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *grad_norm = (float)total;
        if (skip) *skipped = *skipped + 1;            // one writer: no atomic
    }
    if (skip) return;                                 // nothing of p / m / v / the step counters is touched
    double coef = 1.0;
    if (flags & 1) {
        coef = (double)max_norm / (total + 1e-6);     // torch.nn.utils.clip_grad_norm_
        if (coef >= 1.0) coef = 1.0;                  // (a NaN stays NaN, as under torch.clamp)
    }
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int r = opt_find_row(rows, n_rows, chunk);
        const FabindAdamRow row = rows[r];
        const float t_old = snap[r];
        const double t = (double)t_old + 1.0;
        const double bc1 = 1.0 - pow(row.beta1, t), bc2 = 1.0 - pow(row.beta2, t);
        OptCoef c;
        c.coef = (float)coef;
        c.wd = (float)row.weight_decay;
        c.decay = (float)(1.0 - row.lr * row.weight_decay);
        c.omb1 = (float)(1.0 - row.beta1);
        c.beta2 = (float)row.beta2;
        c.omb2 = (float)(1.0 - row.beta2);
        c.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
        c.step_size = (float)(row.lr / bc1);
        c.eps = (float)row.eps;
        c.decoupled = row.decoupled && row.weight_decay != 0.0;
        const long long off = (long long)(chunk - row.chunk0) * FB_OPT_CHUNK;
        const long long left = row.numel - off;
        const int n = left < FB_OPT_CHUNK ? (int)left : FB_OPT_CHUNK;
        const bool gvec = ((uintptr_t)row.g & 15) == 0;
        const bool pvec = ((((uintptr_t)row.p) | ((uintptr_t)row.m) | ((uintptr_t)row.v)) & 15) == 0;
        float* p = row.p + off;
        const float* g = row.g + off;
        float* m = row.m + off;
        float* v = row.v + off;
        if (pvec) {
            if (gvec) opt_chunk_adam<true, true>(p, g, m, v, n, c); else opt_chunk_adam<false, true>(p, g, m, v, n, c);
        } else {
            if (gvec) opt_chunk_adam<true, false>(p, g, m, v, n, c); else opt_chunk_adam<false, false>(p, g, m, v, n, c);
        }
        if (chunk == row.chunk0 && threadIdx.x == 0) steps[row.step_idx] = t_old + 1.0f;
    }
}

static int opt_grid(int n_chunks) { return n_chunks < FB_OPT_MAX_GRID ? n_chunks : FB_OPT_MAX_GRID; }

extern "C" int fabind_multi_sqnorm(const FabindAdamRow* rows_dev, int n_rows, int n_chunks, const float* steps, float* partials,
                                   float* snap, hipStream_t stream) {
    if (n_rows <= 0 || n_chunks <= 0) return 0;
    FB_REQUIRE(rows_dev != nullptr && steps != nullptr && partials != nullptr && snap != nullptr, "fabind_multi_sqnorm: null operand");
    FB_REQUIRE(n_chunks >= n_rows, "fabind_multi_sqnorm: every row owns at least one chunk");
    hipLaunchKernelGGL(multi_sqnorm_kernel, dim3(opt_grid(n_chunks)), dim3(256), 0, stream, rows_dev, n_rows, n_chunks, steps, partials,
                       snap);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_multi_adam(const FabindAdamRow* rows_dev, int n_rows, int n_chunks, const float* partials, const float* snap,
                                 float* steps, float max_norm, int flags, float* grad_norm, int* skipped, hipStream_t stream) {
    if (n_rows <= 0 || n_chunks <= 0) return 0;
    FB_REQUIRE(rows_dev != nullptr && steps != nullptr && partials != nullptr && snap != nullptr && grad_norm != nullptr && skipped != nullptr,
               "fabind_multi_adam: null operand");
    FB_REQUIRE(n_chunks >= n_rows, "fabind_multi_adam: every row owns at least one chunk");
    FB_REQUIRE(!(flags & 1) || max_norm >= 0.f, "fabind_multi_adam: max_norm >= 0 when clipping");
    hipLaunchKernelGGL(multi_adam_kernel, dim3(opt_grid(n_chunks)), dim3(256), 0, stream, rows_dev, n_rows, n_chunks, partials, snap,
                       steps, max_norm, flags, grad_norm, skipped);
    FB_CHECK_LAUNCH();
    return 0;
}
