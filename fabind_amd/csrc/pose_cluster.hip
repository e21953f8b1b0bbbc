// Poses of one complex against each other: the symmetry-corrected RMSD of every pose pair, and leader clustering on it
// (the step every sampling docking tool reports beside its learned score; FABind+'s sampling evaluation, test_sampling_fabind.py:159-191,
// ranks the S samples of a complex by confidence alone).
//
// pose_pair_kernel: D[b, s, t] = min_{a in Aut(b)} sqrt((1 / n_b) sum_i |x_s[a[i]] - x_t[i]|^2), no centring, no superposition -- the
//   definition of sym_score_kernel (symmetry.hip), which scores S poses against ONE reference and re-reads the permutation for every pair.
//   Here the loops are the other way round.  One work-group per (ligand, tile I of rows, tile J >= I of columns), eight poses to a tile
//   (fewer when 2 x 8 poses of the largest ligand would not leave room for two work-groups in a CU's LDS); both tiles' coordinates live
//   in LDS, xyz interleaved: the lanes of a wave read dwords 3 i + d, a stride coprime to the 32 banks of ds_read_b32.  The work items
//   of a group are (k, s): automorphism k and row pose s of tile I, item q = k * rows + s dealt to wave q mod 4.  A wave keeps a_k[i]
//   of its lanes in registers (n <= 256: at most four per lane, loaded when k changes: once per wave and (tile pair, k); larger ligands
//   re-read the row), gathers x_s[a_k[i]] once per item and sums against ALL column poses of the tile under it: eight accumulators per
//   lane, each over the atoms i = lane, lane + 64, ... in ascending order, then one packed butterfly (pose_reduce8) for the eight sums.
//   The minimum over k is an integer atomicMin on the bit pattern of the non-negative sum in LDS: the order of the bit patterns of
//   non-negative floats is their numerical order, so the result does not depend on which wave arrives first (the all-ones start pattern
//   is a NaN: it survives only if every sum is NaN).  The sum of a pair is formed by the same operations in the same order whatever the
//   tile, the column slot, the number of poses or the other ligands of the batch: D[b, s, t] depends on ligand b and poses s, t alone,
//   bit for bit.  Each unordered pair is computed once (s < t) and written to both triangles; the diagonal is +0.0.  No float atomics.
// pose_cluster_kernel: leader clustering, one wave per ligand.  Rank the poses by descending confidence (ties keep pose order, NaN
//   last); the best unassigned pose leads the next cluster and takes every unassigned t with D[leader, t] < threshold (strict; a NaN
//   distance joins nothing).  Integer and comparison work only.
#include "common.h"
#include "fabind_hip.h"

#define POSE_MAX_S 512
#define POSE_MAX_N 2048
#define POSE_TILE 8                               // most poses per tile = the column poses a wave sums at once
#define POSE_LDS_BYTES 65536                      // coordinates of two tiles + the tile's minima: two work-groups fit a CU's 160 KB
#define POSE_THREADS 256
#define POSE_REG_N 256                            // up to this many atoms the permutation of a wave stays in registers

// Every rounding of a pair's sum is written out: with contraction left to the compiler, two copies of an unrolled loop could be fused
// differently, and a distance must not depend on the column slot its pose happens to occupy.
#pragma clang fp contract(off)

// |g - x|^2 of one atom: three rounded differences, one product, two fused multiply-adds
__device__ __forceinline__ float pose_d2(float gx, float gy, float gz, const float* x) {
    const float dx = gx - x[0], dy = gy - x[1], dz = gz - x[2];
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The butterfly sum over the 64 lanes (partners lane ^ 32, ^ 16, ..., ^ 1: the tree of wave_sum, so the same bits) of eight values
// per lane at once.  The first three levels halve what a lane keeps -- a lane sends the half its partner keeps -- so eight sums cost
// 4 + 2 + 1 + 3 exchanges instead of 48.  The sum of v[t] ends in the lanes with (lane & 7) == 0 and
// t = 4 * bit5(lane) + 2 * bit4(lane) + bit3(lane).
__device__ __forceinline__ float pose_reduce8(const float (&v)[8], int ln) {
    const bool h5 = ln & 32, h4 = ln & 16, h3 = ln & 8;
    float w[4], u[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (h5 ? v[j + 4] : v[j]) + __shfl_xor(h5 ? v[j] : v[j + 4], 32, 64);
#pragma unroll
    for (int j = 0; j < 2; ++j) u[j] = (h4 ? w[j + 2] : w[j]) + __shfl_xor(h4 ? w[j] : w[j + 2], 16, 64);
    float r = (h3 ? u[1] : u[0]) + __shfl_xor(h3 ? u[0] : u[1], 8, 64);
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    return r;
}

static int pose_tile_size(int n_pose, int max_atoms) {
    int ts = n_pose < POSE_TILE ? n_pose : POSE_TILE;
    const long per = 24L * (max_atoms > 1 ? max_atoms : 1);          // bytes of one pose in both tiles
    while (ts > 1 && per * ts + 4L * ts * ts > POSE_LDS_BYTES) --ts;
    return ts;
}

__global__ __launch_bounds__(POSE_THREADS) void pose_pair_kernel(const float* __restrict__ poses, int n_pose, int n_atoms,
                                                                 const int* __restrict__ atom_off, const int* __restrict__ flat_off,
                                                                 const int* __restrict__ auto_cnt, const int* __restrict__ flat, int max_atoms,
                                                                 int ts, int n_tiles, float* __restrict__ D) {
    extern __shared__ unsigned pose_sm[];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const int n_tp = n_tiles * (n_tiles + 1) / 2;
    const int b = blockIdx.x / n_tp;
    int p = blockIdx.x - b * n_tp, I = 0;
    while (p >= n_tiles - I) { p -= n_tiles - I; ++I; }
    const int J = I + p;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const int s0 = I * ts, t0 = J * ts;
    const int rows = min(ts, n_pose - s0), cols = min(ts, n_pose - t0);
    unsigned* best = pose_sm;                                         // [rows][ts] bit patterns of the smallest sum
    float* xi = reinterpret_cast<float*>(pose_sm + ts * ts);          // [rows][3 n]
    float* xj = I == J ? xi : xi + (size_t)ts * 3 * n;                // [cols][3 n]
    float* Db = D + (size_t)b * n_pose * n_pose;
    if (n <= 0 || n > max_atoms) {                                    // an empty ligand: every distance is 0
        const float v = n <= 0 ? 0.f : NAN;                           // (a ligand larger than the LDS was sized for: NaN, nothing staged)
        for (int e = tid; e < rows * cols; e += POSE_THREADS) {
            const int s = s0 + e / cols, t = t0 + e % cols;
            Db[(size_t)s * n_pose + t] = s == t ? 0.f : v;
            Db[(size_t)t * n_pose + s] = s == t ? 0.f : v;
        }
        return;
    }
    for (int r = 0; r < rows; ++r) {
        const float* src = poses + ((size_t)(s0 + r) * n_atoms + a0) * 3;
        for (int i = tid; i < 3 * n; i += POSE_THREADS) xi[(size_t)r * 3 * n + i] = src[i];
    }
    if (I != J)
        for (int r = 0; r < cols; ++r) {
            const float* src = poses + ((size_t)(t0 + r) * n_atoms + a0) * 3;
            for (int i = tid; i < 3 * n; i += POSE_THREADS) xj[(size_t)r * 3 * n + i] = src[i];
        }
    for (int e = tid; e < rows * ts; e += POSE_THREADS) best[e] = 0xffffffffu;
    __syncthreads();
    const int base = flat_off[b];
    const int K = min(auto_cnt[b], (flat_off[b + 1] - base) / n);     // never past the ligand's slot of the table
    const int nk = max(K, 1);                                         // K <= 0: the identity alone (plain RMSD)
    const bool in_regs = n <= POSE_REG_N;
    int a[4] = {ln, ln + 64, ln + 128, ln + 192};
    int k_have = -1;
    for (int q = wv; q < nk * rows; q += 4) {
        const int k = q / rows, s = q - k * rows;
        const int t_lo = I == J ? s + 1 : 0;                          // the diagonal tile: the upper triangle only
        if (t_lo >= cols) continue;
        const int* ak = flat + base + (size_t)k * n;
        if (in_regs && K > 0 && k != k_have) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = ln + 64 * c;
                if (i < n) {
                    const int j = ak[i];
                    a[c] = (unsigned)j < (unsigned)n ? j : i;         // an entry out of range falls back to i
                }
            }
            k_have = k;
        }
        const float* xs = xi + (size_t)s * 3 * n;
        float v[POSE_TILE];
#pragma unroll
        for (int t = 0; t < POSE_TILE; ++t) v[t] = 0.f;
        if (in_regs) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = ln + 64 * c;
                if (i < n) {
                    const float gx = xs[3 * a[c]], gy = xs[3 * a[c] + 1], gz = xs[3 * a[c] + 2];
#pragma unroll
                    for (int t = 0; t < POSE_TILE; ++t)
                        if (t >= t_lo && t < cols) v[t] += pose_d2(gx, gy, gz, xj + (size_t)t * 3 * n + 3 * i);
                }
            }
        } else {
            for (int i = ln; i < n; i += 64) {
                int j = K > 0 ? ak[i] : i;
                j = (unsigned)j < (unsigned)n ? j : i;
                const float gx = xs[3 * j], gy = xs[3 * j + 1], gz = xs[3 * j + 2];
#pragma unroll
                for (int t = 0; t < POSE_TILE; ++t)
                    if (t >= t_lo && t < cols) v[t] += pose_d2(gx, gy, gz, xj + (size_t)t * 3 * n + 3 * i);
            }
        }
        const float r = pose_reduce8(v, ln);
        const int t = ((ln >> 5) & 1) * 4 + ((ln >> 4) & 1) * 2 + ((ln >> 3) & 1);
        if ((ln & 7) == 0 && t >= t_lo && t < cols) atomicMin(&best[s * ts + t], __float_as_uint(r));
    }
    __syncthreads();
    const float fn = (float)n;
    for (int e = tid; e < rows * cols; e += POSE_THREADS) {
        const int s = e / cols, t = e - s * cols;
        const int sg = s0 + s, tg = t0 + t;
        if (I == J && t < s) continue;
        if (sg == tg) { Db[(size_t)sg * n_pose + sg] = 0.f; continue; }
        const float d = sqrtf(__uint_as_float(best[s * ts + t]) / fn);
        Db[(size_t)sg * n_pose + tg] = d;
        Db[(size_t)tg * n_pose + sg] = d;
    }
}

// true when pose u comes before pose s in the ranking: descending confidence, NaN last, equal keys in pose order
__device__ __forceinline__ bool pose_before(float cu, int u, float cs, int s) {
    const bool nu = cu != cu, ns = cs != cs;
    if (nu != ns) return ns;
    if (nu) return u < s;
    return cu > cs || (cu == cs && u < s);
}

__global__ __launch_bounds__(64) void pose_cluster_kernel(const float* __restrict__ D, const float* __restrict__ conf, int n_pose,
                                                          int n_lig, float threshold, int* __restrict__ cluster_id,
                                                          int* __restrict__ leader, int* __restrict__ size, int* __restrict__ n_clusters) {
    __shared__ float cf[POSE_MAX_S];
    __shared__ int order[POSE_MAX_S], cid[POSE_MAX_S];
    const int b = blockIdx.x, ln = threadIdx.x, S = n_pose;
    const float* Db = D + (size_t)b * S * S;
    for (int s = ln; s < S; s += 64) { cf[s] = conf[(size_t)s * n_lig + b]; cid[s] = -1; }
    __syncthreads();
    for (int s = ln; s < S; s += 64) {
        const float cs = cf[s];
        int rank = 0;
        for (int u = 0; u < S; ++u) rank += pose_before(cf[u], u, cs, s);
        order[rank] = s;                                              // the keys (confidence, pose) are distinct: a permutation
    }
    __syncthreads();
    int ncl = 0;
    for (int r = 0; r < S; ++r) {
        const int p = order[r];
        if (cid[p] >= 0) continue;                                    // the same for every lane: cid is read after the barrier below
        int cnt = 0;
        for (int t = ln; t < S; t += 64)
            if (cid[t] < 0 && (t == p || Db[(size_t)p * S + t] < threshold)) { cid[t] = ncl; ++cnt; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (ln == 0) { leader[(size_t)ncl * n_lig + b] = p; size[(size_t)ncl * n_lig + b] = cnt; }
        ++ncl;
        __syncthreads();
    }
    for (int s = ln; s < S; s += 64) {
        cluster_id[(size_t)s * n_lig + b] = cid[s];
        if (s >= ncl) { leader[(size_t)s * n_lig + b] = -1; size[(size_t)s * n_lig + b] = 0; }
    }
    if (ln == 0) n_clusters[b] = ncl;
}

extern "C" int fabind_pose_pair_rmsd(const float* poses, int n_pose, int n_atoms, const int* atom_off, const int* flat_off,
                                     const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* D, hipStream_t stream) {
    FB_REQUIRE(n_pose <= POSE_MAX_S, "fabind_pose_pair_rmsd: at most 512 poses");
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= POSE_MAX_N, "fabind_pose_pair_rmsd: at most 2048 atoms per ligand");
    if (n_ligands <= 0 || n_pose <= 0) return 0;
    const int ts = pose_tile_size(n_pose, max_atoms);
    const int n_tiles = (n_pose + ts - 1) / ts;
    const long blocks = (long)n_ligands * (n_tiles * (n_tiles + 1) / 2);
    FB_REQUIRE(blocks < (1L << 31), "fabind_pose_pair_rmsd: too many (ligand, tile pair) work-groups; split the batch");
    const size_t lds = (size_t)4 * ts * ts + (size_t)24 * ts * (max_atoms > 1 ? max_atoms : 1);
    hipLaunchKernelGGL(pose_pair_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), lds, stream, poses, n_pose, n_atoms, atom_off, flat_off,
                       auto_cnt, flat, max_atoms, ts, n_tiles, D);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_pose_cluster(const float* D, const float* conf, int n_pose, int n_ligands, float threshold, int* cluster_id,
                                   int* leader, int* size, int* n_clusters, hipStream_t stream) {
    FB_REQUIRE(n_pose <= POSE_MAX_S, "fabind_pose_cluster: at most 512 poses");
    if (n_ligands <= 0 || n_pose <= 0) return 0;
    hipLaunchKernelGGL(pose_cluster_kernel, dim3(n_ligands), dim3(64), 0, stream, D, conf, n_pose, n_ligands, threshold, cluster_id, leader,
                       size, n_clusters);
    FB_CHECK_LAUNCH();
    return 0;
}
