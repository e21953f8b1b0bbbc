// Conformers of one ligand against each other, or against reference conformers: the heavy-atom RMSD after the best rigid superposition,
// minimised over the ligand's automorphisms (RDKit's GetBestRMS; what pruneRmsThresh of its multi-conformer embedding compares).
// csrc/pose_cluster.hip compares poses that share the protein frame: no centring, no rotation.  Start conformers (csrc/embed.hip) are
// centred and lie in an arbitrary orientation, so here every pair is superposed.
//
//   c_s, c_t  centroids        G_s = sum_i |x_s,i - c_s|^2, G_t likewise
//   S_k = sum_i (x_s[a_k[i]] - c_s) (y_t,i - c_t)^T                             3 x 3
//   lambda_k = the largest eigenvalue of Horn's symmetric 4 x 4 matrix of S_k   (proper rotations only: a mirror image is another conformer)
//   E = min_k max(0, (G_s + G_t) - 2 lambda_k)          D = sqrt(E / n)
//
// conf_rmsd_kernel<PAIR, FIT>: one work-group of 256 threads per (ligand, row tile I, column tile J; J >= I in the pair form), at most
//   eight conformers to a tile (fewer when the two tiles of the largest ligand would not fit the LDS budget).  Staging: one wave per
//   conformer forms the centroid (a fixed-order wave sum in double over the atoms lane, lane + 64, ...), writes the CENTRED coordinates to
//   LDS as doubles ((double)x - c: exact by Sterbenz wherever |x| is within a factor two of |c|, so a far-away frame costs nothing) and
//   sums G in the same order.  A permutation does not move a centroid: c and G are per conformer, not per k.
//   Work: wave w owns the rows s = w and w + 4 of tile I.  For k = 0, 1, ... in ascending order it loads a_k[i] of its lanes into
//   registers (n <= 256: at most four per lane; larger ligands re-read the row), gathers the row conformer's atoms a_k[i] and sums the nine
//   entries of S_k against ALL column conformers of tile J at once: 72 double accumulators per lane, each over the atoms i = lane,
//   lane + 64, ... in ascending order by one fused multiply-add per atom.  Nine packed butterflies (conf_reduce8) leave the nine sums of
//   column conformer t in the eight lanes with lane >> 3 == bit-reversed t, so the 4 x 4 Jacobi eigen-solves (the sweep of fit_horn,
//   csrc/conformer_fit.h, copied: that file compiles under another contraction setting) of the eight column conformers run in different
//   lanes at the same time.  The minimum over k is a running minimum in the owning lane, k ascending, replaced on strictly smaller E
//   only: a fixed order, the lowest k on equal E, no atomics of any kind.
//   Every operation of an entry is fixed by its ligand and its two conformers: the same bits alone, in any batch, among any S / T, in
//   any tile or column slot and on a repeat.  The pair form computes s < t and mirrors; its diagonal is +0.0.
//   With FIT the lane also keeps Horn's eigenvector of the best k and writes the index k, the unit quaternion q and the translation
//   c_t - R(q) c_s in double: R(q) x_s[a_k[i]] + trans is x_s superposed on y_t.
#include "common.h"
#include "fabind_hip.h"

#define CONF_MAX_S 512
#define CONF_MAX_N 2048
#define CONF_TILE 8                               // most conformers per tile = the column conformers a wave sums at once
#define CONF_ROWS_PER_WAVE 2                      // CONF_TILE rows over four waves
#define CONF_LDS_BYTES 65536                      // both tiles centred in double + centroids + G: two work-groups fit a CU's 160 KB
#define CONF_THREADS 256
#define CONF_REG_N 256                            // up to this many atoms the permutation of a wave stays in registers
#define CONF_SWEEPS 16                            // FIT_SWEEPS of csrc/conformer_fit.h

// Every rounding is written out: an entry must not depend on the column slot (the copy of an unrolled loop) it happens to occupy.
#pragma clang fp contract(off)

__device__ __forceinline__ double conf_wave_sum(double v) {           // all 64 lanes get the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// pose_reduce8 (csrc/pose_cluster.hip) in double: the butterfly sum over the 64 lanes of eight values per lane at once.  The sum of v[t]
// ends in the eight lanes with 4 * bit5(lane) + 2 * bit4(lane) + bit3(lane) == t, the same bits in each of them and whatever t is.
__device__ __forceinline__ double conf_reduce8(const double (&v)[8], int ln) {
    const bool h5 = ln & 32, h4 = ln & 16, h3 = ln & 8;
    double w[4], u[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (h5 ? v[j + 4] : v[j]) + __shfl_xor(h5 ? v[j] : v[j + 4], 32, 64);
#pragma unroll
    for (int j = 0; j < 2; ++j) u[j] = (h4 ? w[j + 2] : w[j]) + __shfl_xor(h4 ? w[j] : w[j + 2], 16, 64);
    double r = (h3 ? u[1] : u[0]) + __shfl_xor(h3 ? u[0] : u[1], 8, 64);
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    return r;
}

// The largest eigenvalue of Horn's matrix of S (S[3 x + z] = sum p_x y_z: the rotation takes p onto y) by cyclic Jacobi, per lane.
// VEC: its eigenvector too (the unit quaternion, normalised).  The arithmetic on `a` does not depend on VEC.
template <bool VEC>
__device__ __forceinline__ double conf_horn(const double (&S)[9], double (&q)[4]) {
    double a[4][4], v[4][4];
    a[0][0] = S[0] + S[4] + S[8];
    a[1][1] = S[0] - S[4] - S[8];
    a[2][2] = -S[0] + S[4] - S[8];
    a[3][3] = -S[0] - S[4] + S[8];
    a[0][1] = a[1][0] = S[5] - S[7];
    a[0][2] = a[2][0] = S[6] - S[2];
    a[0][3] = a[3][0] = S[1] - S[3];
    a[1][2] = a[2][1] = S[1] + S[3];
    a[1][3] = a[3][1] = S[6] + S[2];
    a[2][3] = a[3][2] = S[5] + S[7];
    if (VEC) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int z = 0; z < 4; ++z) v[x][z] = x == z ? 1. : 0.;
    }
    for (int sweep = 0; sweep < CONF_SWEEPS; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (off == 0.) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                const double apq = a[p][r];
                if (apq == 0.) continue;
                const double g = 100. * fabs(apq);
                if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[r][r]) + g == fabs(a[r][r])) {
                    a[p][r] = a[r][p] = 0.;
                    continue;
                }
                const double theta = (a[r][r] - a[p][p]) / (2. * apq);
                const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double cs = 1. / sqrt(t * t + 1.), sn = t * cs;
#pragma unroll
                for (int x = 0; x < 4; ++x) {                          // a <- a G, v <- v G
                    const double xp = a[x][p], xq = a[x][r];
                    a[x][p] = cs * xp - sn * xq;
                    a[x][r] = sn * xp + cs * xq;
                    if (VEC) {
                        const double vp = v[x][p], vq = v[x][r];
                        v[x][p] = cs * vp - sn * vq;
                        v[x][r] = sn * vp + cs * vq;
                    }
                }
#pragma unroll
                for (int x = 0; x < 4; ++x) {                          // a <- G^T a
                    const double px = a[p][x], qx = a[r][x];
                    a[p][x] = cs * px - sn * qx;
                    a[r][x] = sn * px + cs * qx;
                }
                a[p][r] = a[r][p] = 0.;
            }
    }
    double best = a[0][0];
    if (VEC) { q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0]; }
#pragma unroll
    for (int x = 1; x < 4; ++x)
        if (a[x][x] > best) {                                          // the first of equal eigenvalues
            best = a[x][x];
            if (VEC) {
#pragma unroll
                for (int z = 0; z < 4; ++z) q[z] = v[z][x];
            }
        }
    if (VEC) {
        const double qn = 1. / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
        for (int z = 0; z < 4; ++z) q[z] = q[z] * qn;
    }
    return best;
}

static size_t conf_lds_bytes(int ts, int max_atoms) {                  // centroids [2 ts][3] + G [2 ts] + two tiles of [ts][3][n] doubles
    return (size_t)8 * (8 * ts) + (size_t)48 * ts * (max_atoms > 1 ? max_atoms : 1);
}

static int conf_tile_size(int n_conf, int max_atoms) {
    int ts = n_conf < CONF_TILE ? n_conf : CONF_TILE;
    while (ts > 1 && conf_lds_bytes(ts, max_atoms) > CONF_LDS_BYTES) --ts;
    return ts;                                                         // ts = 1 above 1364 atoms needs up to 96 KB: one work-group per CU
}

// One wave: conformer src (fp32 [n][3] of this ligand) -> centred doubles dst [3][n], its centroid cen[3] and G.
__device__ __forceinline__ void conf_stage(const float* __restrict__ src, int n, int ln, double* dst, double* cen, double* G) {
    double c[3] = {0., 0., 0.};
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) c[d] += (double)src[3 * i + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = conf_wave_sum(c[d]) / (double)n;
    double g = 0.;
    for (int i = ln; i < n; i += 64) {
        const double px = (double)src[3 * i] - c[0], py = (double)src[3 * i + 1] - c[1], pz = (double)src[3 * i + 2] - c[2];
        dst[i] = px; dst[n + i] = py; dst[2 * n + i] = pz;
        g += fma(pz, pz, fma(py, py, px * px));
    }
    g = conf_wave_sum(g);
    if (ln == 0) { cen[0] = c[0]; cen[1] = c[1]; cen[2] = c[2]; *G = g; }
}

template <bool PAIR, bool FIT>
__global__ __launch_bounds__(CONF_THREADS, 2) void conf_rmsd_kernel(const float* __restrict__ X, int n_x, const float* __restrict__ Y, int n_y,
                                                                    int n_atoms, const int* __restrict__ atom_off,
                                                                    const int* __restrict__ flat_off, const int* __restrict__ auto_cnt,
                                                                    const int* __restrict__ flat, int max_atoms, int ts, int n_it, int n_jt,
                                                                    float* __restrict__ D, int* __restrict__ auto_index,
                                                                    double* __restrict__ quat, double* __restrict__ trans) {
    extern __shared__ double conf_sm[];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    int b, I, J;
    if (PAIR) {
        const int n_tp = n_it * (n_it + 1) / 2;
        b = blockIdx.x / n_tp;
        int p = blockIdx.x - b * n_tp;
        I = 0;
        while (p >= n_it - I) { p -= n_it - I; ++I; }
        J = I + p;
    } else {
        const int n_tp = n_it * n_jt;
        b = blockIdx.x / n_tp;
        const int p = blockIdx.x - b * n_tp;
        I = p / n_jt;
        J = p - I * n_jt;
    }
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const int s0 = I * ts, t0 = J * ts;
    const int rows = min(ts, n_x - s0), cols = min(ts, n_y - t0);
    const bool diag = PAIR && I == J;
    float* Db = D + (size_t)b * n_x * n_y;
    if (n <= 0 || n > max_atoms) {                                     // an empty ligand: every distance is 0, the fit is the identity
        const float v = n <= 0 ? 0.f : NAN;                            // (a ligand larger than the LDS was sized for: NaN, nothing staged)
        for (int e = tid; e < rows * cols; e += CONF_THREADS) {
            const int s = s0 + e / cols, t = t0 + e % cols;
            if (PAIR) {
                Db[(size_t)s * n_y + t] = s == t ? 0.f : v;
                Db[(size_t)t * n_y + s] = s == t ? 0.f : v;
            } else {
                Db[(size_t)s * n_y + t] = v;
            }
            if (FIT) {
                const size_t o = ((size_t)b * n_x + s) * n_y + t;
                const double w = n <= 0 ? 0. : (double)NAN;
                auto_index[o] = 0;
                quat[4 * o] = n <= 0 ? 1. : w; quat[4 * o + 1] = w; quat[4 * o + 2] = w; quat[4 * o + 3] = w;
                trans[3 * o] = w; trans[3 * o + 1] = w; trans[3 * o + 2] = w;
            }
        }
        return;
    }
    double* cen = conf_sm;                                             // [2 ts][3]
    double* Gs = conf_sm + 6 * ts;                                     // [2 ts]
    double* xi = conf_sm + 8 * ts;                                     // [rows][3][n]
    double* xj = diag ? xi : xi + (size_t)ts * 3 * n;                  // [cols][3][n]
    const int cslot = diag ? 0 : ts;                                   // where the column tile's centroids and G start
    const int n_stage = diag ? rows : rows + cols;
    for (int r = wv; r < n_stage; r += 4) {
        if (r < rows)
            conf_stage(X + ((size_t)(s0 + r) * n_atoms + a0) * 3, n, ln, xi + (size_t)r * 3 * n, cen + 3 * r, Gs + r);
        else
            conf_stage(Y + ((size_t)(t0 + r - rows) * n_atoms + a0) * 3, n, ln, xj + (size_t)(r - rows) * 3 * n, cen + 3 * (ts + r - rows),
                       Gs + ts + r - rows);
    }
    __syncthreads();
    const int base = flat_off[b];
    const int K = min(auto_cnt[b], (flat_off[b + 1] - base) / n);      // never past the ligand's slot of the table
    const int nk = max(K, 1);                                          // K <= 0: the identity alone
    const bool in_regs = n <= CONF_REG_N;
    const int tl = ((ln >> 5) & 1) * 4 + ((ln >> 4) & 1) * 2 + ((ln >> 3) & 1);          // the column conformer this lane solves
    double bestE[CONF_ROWS_PER_WAVE], bestQ[CONF_ROWS_PER_WAVE][4];
    int bestK[CONF_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < CONF_ROWS_PER_WAVE; ++r) {
        bestE[r] = 0.; bestK[r] = 0;
        bestQ[r][0] = 1.; bestQ[r][1] = 0.; bestQ[r][2] = 0.; bestQ[r][3] = 0.;
    }
    int a[4] = {ln, ln + 64, ln + 128, ln + 192};
    for (int k = 0; k < nk; ++k) {
        const int* ak = flat + base + (size_t)k * n;
        if (in_regs && K > 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = ln + 64 * c;
                if (i < n) {
                    const int j = ak[i];
                    a[c] = (unsigned)j < (unsigned)n ? j : i;          // an entry out of range falls back to i
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CONF_ROWS_PER_WAVE; ++r) {
            const int s = wv + 4 * r;
            const int t_lo = diag ? s + 1 : 0;                         // the diagonal tile: the upper triangle only
            if (s >= rows || t_lo >= cols) continue;                   // wave-uniform
            const double* xs = xi + (size_t)s * 3 * n;
            double acc[9][CONF_TILE];
#pragma unroll
            for (int e = 0; e < 9; ++e)
#pragma unroll
                for (int t = 0; t < CONF_TILE; ++t) acc[e][t] = 0.;
            if (in_regs) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = ln + 64 * c;
                    if (i < n) {
                        const double g[3] = {xs[a[c]], xs[n + a[c]], xs[2 * n + a[c]]};
#pragma unroll
                        for (int t = 0; t < CONF_TILE; ++t)
                            if (t >= t_lo && t < cols) {
                                const double* y = xj + (size_t)t * 3 * n + i;
                                const double y0 = y[0], y1 = y[n], y2 = y[2 * n];
#pragma unroll
                                for (int x = 0; x < 3; ++x) {
                                    acc[3 * x][t] = fma(g[x], y0, acc[3 * x][t]);
                                    acc[3 * x + 1][t] = fma(g[x], y1, acc[3 * x + 1][t]);
                                    acc[3 * x + 2][t] = fma(g[x], y2, acc[3 * x + 2][t]);
                                }
                            }
                    }
                }
            } else {
                for (int i = ln; i < n; i += 64) {
                    int j = K > 0 ? ak[i] : i;
                    j = (unsigned)j < (unsigned)n ? j : i;
                    const double g[3] = {xs[j], xs[n + j], xs[2 * n + j]};
#pragma unroll
                    for (int t = 0; t < CONF_TILE; ++t)
                        if (t >= t_lo && t < cols) {
                            const double* y = xj + (size_t)t * 3 * n + i;
                            const double y0 = y[0], y1 = y[n], y2 = y[2 * n];
#pragma unroll
                            for (int x = 0; x < 3; ++x) {
                                acc[3 * x][t] = fma(g[x], y0, acc[3 * x][t]);
                                acc[3 * x + 1][t] = fma(g[x], y1, acc[3 * x + 1][t]);
                                acc[3 * x + 2][t] = fma(g[x], y2, acc[3 * x + 2][t]);
                            }
                        }
                }
            }
            double Sk[9], q[4] = {1., 0., 0., 0.};
#pragma unroll
            for (int e = 0; e < 9; ++e) Sk[e] = conf_reduce8(acc[e], ln);
            const double lam = conf_horn<FIT>(Sk, q);                  // lanes of a column slot past `cols` solve the zero matrix
            const int tc = tl < cols ? tl : 0;
            const double e0 = (Gs[s] + Gs[cslot + tc]) - 2. * lam;
            const double E = e0 > 0. ? e0 : (e0 != e0 ? e0 : 0.);      // max(0, .) that keeps a NaN
            if (k == 0 || E < bestE[r] || E != E) {                    // k ascending, strictly smaller only: the lowest k on equal E
                bestE[r] = E; bestK[r] = k;
                if (FIT) { bestQ[r][0] = q[0]; bestQ[r][1] = q[1]; bestQ[r][2] = q[2]; bestQ[r][3] = q[3]; }
            }
        }
    }
    const double dn = (double)n;
#pragma unroll
    for (int r = 0; r < CONF_ROWS_PER_WAVE; ++r) {
        const int s = wv + 4 * r;
        const int t_lo = diag ? s + 1 : 0;
        if (s >= rows || (ln & 7) != 0 || tl < t_lo || tl >= cols) continue;
        const int sg = s0 + s, tg = t0 + tl;
        const float d = (float)sqrt(bestE[r] / dn);
        Db[(size_t)sg * n_y + tg] = d;
        if (PAIR) Db[(size_t)tg * n_y + sg] = d;
        if (FIT) {
            const size_t o = ((size_t)b * n_x + sg) * n_y + tg;
            const double q0 = bestQ[r][0], qx = bestQ[r][1], qy = bestQ[r][2], qz = bestQ[r][3];
            const double* cs = cen + 3 * s;
            const double* ct = cen + 3 * (cslot + tl);
            double R[3][3];
            R[0][0] = q0 * q0 + qx * qx - qy * qy - qz * qz; R[0][1] = 2. * (qx * qy - q0 * qz); R[0][2] = 2. * (qx * qz + q0 * qy);
            R[1][0] = 2. * (qy * qx + q0 * qz); R[1][1] = q0 * q0 - qx * qx + qy * qy - qz * qz; R[1][2] = 2. * (qy * qz - q0 * qx);
            R[2][0] = 2. * (qz * qx - q0 * qy); R[2][1] = 2. * (qz * qy + q0 * qx); R[2][2] = q0 * q0 - qx * qx - qy * qy + qz * qz;
            auto_index[o] = bestK[r];
            quat[4 * o] = q0; quat[4 * o + 1] = qx; quat[4 * o + 2] = qy; quat[4 * o + 3] = qz;
#pragma unroll
            for (int d3 = 0; d3 < 3; ++d3) trans[3 * o + d3] = ct[d3] - (R[d3][0] * cs[0] + R[d3][1] * cs[1] + R[d3][2] * cs[2]);
        }
    }
    if (diag)
        for (int s = tid; s < rows; s += CONF_THREADS) Db[(size_t)(s0 + s) * n_y + s0 + s] = 0.f;
}

template <bool PAIR, bool FIT>
static int conf_launch(const float* X, int n_x, const float* Y, int n_y, int n_atoms, const int* atom_off, const int* flat_off,
                       const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* D, int* auto_index, double* quat,
                       double* trans, const char* what, hipStream_t stream) {
    const int ts = conf_tile_size(n_x > n_y ? n_x : n_y, max_atoms);
    const int n_it = (n_x + ts - 1) / ts, n_jt = (n_y + ts - 1) / ts;
    const long blocks = (long)n_ligands * (PAIR ? (long)n_it * (n_it + 1) / 2 : (long)n_it * n_jt);
    FB_REQUIRE(blocks < (1L << 31), what);
    const size_t lds = conf_lds_bytes(ts, max_atoms);
    if (lds > CONF_LDS_BYTES) {
        const hipError_t e_ = hipFuncSetAttribute((const void*)conf_rmsd_kernel<PAIR, FIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e_ != hipSuccess) { fabind_set_error(hipGetErrorString(e_)); return (int)e_; }
    }
    hipLaunchKernelGGL((conf_rmsd_kernel<PAIR, FIT>), dim3((unsigned)blocks), dim3(CONF_THREADS), lds, stream, X, n_x, Y, n_y, n_atoms,
                       atom_off, flat_off, auto_cnt, flat, max_atoms, ts, n_it, n_jt, D, auto_index, quat, trans);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_conformer_pair_rmsd(const float* X, int n_conf, int n_atoms, const int* atom_off, const int* flat_off,
                                          const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* D, hipStream_t stream) {
    FB_REQUIRE(n_conf <= CONF_MAX_S, "fabind_conformer_pair_rmsd: at most 512 conformers");
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= CONF_MAX_N, "fabind_conformer_pair_rmsd: at most 2048 atoms per ligand");
    if (n_ligands <= 0 || n_conf <= 0) return 0;
    return conf_launch<true, false>(X, n_conf, X, n_conf, n_atoms, atom_off, flat_off, auto_cnt, flat, n_ligands, max_atoms, D, nullptr, nullptr,
                                    nullptr, "fabind_conformer_pair_rmsd: too many (ligand, tile pair) work-groups; split the batch", stream);
}

extern "C" int fabind_conformer_cross_rmsd(const float* X, int n_conf, const float* Y, int n_ref, int n_atoms, const int* atom_off,
                                           const int* flat_off, const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* D,
                                           int* auto_index, double* quat, double* trans, hipStream_t stream) {
    FB_REQUIRE(n_conf <= CONF_MAX_S && n_ref <= CONF_MAX_S, "fabind_conformer_cross_rmsd: at most 512 conformers on either side");
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= CONF_MAX_N, "fabind_conformer_cross_rmsd: at most 2048 atoms per ligand");
    const bool fit = auto_index != nullptr;
    FB_REQUIRE(fit == (quat != nullptr) && fit == (trans != nullptr),
               "fabind_conformer_cross_rmsd: auto_index, quat and trans are given together or not at all");
    if (n_ligands <= 0 || n_conf <= 0 || n_ref <= 0) return 0;
    const char* what = "fabind_conformer_cross_rmsd: too many (ligand, tile pair) work-groups; split the batch";
    if (fit)
        return conf_launch<false, true>(X, n_conf, Y, n_ref, n_atoms, atom_off, flat_off, auto_cnt, flat, n_ligands, max_atoms, D, auto_index,
                                        quat, trans, what, stream);
    return conf_launch<false, false>(X, n_conf, Y, n_ref, n_atoms, atom_off, flat_off, auto_cnt, flat, n_ligands, max_atoms, D, nullptr, nullptr,
                                     nullptr, what, stream);
}
