// Fit the start conformer to a target pose over its rotatable-bond dihedrals and one rigid motion (the inverse of
// conformer_perturb_kernel): local geometry -- bond lengths, angles, rings -- stays exactly that of the start conformer.
//
// conformer_fit_kernel: one work-group of ONE wave per (ligand, pose), all iterations inside the launch.  One wave because the
//   Cholesky and the two substitutions are sequential in the order of the system, every cross-lane step is then a butterfly or a
//   broadcast (no cross-wave partial sums whose order would have to be fixed, barriers that cost nothing), and the normal matrix of
//   a typical ligand (40 atoms, 8 torsions: 105 entries) is two rounds of 64 lanes.  LDS is sized by the launch (largest ligand, most
//   torsions): 16 KB for 60 atoms and 28 torsions, 54 KB at the limits.  Two packed triangles are held, H and its damped factor: a
//   rejected trial changes only lam, so the retry is a copy, a Cholesky and a pose; with one triangle factored in place it would have
//   to accumulate H again, the largest part of an iteration, up to 8 times in a row.  What one wave costs: 64 ligands x 40 poses are
//   2560 waves, 2048 of them resident at once (two per SIMD at 174 VGPRs), so the launch lasts about as long as its slowest
//   work-group (one that runs into the iteration cap); four waves per work-group would shorten exactly that and are the next step
//   if the fit ever sits on a critical path.
//   pose(a): the centred start conformer is copied, the torsions are applied one after another as relative rotations by a[t] in
//   float32 -- the rule and the arithmetic of conformer_perturb_kernel: axis j -> k through p_j, the atoms of `side` other than k move,
//   a zero-length axis skips the torsion -- then the optimal proper rotation and translation onto the target by Horn's quaternion
//   method in double: centroids, the 3 x 3 cross-covariance (each lane its atoms in ascending order, then the butterfly), the
//   eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix by cyclic Jacobi (at most 16 sweeps).  The pose is held as
//   float32 in the frame where the target's centroid is the origin; the centroid is subtracted on load and added on store.
//   One iteration (damped Gauss-Newton): column c of the Jacobian at the pose X is w_c x X_i + m_c on the atoms of its mask: torsion
//   t: w = u_t (unit axis of X), m = -u_t x X_j, mask = side minus k; translation d: w = 0, m = e_d; rotation d: w = e_d,
//   m = -e_d x centroid; both on all atoms.  H = J^T J (packed lower triangle, lane L owns entries L, L + 64, ... and runs over the
//   atoms in ascending order) and g = J^T (y - X) in double; (H + lam (diag H + 1e-12)) d = g by Cholesky (column by column, lane i
//   forms entry (i, j) from rows i and j), the substitutions with the vector in registers.  Trial a + d[:T] wrapped to (-pi, pi];
//   accepted iff E(trial) < E, then lam = max(lam / 10, 1e-9); else lam *= 10 and the solve is repeated, 8 rejections in a row stop
//   (code 2).  An accepted step that lowered E by no more than tol * E stops (code 0), max_iters accepted steps stop (code 1).
//   A ligand of more than 256 atoms (status 3) is fitted rigidly straight from global memory; one of more than 58 torsions (status 4)
//   rigidly from LDS; both get zero angles.  No atomics, no inline assembly; every sum has a fixed order that depends on the ligand
//   alone: the same bits alone, in any batch and among any number of poses.
#include "common.h"
#include "fabind_hip.h"
#include "conformer_fit.h"

#define FIT_MAX_N 256
#define FIT_MAX_T 58
#define FIT_MAX_REJECT 8
#define FIT_PI 3.14159265358979323846

// pose(ang): sp <- torsions on sx0, then the rigid fit onto sy; returns E = sum |sp - sy|^2 (the same bits in every lane).
__device__ __forceinline__ double fit_pose(int n, int T, int ln, const float* sx0, const double* sy, const int* squad,
                                           const uint32_t* smask, const float* ang, float* sp) {
    fit_torsions(n, T, ln, sx0, squad, smask, ang, sp);
    FitRigid r;
    fit_horn(n, ln, [&](int i, int d) { return (double)sp[3 * i + d]; }, [&](int i, int d) { return sy[3 * i + d]; }, r);
    double e = 0.;
    for (int i = ln; i < n; i += 64) {                                 // each lane rewrites and reads back its own atoms only
        const double px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float xf = (float)fit_image(r, px, py, pz, d);
            sp[3 * i + d] = xf;
            const double df = (double)xf - sy[3 * i + d];
            e += df * df;
        }
    }
    e = fit_wave_sum(e);
    __syncthreads();
    return e;
}

__global__ __launch_bounds__(64) void conformer_fit_kernel(const float* __restrict__ x0g, const float* __restrict__ tgt,
                                                           const int* __restrict__ atom_off, int n_atoms, const int* __restrict__ tor_off,
                                                           const int* __restrict__ quad, const uint32_t* __restrict__ side, int t_total,
                                                           int n_cap, int t_cap, int max_iters, float tol, float* __restrict__ coords,
                                                           float* __restrict__ angles, float* __restrict__ rmsd0, float* __restrict__ rmsd,
                                                           int* __restrict__ iters, int* __restrict__ stop, int* __restrict__ status,
                                                           double* __restrict__ trace) {
    extern __shared__ double fit_lds[];
    const int b = blockIdx.x, s = blockIdx.y, ln = threadIdx.x, B = gridDim.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const int t0 = tor_off != nullptr ? tor_off[b] : 0;
    const int Tplan = tor_off != nullptr ? max(0, min(tor_off[b + 1], t_total) - t0) : 0;
    const int st = n > n_cap ? 3 : Tplan > t_cap ? 4 : 0;              // n_cap <= 256, t_cap <= 58: nothing past the LDS carved below
    const size_t o = (size_t)s * B + b;
    if (s == 0 && ln == 0) status[b] = st;
    if (angles != nullptr)
        for (int t = ln; t < Tplan; t += 64) angles[(size_t)s * t_total + t0 + t] = 0.f;
    double* tr = trace != nullptr ? trace + o * (size_t)max_iters : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const float* xb = x0g + (size_t)a0 * 3;
    const float* yb = tgt + ((size_t)s * n_atoms + a0) * 3;
    float* ob = coords + ((size_t)s * n_atoms + a0) * 3;
    if (n <= 0 || st == 3) {
        double e = 0.;
        if (n > 0) {                                                   // more atoms than LDS holds: the rigid fit from global memory
            FitRigid r;
            fit_horn(n, ln, [&](int i, int d) { return (double)xb[3 * i + d]; }, [&](int i, int d) { return (double)yb[3 * i + d]; }, r);
            for (int i = ln; i < n; i += 64) {
                const double px = xb[3 * i], py = xb[3 * i + 1], pz = xb[3 * i + 2];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float xf = (float)fit_image(r, px, py, pz, d);
                    ob[3 * i + d] = xf;
                    const double df = (double)xf - (double)yb[3 * i + d];
                    e += df * df;
                }
            }
            e = fit_wave_sum(e);
        }
        if (ln == 0) {
            const float rm = n > 0 ? (float)sqrt(e / (double)n) : 0.f;
            rmsd0[o] = rm; rmsd[o] = rm; iters[o] = 0; stop[o] = max_iters > 0 ? 0 : 1;
        }
        if (tr != nullptr)
            for (int i = ln; i < max_iters; i += 64) tr[i] = qnan;
        return;
    }
    const int T = st == 0 ? Tplan : 0, M = T + 6, mc = t_cap + 6, ntri = mc * (mc + 1) / 2;
    double* sy = fit_lds;                                              // [3 n_cap] the target, its centroid at the origin
    double* sH = sy + 3 * n_cap;                                       // [ntri] J^T J, packed lower triangle
    double* sL = sH + ntri;                                            // [ntri] its damped Cholesky factor
    double* scol = sL + ntri;                                          // [6 mc] (w, m) of every column
    float* sx0 = (float*)(scol + 6 * mc);                              // [3 n_cap] the start conformer, centred
    float* sp = sx0 + 3 * n_cap;                                       // [3 n_cap] the trial pose
    float* sX = sp + 3 * n_cap;                                        // [3 n_cap] the accepted pose
    float* sa = sX + 3 * n_cap;                                        // [t_cap] accepted angles
    float* sat = sa + t_cap;                                           // [t_cap] trial angles
    uint32_t* smask = (uint32_t*)(sat + t_cap);                        // [8 mc] the atoms every column moves
    int* squad = (int*)(smask + 8 * mc);                               // [4 t_cap]
    double cx[3] = {0., 0., 0.}, cy[3] = {0., 0., 0.};
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { cx[d] += (double)xb[3 * i + d]; cy[d] += (double)yb[3 * i + d]; }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { cx[d] = fit_wave_sum(cx[d]) / (double)n; cy[d] = fit_wave_sum(cy[d]) / (double)n; }
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sx0[3 * i + d] = (float)((double)xb[3 * i + d] - cx[d]);
            sy[3 * i + d] = (double)yb[3 * i + d] - cy[d];
        }
    }
    for (int t = ln; t < T; t += 64) {
        const int* q = quad + (size_t)(t0 + t) * 4;
        const int qi = q[0], qj = q[1], qk = q[2], ql = q[3];
        const bool ok = (unsigned)qi < (unsigned)n && (unsigned)qj < (unsigned)n && (unsigned)qk < (unsigned)n && (unsigned)ql < (unsigned)n;
        squad[4 * t] = ok ? qi : -1; squad[4 * t + 1] = ok ? qj : -1; squad[4 * t + 2] = ok ? qk : -1; squad[4 * t + 3] = ok ? ql : -1;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            uint32_t m = ok ? side[(size_t)(t0 + t) * 8 + w] : 0u;
            if (ok && w == (qk >> 5)) m &= ~(1u << (qk & 31));         // k is on the axis: it never moves
            smask[8 * t + w] = m;
        }
        sa[t] = 0.f;
    }
    for (int i = ln; i < 48; i += 64) smask[8 * T + i] = 0xffffffffu;  // translations and rotations: every atom
    __syncthreads();
    double E = fit_pose(n, T, ln, sx0, sy, squad, smask, sa, sp);
    for (int i = ln; i < 3 * n; i += 64) sX[i] = sp[i];
    __syncthreads();
    const double E0 = E;
    double lam = 1e-3;
    int it = 0, code = max_iters > 0 ? 0 : 1;
    bool done = T == 0 || n <= 2 || max_iters <= 0;
    while (!done) {
        // ---- the columns of the Jacobian at sX
        double mx = 0., my = 0., mz = 0.;
        for (int i = ln; i < n; i += 64) { mx += (double)sX[3 * i]; my += (double)sX[3 * i + 1]; mz += (double)sX[3 * i + 2]; }
        mx = fit_wave_sum(mx) / (double)n; my = fit_wave_sum(my) / (double)n; mz = fit_wave_sum(mz) / (double)n;
        if (ln < M) {
            double w[3] = {0., 0., 0.}, m[3] = {0., 0., 0.};
            if (ln < T) {
                const int qj = squad[4 * ln + 1], qk = squad[4 * ln + 2];
                if (qj >= 0) {
                    const double pj[3] = {(double)sX[3 * qj], (double)sX[3 * qj + 1], (double)sX[3 * qj + 2]};
                    const double ax = (double)sX[3 * qk] - pj[0], ay = (double)sX[3 * qk + 1] - pj[1], az = (double)sX[3 * qk + 2] - pj[2];
                    const double l2 = ax * ax + ay * ay + az * az;
                    if (l2 > 0.) {
                        const double inv = 1. / sqrt(l2);
                        w[0] = ax * inv; w[1] = ay * inv; w[2] = az * inv;
                        m[0] = -(w[1] * pj[2] - w[2] * pj[1]);
                        m[1] = -(w[2] * pj[0] - w[0] * pj[2]);
                        m[2] = -(w[0] * pj[1] - w[1] * pj[0]);
                    }
                }
            } else if (ln < T + 3) {
                m[ln - T] = 1.;
            } else {
                const int d = ln - T - 3;
                w[d] = 1.;
                if (d == 0) { m[1] = mz; m[2] = -my; }                 // -(e_x x c) = (0, c_z, -c_y)
                if (d == 1) { m[0] = -mz; m[2] = mx; }                 // -(e_y x c) = (-c_z, 0, c_x)
                if (d == 2) { m[0] = my; m[1] = -mx; }                 // -(e_z x c) = (c_y, -c_x, 0)
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) { scol[6 * ln + d] = w[d]; scol[6 * ln + 3 + d] = m[d]; }
        }
        __syncthreads();
        // ---- H = J^T J: lane L owns entries L, L + 64, ... of the packed triangle and runs over the atoms in ascending order
        const int nent = M * (M + 1) / 2;
        for (int e = ln; e < nent; e += 64) {
            int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
            while ((i + 1) * (i + 2) / 2 <= e) ++i;
            while (i * (i + 1) / 2 > e) --i;
            const int j = e - i * (i + 1) / 2;
            const double wi0 = scol[6 * i], wi1 = scol[6 * i + 1], wi2 = scol[6 * i + 2];
            const double mi0 = scol[6 * i + 3], mi1 = scol[6 * i + 4], mi2 = scol[6 * i + 5];
            const double wj0 = scol[6 * j], wj1 = scol[6 * j + 1], wj2 = scol[6 * j + 2];
            const double mj0 = scol[6 * j + 3], mj1 = scol[6 * j + 4], mj2 = scol[6 * j + 5];
            double acc = 0.;
            for (int w = 0; w * 32 < n; ++w) {
                const uint32_t mw = smask[8 * i + w] & smask[8 * j + w];
                if (mw == 0u) continue;                                // nothing to add: the order of the rest is unchanged
                const int hi = min(32, n - w * 32);
                for (int bit = 0; bit < hi; ++bit) {
                    if (!((mw >> bit) & 1u)) continue;
                    const int a = w * 32 + bit;
                    const double x = (double)sX[3 * a], y = (double)sX[3 * a + 1], z = (double)sX[3 * a + 2];
                    const double ji0 = (wi1 * z - wi2 * y) + mi0, ji1 = (wi2 * x - wi0 * z) + mi1, ji2 = (wi0 * y - wi1 * x) + mi2;
                    const double jj0 = (wj1 * z - wj2 * y) + mj0, jj1 = (wj2 * x - wj0 * z) + mj1, jj2 = (wj0 * y - wj1 * x) + mj2;
                    acc += ji0 * jj0 + ji1 * jj1 + ji2 * jj2;
                }
            }
            sH[e] = acc;
        }
        // ---- g = J^T (y - X): lane c owns column c
        double gc = 0.;
        if (ln < M) {
            const double w0 = scol[6 * ln], w1 = scol[6 * ln + 1], w2 = scol[6 * ln + 2];
            const double m0 = scol[6 * ln + 3], m1 = scol[6 * ln + 4], m2 = scol[6 * ln + 5];
            for (int a = 0; a < n; ++a) {
                if (!((smask[8 * ln + (a >> 5)] >> (a & 31)) & 1u)) continue;
                const double x = (double)sX[3 * a], y = (double)sX[3 * a + 1], z = (double)sX[3 * a + 2];
                const double j0 = (w1 * z - w2 * y) + m0, j1 = (w2 * x - w0 * z) + m1, j2 = (w0 * y - w1 * x) + m2;
                gc += j0 * (sy[3 * a] - x) + j1 * (sy[3 * a + 1] - y) + j2 * (sy[3 * a + 2] - z);
            }
        }
        __syncthreads();
        int rejected = 0;
        for (;;) {
            // ---- (H + lam (diag H + 1e-12)) d = g by Cholesky; lane i owns row i
            for (int e = ln; e < nent; e += 64) sL[e] = sH[e];
            __syncthreads();
            if (ln < M) sL[fit_tri(ln, ln)] += lam * (sH[fit_tri(ln, ln)] + 1e-12);
            bool fail = false;
            __syncthreads();
            for (int j = 0; j < M; ++j) {                              // column j: row i against row j over the columns before j
                double sij = 0.;                                       // (reads only in the loop: the LDS latency overlaps)
                if (ln >= j && ln < M) {
                    const double* ri = sL + fit_tri(ln, 0);
                    const double* rj = sL + fit_tri(j, 0);
                    sij = ri[j];
                    for (int k = 0; k < j; ++k) sij -= ri[k] * rj[k];
                }
                const double djj = __shfl(sij, j, 64);
                if (!(djj > 0.)) { fail = true; break; }               // wave-uniform (also NaN)
                const double piv = sqrt(djj);
                if (ln >= j && ln < M) sL[fit_tri(ln, j)] = ln == j ? piv : sij / piv;
                __syncthreads();
            }
            __syncthreads();
            double Et = 0.;
            if (!fail) {
                double z = ln < M ? gc : 0.;
                for (int j = 0; j < M; ++j) {                          // L z = g
                    const double zj = __shfl(z, j, 64) / sL[fit_tri(j, j)];
                    if (ln == j) z = zj;
                    else if (ln > j && ln < M) z -= sL[fit_tri(ln, j)] * zj;
                }
                for (int j = M - 1; j >= 0; --j) {                     // L^T d = z
                    const double dj = __shfl(z, j, 64) / sL[fit_tri(j, j)];
                    if (ln == j) z = dj;
                    else if (ln < j) z -= sL[fit_tri(j, ln)] * dj;
                }
                if (ln < T) {
                    const double a = (double)sa[ln] + z;
                    sat[ln] = (float)(a - 2. * FIT_PI * ceil((a - FIT_PI) / (2. * FIT_PI)));
                }
                __syncthreads();
                Et = fit_pose(n, T, ln, sx0, sy, squad, smask, sat, sp);
            }
            if (!fail && Et < E) {                                     // wave-uniform: every lane holds the same bits of Et and E
                const double drop = E - Et;
                const bool small = drop <= (double)tol * E;
                E = Et;
                for (int i = ln; i < 3 * n; i += 64) sX[i] = sp[i];
                for (int t = ln; t < T; t += 64) sa[t] = sat[t];
                lam = fmax(lam / 10., 1e-9);
                if (tr != nullptr && ln == 0) tr[it] = E;
                ++it;
                if (small) { code = 0; done = true; }
                else if (it >= max_iters) { code = 1; done = true; }
                __syncthreads();
                break;
            }
            lam *= 10.;
            if (++rejected >= FIT_MAX_REJECT) { code = 2; done = true; break; }
        }
    }
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) ob[3 * i + d] = (float)((double)sX[3 * i + d] + cy[d]);
    }
    if (angles != nullptr)
        for (int t = ln; t < T; t += 64) angles[(size_t)s * t_total + t0 + t] = sa[t];
    if (ln == 0) {
        rmsd0[o] = (float)sqrt(E0 / (double)n); rmsd[o] = (float)sqrt(E / (double)n); iters[o] = it; stop[o] = code;
    }
    if (tr != nullptr)
        for (int i = it + ln; i < max_iters; i += 64) tr[i] = qnan;
}

extern "C" int fabind_conformer_fit(const float* x0, const float* target, const int* atom_off, int n_ligands, int n_atoms, int n_poses,
                                    const int* tor_off, const int* quad, const unsigned* side, int t_total, int max_atoms,
                                    int max_torsions, int max_iters, float tol, float* coords, float* angles, float* rmsd0, float* rmsd,
                                    int* iters, int* stop, int* status, double* trace, hipStream_t stream) {
    if (n_ligands <= 0 || n_poses <= 0) return 0;
    FB_REQUIRE(n_poses <= 65535, "fabind_conformer_fit: at most 65535 poses");
    FB_REQUIRE(max_iters >= 0 && max_iters <= 65536, "fabind_conformer_fit: max_iters in [0, 65536]");
    FB_REQUIRE(t_total >= 0 && max_atoms >= 0 && max_torsions >= 0, "fabind_conformer_fit: t_total, max_atoms, max_torsions >= 0");
    FB_REQUIRE(tor_off == nullptr || t_total == 0 || (quad != nullptr && side != nullptr && angles != nullptr),
               "fabind_conformer_fit: a torsion plan needs quad, side and angles");
    FB_REQUIRE(coords != nullptr && rmsd0 != nullptr && rmsd != nullptr && iters != nullptr && stop != nullptr && status != nullptr,
               "fabind_conformer_fit: coords, rmsd0, rmsd, iters, stop and status are needed");
    const int n_cap = max_atoms < 1 ? 1 : max_atoms > FIT_MAX_N ? FIT_MAX_N : max_atoms;
    const int t_cap = tor_off == nullptr ? 0 : max_torsions > FIT_MAX_T ? FIT_MAX_T : max_torsions;
    const int mc = t_cap + 6, ntri = mc * (mc + 1) / 2;
    const size_t lds = sizeof(double) * ((size_t)3 * n_cap + 2 * (size_t)ntri + 6 * (size_t)mc) +
                       sizeof(float) * ((size_t)9 * n_cap + 2 * (size_t)t_cap) + sizeof(int) * ((size_t)8 * mc + 4 * (size_t)t_cap);
    hipLaunchKernelGGL(conformer_fit_kernel, dim3(n_ligands, n_poses), dim3(64), lds, stream, x0, target, atom_off, n_atoms, tor_off, quad,
                       (const uint32_t*)side, t_total, n_cap, t_cap, max_iters, tol, coords, angles, rmsd0, rmsd, iters, stop, status, trace);
    FB_CHECK_LAUNCH();
    return 0;
}
