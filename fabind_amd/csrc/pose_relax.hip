// Relax sampled poses out of contact with the protein and with themselves, in torsion space (no counterpart in the reference: its
// post-optimisation never sees the protein).  The start conformer moves over its rotatable-bond dihedrals and one explicit rigid motion
// (a unit quaternion and a translation, both in double); bond lengths, angles and rings stay exactly the start conformer's.
// DESIGN.md section 19 has the definitions and bounds.
//
//   E = w_fit sum_i |X_i - y_i|^2 + w_prot sum_{i,p} max(0, c_prot (r_i + r_p) - |X_i - P_p|)^2
//     + w_intra sum_{i<j} max(0, c_intra (r_i + r_j) - |X_i - X_j|)^2      p: every kept protein atom, (i, j): the PAIR_CLASH pairs
//
// pose_relax_kernel: one work-group of ONE wave per (complex, pose), all iterations inside the launch, LDS sized by the launch -- the
//   frame of csrc/conformer_fit.hip, whose routines (conformer_fit.h: the torsion pass, Horn's fit, the wave sum) it shares.
//   X(a, q, t) = R(q) torsions(x0c, a) + t is rebuilt from the centred start conformer on every trial (float32 torsion pass, the rigid
//   motion in double, the pose held as float32 in the frame where the target's centroid is the origin); protein atoms are brought into
//   that frame in double when they are read.  The rigid motion starts as the Horn fit of torsions(x0c, angles0) onto the target.
//   One evaluation (relax_eval): lane L owns atoms L, L + 64, ...; an atom walks the 27 cells round it in a fixed order (cells are sorted
//   by atom id) and then its row of pair classes, and leaves A_i = w_fit I + w_prot sum n n^T (+ 2 w_intra n n^T per intra pair, the
//   positive semi-definite majorant of the cross terms) and b_i = w_fit (y_i - X_i) + w_prot sum (reach - d) n (+- w_intra (reach - d) n)
//   in LDS; the three sums run per lane in ascending order, then a butterfly.  A pair is active iff d < reach; at d = 0 it has an energy
//   and no direction.
//   One iteration (damped Gauss-Newton, the fit's schedule): every column of the Jacobian is w x X_i + m (T torsions, three
//   translations, three rotations about the centroid c); H = sum_i J_i^T A_i J_i and g = sum_i J_i^T b_i (grad E = -2 g exactly);
//   (H + lam (diag H + 1e-12)) d = g by Cholesky; trial angles a + d[:T] wrapped to (-pi, pi], q' = exp(omega) q renormalised,
//   t' = c + exp(omega) (t - c) + tau; accepted iff E(trial) < E, then lam = max(lam / 10, 1e-9), else lam *= 10; stop codes 0
//   (E - E' <= tol E), 1 (iteration cap), 2 (8 rejections in a row), 3 (a non-finite input: NaN outputs).
//   More than 256 atoms (status 3): the Horn image from global memory, no iteration; more than 58 torsions (status 4): relaxed rigidly.
//   No atomics, no inline assembly, plain vector stores; every sum has a fixed order that depends on the complex and the pose alone:
//   the same bits alone, in any batch, among any number of poses and on a repeat.
#include "common.h"
#include "fabind_hip.h"
#include "conformer_fit.h"

#pragma clang fp contract(off)

#define RX_MAX_N 256
#define RX_MAX_T 58
#define RX_MAX_REJECT 8
#define RX_PI 3.14159265358979323846
#define RX_CLAMP 536870912.0                                           // 2^29, the cell clamp of csrc/protein_contacts.hip
#define RX_NO_INTRA 8
#define RX_NO_PROTEIN 16

struct RelaxParams { double w_fit, w_prot, w_intra, c_prot, c_intra; };
struct RelaxGrid {                                                     // the complex's cell list; have = 0: no protein term
    int have, c0, k0, k1, ox, oy, oz, dx, dy, dz;
    const int* cell_ptr;
    const float* xyz;
    const float* rad;
    double edge, cy[3];
};

__device__ __forceinline__ bool rx_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }
__device__ __forceinline__ int rx_cell(double x, double edge) {
    const double q = floor(x / edge);
    return (int)(q < -RX_CLAMP ? -RX_CLAMP : q > RX_CLAMP ? RX_CLAMP : q);
}

__device__ __forceinline__ void rx_rotation(const double q[4], double R[3][3]) {
    const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
    R[0][0] = q0 * q0 + qx * qx - qy * qy - qz * qz; R[0][1] = 2. * (qx * qy - q0 * qz); R[0][2] = 2. * (qx * qz + q0 * qy);
    R[1][0] = 2. * (qy * qx + q0 * qz); R[1][1] = q0 * q0 - qx * qx + qy * qy - qz * qz; R[1][2] = 2. * (qy * qz - q0 * qx);
    R[2][0] = 2. * (qz * qx - q0 * qy); R[2][1] = 2. * (qz * qy + q0 * qx); R[2][2] = q0 * q0 - qx * qx - qy * qy + qz * qz;
}

// sp <- R(q) torsions(sx0, ang) + t as float32; each lane rewrites its own atoms only
__device__ __forceinline__ void rx_pose(int n, int T, int ln, const float* sx0, const int* squad, const uint32_t* smask, const float* ang,
                                        const double q[4], const double t[3], float* sp) {
    fit_torsions(n, T, ln, sx0, squad, smask, ang, sp);
    double R[3][3];
    rx_rotation(q, R);
    for (int i = ln; i < n; i += 64) {
        const double px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) sp[3 * i + d] = (float)(((R[d][0] * px + R[d][1] * py) + R[d][2] * pz) + t[d]);
    }
    __syncthreads();
}

// one active pair into the atom's A (packed 00 01 02 11 12 22) and b: n = e / d, A += wa n n^T, b += wb rho n
__device__ __forceinline__ void rx_push(double ex, double ey, double ez, double d, double rho, double wa, double wb, double A[6], double b[3]) {
    if (!(d > 0.)) return;
    const double inv = 1. / d, nx = ex * inv, ny = ey * inv, nz = ez * inv;
    A[0] += wa * (nx * nx); A[1] += wa * (nx * ny); A[2] += wa * (nx * nz);
    A[3] += wa * (ny * ny); A[4] += wa * (ny * nz); A[5] += wa * (nz * nz);
    const double f = wb * rho;
    b[0] += f * nx; b[1] += f * ny; b[2] += f * nz;
}

// The three unweighted sums of E at the pose sp (the same bits in every lane), and A_i / b_i of every atom into sA [6 n] / sb [3 n].
__device__ __forceinline__ void rx_eval(int n, int ln, const float* sp, const double* sy, const float* srad, const uint32_t* scls,
                                        const RelaxGrid& g, const RelaxParams& w, double* sA, double* sb, double e[3]) {
    double ef = 0., ep = 0., ei = 0.;
    for (int i = ln; i < n; i += 64) {
        const double x = sp[3 * i], y = sp[3 * i + 1], z = sp[3 * i + 2], ri = (double)srad[i];
        const double rx = sy[3 * i] - x, ry = sy[3 * i + 1] - y, rz = sy[3 * i + 2] - z;
        ef += (rx * rx + ry * ry) + rz * rz;
        double A[6] = {w.w_fit, 0., 0., w.w_fit, 0., w.w_fit}, b[3] = {w.w_fit * rx, w.w_fit * ry, w.w_fit * rz};
        if (g.have) {
            const int ccx = rx_cell(x + g.cy[0], g.edge) - g.ox, ccy = rx_cell(y + g.cy[1], g.edge) - g.oy, ccz = rx_cell(z + g.cy[2], g.edge) - g.oz;
            for (int k = 0; k < 27; ++k) {
                const int cx = ccx + (k % 3 - 1), cy = ccy + ((k / 3) % 3 - 1), cz = ccz + (k / 9 - 1);
                if ((unsigned)cx >= (unsigned)g.dx || (unsigned)cy >= (unsigned)g.dy || (unsigned)cz >= (unsigned)g.dz) continue;
                const int cid = g.c0 + (cz * g.dy + cy) * g.dx + cx;   // < c0 + dx dy dz = the complex's cells (checked on entry)
                const int q0 = max(g.cell_ptr[cid], g.k0), q1 = min(g.cell_ptr[cid + 1], g.k1);
                for (int q = q0; q < q1; ++q) {
                    const double ex = x - ((double)g.xyz[3 * (size_t)q] - g.cy[0]), ey = y - ((double)g.xyz[3 * (size_t)q + 1] - g.cy[1]),
                                 ez = z - ((double)g.xyz[3 * (size_t)q + 2] - g.cy[2]);
                    const double d = sqrt((ex * ex + ey * ey) + ez * ez), reach = w.c_prot * (ri + (double)g.rad[q]);
                    if (d < reach) {
                        const double rho = reach - d;
                        ep += rho * rho;
                        rx_push(ex, ey, ez, d, rho, w.w_prot, w.w_prot, A, b);
                    }
                }
            }
        }
        if (scls != nullptr) {
            const uint32_t* row = scls + 16 * i;
            for (int j = 0; j < n; ++j) {
                if (((row[j >> 4] >> (2 * (j & 15))) & 3u) != 3u) continue;
                const double ex = x - (double)sp[3 * j], ey = y - (double)sp[3 * j + 1], ez = z - (double)sp[3 * j + 2];
                const double d = sqrt((ex * ex + ey * ey) + ez * ez), reach = w.c_intra * (ri + (double)srad[j]);
                if (d < reach) {
                    const double rho = reach - d;
                    if (j > i) ei += rho * rho;
                    rx_push(ex, ey, ez, d, rho, 2. * w.w_intra, w.w_intra, A, b);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) sA[6 * i + k] = A[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) sb[3 * i + k] = b[k];
    }
    e[0] = fit_wave_sum(ef); e[1] = fit_wave_sum(ep); e[2] = fit_wave_sum(ei);
    __syncthreads();
}

__device__ __forceinline__ double rx_total(const double e[3], const RelaxParams& w) {
    return (w.w_fit * e[0] + w.w_prot * e[1]) + w.w_intra * e[2];
}

__global__ __launch_bounds__(64) void pose_relax_kernel(
    const float* __restrict__ x0g, const float* __restrict__ tgt, const float* __restrict__ angles0, const int* __restrict__ atom_off,
    int n_atoms, const int* __restrict__ tor_off, const int* __restrict__ quad, const uint32_t* __restrict__ side, int t_total, int n_cap,
    int t_cap, const int* __restrict__ plan_status, const uint32_t* __restrict__ cls, const float* __restrict__ lig_radii,
    const int* __restrict__ grid_status, const int* __restrict__ origin, const int* __restrict__ dims, const int* __restrict__ cell_off,
    const int* __restrict__ kept_off, const int* __restrict__ cell_ptr, const float* __restrict__ pxyz, const float* __restrict__ prad,
    float edge_f, RelaxParams w, int max_iters, float tol, float* __restrict__ coords, float* __restrict__ angles,
    double* __restrict__ energy0, double* __restrict__ energy, int* __restrict__ iters, int* __restrict__ stop, int* __restrict__ status,
    double* __restrict__ trace) {
    extern __shared__ double rx_lds[];
    const int b = blockIdx.x, s = blockIdx.y, ln = threadIdx.x, B = gridDim.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const int t0 = tor_off != nullptr ? tor_off[b] : 0;
    const int Tplan = tor_off != nullptr ? max(0, min(tor_off[b + 1], t_total) - t0) : 0;
    const bool intra = plan_status != nullptr && cls != nullptr && plan_status[b] == 0;
    RelaxGrid g;
    g.have = 0;
    if (grid_status != nullptr && grid_status[b] == 0) {
        g.c0 = cell_off[b]; g.k0 = kept_off[b]; g.k1 = kept_off[b + 1];
        g.ox = origin[3 * b]; g.oy = origin[3 * b + 1]; g.oz = origin[3 * b + 2];
        g.dx = dims[3 * b]; g.dy = dims[3 * b + 1]; g.dz = dims[3 * b + 2];
        // a grid whose box and cells disagree is never indexed
        g.have = g.dx >= 0 && g.dy >= 0 && g.dz >= 0 && (long long)g.dx * g.dy * g.dz == (long long)(cell_off[b + 1] - g.c0) && g.k1 >= g.k0 && g.c0 >= 0;
    }
    g.cell_ptr = cell_ptr; g.xyz = pxyz; g.rad = prad; g.edge = (double)edge_f;
    const int code = n > n_cap ? 3 : Tplan > t_cap ? 4 : 0;            // n_cap <= 256, t_cap <= 58: nothing past the LDS carved below
    const int st = code | (intra ? 0 : RX_NO_INTRA) | (g.have ? 0 : RX_NO_PROTEIN);
    const size_t o = (size_t)s * B + b;
    if (s == 0 && ln == 0) status[b] = st;
    if (angles != nullptr)
        for (int t = ln; t < Tplan; t += 64) angles[(size_t)s * t_total + t0 + t] = 0.f;
    double* tr = trace != nullptr ? trace + o * (size_t)max_iters : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const float* xb = x0g + (size_t)a0 * 3;
    const float* yb = tgt + ((size_t)s * n_atoms + a0) * 3;
    float* ob = coords + ((size_t)s * n_atoms + a0) * 3;
    const int T = code == 0 ? Tplan : 0;
    const float* a0g = angles0 != nullptr && T > 0 ? angles0 + (size_t)s * t_total + t0 : nullptr;
    // ---- a NaN or infinite input ends this pose alone
    bool finite = true;
    for (int i = ln; i < 3 * max(n, 0); i += 64) finite &= rx_finite(xb[i]) && rx_finite(yb[i]);
    if (a0g != nullptr)
        for (int t = ln; t < T; t += 64) finite &= rx_finite(a0g[t]);
    if (__ballot(!finite) != 0ull) {
        const float fnan = __uint_as_float(0x7fc00000u);
        for (int i = ln; i < 3 * n; i += 64) ob[i] = fnan;
        if (angles != nullptr)
            for (int t = ln; t < Tplan; t += 64) angles[(size_t)s * t_total + t0 + t] = fnan;
        if (ln < 3) { energy0[o * 3 + ln] = qnan; energy[o * 3 + ln] = qnan; }
        if (ln == 0) { iters[o] = 0; stop[o] = 3; }
        if (tr != nullptr)
            for (int i = ln; i < max_iters; i += 64) tr[i] = qnan;
        return;
    }
    if (n <= 0 || code == 3) {
        double e = 0.;
        if (n > 0) {                                                   // more atoms than LDS holds: the Horn image from global memory
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
        if (ln < 3) {                                                  // the protein and intra sums of such a ligand are not evaluated
            const double v = ln == 0 ? e : n > 0 ? qnan : 0.;
            energy0[o * 3 + ln] = v; energy[o * 3 + ln] = v;
        }
        if (ln == 0) { iters[o] = 0; stop[o] = max_iters > 0 ? 0 : 1; }
        if (tr != nullptr)
            for (int i = ln; i < max_iters; i += 64) tr[i] = qnan;
        return;
    }
    const int M = T + 6, mc = t_cap + 6, ntri = mc * (mc + 1) / 2;
    double* sy = rx_lds;                                               // [3 n_cap] the target, its centroid at the origin
    double* sH = sy + 3 * n_cap;                                       // [ntri] sum J^T A J, packed lower triangle
    double* sL = sH + ntri;                                            // [ntri] its damped Cholesky factor
    double* scol = sL + ntri;                                          // [6 mc] (w, m) of every column
    double* sA = scol + 6 * mc;                                        // [6 n_cap] A_i at the accepted pose
    double* sb = sA + 6 * n_cap;                                       // [3 n_cap] b_i
    double* sAt = sb + 3 * n_cap;                                      // [6 n_cap] the same at the trial pose
    double* sbt = sAt + 6 * n_cap;                                     // [3 n_cap]
    float* sx0 = (float*)(sbt + 3 * n_cap);                            // [3 n_cap] the start conformer, centred
    float* sp = sx0 + 3 * n_cap;                                       // [3 n_cap] the trial pose
    float* sX = sp + 3 * n_cap;                                        // [3 n_cap] the accepted pose
    float* srad = sX + 3 * n_cap;                                      // [n_cap]
    float* sa = srad + n_cap;                                          // [t_cap] accepted angles
    float* sat = sa + t_cap;                                           // [t_cap] trial angles
    uint32_t* smask = (uint32_t*)(sat + t_cap);                        // [8 mc] the atoms every column moves
    uint32_t* scls = smask + 8 * mc;                                   // [16 n_cap] the pair classes of every atom's row
    int* squad = (int*)(scls + 16 * n_cap);                            // [4 t_cap]
    double cx[3] = {0., 0., 0.}, cy[3] = {0., 0., 0.};
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { cx[d] += (double)xb[3 * i + d]; cy[d] += (double)yb[3 * i + d]; }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { cx[d] = fit_wave_sum(cx[d]) / (double)n; cy[d] = fit_wave_sum(cy[d]) / (double)n; g.cy[d] = cy[d]; }
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sx0[3 * i + d] = (float)((double)xb[3 * i + d] - cx[d]);
            sy[3 * i + d] = (double)yb[3 * i + d] - cy[d];
        }
        srad[i] = lig_radii != nullptr ? lig_radii[a0 + i] : 0.f;
    }
    if (intra)
        for (int i = ln; i < 16 * n; i += 64) scls[i] = cls[(size_t)a0 * 16 + i];
    for (int t = ln; t < T; t += 64) {
        const int* q = quad + (size_t)(t0 + t) * 4;
        const int qi = q[0], qj = q[1], qk = q[2], ql = q[3];
        const bool ok = (unsigned)qi < (unsigned)n && (unsigned)qj < (unsigned)n && (unsigned)qk < (unsigned)n && (unsigned)ql < (unsigned)n;
        squad[4 * t] = ok ? qi : -1; squad[4 * t + 1] = ok ? qj : -1; squad[4 * t + 2] = ok ? qk : -1; squad[4 * t + 3] = ok ? ql : -1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t m = ok ? side[(size_t)(t0 + t) * 8 + k] : 0u;
            if (ok && k == (qk >> 5)) m &= ~(1u << (qk & 31));         // k is on the axis: it never moves
            smask[8 * t + k] = m;
        }
        sa[t] = a0g != nullptr ? a0g[t] : 0.f;
    }
    for (int i = ln; i < 48; i += 64) smask[8 * T + i] = 0xffffffffu;  // translations and rotations: every atom
    __syncthreads();
    // ---- the start: the Horn fit of torsions(x0c, angles0) onto the target
    double q[4], tv[3];
    {
        fit_torsions(n, T, ln, sx0, squad, smask, sa, sp);
        FitRigid r;
        fit_horn(n, ln, [&](int i, int d) { return (double)sp[3 * i + d]; }, [&](int i, int d) { return sy[3 * i + d]; }, r);
#pragma unroll
        for (int d = 0; d < 4; ++d) q[d] = r.q[d];
#pragma unroll
        for (int d = 0; d < 3; ++d) tv[d] = r.cy[d] - ((r.R[d][0] * r.cp[0] + r.R[d][1] * r.cp[1]) + r.R[d][2] * r.cp[2]);
        __syncthreads();
    }
    rx_pose(n, T, ln, sx0, squad, smask, sa, q, tv, sp);
    const uint32_t* cl = intra ? scls : nullptr;
    double es[3];
    rx_eval(n, ln, sp, sy, srad, cl, g, w, sAt, sbt, es);
    for (int i = ln; i < 3 * n; i += 64) { sX[i] = sp[i]; sb[i] = sbt[i]; }
    for (int i = ln; i < 6 * n; i += 64) sA[i] = sAt[i];
    __syncthreads();
    double E = rx_total(es, w);
    if (ln < 3) energy0[o * 3 + ln] = ln == 0 ? es[0] : ln == 1 ? es[1] : es[2];
    double lam = 1e-3;
    int it = 0, scode = max_iters > 0 ? 0 : 1;
    bool done = max_iters <= 0 || E == 0.;
    while (!done) {
        // ---- the columns of the Jacobian at sX
        double mx = 0., my = 0., mz = 0.;
        for (int i = ln; i < n; i += 64) { mx += (double)sX[3 * i]; my += (double)sX[3 * i + 1]; mz += (double)sX[3 * i + 2]; }
        mx = fit_wave_sum(mx) / (double)n; my = fit_wave_sum(my) / (double)n; mz = fit_wave_sum(mz) / (double)n;
        if (ln < M) {
            double cw[3] = {0., 0., 0.}, cm[3] = {0., 0., 0.};
            if (ln < T) {
                const int qj = squad[4 * ln + 1], qk = squad[4 * ln + 2];
                if (qj >= 0) {
                    const double pj[3] = {(double)sX[3 * qj], (double)sX[3 * qj + 1], (double)sX[3 * qj + 2]};
                    const double ax = (double)sX[3 * qk] - pj[0], ay = (double)sX[3 * qk + 1] - pj[1], az = (double)sX[3 * qk + 2] - pj[2];
                    const double l2 = ax * ax + ay * ay + az * az;
                    if (l2 > 0.) {
                        const double inv = 1. / sqrt(l2);
                        cw[0] = ax * inv; cw[1] = ay * inv; cw[2] = az * inv;
                        cm[0] = -(cw[1] * pj[2] - cw[2] * pj[1]);
                        cm[1] = -(cw[2] * pj[0] - cw[0] * pj[2]);
                        cm[2] = -(cw[0] * pj[1] - cw[1] * pj[0]);
                    }
                }
            } else if (ln < T + 3) {
                cm[ln - T] = 1.;
            } else {
                const int d = ln - T - 3;
                cw[d] = 1.;
                if (d == 0) { cm[1] = mz; cm[2] = -my; }               // -(e_x x c) = (0, c_z, -c_y)
                if (d == 1) { cm[0] = -mz; cm[2] = mx; }               // -(e_y x c) = (-c_z, 0, c_x)
                if (d == 2) { cm[0] = my; cm[1] = -mx; }               // -(e_z x c) = (c_y, -c_x, 0)
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) { scol[6 * ln + d] = cw[d]; scol[6 * ln + 3 + d] = cm[d]; }
        }
        __syncthreads();
        // ---- H = sum J_i^T A_i J_i: lane L owns entries L, L + 64, ... of the packed triangle and runs over the atoms in ascending order
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
            for (int k = 0; k * 32 < n; ++k) {
                const uint32_t mw = smask[8 * i + k] & smask[8 * j + k];
                if (mw == 0u) continue;                                // nothing to add: the order of the rest is unchanged
                const int hi = min(32, n - k * 32);
                for (int bit = 0; bit < hi; ++bit) {
                    if (!((mw >> bit) & 1u)) continue;
                    const int a = k * 32 + bit;
                    const double x = (double)sX[3 * a], y = (double)sX[3 * a + 1], z = (double)sX[3 * a + 2];
                    const double ji0 = (wi1 * z - wi2 * y) + mi0, ji1 = (wi2 * x - wi0 * z) + mi1, ji2 = (wi0 * y - wi1 * x) + mi2;
                    const double jj0 = (wj1 * z - wj2 * y) + mj0, jj1 = (wj2 * x - wj0 * z) + mj1, jj2 = (wj0 * y - wj1 * x) + mj2;
                    const double* A = sA + 6 * a;
                    const double u0 = (A[0] * jj0 + A[1] * jj1) + A[2] * jj2, u1 = (A[1] * jj0 + A[3] * jj1) + A[4] * jj2,
                                 u2 = (A[2] * jj0 + A[4] * jj1) + A[5] * jj2;
                    acc += (ji0 * u0 + ji1 * u1) + ji2 * u2;
                }
            }
            sH[e] = acc;
        }
        // ---- g = sum J_i^T b_i: lane c owns column c
        double gc = 0.;
        if (ln < M) {
            const double w0 = scol[6 * ln], w1 = scol[6 * ln + 1], w2 = scol[6 * ln + 2];
            const double m0 = scol[6 * ln + 3], m1 = scol[6 * ln + 4], m2 = scol[6 * ln + 5];
            for (int a = 0; a < n; ++a) {
                if (!((smask[8 * ln + (a >> 5)] >> (a & 31)) & 1u)) continue;
                const double x = (double)sX[3 * a], y = (double)sX[3 * a + 1], z = (double)sX[3 * a + 2];
                const double j0 = (w1 * z - w2 * y) + m0, j1 = (w2 * x - w0 * z) + m1, j2 = (w0 * y - w1 * x) + m2;
                gc += (j0 * sb[3 * a] + j1 * sb[3 * a + 1]) + j2 * sb[3 * a + 2];
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
                double sij = 0.;
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
            double Et = 0., et[3] = {0., 0., 0.}, qt[4] = {1., 0., 0., 0.}, tt[3] = {0., 0., 0.};
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
                    sat[ln] = (float)(a - 2. * RX_PI * ceil((a - RX_PI) / (2. * RX_PI)));
                }
                // ---- the rigid step about the centroid: q' = exp(omega) q renormalised, t' = c + exp(omega) (t - c) + tau
                const double tau[3] = {__shfl(z, T, 64), __shfl(z, T + 1, 64), __shfl(z, T + 2, 64)};
                const double om[3] = {__shfl(z, T + 3, 64), __shfl(z, T + 4, 64), __shfl(z, T + 5, 64)};
                const double th = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
                double qe[4] = {1., 0., 0., 0.};
                if (th > 0.) {
                    const double sh = sin(0.5 * th) / th;
                    qe[0] = cos(0.5 * th); qe[1] = sh * om[0]; qe[2] = sh * om[1]; qe[3] = sh * om[2];
                }
                qt[0] = ((qe[0] * q[0] - qe[1] * q[1]) - qe[2] * q[2]) - qe[3] * q[3];
                qt[1] = ((qe[0] * q[1] + qe[1] * q[0]) + qe[2] * q[3]) - qe[3] * q[2];
                qt[2] = ((qe[0] * q[2] - qe[1] * q[3]) + qe[2] * q[0]) + qe[3] * q[1];
                qt[3] = ((qe[0] * q[3] + qe[1] * q[2]) - qe[2] * q[1]) + qe[3] * q[0];
                const double qn = 1. / sqrt(((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3]);
#pragma unroll
                for (int d = 0; d < 4; ++d) qt[d] *= qn;
                double Re[3][3];
                rx_rotation(qe, Re);
                const double c[3] = {mx, my, mz}, u[3] = {tv[0] - mx, tv[1] - my, tv[2] - mz};
#pragma unroll
                for (int d = 0; d < 3; ++d) tt[d] = (c[d] + ((Re[d][0] * u[0] + Re[d][1] * u[1]) + Re[d][2] * u[2])) + tau[d];
                __syncthreads();
                rx_pose(n, T, ln, sx0, squad, smask, sat, qt, tt, sp);
                rx_eval(n, ln, sp, sy, srad, cl, g, w, sAt, sbt, et);
                Et = rx_total(et, w);
            }
            if (!fail && Et < E) {                                     // wave-uniform: every lane holds the same bits of Et and E
                const double drop = E - Et;
                const bool small = drop <= (double)tol * E;
                E = Et;
#pragma unroll
                for (int d = 0; d < 3; ++d) { es[d] = et[d]; tv[d] = tt[d]; }
#pragma unroll
                for (int d = 0; d < 4; ++d) q[d] = qt[d];
                for (int i = ln; i < 3 * n; i += 64) { sX[i] = sp[i]; sb[i] = sbt[i]; }
                for (int i = ln; i < 6 * n; i += 64) sA[i] = sAt[i];
                for (int t = ln; t < T; t += 64) sa[t] = sat[t];
                lam = fmax(lam / 10., 1e-9);
                if (tr != nullptr && ln == 0) tr[it] = E;
                ++it;
                if (small) { scode = 0; done = true; }
                else if (it >= max_iters) { scode = 1; done = true; }
                __syncthreads();
                break;
            }
            lam *= 10.;
            if (++rejected >= RX_MAX_REJECT) { scode = 2; done = true; break; }
        }
    }
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) ob[3 * i + d] = (float)((double)sX[3 * i + d] + cy[d]);
    }
    if (angles != nullptr)
        for (int t = ln; t < T; t += 64) angles[(size_t)s * t_total + t0 + t] = sa[t];
    if (ln < 3) energy[o * 3 + ln] = ln == 0 ? es[0] : ln == 1 ? es[1] : es[2];
    if (ln == 0) { iters[o] = it; stop[o] = scode; }
    if (tr != nullptr)
        for (int i = it + ln; i < max_iters; i += 64) tr[i] = qnan;
}

static size_t rx_lds_bytes(int n_cap, int t_cap) {
    const size_t mc = (size_t)t_cap + 6, ntri = mc * (mc + 1) / 2;
    return sizeof(double) * ((size_t)21 * n_cap + 2 * ntri + 6 * mc) + sizeof(float) * ((size_t)10 * n_cap + 2 * (size_t)t_cap) +
           sizeof(int) * (8 * mc + (size_t)16 * n_cap + 4 * (size_t)t_cap);
}

extern "C" int fabind_pose_relax(const float* x0, const float* target, const float* angles0, const int* atom_off, int n_complex, int n_atoms,
                                 int n_poses, const int* tor_off, const int* quad, const unsigned* side, int t_total, int max_atoms,
                                 int max_torsions, const int* plan_status, const unsigned* cls, const float* lig_radii,
                                 const int* grid_status, const int* origin, const int* dims, const int* cell_off, const int* kept_off,
                                 const int* cell_ptr, const float* prot_xyz, const float* prot_radii, float edge, float max_reach,
                                 float w_fit, float w_prot, float w_intra, float c_prot, float c_intra, int max_iters, float tol,
                                 float* coords, float* angles, double* energy0, double* energy, int* iters, int* stop, int* status,
                                 double* trace, hipStream_t stream) {
    if (n_complex <= 0 || n_poses <= 0) return 0;
    FB_REQUIRE(n_poses <= 65535, "fabind_pose_relax: at most 65535 poses");
    FB_REQUIRE(max_iters >= 0 && max_iters <= 65536, "fabind_pose_relax: max_iters in [0, 65536]");
    FB_REQUIRE(t_total >= 0 && max_atoms >= 0 && max_torsions >= 0, "fabind_pose_relax: t_total, max_atoms, max_torsions >= 0");
    FB_REQUIRE(tor_off == nullptr || t_total == 0 || (quad != nullptr && side != nullptr && angles != nullptr),
               "fabind_pose_relax: a torsion plan needs quad, side and angles");
    FB_REQUIRE(x0 != nullptr && target != nullptr && atom_off != nullptr && coords != nullptr && energy0 != nullptr && energy != nullptr &&
                   iters != nullptr && stop != nullptr && status != nullptr,
               "fabind_pose_relax: x0, target, atom_off, coords, energy0, energy, iters, stop and status are needed");
    FB_REQUIRE(plan_status == nullptr || cls == nullptr || lig_radii != nullptr, "fabind_pose_relax: the intra term needs the ligand radii");
    FB_REQUIRE(grid_status == nullptr || (lig_radii != nullptr && origin != nullptr && dims != nullptr && cell_off != nullptr &&
                                          kept_off != nullptr && cell_ptr != nullptr),
               "fabind_pose_relax: the protein term needs the ligand radii and the grid's origin, dims, offsets and cell_ptr");
    FB_REQUIRE(w_fit >= 0.0f && w_prot >= 0.0f && w_intra >= 0.0f && c_prot >= 0.0f && c_intra >= 0.0f && w_fit <= 3.4028234663852886e38f &&
                   w_prot <= 3.4028234663852886e38f && w_intra <= 3.4028234663852886e38f && c_prot <= 3.4028234663852886e38f &&
                   c_intra <= 3.4028234663852886e38f,
               "fabind_pose_relax: weights and reach factors must be finite and >= 0");
    FB_REQUIRE(grid_status == nullptr || (edge > 0.0f && edge <= 3.4028234663852886e38f && max_reach >= 0.0f && max_reach <= edge),
               "fabind_pose_relax: edge positive and finite, and c_prot * (largest ligand radius + largest protein radius) <= edge");
    const int n_cap = max_atoms < 1 ? 1 : max_atoms > RX_MAX_N ? RX_MAX_N : max_atoms;
    const int t_cap = tor_off == nullptr ? 0 : max_torsions > RX_MAX_T ? RX_MAX_T : max_torsions;
    const size_t lds = rx_lds_bytes(n_cap, t_cap);
    static bool attr_set = false;
    if (!attr_set) {                                                   // 109,424 B at the limits: past the 64 KiB a launch gets by default
        const hipError_t e = hipFuncSetAttribute((const void*)pose_relax_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)rx_lds_bytes(RX_MAX_N, RX_MAX_T));
        if (e != hipSuccess) { fabind_set_error(hipGetErrorString(e)); return (int)e; }
        attr_set = true;
    }
    RelaxParams w;
    w.w_fit = (double)w_fit; w.w_prot = (double)w_prot; w.w_intra = (double)w_intra; w.c_prot = (double)c_prot; w.c_intra = (double)c_intra;
    hipLaunchKernelGGL(pose_relax_kernel, dim3(n_complex, n_poses), dim3(64), lds, stream, x0, target, angles0, atom_off, n_atoms, tor_off, quad,
                       (const uint32_t*)side, t_total, n_cap, t_cap, plan_status, (const uint32_t*)cls, lig_radii, grid_status, origin, dims,
                       cell_off, kept_off, cell_ptr, prot_xyz, prot_radii, edge, w, max_iters, tol, coords, angles, energy0, energy, iters, stop,
                       status, trace);
    FB_CHECK_LAUNCH();
    return 0;
}
