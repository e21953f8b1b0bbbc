// Ligand poses from a predicted protein-ligand distance map (reference FABind/fabind/utils/generation_utils.py:42-120, the
// TankBind-style generation): `epochs` Adam iterations (lr 0.1, betas 0.9/0.999, eps 1e-8) on the ligand coordinates x against
//
//   dis_ik = min(|p_i - x_k|, 10),  r_ik = dis_ik - y_pred[i, k]
//   interaction   = sum |r|  (mode 0)  |  sum r^2  (mode 1)  |  sum (|r| + 1e-5)^0.5  (mode 2)
//   configuration = sum_{listed (k,j)} | |x_k - x_j| - D_kj |  [+ 2 sum_{k,j} relu(1.22 - |x_k - x_j|) if excluded_volume]
//   loss_t        = interaction                                         for t <  config_start
//                 = interaction + config_rate (t - config_start) configuration   for t >= config_start      (t 0-based)
//
// One work-group per (ligand, repeat) runs ALL epochs in one launch.  The ligand's coordinates, the pocket's coordinates and --
// when they fit -- its block of y_pred and its constraint lists live in LDS; positions, both Adam moments and the true pose sit in
// registers.  A ligand of n atoms is served by teams of T = 2^k lanes, T the largest power of two with 256 / T >= n (T = 1 and two
// atoms per thread above 256 atoms): the lanes of a team split the residue loop, the excluded-volume loop and the constraint list
// of their atom and combine the gradient with a butterfly inside the team.  T depends on n alone and every sum has a fixed
// order (no atomics), so a ligand's result does not depend on the rest of the batch or on the number of repeats, and two runs
// give identical bits.  Gradient conventions follow torch: d|.|/dx = 0 at 0, relu'(0) = 0, cdist' = 0 at distance 0, the clamp
// passes gradient at dis == 10 and blocks it above.  Adam's scalar bias corrections are formed in double, as torch forms them.
// Modes 0 and 1 run in float (RT = float).  Mode 2 runs in double (RT = double: coordinates, moments, distances, sums): its
// gradient 0.5 (|r| + 1e-5)^-0.5 has the slope 8e6 at r = 0, so a residual rounded in float changes a pair's pull by order one and
// a float run leaves the exact iteration by up to 4e-4 A within three epochs; inputs and outputs stay float.
#include "common.h"
#include "fabind_hip.h"

#define DG_THREADS 256
#define DG_APT 2                                  // atoms per thread at T = 1 -> ligands of up to 512 atoms
#define DG_MAX_POCKET 4096                        // pocket residues per complex (48 KiB of LDS)
#define DG_LDS_BUDGET (144 * 1024)                // dynamic LDS per work-group (gfx950: 160 KiB per CU)
#define DG_RED 16                                 // floats of reduction scratch

__device__ __forceinline__ float dg_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double dg_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float dg_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double dg_abs(double v) { return fabs(v); }
template <typename RT> __device__ __forceinline__ RT dg_sign(RT v) { return (RT)((v > (RT)0) - (v < (RT)0)); }
template <typename RT> __device__ __forceinline__ RT dg_wave_sum(RT v) {  // all 64 lanes get the total
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order sums of three values over the work-group; every thread gets the totals
template <typename RT> __device__ __forceinline__ void dg_block_sum3(RT& a, RT& b, RT& c, RT* red) {
    a = dg_wave_sum(a); b = dg_wave_sum(b); c = dg_wave_sum(c);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; red[w] = a; red[4 + w] = b; red[8 + w] = c; }
    __syncthreads();
    a = b = c = (RT)0;
#pragma unroll
    for (int w = 0; w < DG_THREADS / 64; ++w) { a += red[w]; b += red[4 + w]; c += red[8 + w]; }
}

// A loop-invariant pointer that only the reporting thread uses, kept in a vector register pair: the epoch loop's uniform state
// (sizes, offsets, loop masks) fills the wave's scalar registers, and these six pointers would otherwise be parked and fetched back.
template <typename P> __device__ __forceinline__ P* dg_in_vgpr(P* p) { asm volatile("" : "+v"(p)); return p; }

// the launch's arguments as one kernarg block: the kernel reads a field where it needs it and holds no copy of the rest in SGPRs
struct DgArgs {
    const float *x0, *truth, *pocket, *y_pred, *con_d;
    const int *pocket_off, *atom_off, *con_ptr, *con_idx;
    const long long* y_off;
    float *x_out, *loss_out, *terms_out, *rmsd_out, *trace_loss, *trace_rmsd;
    double config_rate, lr;
    int n_ligands, n_atoms, max_atoms, max_pocket, max_con, max_y, excluded_volume, mode, epochs, config_start;
};

template <typename RT, bool Y_LDS, bool C_LDS>
__global__ __launch_bounds__(DG_THREADS) void distgen_kernel(const DgArgs A) {
    const float* __restrict__ x0 = A.x0; const float* __restrict__ truth = A.truth; const float* __restrict__ pocket = A.pocket;
    const int* __restrict__ pocket_off = A.pocket_off; const float* __restrict__ y_pred = A.y_pred; const long long* __restrict__ y_off = A.y_off;
    const int* __restrict__ atom_off = A.atom_off; const int* __restrict__ con_ptr = A.con_ptr; const int* __restrict__ con_idx = A.con_idx;
    const float* __restrict__ con_d = A.con_d;
    const int n_ligands = A.n_ligands, n_atoms = A.n_atoms, max_atoms = A.max_atoms, max_pocket = A.max_pocket, max_con = A.max_con,
              max_y = A.max_y, excluded_volume = A.excluded_volume, epochs = A.epochs, config_start = A.config_start;
    const int mode = sizeof(RT) == sizeof(double) ? 2 : (A.mode == 1 ? 1 : 0);      // the launcher sends mode 2, and only mode 2, to the double forms
    const double config_rate = A.config_rate, lr = A.lr;
    float* const x_out = dg_in_vgpr(A.x_out); float* const loss_out = dg_in_vgpr(A.loss_out); float* const terms_out = dg_in_vgpr(A.terms_out);
    float* const rmsd_out = dg_in_vgpr(A.rmsd_out); float* const trace_loss = dg_in_vgpr(A.trace_loss); float* const trace_rmsd = dg_in_vgpr(A.trace_rmsd);
    extern __shared__ __align__(16) unsigned char sm[];
    const int lig = blockIdx.x, rep = blockIdx.y, tid = threadIdx.x;
    const int a0 = atom_off[lig], n = atom_off[lig + 1] - a0;
    const int p0 = pocket_off[lig], P = pocket_off[lig + 1] - p0;
    const int c0 = con_ptr[a0], nc = con_ptr[a0 + n] - c0;
    const int ns = n | 1;                         // odd row stride of the LDS copy of y_pred: residues of one team hit distinct banks
    // the host sized the LDS from these maxima; a block that exceeds them touches nothing
    if (n > max_atoms || P > max_pocket || (C_LDS && nc > max_con) || (Y_LDS && (long long)P * ns > max_y)) return;
    RT* sx = (RT*)sm;                             // [n][3] current coordinates
    RT* red = sx + 3 * max_atoms;                 // [DG_RED]
    float* sp = (float*)(red + DG_RED);           // [P][3] pocket
    int* scj = (int*)(sp + 3 * max_pocket);       // [nc] constraint partner (local atom id)
    float* scd = (float*)(scj + (C_LDS ? max_con : 0));   // [nc] constraint target distance
    float* sy = scd + (C_LDS ? max_con : 0);      // [P][ns] y_pred
    const float* xin = x0 + ((size_t)rep * n_atoms + a0) * 3;
    const float* yg = y_pred + y_off[lig];
    for (int i = tid; i < 3 * n; i += DG_THREADS) sx[i] = xin[i];
    for (int i = tid; i < 3 * P; i += DG_THREADS) sp[i] = pocket[(size_t)p0 * 3 + i];
    if (C_LDS)
        for (int e = tid; e < nc; e += DG_THREADS) { scj[e] = con_idx[c0 + e] - a0; scd[e] = con_d[c0 + e]; }
    if (Y_LDS)
        for (int i = tid; i < P * n; i += DG_THREADS) { const int r = i / n; sy[r * ns + (i - r * n)] = yg[i]; }
    __syncthreads();

    int T = 1;                                    // lanes per atom
    while (T < 64 && DG_THREADS / (2 * T) >= n) T *= 2;
    const int n_teams = DG_THREADS / T, team = tid / T, lane = tid - team * T;

    RT x[DG_APT][3], tr[DG_APT][3], m[DG_APT][3], v[DG_APT][3];
    int e0[DG_APT], e1[DG_APT];
#pragma unroll
    for (int a = 0; a < DG_APT; ++a) {
        const int k = team + a * n_teams;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[a][c] = k < n ? sx[3 * k + c] : (RT)0;
            tr[a][c] = k < n ? (RT)truth[(size_t)(a0 + k) * 3 + c] : (RT)0;
            m[a][c] = (RT)0; v[a][c] = (RT)0;
        }
        e0[a] = k < n ? con_ptr[a0 + k] - c0 : 0;
        e1[a] = k < n ? con_ptr[a0 + k + 1] - c0 : 0;
    }
    const size_t out = (size_t)rep * n_ligands + lig;
    double b1t = 1.0, b2t = 1.0;                  // beta^t
    for (int t = 0; t < epochs; ++t) {
        const bool last = t == epochs - 1, report = last || trace_loss != nullptr;
        const bool with_cfg = t >= config_start;
        const RT w = with_cfg ? (RT)(config_rate * (double)(t - config_start)) : (RT)0;
        RT g[DG_APT][3], li = (RT)0, lc = (RT)0;
#pragma unroll
        for (int a = 0; a < DG_APT; ++a) {
            const int k = team + a * n_teams;
            const bool act = k < n;               // uniform over a team
            RT gi0 = (RT)0, gi1 = (RT)0, gi2 = (RT)0, gc0 = (RT)0, gc1 = (RT)0, gc2 = (RT)0;
            const int Pk = act ? P : 0;
            for (int i = lane; i < Pk; i += T) {
                const RT dx = x[a][0] - sp[3 * i], dy = x[a][1] - sp[3 * i + 1], dz = x[a][2] - sp[3 * i + 2];
                const RT d = dg_sqrt(dx * dx + dy * dy + dz * dz);
                const RT yv = Y_LDS ? sy[i * ns + k] : yg[(size_t)i * n + k];
                const RT r = (d < (RT)10 ? d : (RT)10) - yv;
                RT dr;
                if (mode == 0) { li += dg_abs(r); dr = dg_sign(r); }
                else if (mode == 1) { li += r * r; dr = (RT)2 * r; }
                else { const RT q = dg_sqrt(dg_abs(r) + (RT)1e-5); li += q; dr = (RT)0.5 / q * dg_sign(r); }
                if (d <= (RT)10 && d > (RT)0) { const RT s = dr / d; gi0 += s * dx; gi1 += s * dy; gi2 += s * dz; }
            }
            if (with_cfg || last) {
                if (excluded_volume) {
                    const int nk = act ? n : 0;
                    for (int j = lane; j < nk; j += T) {      // 2 relu(1.22 - d) for (k,j) and for (j,k); j == k adds the constant 2.44
                        const RT dx = x[a][0] - sx[3 * j], dy = x[a][1] - sx[3 * j + 1], dz = x[a][2] - sx[3 * j + 2];
                        const RT d = dg_sqrt(dx * dx + dy * dy + dz * dz);
                        if (d < (RT)1.22) {
                            lc += (RT)2 * ((RT)1.22 - d);
                            if (d > (RT)0) { const RT s = (RT)-4 / d; gc0 += s * dx; gc1 += s * dy; gc2 += s * dz; }
                        }
                    }
                }
                for (int e = e0[a] + lane; e < e1[a]; e += T) {   // every listed ordered pair sits in both ends' lists: loss 1/2, gradient 1
                    const int j = C_LDS ? scj[e] : con_idx[c0 + e] - a0;
                    const RT D = C_LDS ? scd[e] : con_d[c0 + e];
                    const RT dx = x[a][0] - sx[3 * j], dy = x[a][1] - sx[3 * j + 1], dz = x[a][2] - sx[3 * j + 2];
                    const RT d = dg_sqrt(dx * dx + dy * dy + dz * dz);
                    const RT dev = d - D;
                    lc += (RT)0.5 * dg_abs(dev);
                    if (d > (RT)0) { const RT s = dg_sign(dev) / d; gc0 += s * dx; gc1 += s * dy; gc2 += s * dz; }
                }
            }
            g[a][0] = gi0 + w * gc0; g[a][1] = gi1 + w * gc1; g[a][2] = gi2 + w * gc2;
            for (int o = T >> 1; o > 0; o >>= 1) {            // butterfly inside the team: every lane ends with the same total
                g[a][0] += __shfl_xor(g[a][0], o, 64);
                g[a][1] += __shfl_xor(g[a][1], o, 64);
                g[a][2] += __shfl_xor(g[a][2], o, 64);
            }
        }
        __syncthreads();                          // every thread has read the old coordinates
        b1t *= 0.9; b2t *= 0.999;
        const RT step = (RT)(lr / (1.0 - b1t)), bc2 = (RT)sqrt(1.0 - b2t);
        RT sq = (RT)0;
#pragma unroll
        for (int a = 0; a < DG_APT; ++a) {
            const int k = team + a * n_teams;
            if (k >= n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                m[a][c] = m[a][c] + (RT)0.1 * (g[a][c] - m[a][c]);
                v[a][c] = (RT)0.999 * v[a][c] + (RT)0.001 * g[a][c] * g[a][c];
                x[a][c] -= step * m[a][c] / (dg_sqrt(v[a][c]) / bc2 + (RT)1e-8);
                if (lane == 0) {
                    sx[3 * k + c] = x[a][c];
                    const RT dq = tr[a][c] - x[a][c];
                    sq += dq * dq;
                }
            }
        }
        if (report) {                             // loss of this epoch (before its step), RMSD after the step
            dg_block_sum3(li, lc, sq, red);
            const RT loss = with_cfg ? li + w * lc : li, rmsd = dg_sqrt(sq / (RT)max(n, 1));
            if (tid == 0) {
                if (trace_loss) { trace_loss[out * epochs + t] = (float)loss; trace_rmsd[out * epochs + t] = (float)rmsd; }
                if (last) { loss_out[out] = (float)loss; terms_out[2 * out] = (float)li; terms_out[2 * out + 1] = (float)lc; rmsd_out[out] = (float)rmsd; }
            }
        }
        __syncthreads();
    }
    float* xo = x_out + ((size_t)rep * n_atoms + a0) * 3;
#pragma unroll
    for (int a = 0; a < DG_APT; ++a) {
        const int k = team + a * n_teams;
        if (k >= n || lane != 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) xo[3 * k + c] = (float)x[a][c];
    }
}

extern "C" int fabind_distmap_generate(const float* x0, const float* truth, const float* pocket, const int* pocket_off,
                                       const float* y_pred, const long long* y_off, const int* atom_off, const int* con_ptr,
                                       const int* con_idx, const float* con_d, int n_ligands, int n_repeat, int n_atoms, int max_atoms,
                                       int max_pocket, int max_con, long max_y, int excluded_volume, int mode, int epochs,
                                       int config_start, const double* rate_lr, float* x_out, float* loss_out, float* terms_out,
                                       float* rmsd_out, float* trace_loss, float* trace_rmsd, hipStream_t stream) {
    if (n_ligands <= 0 || n_repeat <= 0) return 0;
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= DG_THREADS * DG_APT, "fabind_distmap_generate: at most 512 atoms per ligand");
    FB_REQUIRE(max_pocket >= 0 && max_pocket <= DG_MAX_POCKET, "fabind_distmap_generate: at most 4096 pocket residues per complex");
    FB_REQUIRE(mode >= 0 && mode <= 2, "fabind_distmap_generate: mode is 0, 1 or 2");
    FB_REQUIRE(epochs >= 1, "fabind_distmap_generate: epochs >= 1");
    FB_REQUIRE(rate_lr != nullptr, "fabind_distmap_generate: rate_lr (host {config_rate, lr}) missing");
    const double config_rate = rate_lr[0], lr = rate_lr[1];
    FB_REQUIRE(n_repeat <= 65535, "fabind_distmap_generate: at most 65535 repeats");
    FB_REQUIRE(max_con >= 0 && max_y >= 0, "fabind_distmap_generate: negative size");
    FB_REQUIRE(con_ptr != nullptr && (max_con == 0 || (con_idx != nullptr && con_d != nullptr)), "fabind_distmap_generate: constraint lists missing");
    FB_REQUIRE((trace_loss == nullptr) == (trace_rmsd == nullptr), "fabind_distmap_generate: pass both trace buffers or neither");
    const bool dbl = mode == 2;                   // mode 2 iterates in double (see the head of this file)
    size_t lds = (size_t)(3 * max_atoms + DG_RED) * (dbl ? sizeof(double) : sizeof(float)) + (size_t)3 * max_pocket * sizeof(float);   // at most 60 KiB
    const bool c_lds = lds + (size_t)max_con * 8 <= DG_LDS_BUDGET;
    if (c_lds) lds += (size_t)max_con * 8;
    const bool y_lds = lds + (size_t)max_y * 4 <= DG_LDS_BUDGET;
    if (y_lds) lds += (size_t)max_y * 4;
    DgArgs A;
    A.x0 = x0; A.truth = truth; A.pocket = pocket; A.y_pred = y_pred; A.con_d = con_d; A.pocket_off = pocket_off; A.atom_off = atom_off;
    A.con_ptr = con_ptr; A.con_idx = con_idx; A.y_off = y_off; A.x_out = x_out; A.loss_out = loss_out; A.terms_out = terms_out;
    A.rmsd_out = rmsd_out; A.trace_loss = trace_loss; A.trace_rmsd = trace_rmsd; A.config_rate = config_rate; A.lr = lr;
    A.n_ligands = n_ligands; A.n_atoms = n_atoms; A.max_atoms = max_atoms; A.max_pocket = max_pocket; A.max_con = max_con;
    A.max_y = (int)(y_lds ? max_y : 0); A.excluded_volume = excluded_volume; A.mode = mode; A.epochs = epochs; A.config_start = config_start;
    // more than 64 KiB of dynamic LDS needs the attribute raised, per device: set it on every such launch (a host-side table lookup)
#define DG_LAUNCH(RR, YY, CC)                                                                                                       \
    do {                                                                                                                            \
        if (lds > 64 * 1024) {                                                                                                      \
            const hipError_t e_ = hipFuncSetAttribute((const void*)distgen_kernel<RR, YY, CC>, hipFuncAttributeMaxDynamicSharedMemorySize, DG_LDS_BUDGET); \
            if (e_ != hipSuccess) { fabind_set_error(hipGetErrorString(e_)); return (int)e_; }                                      \
        }                                                                                                                           \
        hipLaunchKernelGGL((distgen_kernel<RR, YY, CC>), dim3(n_ligands, n_repeat), dim3(DG_THREADS), lds, stream, A);               \
    } while (0)
#define DG_FORMS(RR)                                  \
    do {                                              \
        if (y_lds && c_lds) DG_LAUNCH(RR, true, true);  \
        else if (y_lds) DG_LAUNCH(RR, true, false);     \
        else if (c_lds) DG_LAUNCH(RR, false, true);     \
        else DG_LAUNCH(RR, false, false);               \
    } while (0)
    if (dbl) DG_FORMS(double);
    else DG_FORMS(float);
#undef DG_FORMS
#undef DG_LAUNCH
    FB_CHECK_LAUNCH();
    return 0;
}
