// A Vina-style intermolecular energy of every sampled pose against ALL heavy atoms of its protein (no counterpart in the reference; the
// functional form and constants of AutoDock Vina 1.1.2 -- Trott, Olson 2010 -- with the X-Score atom roles, restated for a whole
// batch).  Energies only: no gradients, no pose moves.  DESIGN.md section 22 has the definition, the typing conventions and the bound.
//
// fabind_pose_score, pose_score_kernel: one wave per (complex, pose), eight waves = eight poses of ONE complex per work-group, the
//   layout of pose_protein_kernel (csrc/protein_contacts.hip): the ligand's type words staged into LDS once, every wave keeps its pose
//   and the cells of its atoms in LDS.  The protein comes from the cell list of fabind_protein_grid; edge >= cutoff puts every protein
//   atom within the cutoff in one of the 27 cells around a ligand atom.
//   A type word is a radius class (bits 0-3, PS_RADIUS) and three role bits (16 hydrophobic, 32 donor, 64 acceptor); the ligand's are
//   lig_types[atom], the protein's prot_types[prot_off[b] + atom_id] with the atom_id the grid stores (hydrogens counted).
//   Work: half a wave per ligand atom, lane k < 27 of the half walks cell k of the 27 around the atom, its atoms in stored order.  All
//   arithmetic is float64 on the float32 inputs, without contraction: r^2 = (dx dx + dy dy) + dz dz, a pair counts when r^2 < cutoff^2,
//   d = (sqrt(r^2) - R_i) - R_j, and the five terms are those of the restatement operation by operation (tests/score_refs.py).
//   Sums: a lane adds its pairs in walk order; an atom's energy is the butterfly over its 32 lanes, a pose's five sums and its pair
//   count the butterfly over the 64 lanes of what every lane gathered over its atoms.  A wave's result depends on its complex and pose
//   alone: the same bits alone, in any batch, among any S and on a repeat.  No float atomics, no inline assembly, plain vector stores.
#include "common.h"
#include "fabind_hip.h"

#pragma clang fp contract(off)

#define PS_WAVES 8
#define PS_MAX_N 256
#define PS_CLAMP 536870912.0                                           // 2^29, the clamp of the grid's cells
#define PS_HYDROPHOBIC 16
#define PS_DONOR 32
#define PS_ACCEPTOR 64
#define PS_FLAG_NONFINITE 128
#define PS_FLAG_UNCHECKED 256
#define PS_METAL 9

// radius (A) of a class: C, N, O, P, S, F, Cl, Br, I, metal; the unused classes read as metals
__constant__ double ps_radius[16] = {1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2};

__device__ __forceinline__ bool ps_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and the infinities
__device__ __forceinline__ int ps_cell(double x, double edge) {
    const double q = floor(x / edge);
    return (int)(q < -PS_CLAMP ? -PS_CLAMP : q > PS_CLAMP ? PS_CLAMP : q);
}

__global__ __launch_bounds__(PS_WAVES * 64) void pose_score_kernel(
    const float* __restrict__ poses, int n_pose, int n_atoms, const int* __restrict__ atom_off, int blocks_per_complex, int max_atoms,
    const int* __restrict__ lig_status, const int* __restrict__ lig_types, const int* __restrict__ n_torsions,
    const int* __restrict__ grid_status, const int* __restrict__ origin, const int* __restrict__ dims, const int* __restrict__ cell_off,
    const int* __restrict__ kept_off, const int* __restrict__ cell_ptr, const float* __restrict__ pxyz, const int* __restrict__ pid,
    const int* __restrict__ prot_off, const int* __restrict__ prot_types, float edge_f, float cutoff_f, const double* __restrict__ params,
    float* __restrict__ terms, float* __restrict__ inter, float* __restrict__ total, int* __restrict__ n_pairs, float* __restrict__ per_atom,
    int* __restrict__ flags) {
    extern __shared__ __align__(16) unsigned char ps_smem[];
    int* stype = (int*)ps_smem;                                        // [max_atoms]
    float* sx = (float*)(stype + max_atoms);                           // [PS_WAVES][max_atoms * 3]
    int* sc = (int*)(sx + (size_t)PS_WAVES * max_atoms * 3);           // [PS_WAVES][max_atoms * 3]: the cell of every atom of the pose
    const int b = blockIdx.x / blocks_per_complex, wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int s = (blockIdx.x % blocks_per_complex) * PS_WAVES + wave;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const size_t row = (size_t)b * n_pose + (s < n_pose ? s : 0);
    const float qnan = __uint_as_float(0x7fc00000u);
    const int c0 = cell_off[b], nc = cell_off[b + 1] - c0, k0 = kept_off[b], k1 = kept_off[b + 1];
    const int p0 = prot_off[b], np = prot_off[b + 1] - p0;
    const int ox = origin[3 * b], oy = origin[3 * b + 1], oz = origin[3 * b + 2], dx = dims[3 * b], dy = dims[3 * b + 1], dz = dims[3 * b + 2];
    // block-uniform: nothing is scored (the last tests: a grid whose box and cells disagree is never indexed)
    const bool unchecked = lig_status[b] != 0 || grid_status[b] != 0 || n > max_atoms || n < 0 || dx < 0 || dy < 0 || dz < 0 ||
                           (long long)dx * dy * dz != (long long)nc || k1 < k0 || np < 0;
    if (unchecked) {
        if (s < n_pose) {
            if (ln < 5) terms[row * 5 + ln] = qnan;
            if (ln == 0) { inter[row] = qnan; total[row] = qnan; n_pairs[row] = 0; flags[row] = PS_FLAG_UNCHECKED; }
            if (per_atom != nullptr && a0 >= 0 && n > 0 && (long long)a0 + n <= (long long)n_atoms)
                for (int i = ln; i < n; i += 64) per_atom[(size_t)s * n_atoms + a0 + i] = qnan;
        }
        return;
    }
    const double edge = (double)edge_f;
    for (int i = threadIdx.x; i < n; i += PS_WAVES * 64) stype[i] = lig_types[a0 + i];
    float* px = sx + (size_t)wave * max_atoms * 3;
    int* pc = sc + (size_t)wave * max_atoms * 3;
    bool finite = true;
    if (s < n_pose) {
        const float* src = poses + ((size_t)s * n_atoms + a0) * 3;
        for (int i = ln; i < 3 * n; i += 64) {
            const float v = src[i];
            px[i] = v;
            const bool f = ps_finite(v);
            finite &= f;
            pc[i] = f ? ps_cell((double)v, edge) : 0;
        }
    }
    __syncthreads();                                                   // the only barrier: from here on every wave is on its own
    if (s >= n_pose) return;
    float* pa_out = per_atom != nullptr ? per_atom + (size_t)s * n_atoms + a0 : nullptr;
    if (__ballot(!finite) != 0ull) {
        if (ln < 5) terms[row * 5 + ln] = qnan;
        if (ln == 0) { inter[row] = qnan; total[row] = qnan; n_pairs[row] = 0; flags[row] = PS_FLAG_NONFINITE; }
        if (pa_out != nullptr)
            for (int i = ln; i < n; i += 64) pa_out[i] = qnan;
        return;
    }
    const double w0 = params[0], w1 = params[1], w2 = params[2], w3 = params[3], w4 = params[4], tw = params[5];
    const double cut2 = (double)cutoff_f * (double)cutoff_f;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;          // this lane's share of the pose's five sums
    int cnt = 0;
    const int half = ln >> 5, k = ln & 31;
    for (int base = 0; base < n; base += 2) {                          // wave-uniform trip count: the shuffles below see every lane
        const int i = base + half;
        double ea = 0.0;                                               // this lane's share of atom i's weighted energy
        if (i < n && k < 27) {
            const int cx = pc[3 * i] + (k % 3 - 1) - ox, cy = pc[3 * i + 1] + ((k / 3) % 3 - 1) - oy, cz = pc[3 * i + 2] + (k / 9 - 1) - oz;
            if ((unsigned)cx < (unsigned)dx && (unsigned)cy < (unsigned)dy && (unsigned)cz < (unsigned)dz) {
                const int cid = c0 + (cz * dy + cy) * dx + cx;
                const int q0 = max(cell_ptr[cid], k0), q1 = min(cell_ptr[cid + 1], k1);
                const double xi = (double)px[3 * i], yi = (double)px[3 * i + 1], zi = (double)px[3 * i + 2];
                const int ti = stype[i];
                const double ri = ps_radius[ti & 15];
                for (int q = q0; q < q1; ++q) {
                    const double ex = xi - (double)pxyz[3 * (size_t)q], ey = yi - (double)pxyz[3 * (size_t)q + 1], ez = zi - (double)pxyz[3 * (size_t)q + 2];
                    const double r2 = (ex * ex + ey * ey) + ez * ez;
                    if (!(r2 < cut2)) continue;
                    const int j = pid[q];
                    const int tj = (unsigned)j < (unsigned)np ? prot_types[p0 + j] : PS_METAL;   // an id outside the complex: a metal without a role
                    const double d = (sqrt(r2) - ri) - ps_radius[tj & 15];
                    const double u1 = d / 0.5, u2 = (d - 3.0) / 2.0;
                    const double g1 = exp(-(u1 * u1)), g2 = exp(-(u2 * u2));
                    const double rep = d < 0.0 ? d * d : 0.0;
                    double hyd = 0.0, hb = 0.0;
                    if ((ti & tj & PS_HYDROPHOBIC) != 0) hyd = d < 0.5 ? 1.0 : d < 1.5 ? 1.5 - d : 0.0;
                    if (((ti & PS_DONOR) != 0 && (tj & PS_ACCEPTOR) != 0) || ((ti & PS_ACCEPTOR) != 0 && (tj & PS_DONOR) != 0))
                        hb = d < -0.7 ? 1.0 : d < 0.0 ? -d / 0.7 : 0.0;
                    t0 += g1; t1 += g2; t2 += rep; t3 += hyd; t4 += hb;
                    ea += (((w0 * g1 + w1 * g2) + w2 * rep) + w3 * hyd) + w4 * hb;
                    ++cnt;
                }
            }
        }
        if (pa_out != nullptr) {                                       // wave-uniform
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) ea += __shfl_xor(ea, o, 64);
            if (k == 0 && i < n) pa_out[i] = (float)ea;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t0 += __shfl_xor(t0, o, 64); t1 += __shfl_xor(t1, o, 64); t2 += __shfl_xor(t2, o, 64);
        t3 += __shfl_xor(t3, o, 64); t4 += __shfl_xor(t4, o, 64); cnt += __shfl_xor(cnt, o, 64);
    }
    if (ln == 0) {
        const double e = (((w0 * t0 + w1 * t1) + w2 * t2) + w3 * t3) + w4 * t4;
        const int nt = n_torsions != nullptr ? n_torsions[b] : 0;
        float* t_out = terms + row * 5;
        t_out[0] = (float)t0; t_out[1] = (float)t1; t_out[2] = (float)t2; t_out[3] = (float)t3; t_out[4] = (float)t4;
        inter[row] = (float)e;
        total[row] = (float)(e / (1.0 + tw * (double)nt));
        n_pairs[row] = cnt;
        flags[row] = 0;
    }
}

extern "C" int fabind_pose_score(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_complex, int max_atoms,
                                 const int* lig_status, const int* lig_types, const int* n_torsions, const int* grid_status,
                                 const int* origin, const int* dims, const int* cell_off, const int* kept_off, const int* cell_ptr,
                                 const float* xyz, const int* atom_id, const int* prot_off, const int* prot_types, float edge, float cutoff,
                                 const double* params, float* terms, float* inter, float* total, int* n_pairs, float* per_atom, int* flags,
                                 hipStream_t stream) {
    if (n_complex <= 0 || n_pose <= 0) return 0;
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= PS_MAX_N, "fabind_pose_score: max_atoms in [0, 256]");
    FB_REQUIRE(atom_off != nullptr && lig_status != nullptr && grid_status != nullptr && origin != nullptr && dims != nullptr &&
                   cell_off != nullptr && kept_off != nullptr && cell_ptr != nullptr && prot_off != nullptr && params != nullptr &&
                   terms != nullptr && inter != nullptr && total != nullptr && n_pairs != nullptr && flags != nullptr,
               "fabind_pose_score: atom_off, both statuses, the grid's offsets, prot_off, params and the five outputs are needed");
    FB_REQUIRE(edge > 0.0f && edge <= 3.4028234663852886e38f && cutoff >= 0.0f && cutoff <= edge,
               "fabind_pose_score: 0 <= cutoff <= edge, edge positive and finite (build the cell list with protein_grid(edge=8.0))");
    const long long per = ((long long)n_pose + PS_WAVES - 1) / PS_WAVES;
    FB_REQUIRE(per * (long long)n_complex < 2147483647ll, "fabind_pose_score: too many (complex, pose) blocks for one launch");
    const size_t lds = (size_t)max_atoms * (4 + PS_WAVES * 24);
    hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)(per * n_complex)), dim3(PS_WAVES * 64), lds, stream, poses, n_pose, n_atoms, atom_off,
                       (int)per, max_atoms, lig_status, lig_types, n_torsions, grid_status, origin, dims, cell_off, kept_off, cell_ptr, xyz,
                       atom_id, prot_off, prot_types, edge, cutoff, params, terms, inter, total, n_pairs, per_atom, flags);
    FB_CHECK_LAUNCH();
    return 0;
}
