// Ligand poses against ALL heavy atoms of the protein (no counterpart in the reference; the two intermolecular tests of PoseBusters --
// Buttenschoen, Morris, Deane 2024 -- restated for a whole batch): the smallest ligand-protein distance as a fraction of the van der
// Waals radius sum, and the share of the ligand's volume that overlaps the protein.  DESIGN.md section 18 has the definitions and bounds.
//
// fabind_protein_grid: a cell list per complex, built once per protein and reused by every sampling round.
//   The cell of an atom along an axis is floor(double(x) / double(edge)), an IEEE division (right for negative x and for -0.0), clamped
//   to +-2^29; cells are numbered by their linear id within the complex's box, x fastest.  Atoms with Z <= 1 are dropped.
//   Count mode (cell_off = NULL), pg_count_kernel, one work-group per complex: the box (origin, dims), status (0; 6 = a non-finite
//   coordinate; 7 = a box of more than 2^20 cells: such complexes have no cells and no entries) and counts [B, 2] = (cells, kept atoms).
//   Write mode, at the caller's offsets: pg_hist_kernel (cell of every atom; the occupancy histogram by integer atomics) ->
//   fabind_exclusive_scan (cell_ptr) -> pg_scatter_kernel (atom ids into their cell's slots, in arrival order) -> pg_place_kernel (the
//   rank of an id within its cell = the number of smaller ids there: the final place).  Atomics size and fill the cells; the ORDER is
//   by (cell, original id) whatever the scheduling.
// fabind_pose_protein_check, pose_protein_kernel: one wave per (complex, pose), eight waves = eight poses of ONE complex per work-group
//   (the ligand radii staged into LDS once; every wave keeps its pose and the cells of its atoms in LDS).  All arithmetic on coordinates
//   is float64 on the float32 inputs, without contraction (the sums of squares are those of the restatement, bit for bit).
//   Pairs: lanes stride over (ligand atom, one of the 27 cells around it); edge >= cutoff puts every protein atom within the cutoff in
//   one of them.  Each lane keeps its best (ratio, ligand id, protein id) under one total order -- NaN first, then the smaller ratio,
//   then the lower ids -- and a butterfly under the same order makes the wave's.
//   Volume: atom i owns the lattice points spacing * k inside its scaled sphere that no atom j < i covers, so every ligand point is
//   counted once; lanes stride over the candidates of atom i's bounding cube.  An owned point is a protein point when a kept protein
//   atom of the cells within vdw_scale * r_max of it (never beyond the 27) covers it.
//   A wave's result depends on its complex and pose alone: the same bits alone, in any batch and among any S.  No float atomics, no
//   inline assembly, plain vector stores.
#include "common.h"
#include "fabind_hip.h"

#pragma clang fp contract(off)

#define PG_THREADS 256
#define PG_BX 32
#define PG_MAX_CELLS (1 << 20)
#define PG_CLAMP 536870912.0                                           // 2^29
#define PP_WAVES 8
#define PP_MAX_N 256
#define PP_FLAG_CLASH 1
#define PP_FLAG_OVERLAP 2
#define PP_FLAG_NONFINITE 128
#define PP_FLAG_UNCHECKED 256
#define PP_NONE 0x7fffffff

// the same table as csrc/pose_check.hip (Bondi 1964; B and Si from Mantina et al. 2009), every other element 2.00
__constant__ float pg_bondi[54] = {
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.92f, 1.70f, 1.55f, 1.52f, 1.47f, 2.00f, 2.00f, 2.00f, 2.00f, 2.10f, 1.80f, 1.80f, 1.75f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.90f, 1.85f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.98f};

__device__ __forceinline__ bool pg_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and the infinities
__device__ __forceinline__ int pg_clampi(double q) { return (int)(q < -PG_CLAMP ? -PG_CLAMP : q > PG_CLAMP ? PG_CLAMP : q); }
__device__ __forceinline__ int pg_cell(double x, double edge) { return pg_clampi(floor(x / edge)); }

__global__ __launch_bounds__(PG_THREADS) void pg_count_kernel(const float* __restrict__ xyz, const int* __restrict__ z,
                                                              const int* __restrict__ off, float edge_f, int* __restrict__ origin,
                                                              int* __restrict__ dims, int* __restrict__ status, int* __restrict__ counts) {
    __shared__ int lo[3], hi[3], kept, bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int a0 = off[b], n = off[b + 1] - a0;
    const double edge = (double)edge_f;
    if (t < 3) { lo[t] = 0x7fffffff; hi[t] = -0x7fffffff - 1; }
    if (t == 0) { kept = 0; bad = 0; }
    __syncthreads();
    int l[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, h[3] = {-0x7fffffff - 1, -0x7fffffff - 1, -0x7fffffff - 1}, cnt = 0;
    bool nonfinite = false;
    for (int i = t; i < n; i += PG_THREADS) {
        const float* p = xyz + 3 * (size_t)(a0 + i);
        const float x = p[0], y = p[1], w = p[2];
        if (!(pg_finite(x) && pg_finite(y) && pg_finite(w))) { nonfinite = true; continue; }
        if (z[a0 + i] <= 1) continue;
        const int c[3] = {pg_cell((double)x, edge), pg_cell((double)y, edge), pg_cell((double)w, edge)};
#pragma unroll
        for (int k = 0; k < 3; ++k) { l[k] = min(l[k], c[k]); h[k] = max(h[k], c[k]); }
        ++cnt;
    }
    if (nonfinite) bad = 1;
    if (cnt > 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&lo[k], l[k]); atomicMax(&hi[k], h[k]); }   // integer extrema in LDS: order-free
        atomicAdd(&kept, cnt);
    }
    __syncthreads();
    if (t == 0) {
        int st = 0, o[3] = {0, 0, 0}, d[3] = {0, 0, 0}, cells = 0, k_out = 0;
        if (bad) st = 6;
        else if (kept > 0) {
            const long long dx = (long long)hi[0] - lo[0] + 1, dy = (long long)hi[1] - lo[1] + 1, dz = (long long)hi[2] - lo[2] + 1;
            if (dx > PG_MAX_CELLS || dy > PG_MAX_CELLS || dz > PG_MAX_CELLS || dx * dy > PG_MAX_CELLS || dx * dy * dz > PG_MAX_CELLS) st = 7;
            else {
                o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2];
                d[0] = (int)dx; d[1] = (int)dy; d[2] = (int)dz;
                cells = (int)(dx * dy * dz);
                k_out = kept;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { origin[3 * b + k] = o[k]; dims[3 * b + k] = d[k]; }
        status[b] = st;
        counts[2 * b] = cells;
        counts[2 * b + 1] = k_out;
    }
}

// the cell of every atom (local linear id, -1 = not kept) and the occupancy histogram; grid (PG_BX, B)
__global__ __launch_bounds__(PG_THREADS) void pg_hist_kernel(const float* __restrict__ xyz, const int* __restrict__ z, const int* __restrict__ off,
                                                             float edge_f, const int* __restrict__ origin, const int* __restrict__ dims,
                                                             const int* __restrict__ status, const int* __restrict__ cell_off,
                                                             int* __restrict__ cell_of, int* __restrict__ cell_fill) {
    const int b = blockIdx.y;
    const int a0 = off[b], n = off[b + 1] - a0;
    const int c0 = cell_off[b], nc = cell_off[b + 1] - c0;
    const bool live = status[b] == 0;
    const double edge = (double)edge_f;
    const int ox = origin[3 * b], oy = origin[3 * b + 1], oz = origin[3 * b + 2], dx = dims[3 * b], dy = dims[3 * b + 1], dz = dims[3 * b + 2];
    for (int i = blockIdx.x * PG_THREADS + threadIdx.x; i < n; i += PG_BX * PG_THREADS) {
        int cid = -1;
        if (live && z[a0 + i] > 1) {
            const float* p = xyz + 3 * (size_t)(a0 + i);
            const int cx = pg_cell((double)p[0], edge) - ox, cy = pg_cell((double)p[1], edge) - oy, cz = pg_cell((double)p[2], edge) - oz;
            if ((unsigned)cx < (unsigned)dx && (unsigned)cy < (unsigned)dy && (unsigned)cz < (unsigned)dz) {
                const long long lin = ((long long)cz * dy + cy) * dx + cx;
                if (lin < nc) cid = (int)lin;                         // never past the caller's cells (sized by the count pass)
            }
        }
        cell_of[a0 + i] = cid;
        if (cid >= 0) atomicAdd(&cell_fill[c0 + cid], 1);
    }
}

// atom ids into the slots of their cell, in arrival order (pg_place_kernel orders them); cell_fill starts at 0 again
__global__ __launch_bounds__(PG_THREADS) void pg_scatter_kernel(const int* __restrict__ off, const int* __restrict__ cell_off,
                                                                const int* __restrict__ kept_off, const int* __restrict__ cell_of,
                                                                const int* __restrict__ cell_ptr, int* __restrict__ cell_fill,
                                                                int* __restrict__ slot) {
    const int b = blockIdx.y;
    const int a0 = off[b], n = off[b + 1] - a0, c0 = cell_off[b], k0 = kept_off[b], k1 = kept_off[b + 1];
    for (int i = blockIdx.x * PG_THREADS + threadIdx.x; i < n; i += PG_BX * PG_THREADS) {
        const int cid = cell_of[a0 + i];
        if (cid < 0) continue;
        const int q0 = cell_ptr[c0 + cid], q1 = cell_ptr[c0 + cid + 1];
        const int q = q0 + atomicAdd(&cell_fill[c0 + cid], 1);
        if (q >= k0 && q < k1 && q < q1) slot[q] = i;
    }
}

__global__ __launch_bounds__(PG_THREADS) void pg_place_kernel(const float* __restrict__ xyz, const int* __restrict__ z, const int* __restrict__ off,
                                                              const float* __restrict__ radii_in, const int* __restrict__ cell_off,
                                                              const int* __restrict__ kept_off, const int* __restrict__ cell_of,
                                                              const int* __restrict__ cell_ptr, const int* __restrict__ slot,
                                                              float* __restrict__ out_xyz, float* __restrict__ out_r, int* __restrict__ out_id) {
    const int b = blockIdx.y;
    const int a0 = off[b], n = off[b + 1] - a0, c0 = cell_off[b], k0 = kept_off[b], k1 = kept_off[b + 1];
    for (int p = k0 + blockIdx.x * PG_THREADS + threadIdx.x; p < k1; p += PG_BX * PG_THREADS) {
        const int i = slot[p];
        if ((unsigned)i >= (unsigned)n) continue;
        const int cid = cell_of[a0 + i];
        if (cid < 0) continue;
        const int q0 = max(cell_ptr[c0 + cid], k0), q1 = min(cell_ptr[c0 + cid + 1], k1);
        int rank = 0;
        for (int q = q0; q < q1; ++q) rank += slot[q] < i;
        const int dst = q0 + rank;
        if (dst >= q1) continue;
        const int zi = z[a0 + i];
        out_id[dst] = i;
        out_r[dst] = radii_in != nullptr ? radii_in[a0 + i] : (zi >= 0 && zi < 54 ? pg_bondi[zi] : 2.00f);
        out_xyz[3 * (size_t)dst] = xyz[3 * (size_t)(a0 + i)];
        out_xyz[3 * (size_t)dst + 1] = xyz[3 * (size_t)(a0 + i) + 1];
        out_xyz[3 * (size_t)dst + 2] = xyz[3 * (size_t)(a0 + i) + 2];
    }
}

// ------------------------------------------------------------------------------------------------ the check
// is (r1, i1, j1) ahead of (r2, i2, j2)?  NaN first, then the smaller ratio, then the lower ligand id, then the lower protein id
__device__ __forceinline__ bool pp_ahead(double r1, int i1, int j1, double r2, int i2, int j2) {
    const bool n1 = r1 != r1, n2 = r2 != r2;
    if (n1 != n2) return n1;
    if (!n1 && r1 != r2) return r1 < r2;
    if (i1 != i2) return i1 < i2;
    return j1 < j2;
}
__device__ __forceinline__ double pp_min(double a, double b) { return a != a ? a : b != b ? b : (b < a ? b : a); }   // NaN wins
__device__ __forceinline__ int pp_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(PP_WAVES * 64) void pose_protein_kernel(
    const float* __restrict__ poses, int n_pose, int n_atoms, const int* __restrict__ atom_off, int blocks_per_complex, int max_atoms,
    const int* __restrict__ plan_status, const float* __restrict__ lig_radii, const int* __restrict__ grid_status,
    const int* __restrict__ origin, const int* __restrict__ dims, const int* __restrict__ cell_off, const int* __restrict__ kept_off,
    const int* __restrict__ cell_ptr, const float* __restrict__ pxyz, const float* __restrict__ prad, const int* __restrict__ pid,
    float edge_f, float cutoff_f, float clash_min_f, float overlap_max, float vdw_scale_f, float spacing_f, float rmax_f,
    float* __restrict__ stats, int* __restrict__ counts, int* __restrict__ pair, int* __restrict__ flags) {
    extern __shared__ __align__(16) unsigned char pp_smem[];
    float* srad = (float*)pp_smem;                                     // [max_atoms]
    float* sx = srad + max_atoms;                                      // [PP_WAVES][max_atoms * 3]
    int* sc = (int*)(sx + (size_t)PP_WAVES * max_atoms * 3);           // [PP_WAVES][max_atoms * 3]: the cell of every atom of the pose
    const int b = blockIdx.x / blocks_per_complex, wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int s = (blockIdx.x % blocks_per_complex) * PP_WAVES + wave;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const size_t row = (size_t)b * n_pose + (s < n_pose ? s : 0);
    float* st_out = stats + row * 3;
    int* ct_out = counts + row * 3;
    int* pr_out = pair + row * 2;
    int* fl_out = flags + row;
    const float qnan = __uint_as_float(0x7fc00000u);
    const int c0 = cell_off[b], nc = cell_off[b + 1] - c0, k0 = kept_off[b], k1 = kept_off[b + 1];
    const int ox = origin[3 * b], oy = origin[3 * b + 1], oz = origin[3 * b + 2], dx = dims[3 * b], dy = dims[3 * b + 1], dz = dims[3 * b + 2];
    // block-uniform: no check runs (the last test: a grid whose box and cells disagree is never indexed)
    if (plan_status[b] != 0 || grid_status[b] != 0 || n > max_atoms || n < 0 || dx < 0 || dy < 0 || dz < 0 ||
        (long long)dx * dy * dz != (long long)nc || k1 < k0) {
        if (s < n_pose) {
            if (ln < 3) { st_out[ln] = qnan; ct_out[ln] = 0; }
            if (ln < 2) pr_out[ln] = -1;
            if (ln == 0) *fl_out = PP_FLAG_UNCHECKED;
        }
        return;
    }
    const double edge = (double)edge_f;
    for (int i = threadIdx.x; i < n; i += PP_WAVES * 64) srad[i] = lig_radii[a0 + i];
    float* px = sx + (size_t)wave * max_atoms * 3;
    int* pc = sc + (size_t)wave * max_atoms * 3;
    bool finite = true;
    if (s < n_pose) {
        const float* src = poses + ((size_t)s * n_atoms + a0) * 3;
        for (int i = ln; i < 3 * n; i += 64) {
            const float v = src[i];
            px[i] = v;
            const bool f = pg_finite(v);
            finite &= f;
            pc[i] = f ? pg_cell((double)v, edge) : 0;
        }
    }
    __syncthreads();                                                   // the only barrier: from here on every wave is on its own
    if (s >= n_pose) return;
    if (__ballot(!finite) != 0ull) {
        if (ln < 3) { st_out[ln] = qnan; ct_out[ln] = 0; }
        if (ln < 2) pr_out[ln] = -1;
        if (ln == 0) *fl_out = PP_FLAG_NONFINITE;
        return;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double cut2 = (double)cutoff_f * (double)cutoff_f, clash_min = (double)clash_min_f;
    // ---- pairs within the cutoff: lanes over (ligand atom, neighbouring cell)
    double best = inf, dmin2 = inf;
    int bi = PP_NONE, bj = PP_NONE, n_close = 0;
    for (int w = ln; w < n * 27; w += 64) {
        const int i = w / 27, k = w - 27 * i;
        const int cx = pc[3 * i] + (k % 3 - 1) - ox, cy = pc[3 * i + 1] + ((k / 3) % 3 - 1) - oy, cz = pc[3 * i + 2] + (k / 9 - 1) - oz;
        if ((unsigned)cx >= (unsigned)dx || (unsigned)cy >= (unsigned)dy || (unsigned)cz >= (unsigned)dz) continue;
        const int cid = c0 + (cz * dy + cy) * dx + cx;
        const int q0 = max(cell_ptr[cid], k0), q1 = min(cell_ptr[cid + 1], k1);
        const double xi = (double)px[3 * i], yi = (double)px[3 * i + 1], zi = (double)px[3 * i + 2], ri = (double)srad[i];
        for (int q = q0; q < q1; ++q) {
            const double ex = xi - (double)pxyz[3 * (size_t)q], ey = yi - (double)pxyz[3 * (size_t)q + 1], ez = zi - (double)pxyz[3 * (size_t)q + 2];
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (!(d2 < cut2)) continue;
            const double ratio = sqrt(d2) / (ri + (double)prad[q]);
            const int j = pid[q];
            n_close += ratio < clash_min;
            dmin2 = pp_min(dmin2, d2);
            if (pp_ahead(ratio, i, j, best, bi, bj)) { best = ratio; bi = i; bj = j; }
        }
    }
    // ---- volume lattice: atom i owns the points of its scaled sphere that no earlier atom covers
    const double sp = (double)spacing_f, scale = (double)vdw_scale_f;
    const double rpad = scale * (double)rmax_f * 1.000001 + 1e-9;      // reach of a protein sphere, padded: only narrows the 27 cells
    int n_lig = 0, n_both = 0;
    for (int i = 0; i < n; ++i) {
        const double xi = (double)px[3 * i], yi = (double)px[3 * i + 1], zi = (double)px[3 * i + 2];
        const double R = scale * (double)srad[i], R2 = R * R, Rp = R * 1.000001 + 1e-9;
        if (!(R >= 0.0)) continue;
        const int kx0 = pg_clampi(ceil((xi - Rp) / sp)), kx1 = pg_clampi(floor((xi + Rp) / sp));
        const int ky0 = pg_clampi(ceil((yi - Rp) / sp)), ky1 = pg_clampi(floor((yi + Rp) / sp));
        const int kz0 = pg_clampi(ceil((zi - Rp) / sp)), kz1 = pg_clampi(floor((zi + Rp) / sp));
        if (kx1 < kx0 || ky1 < ky0 || kz1 < kz0) continue;
        // (the host bounds vdw_scale * r / spacing by 16: at most 35 candidates per axis)
        const int nx = min(kx1 - kx0 + 1, 64), ny = min(ky1 - ky0 + 1, 64), nz = min(kz1 - kz0 + 1, 64);
        for (int c = ln; c < nx * ny * nz; c += 64) {
            const int ix = c % nx, iy = (c / nx) % ny, iz = c / (nx * ny);
            const double gx = sp * (double)(kx0 + ix), gy = sp * (double)(ky0 + iy), gz = sp * (double)(kz0 + iz);
            {
                const double ex = gx - xi, ey = gy - yi, ez = gz - zi;
                if (!(ex * ex + ey * ey + ez * ez <= R2)) continue;
            }
            bool owned = true;
            for (int j = 0; j < i && owned; ++j) {
                const double ex = gx - (double)px[3 * j], ey = gy - (double)px[3 * j + 1], ez = gz - (double)px[3 * j + 2];
                const double Rj = scale * (double)srad[j];
                owned = !(ex * ex + ey * ey + ez * ez <= Rj * Rj);
            }
            if (!owned) continue;
            ++n_lig;
            if (nc == 0) continue;
            const int gcx = pg_cell(gx, edge), gcy = pg_cell(gy, edge), gcz = pg_cell(gz, edge);
            const int x0 = max(max(pg_cell(gx - rpad, edge), gcx - 1) - ox, 0), x1 = min(min(pg_cell(gx + rpad, edge), gcx + 1) - ox, dx - 1);
            const int y0 = max(max(pg_cell(gy - rpad, edge), gcy - 1) - oy, 0), y1 = min(min(pg_cell(gy + rpad, edge), gcy + 1) - oy, dy - 1);
            const int z0 = max(max(pg_cell(gz - rpad, edge), gcz - 1) - oz, 0), z1 = min(min(pg_cell(gz + rpad, edge), gcz + 1) - oz, dz - 1);
            bool hit = false;
            for (int cz = z0; cz <= z1 && !hit; ++cz)
                for (int cy = y0; cy <= y1 && !hit; ++cy)
                    for (int cx = x0; cx <= x1 && !hit; ++cx) {
                        const int cid = c0 + (cz * dy + cy) * dx + cx;
                        const int q0 = max(cell_ptr[cid], k0), q1 = min(cell_ptr[cid + 1], k1);
                        for (int q = q0; q < q1; ++q) {
                            const double ex = gx - (double)pxyz[3 * (size_t)q], ey = gy - (double)pxyz[3 * (size_t)q + 1],
                                         ez = gz - (double)pxyz[3 * (size_t)q + 2];
                            const double Rq = scale * (double)prad[q];
                            if (ex * ex + ey * ey + ez * ez <= Rq * Rq) { hit = true; break; }
                        }
                    }
            n_both += hit;
        }
    }
    // ---- the wave's result
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double r2 = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(bi, o, 64), j2 = __shfl_xor(bj, o, 64);
        if (pp_ahead(r2, i2, j2, best, bi, bj)) { best = r2; bi = i2; bj = j2; }
        dmin2 = pp_min(dmin2, __shfl_xor(dmin2, o, 64));
    }
    n_close = pp_wave_sum(n_close);
    n_lig = pp_wave_sum(n_lig);
    n_both = pp_wave_sum(n_both);
    if (ln == 0) {
        const float o0 = (float)best, o1 = (float)sqrt(dmin2), o2 = n_lig > 0 ? (float)((double)n_both / (double)n_lig) : 0.0f;
        int f = 0;
        if (o0 < clash_min_f) f |= PP_FLAG_CLASH;
        if (o2 > overlap_max) f |= PP_FLAG_OVERLAP;
        st_out[0] = o0; st_out[1] = o1; st_out[2] = o2;
        ct_out[0] = n_close; ct_out[1] = n_lig; ct_out[2] = n_both;
        pr_out[0] = bi == PP_NONE ? -1 : bi;
        pr_out[1] = bi == PP_NONE ? -1 : bj;
        *fl_out = f;
    }
}

extern "C" int fabind_protein_grid(const float* prot_xyz, const int* prot_z, const int* prot_off, int n_complex, const float* radii_in,
                                   float edge, int* origin, int* dims, int* status, int* counts, const int* cell_off, const int* kept_off,
                                   int n_cells, int n_kept, int* cell_of, int* cell_fill, int* slot, int* cell_ptr, float* xyz, float* radii,
                                   int* atom_id, hipStream_t stream) {
    if (n_complex <= 0) return 0;
    FB_REQUIRE(edge > 0.0f && edge <= 3.4028234663852886e38f, "fabind_protein_grid: edge must be positive and finite");
    FB_REQUIRE(prot_off != nullptr && origin != nullptr && dims != nullptr && status != nullptr,
               "fabind_protein_grid: prot_off, origin, dims and status are needed in both modes (prot_xyz and prot_z unless every complex is empty)");
    if (cell_off == nullptr) {
        FB_REQUIRE(counts != nullptr, "fabind_protein_grid: count mode needs counts");
        hipLaunchKernelGGL(pg_count_kernel, dim3(n_complex), dim3(PG_THREADS), 0, stream, prot_xyz, prot_z, prot_off, edge, origin, dims, status,
                           counts);
        FB_CHECK_LAUNCH();
        return 0;
    }
    FB_REQUIRE(n_cells >= 0 && n_kept >= 0 && kept_off != nullptr && cell_ptr != nullptr && cell_of != nullptr,
               "fabind_protein_grid: write mode needs kept_off, cell_of and cell_ptr [n_cells + 1]");
    FB_REQUIRE(n_cells == 0 || cell_fill != nullptr, "fabind_protein_grid: write mode needs cell_fill [n_cells]");
    FB_REQUIRE(n_kept == 0 || (n_cells > 0 && slot != nullptr && xyz != nullptr && radii != nullptr && atom_id != nullptr),
               "fabind_protein_grid: write mode needs slot, xyz, radii and atom_id [n_kept]");
    FB_REQUIRE(n_complex <= 65535, "fabind_protein_grid: at most 65535 complexes per call");
    const dim3 grid(PG_BX, n_complex);
    if (n_cells > 0) {
        hipError_t e = hipMemsetAsync(cell_fill, 0, (size_t)n_cells * sizeof(int), stream);
        if (e != hipSuccess) { fabind_set_error(hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(pg_hist_kernel, grid, dim3(PG_THREADS), 0, stream, prot_xyz, prot_z, prot_off, edge, origin, dims, status, cell_off,
                       cell_of, cell_fill);
    FB_CHECK_LAUNCH();
    const int rc = fabind_exclusive_scan(cell_fill, cell_ptr, n_cells, stream);
    if (rc != 0) return rc;
    if (n_kept > 0) {
        hipError_t e = hipMemsetAsync(cell_fill, 0, (size_t)n_cells * sizeof(int), stream);
        if (e != hipSuccess) { fabind_set_error(hipGetErrorString(e)); return (int)e; }
        hipLaunchKernelGGL(pg_scatter_kernel, grid, dim3(PG_THREADS), 0, stream, prot_off, cell_off, kept_off, cell_of, cell_ptr, cell_fill, slot);
        FB_CHECK_LAUNCH();
        hipLaunchKernelGGL(pg_place_kernel, grid, dim3(PG_THREADS), 0, stream, prot_xyz, prot_z, prot_off, radii_in, cell_off, kept_off, cell_of,
                           cell_ptr, slot, xyz, radii, atom_id);
        FB_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int fabind_pose_protein_check(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_complex, int max_atoms,
                                         const int* plan_status, const float* lig_radii, const int* grid_status, const int* origin,
                                         const int* dims, const int* cell_off, const int* kept_off, const int* cell_ptr, const float* xyz,
                                         const float* radii, const int* atom_id, float edge, float cutoff, float clash_min, float overlap_max,
                                         float vdw_scale, float spacing, float max_radius, float* stats, int* counts, int* pair, int* flags,
                                         hipStream_t stream) {
    if (n_complex <= 0 || n_pose <= 0) return 0;
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= PP_MAX_N, "fabind_pose_protein_check: max_atoms in [0, 256]");
    FB_REQUIRE(atom_off != nullptr && plan_status != nullptr && grid_status != nullptr && origin != nullptr && dims != nullptr &&
                   cell_off != nullptr && kept_off != nullptr && cell_ptr != nullptr && stats != nullptr && counts != nullptr &&
                   pair != nullptr && flags != nullptr,
               "fabind_pose_protein_check: atom_off, both statuses, the grid's offsets and the four outputs are needed");
    FB_REQUIRE(edge > 0.0f && edge <= 3.4028234663852886e38f && cutoff >= 0.0f && cutoff <= edge,
               "fabind_pose_protein_check: 0 <= cutoff <= edge, edge positive and finite");
    FB_REQUIRE(spacing > 0.0f && vdw_scale >= 0.0f && max_radius >= 0.0f && vdw_scale * max_radius <= edge,
               "fabind_pose_protein_check: spacing > 0 and 0 <= vdw_scale * max_radius <= edge");
    const long long per = ((long long)n_pose + PP_WAVES - 1) / PP_WAVES;
    FB_REQUIRE(per * (long long)n_complex < 2147483647ll, "fabind_pose_protein_check: too many (complex, pose) blocks for one launch");
    const size_t lds = (size_t)max_atoms * (4 + PP_WAVES * 24);
    hipLaunchKernelGGL(pose_protein_kernel, dim3((unsigned)(per * n_complex)), dim3(PP_WAVES * 64), lds, stream, poses, n_pose, n_atoms,
                       atom_off, (int)per, max_atoms, plan_status, lig_radii, grid_status, origin, dims, cell_off, kept_off, cell_ptr, xyz,
                       radii, atom_id, edge, cutoff, clash_min, overlap_max, vdw_scale, spacing, max_radius, stats, counts, pair, flags);
    FB_CHECK_LAUNCH();
    return 0;
}
