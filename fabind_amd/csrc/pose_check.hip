// Physical validity of sampled ligand poses (no counterpart in the reference; the checks are those of PoseBusters -- Buttenschoen,
// Morris, Deane 2024 -- restated as ratios against the start conformer): bond lengths, 1-3 ("angle") distances, internal clashes,
// flatness of aromatic systems and of double bonds, stereo centres, distance to the protein's C-alpha atoms.
//
// validity_plan_kernel: one work-group of 256 threads per ligand (n <= 256 heavy atoms), thread t = atom t, integer work in LDS.
//   Adjacency rows are 256-bit sets (4 x u64).  With S1(t) = N(t) + {t}: S2(t) = union of S1(j) over j in S1(t), S3(t) = union of S1(j)
//   over j in S2(t) -- three rounds of neighbour-set unions -- give the hop class of every pair: BONDED (1) = N(t), ANGLE (2) = S2 - S1,
//   exempt (0) = S3 - S2 (1-4 pairs), the atom itself and ids >= n, CLASH (3) = everything else (h >= 4 or another component); two bits
//   per pair, 16 words per atom row.  Ratio pairs (t, j), j > t, class 1 or 2, go to a CSR list in ascending (t, j) with
//   d0 = sqrt(sum of the float64 squares of the float32 differences of the start conformer).
//   Planar groups: an aromatic system = a connected component (>= 4 atoms) of the AROMATIC-coded bonds, found by min-label propagation,
//   keyed by its lowest atom; a double-bond group = the two ends of a DOUBLE-coded bond (both C, N or O, both of degree <= 3) and all
//   their neighbours (>= 4 atoms), keyed by the bond's lower end.  Groups are listed by key atom, the aromatic group of a key before its
//   double-bond groups, those by their other end; the atoms of a group ascending.
//   Stereo centres: degree 3 or 4, no AROMATIC / DOUBLE / TRIPLE bond, no nitrogen unless of degree 4, |V0| >= min_volume with
//   V0 = det[n1 - c, n2 - c, n3 - c] (degree 3) or det[n1 - n4, n2 - n4, n3 - n4] (degree 4), neighbours ascending, float32 differences,
//   float64 determinant; dropped when an automorphism of the ligand fixes the centre and permutes its neighbours oddly.
//   Count mode (offs = NULL) writes counts [B, 4] = (pairs, groups, group atoms, centres) and status (0; 3 = more than 256 atoms; 5 = a
//   bonded or angle pair at distance 0 in the start conformer: such ligands get no entries); write mode fills the caller's slots at
//   offs [4, B + 1].  Prefix sums over the 256 threads are serial sums over an LDS vector: the plan is built once.
// pose_check_kernel: one wave per (ligand, pose), eight waves = eight poses of ONE ligand per work-group, so the class rows and radii
//   of the ligand are staged into LDS once; every wave keeps its pose in LDS as float32.  All arithmetic on coordinates is float64 on the
//   float32 inputs (DESIGN.md section 17 derives the bounds).  Lanes stride over the ratio pairs, over j for the clash loop (i is
//   wave-uniform), over groups (covariance sums in atom order, eight cyclic Jacobi sweeps on the 3 x 3 matrix), over centres and over the
//   complex's C-alpha atoms; minima and maxima go through butterflies that propagate NaN.  A wave's result depends on its ligand and
//   pose alone: the same bits alone, in any batch and among any S.  No atomics, no inline assembly, plain vector stores.
#include "common.h"
#include "fabind_hip.h"

#define VP_MAX_N 256
#define VP_W 4
#define VC_WAVES 8
#define VC_FLAG_BOND 1
#define VC_FLAG_ANGLE 2
#define VC_FLAG_CLASH 4
#define VC_FLAG_AROMATIC 8
#define VC_FLAG_DOUBLE 16
#define VC_FLAG_CHIRALITY 32
#define VC_FLAG_PROTEIN 64
#define VC_FLAG_NONFINITE 128
#define VC_FLAG_UNCHECKED 256

// Bondi van der Waals radii (A. Bondi, J. Phys. Chem. 68 (1964) 441; B and Si from Mantina et al., J. Phys. Chem. A 113 (2009) 5806)
// by atomic number 0 .. 53; every other element 2.00
__constant__ float vp_bondi[54] = {
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.92f, 1.70f, 1.55f, 1.52f, 1.47f, 2.00f, 2.00f, 2.00f, 2.00f, 2.10f, 1.80f, 1.80f, 1.75f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.90f, 1.85f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.98f};

__device__ __forceinline__ int vp_popc(const uint64_t* r) { return __popcll(r[0]) + __popcll(r[1]) + __popcll(r[2]) + __popcll(r[3]); }
__device__ __forceinline__ bool vp_bit(const uint64_t* r, int j) {
    bool v = false;
#pragma unroll
    for (int w = 0; w < VP_W; ++w)
        if (w == (j >> 6)) v = (r[w] >> (j & 63)) & 1;
    return v;
}
__device__ __forceinline__ void vp_set(uint64_t* r, int j) {
#pragma unroll
    for (int w = 0; w < VP_W; ++w)
        if (w == (j >> 6)) r[w] |= 1ull << (j & 63);
}

// exclusive prefix of v over the 256 threads (and the total), by a serial sum over an LDS vector
__device__ __forceinline__ int vp_scan(int v, int* sh, int t, int* total) {
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    int p = 0, tot = 0;
    for (int i = 0; i < VP_MAX_N; ++i) {
        const int c = sh[i];
        tot += c;
        if (i < t) p += c;
    }
    *total = tot;
    return p;
}

__device__ __forceinline__ double vp_det3(const float* a, const float* b, const float* c, const float* o) {
    const double ax = (double)(a[0] - o[0]), ay = (double)(a[1] - o[1]), az = (double)(a[2] - o[2]);
    const double bx = (double)(b[0] - o[0]), by = (double)(b[1] - o[1]), bz = (double)(b[2] - o[2]);
    const double cx = (double)(c[0] - o[0]), cy = (double)(c[1] - o[1]), cz = (double)(c[2] - o[2]);
    return ax * (by * cz - bz * cy) - ay * (bx * cz - bz * cx) + az * (bx * cy - by * cx);
}

__global__ __launch_bounds__(VP_MAX_N) void validity_plan_kernel(
    const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx, const int* __restrict__ nbr_code, const int* __restrict__ atom_off,
    int n_ligands, const int* __restrict__ z, const float* __restrict__ x0, const float* __restrict__ radii_in, float min_volume,
    const int* __restrict__ auto_flat, const int* __restrict__ auto_off, const int* __restrict__ auto_cnt, int* __restrict__ counts,
    int* __restrict__ status, const int* __restrict__ offs, uint32_t* __restrict__ cls, float* __restrict__ radii,
    int* __restrict__ pair_ij, int* __restrict__ pair_kind, double* __restrict__ pair_d0, int* __restrict__ group,
    int* __restrict__ gatoms, int* __restrict__ centre, double* __restrict__ centre_v0) {
    __shared__ uint64_t adj[VP_MAX_N][VP_W];
    __shared__ int lab[2][VP_MAX_N];
    __shared__ int sh[VP_MAX_N];
    __shared__ int bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const bool write = offs != nullptr;
    if (write)
        for (int i = t; i < n; i += VP_MAX_N) {
            const int zi = z[a0 + i];
            radii[a0 + i] = radii_in != nullptr ? radii_in[a0 + i] : (zi >= 0 && zi < 54 ? vp_bondi[zi] : 2.00f);
        }
    if (n > VP_MAX_N || (write && status[b] != 0)) {                   // block-uniform
        if (!write && t == 0) {
            status[b] = 3;
            for (int k = 0; k < 4; ++k) counts[4 * b + k] = 0;
        }
        return;
    }
    if (t == 0) bad = 0;
    uint64_t r[VP_W] = {0, 0, 0, 0}, ra[VP_W] = {0, 0, 0, 0};
    bool hasA = false, hasD = false, hasT = false;
    const bool live = t < n;
    const int q0 = live ? nbr_ptr[a0 + t] : 0, q1 = live ? nbr_ptr[a0 + t + 1] : 0;
    for (int q = q0; q < q1; ++q) {
        const int o = nbr_idx[q] - a0, c = nbr_code[q];
        if (o >= 0 && o < n && o != t) {
            vp_set(r, o);
            if (c == 1) { vp_set(ra, o); hasA = true; }
            hasD |= c == 3;
            hasT |= c == 2;
        }
    }
#pragma unroll
    for (int w = 0; w < VP_W; ++w) adj[t][w] = r[w];
    lab[0][t] = hasA ? t : (1 << 20);
    __syncthreads();
    const int deg = vp_popc(r);
    const int zt = live ? z[a0 + t] : 0;
    // ---- hop classes
    uint64_t S1[VP_W], S2[VP_W], S3[VP_W];
#pragma unroll
    for (int w = 0; w < VP_W; ++w) S1[w] = r[w];
    if (live) vp_set(S1, t);
#pragma unroll
    for (int w = 0; w < VP_W; ++w) S2[w] = S1[w];
#pragma unroll
    for (int w = 0; w < VP_W; ++w)
        for (uint64_t m = S1[w]; m; m &= m - 1) {
            const int j = (w << 6) + __ffsll((long long)m) - 1;
#pragma unroll
            for (int x = 0; x < VP_W; ++x) S2[x] |= adj[j][x];
        }
#pragma unroll
    for (int w = 0; w < VP_W; ++w) S3[w] = S2[w];
#pragma unroll
    for (int w = 0; w < VP_W; ++w)
        for (uint64_t m = S2[w]; m; m &= m - 1) {
            const int j = (w << 6) + __ffsll((long long)m) - 1;
#pragma unroll
            for (int x = 0; x < VP_W; ++x) S3[x] |= adj[j][x];
        }
    // ---- ratio pairs (t, j), j > t, bonded or angle
    uint64_t P[VP_W];
#pragma unroll
    for (int w = 0; w < VP_W; ++w) {
        const uint64_t above = w < (t >> 6) ? 0ull : w == (t >> 6) ? ~((2ull << (t & 63)) - 1ull) : ~0ull;
        P[w] = live ? (S2[w] & above) : 0ull;
    }
    const float* xb = x0 + (size_t)a0 * 3;
    const int npair = vp_popc(P);
    if (!write) {
#pragma unroll
        for (int w = 0; w < VP_W; ++w)
            for (uint64_t m = P[w]; m; m &= m - 1) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
                if (xb[3 * t] == xb[3 * j] && xb[3 * t + 1] == xb[3 * j + 1] && xb[3 * t + 2] == xb[3 * j + 2]) bad = 1;
            }
    }
    // ---- aromatic systems: min-label propagation over the AROMATIC-coded bonds
    int cur = 0;
    for (int it = 0; it < n; ++it) {
        const int l = lab[cur][t];
        int nl = l;
#pragma unroll
        for (int w = 0; w < VP_W; ++w)
            for (uint64_t m = ra[w]; m; m &= m - 1) nl = min(nl, lab[cur][(w << 6) + __ffsll((long long)m) - 1]);
        lab[cur ^ 1][t] = nl;
        cur ^= 1;
        if (!__syncthreads_or(nl != l)) break;
    }
    const int* lb = lab[cur];
    int asize = 0;
    if (live && hasA && lb[t] == t)
        for (int i = 0; i < n; ++i) asize += lb[i] == t;
    if (asize < 4) asize = 0;
    // ---- double-bond groups keyed by their lower end
    const bool cno = zt == 6 || zt == 7 || zt == 8;
    auto double_group = [&](int q, uint64_t* u) -> int {                // the atoms of the group of entry q of t's list, 0 if none
        const int k = nbr_idx[q] - a0;
        if (nbr_code[q] != 3 || k <= t || k >= n || !cno || deg > 3) return 0;
        const int zk = z[a0 + k];
        if (!(zk == 6 || zk == 7 || zk == 8)) return 0;
        uint64_t rk[VP_W];
#pragma unroll
        for (int w = 0; w < VP_W; ++w) rk[w] = adj[k][w];
        if (vp_popc(rk) > 3) return 0;
#pragma unroll
        for (int w = 0; w < VP_W; ++w) u[w] = r[w] | rk[w];
        const int c = vp_popc(u);
        return c >= 4 ? c : 0;
    };
    int ng = asize > 0 ? 1 : 0, nga = asize;
    if (hasD)
        for (int q = q0; q < q1; ++q) {
            uint64_t u[VP_W];
            const int c = double_group(q, u);
            ng += c > 0;
            nga += c;
        }
    // ---- stereo centres
    int nb[4] = {-1, -1, -1, -1};
    double v0 = 0.0;
    bool is_centre = live && (deg == 3 || deg == 4) && !hasA && !hasD && !hasT && (zt != 7 || deg == 4);
    if (is_centre) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < VP_W; ++w)
            for (uint64_t m = r[w]; m; m &= m - 1) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
                if (c == 0) nb[0] = j; else if (c == 1) nb[1] = j; else if (c == 2) nb[2] = j; else nb[3] = j;
                ++c;
            }
        const float* o = deg == 3 ? xb + 3 * t : xb + 3 * nb[3];
        v0 = vp_det3(xb + 3 * nb[0], xb + 3 * nb[1], xb + 3 * nb[2], o);
        is_centre = fabs(v0) >= (double)min_volume;
    }
    if (is_centre && auto_flat != nullptr) {
        const int cnt = auto_cnt[b];
        const int* af = auto_flat + auto_off[b];
        for (int k = 0; k < cnt && is_centre; ++k) {
            const int* a = af + (size_t)k * n;
            if (a[t] != t) continue;
            int p[4] = {0, 1, 2, 3};
            bool ok = true;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < deg) {
                    const int im = a[nb[m]];
                    int at = -1;
#pragma unroll
                    for (int x = 0; x < 4; ++x)
                        if (x < deg && nb[x] == im) at = x;
                    ok &= at >= 0;
                    p[m] = at;
                }
            if (!ok) continue;
            int inv = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int x = m + 1; x < 4; ++x) inv += p[m] > p[x];
            if (inv & 1) is_centre = false;
        }
    }
    // ---- counts, or the lists at the caller's offsets
    int tot_p, tot_g, tot_a, tot_c;
    const int pre_p = vp_scan(npair, sh, t, &tot_p);
    const int pre_g = vp_scan(ng, sh, t, &tot_g);
    const int pre_a = vp_scan(nga, sh, t, &tot_a);
    const int pre_c = vp_scan(is_centre ? 1 : 0, sh, t, &tot_c);
    if (!write) {
        if (t == 0) {
            const bool zero = bad != 0;                                  // (every store to `bad` precedes the barriers of vp_scan)
            status[b] = zero ? 5 : 0;
            counts[4 * b] = zero ? 0 : tot_p;
            counts[4 * b + 1] = zero ? 0 : tot_g;
            counts[4 * b + 2] = zero ? 0 : tot_a;
            counts[4 * b + 3] = zero ? 0 : tot_c;
        }
        return;
    }
    const int B1 = n_ligands + 1;
    const int op = offs[b], og = offs[B1 + b], oa = offs[2 * B1 + b], oc = offs[3 * B1 + b];
    // never past the caller's slots (sized from the counts of the count pass)
    if (offs[b + 1] - op != tot_p || offs[B1 + b + 1] - og != tot_g || offs[2 * B1 + b + 1] - oa != tot_a || offs[3 * B1 + b + 1] - oc != tot_c)
        return;
    if (live) {
        uint32_t* row = cls + (size_t)(a0 + t) * 16;
        for (int k = 0; k < 16; ++k) {
            uint32_t word = 0;
            for (int x = 0; x < 16; ++x) {
                const int j = 16 * k + x;
                uint32_t code = 0;
                if (j < n && j != t) code = vp_bit(r, j) ? 1u : vp_bit(S2, j) ? 2u : vp_bit(S3, j) ? 0u : 3u;
                word |= code << (2 * x);
            }
            row[k] = word;
        }
        int p = op + pre_p;
#pragma unroll
        for (int w = 0; w < VP_W; ++w)
            for (uint64_t m = P[w]; m; m &= m - 1) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
                const double dx = (double)(xb[3 * t] - xb[3 * j]), dy = (double)(xb[3 * t + 1] - xb[3 * j + 1]),
                             dz = (double)(xb[3 * t + 2] - xb[3 * j + 2]);
                pair_ij[2 * (size_t)p] = t;
                pair_ij[2 * (size_t)p + 1] = j;
                pair_kind[p] = vp_bit(r, j) ? 1 : 2;
                pair_d0[p] = sqrt(dx * dx + dy * dy + dz * dz);
                ++p;
            }
        int g = og + pre_g, ga = pre_a;                                // group atoms: positions local to the ligand's slot
        if (asize > 0) {
            group[3 * (size_t)g] = 0; group[3 * (size_t)g + 1] = ga; group[3 * (size_t)g + 2] = asize;
            for (int i = 0; i < n; ++i)
                if (lb[i] == t) gatoms[oa + ga++] = i;
            ++g;
        }
        if (hasD)
            for (int q = q0; q < q1; ++q) {
                uint64_t u[VP_W];
                const int c = double_group(q, u);
                if (c == 0) continue;
                group[3 * (size_t)g] = 1; group[3 * (size_t)g + 1] = ga; group[3 * (size_t)g + 2] = c;
#pragma unroll
                for (int w = 0; w < VP_W; ++w)
                    for (uint64_t m = u[w]; m; m &= m - 1) gatoms[oa + ga++] = (w << 6) + __ffsll((long long)m) - 1;
                ++g;
            }
        if (is_centre) {
            int* cw = centre + 5 * (size_t)(oc + pre_c);
            cw[0] = t; cw[1] = nb[0]; cw[2] = nb[1]; cw[3] = nb[2]; cw[4] = nb[3];
            centre_v0[oc + pre_c] = v0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the checks
__device__ __forceinline__ double vc_min(double a, double b) { return a != a ? a : b != b ? b : (b < a ? b : a); }   // NaN wins
__device__ __forceinline__ double vc_max(double a, double b) { return a != a ? a : b != b ? b : (b > a ? b : a); }
__device__ __forceinline__ double vc_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = vc_min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double vc_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = vc_max(v, __shfl_xor(v, o, 64));
    return v;
}

// one Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index; v.. the eigenvector columns p and q
__device__ __forceinline__ void vc_jrot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                        double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    app -= tt * apq;
    aqq += tt * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double a = v0p, bq = v0q;
    v0p = c * a - s * bq; v0q = s * a + c * bq;
    a = v1p; bq = v1q;
    v1p = c * a - s * bq; v1q = s * a + c * bq;
    a = v2p; bq = v2q;
    v2p = c * a - s * bq; v2q = s * a + c * bq;
}

__global__ __launch_bounds__(VC_WAVES * 64) void pose_check_kernel(
    const float* __restrict__ poses, int n_pose, int n_atoms, const int* __restrict__ atom_off, int n_ligands, int blocks_per_ligand,
    int max_atoms, const int* __restrict__ status, const uint32_t* __restrict__ cls, const float* __restrict__ radii,
    const int* __restrict__ offs, const int* __restrict__ pair_ij, const int* __restrict__ pair_kind, const double* __restrict__ pair_d0,
    const int* __restrict__ group, const int* __restrict__ gatoms, const int* __restrict__ centre, const double* __restrict__ centre_v0,
    const float* __restrict__ pocket, const int* __restrict__ pocket_off, float bond_lo, float bond_hi, float angle_lo, float angle_hi,
    float clash_min, float flat_max, float ca_min, int use_ca, float* __restrict__ stats, int* __restrict__ flags) {
    extern __shared__ __align__(16) unsigned char vc_smem[];
    uint32_t* scls = (uint32_t*)vc_smem;                               // [max_atoms][16]
    float* srad = (float*)(scls + (size_t)max_atoms * 16);             // [max_atoms]
    float* sx = srad + max_atoms;                                      // [VC_WAVES][max_atoms * 3]
    const int b = blockIdx.x / blocks_per_ligand, wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int s = (blockIdx.x % blocks_per_ligand) * VC_WAVES + wave;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    float* st_out = stats + ((size_t)b * n_pose + (s < n_pose ? s : 0)) * 9;
    int* fl_out = flags + (size_t)b * n_pose + (s < n_pose ? s : 0);
    const float qnan = __uint_as_float(0x7fc00000u);
    if (status[b] != 0 || n > max_atoms || n < 0) {                    // block-uniform: no check runs
        if (s < n_pose) {
            if (ln < 9) st_out[ln] = qnan;
            if (ln == 0) *fl_out = VC_FLAG_UNCHECKED;
        }
        return;
    }
    for (int i = threadIdx.x; i < n * 16; i += VC_WAVES * 64) scls[i] = cls[(size_t)a0 * 16 + i];
    for (int i = threadIdx.x; i < n; i += VC_WAVES * 64) srad[i] = radii[a0 + i];
    float* px = sx + (size_t)wave * max_atoms * 3;
    bool finite = true;
    if (s < n_pose) {
        const float* src = poses + ((size_t)s * n_atoms + a0) * 3;
        for (int i = ln; i < 3 * n; i += 64) {
            const float v = src[i];
            px[i] = v;
            finite &= fabsf(v) <= 3.4028234663852886e38f;              // false for NaN and the infinities
        }
    }
    __syncthreads();                                                   // the only barrier: from here on every wave is on its own
    if (s >= n_pose) return;
    if (__ballot(!finite) != 0ull) {
        if (ln < 9) st_out[ln] = qnan;
        if (ln == 0) *fl_out = VC_FLAG_NONFINITE;
        return;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const int B1 = n_ligands + 1;
    double blo = inf, bhi = -inf, alo = inf, ahi = -inf, clash = inf, fa = 0.0, fd = 0.0, chi = inf, ca = inf;
    // ---- bonded and angle pairs: d / d0
    for (int p = offs[b] + ln; p < offs[b + 1]; p += 64) {
        const int i = pair_ij[2 * (size_t)p], j = pair_ij[2 * (size_t)p + 1];
        if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) continue;
        const double dx = (double)px[3 * i] - (double)px[3 * j], dy = (double)px[3 * i + 1] - (double)px[3 * j + 1],
                     dz = (double)px[3 * i + 2] - (double)px[3 * j + 2];
        const double q = sqrt(dx * dx + dy * dy + dz * dz) / pair_d0[p];
        if (pair_kind[p] == 1) { blo = vc_min(blo, q); bhi = vc_max(bhi, q); }
        else { alo = vc_min(alo, q); ahi = vc_max(ahi, q); }
    }
    // ---- clash pairs i < j: d / (r_i + r_j)
    for (int i = 0; i < n; ++i) {
        const double xi = (double)px[3 * i], yi = (double)px[3 * i + 1], zi = (double)px[3 * i + 2], ri = (double)srad[i];
        for (int j = ((i + 1) & ~63) + ln; j < n; j += 64) {
            if (j <= i || ((scls[i * 16 + (j >> 4)] >> (2 * (j & 15))) & 3u) != 3u) continue;
            const double dx = xi - (double)px[3 * j], dy = yi - (double)px[3 * j + 1], dz = zi - (double)px[3 * j + 2];
            clash = vc_min(clash, sqrt(dx * dx + dy * dy + dz * dz) / (ri + (double)srad[j]));
        }
    }
    // ---- planar groups: the largest distance from the least-squares plane
    const int ga0 = offs[2 * B1 + b], ga1 = offs[2 * B1 + b + 1];
    for (int g = offs[B1 + b] + ln; g < offs[B1 + b + 1]; g += 64) {
        const int kind = group[3 * (size_t)g], start = group[3 * (size_t)g + 1], size = group[3 * (size_t)g + 2];
        if (start < 0 || size < 1 || start + size > ga1 - ga0) continue;
        const int* at = gatoms + ga0 + start;
        double cx = 0.0, cy = 0.0, cz = 0.0;
        bool ok = true;
        for (int k = 0; k < size; ++k) {
            const int i = at[k];
            if ((unsigned)i >= (unsigned)n) { ok = false; break; }
            cx += (double)px[3 * i]; cy += (double)px[3 * i + 1]; cz += (double)px[3 * i + 2];
        }
        if (!ok) continue;
        cx /= (double)size; cy /= (double)size; cz /= (double)size;
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
        for (int k = 0; k < size; ++k) {
            const int i = at[k];
            const double dx = (double)px[3 * i] - cx, dy = (double)px[3 * i + 1] - cy, dz = (double)px[3 * i + 2] - cz;
            a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
        }
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
        for (int sweep = 0; sweep < 8; ++sweep) {
            vc_jrot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            vc_jrot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            vc_jrot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        double nx = v00, ny = v10, nz = v20, ev = a00;
        if (a11 < ev) { nx = v01; ny = v11; nz = v21; ev = a11; }
        if (a22 < ev) { nx = v02; ny = v12; nz = v22; }
        double dev = 0.0;
        for (int k = 0; k < size; ++k) {
            const int i = at[k];
            dev = vc_max(dev, fabs(((double)px[3 * i] - cx) * nx + ((double)px[3 * i + 1] - cy) * ny + ((double)px[3 * i + 2] - cz) * nz));
        }
        if (kind == 0) fa = vc_max(fa, dev); else fd = vc_max(fd, dev);
    }
    // ---- stereo centres: V / V0
    for (int c = offs[3 * B1 + b] + ln; c < offs[3 * B1 + b + 1]; c += 64) {
        const int* cw = centre + 5 * (size_t)c;
        const int n1 = cw[1], n2 = cw[2], n3 = cw[3], o = cw[4] >= 0 ? cw[4] : cw[0];
        if ((unsigned)n1 >= (unsigned)n || (unsigned)n2 >= (unsigned)n || (unsigned)n3 >= (unsigned)n || (unsigned)o >= (unsigned)n) continue;
        const double ox = (double)px[3 * o], oy = (double)px[3 * o + 1], oz = (double)px[3 * o + 2];
        const double ax = (double)px[3 * n1] - ox, ay = (double)px[3 * n1 + 1] - oy, az = (double)px[3 * n1 + 2] - oz;
        const double bx = (double)px[3 * n2] - ox, by = (double)px[3 * n2 + 1] - oy, bz = (double)px[3 * n2 + 2] - oz;
        const double ex = (double)px[3 * n3] - ox, ey = (double)px[3 * n3 + 1] - oy, ez = (double)px[3 * n3 + 2] - oz;
        const double v = ax * (by * ez - bz * ey) - ay * (bx * ez - bz * ex) + az * (bx * ey - by * ex);
        chi = vc_min(chi, v / centre_v0[c]);
    }
    // ---- the complex's C-alpha atoms
    if (pocket != nullptr && n > 0) {
        double m2 = inf;
        for (int q = pocket_off[b] + ln; q < pocket_off[b + 1]; q += 64) {
            const double rx = (double)pocket[3 * (size_t)q], ry = (double)pocket[3 * (size_t)q + 1], rz = (double)pocket[3 * (size_t)q + 2];
            for (int i = 0; i < n; ++i) {
                const double dx = rx - (double)px[3 * i], dy = ry - (double)px[3 * i + 1], dz = rz - (double)px[3 * i + 2];
                m2 = vc_min(m2, dx * dx + dy * dy + dz * dz);
            }
        }
        ca = sqrt(m2);
    }
    blo = vc_wave_min(blo); bhi = vc_wave_max(bhi); alo = vc_wave_min(alo); ahi = vc_wave_max(ahi);
    clash = vc_wave_min(clash); fa = vc_wave_max(fa); fd = vc_wave_max(fd); chi = vc_wave_min(chi); ca = vc_wave_min(ca);
    if (ln == 0) {
        const float o0 = (float)blo, o1 = (float)bhi, o2 = (float)alo, o3 = (float)ahi, o4 = (float)clash, o5 = (float)fa, o6 = (float)fd,
                    o7 = (float)chi, o8 = (float)ca;
        int f = 0;
        if (o0 < bond_lo || o1 > bond_hi) f |= VC_FLAG_BOND;
        if (o2 < angle_lo || o3 > angle_hi) f |= VC_FLAG_ANGLE;
        if (o4 < clash_min) f |= VC_FLAG_CLASH;
        if (o5 > flat_max) f |= VC_FLAG_AROMATIC;
        if (o6 > flat_max) f |= VC_FLAG_DOUBLE;
        if (o7 <= 0.0f) f |= VC_FLAG_CHIRALITY;
        if (use_ca && o8 < ca_min) f |= VC_FLAG_PROTEIN;
        st_out[0] = o0; st_out[1] = o1; st_out[2] = o2; st_out[3] = o3; st_out[4] = o4; st_out[5] = o5; st_out[6] = o6; st_out[7] = o7;
        st_out[8] = o8;
        *fl_out = f;
    }
}

extern "C" int fabind_validity_plan(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* atom_off, int n_ligands,
                                    const int* z, const float* x0, const float* radii_in, float min_volume, const int* auto_flat,
                                    const int* auto_off, const int* auto_cnt, int* counts, int* status, const int* offs, unsigned* cls,
                                    float* radii, int* pair_ij, int* pair_kind, double* pair_d0, int* group, int* gatoms, int* centre,
                                    double* centre_v0, hipStream_t stream) {
    if (n_ligands <= 0) return 0;
    FB_REQUIRE(nbr_ptr != nullptr && atom_off != nullptr && status != nullptr,
               "fabind_validity_plan: nbr_ptr, atom_off and status are needed in both modes (z and x0 unless every ligand is empty)");
    FB_REQUIRE(auto_flat == nullptr || (auto_off != nullptr && auto_cnt != nullptr), "fabind_validity_plan: auto_flat needs auto_off and auto_cnt");
    FB_REQUIRE(offs != nullptr || counts != nullptr, "fabind_validity_plan: count mode needs counts");   // (lists of no entries may be NULL)
    hipLaunchKernelGGL(validity_plan_kernel, dim3(n_ligands), dim3(VP_MAX_N), 0, stream, nbr_ptr, nbr_idx, nbr_code, atom_off, n_ligands, z,
                       x0, radii_in, min_volume, auto_flat, auto_off, auto_cnt, counts, status, offs, cls, radii, pair_ij, pair_kind, pair_d0,
                       group, gatoms, centre, centre_v0);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_pose_check(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_ligands, int max_atoms,
                                 const int* status, const unsigned* cls, const float* radii, const int* offs, const int* pair_ij,
                                 const int* pair_kind, const double* pair_d0, const int* group, const int* gatoms, const int* centre,
                                 const double* centre_v0, const float* pocket, const int* pocket_off, float bond_lo, float bond_hi,
                                 float angle_lo, float angle_hi, float clash_min, float flat_max, float ca_min, int use_ca, float* stats,
                                 int* flags, hipStream_t stream) {
    if (n_ligands <= 0 || n_pose <= 0) return 0;
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= VP_MAX_N, "fabind_pose_check: max_atoms in [0, 256]");
    FB_REQUIRE(poses != nullptr && atom_off != nullptr && status != nullptr && offs != nullptr && stats != nullptr && flags != nullptr,
               "fabind_pose_check: poses, atom_off, status, offs, stats and flags are needed");
    FB_REQUIRE(pocket == nullptr || pocket_off != nullptr, "fabind_pose_check: pocket needs pocket_off");
    const long long per = ((long long)n_pose + VC_WAVES - 1) / VC_WAVES;
    FB_REQUIRE(per * (long long)n_ligands < 2147483647ll, "fabind_pose_check: too many (ligand, pose) blocks for one launch");
    const size_t lds = (size_t)max_atoms * (16 * 4 + 4 + VC_WAVES * 12);
    hipLaunchKernelGGL(pose_check_kernel, dim3((unsigned)(per * n_ligands)), dim3(VC_WAVES * 64), lds, stream, poses, n_pose, n_atoms,
                       atom_off, n_ligands, (int)per, max_atoms, status, cls, radii, offs, pair_ij, pair_kind, pair_d0, group, gatoms, centre,
                       centre_v0, pocket, pocket_off, bond_lo, bond_hi, angle_lo, angle_hi, clash_min, flat_max, ca_min, use_ca, stats, flags);
    FB_CHECK_LAUNCH();
    return 0;
}
