// Start conformers from the bond list by distance geometry (the reference calls RDKit: AllChem.EmbedMolecule(mol, ETKDGv2()) +
// MMFFOptimizeMolecule, utils/inference_mol_utils.py:135-144; the steps here are those of Blaney & Dixon, Rev. Comput. Chem. 5 (1994) 299,
// and Havel, "Distance Geometry: Theory, Algorithms, and Chemical Applications" (1998): bounds from topology, triangle smoothing, random
// metric embedding, minimisation of a violation function).  No torsion preferences and no force field: DESIGN.md section 20.
//
// embed_bounds_kernel: one work-group of 256 threads per ligand (n <= 256 heavy atoms), thread t = atom t.  Adjacency rows are 256-bit
//   sets in LDS; four rounds of neighbour-set unions give the pairs one to four bonds apart, min-label propagation the fragments.
//   Thread t writes the bounds of its pairs (t, j), j > t, into the ligand's n x n block: upper at (t, j), lower at (j, t), diagonal 0.
//   The rules are float64 arithmetic on tabulated constants (the sines and cosines of the class angles are table entries; only + - * /
//   and sqrt are evaluated, contraction off), every value rounded once to float32.  Triangle smoothing in float32, k ascending, uppers
//   then lowers, each to its fixed point: the block stays in global memory (256 KiB at n = 256: L2-resident), row k is staged in LDS for each k; pair (i, j) is
//   always updated by the same thread of a 16 x 16 tiling.  The signed-volume terms (quads) go to a list sized by a count pass.
// embed_conformers_kernel: one work-group of 256 threads per (ligand, conformer), thread t = atom t; every try and every minimisation
//   step inside the one launch.  Random distances from the counter hash of csrc/conformer.hip keyed (seed, key, conformer, try, pair);
//   the metric matrix is never stored (its entries are recomputed from the draws); four eigenpairs by power iteration with deflation in
//   float64; Polak-Ribiere+ conjugate gradients with a backtracking line search on E, one evaluation of E and its exact gradient per
//   step.  Coordinates are float32 (the trial point in LDS), all arithmetic on them float64.  Sums over atoms are serial sums over an
//   LDS vector in atom order, computed by every thread alike: every decision is uniform, and a result depends on the ligand, its key,
//   the conformer id and the seed alone.  No atomics, no inline assembly, plain vector stores.
#pragma clang fp contract(off)
#include "common.h"
#include "fabind_hip.h"

#define EB_MAX_N 256
#define EB_W 4
#define EB_TETRA 0
#define EB_TRIGONAL 1
#define EB_LINEAR 2
#define EB_LS_MAX 10
#define EB_SMOOTH_PASSES 16

// Bondi van der Waals radii, the table of csrc/pose_check.hip, by atomic number 0 .. 53; every other element 2.00
__constant__ float eb_bondi[54] = {
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.92f, 1.70f, 1.55f, 1.52f, 1.47f, 2.00f, 2.00f, 2.00f, 2.00f, 2.10f, 1.80f, 1.80f, 1.75f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.90f, 1.85f,
    2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 2.00f, 1.98f};
// (cos, sin) of 109.47 / 120 / 180 degrees (TETRA, TRIGONAL, LINEAR) and of 60 / 90 / 108 degrees (3-, 4-, 5-ring)
__constant__ double eb_cos[6] = {-0.3333333333333333, -0.5, -1.0, 0.5, 0.0, -0.30901699437494745};
__constant__ double eb_sin[6] = {0.9428090415820634, 0.8660254037844386, 0.0, 0.8660254037844386, 1.0, 0.9510565162951535};

__device__ __forceinline__ double eb_covalent(int z) {
    switch (z) {
        case 5: return 0.85; case 6: return 0.75; case 7: return 0.71; case 8: return 0.63; case 9: return 0.64; case 14: return 1.16;
        case 15: return 1.11; case 16: return 1.03; case 17: return 0.99; case 34: return 1.16; case 35: return 1.14; case 53: return 1.33;
        default: return 1.20;
    }
}
__device__ __forceinline__ double eb_code_shift(int code) { return code == 1 ? -0.11 : code == 2 ? -0.30 : code == 3 ? -0.16 : 0.0; }

__device__ __forceinline__ int eb_popc(const uint64_t* r) { return __popcll(r[0]) + __popcll(r[1]) + __popcll(r[2]) + __popcll(r[3]); }
__device__ __forceinline__ bool eb_bit(const uint64_t* r, int j) { return (r[j >> 6] >> (j & 63)) & 1; }
// (masks instead of an indexed word: a register array indexed by a variable would be placed in scratch memory)
__device__ __forceinline__ void eb_set(uint64_t* r, int j) {
    const uint64_t bit = 1ull << (j & 63);
    const int w = j >> 6;
    r[0] |= bit & (0ull - (uint64_t)(w == 0)); r[1] |= bit & (0ull - (uint64_t)(w == 1));
    r[2] |= bit & (0ull - (uint64_t)(w == 2)); r[3] |= bit & (0ull - (uint64_t)(w == 3));
}
__device__ __forceinline__ bool eb_regbit(const uint64_t* r, int j) {
    const uint64_t bit = 1ull << (j & 63);
    const int w = j >> 6;
    return ((r[0] & bit & (0ull - (uint64_t)(w == 0))) | (r[1] & bit & (0ull - (uint64_t)(w == 1))) |
            (r[2] & bit & (0ull - (uint64_t)(w == 2))) | (r[3] & bit & (0ull - (uint64_t)(w == 3)))) != 0ull;
}

// exclusive prefix of v over the 256 threads (and the total), by a serial sum over an LDS vector
__device__ __forceinline__ int eb_scan(int v, int* sh, int t, int* total) {
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    int p = 0, tot = 0;
    for (int i = 0; i < EB_MAX_N; ++i) {
        const int c = sh[i];
        tot += c;
        if (i < t) p += c;
    }
    *total = tot;
    return p;
}

struct EbTopo {                                                       // the ligand's graph as the rules read it
    const uint64_t (*adj)[EB_W];
    const int* geom;
    const int* z;
    const int* nbr_ptr;
    const int* nbr_idx;
    const int* nbr_code;
    int a0;
};

__device__ __forceinline__ int eb_code_of(const EbTopo& g, int a, int b) {
    for (int q = g.nbr_ptr[g.a0 + a]; q < g.nbr_ptr[g.a0 + a + 1]; ++q)
        if (g.nbr_idx[q] - g.a0 == b) return g.nbr_code[q];
    return 5;
}
// the 1-2 distance: r(z_i) + r(z_j) + c(code), a SINGLE bond between two TRIGONAL atoms 0.05 shorter
__device__ __forceinline__ double eb_d0(const EbTopo& g, int i, int j) {
    const int code = eb_code_of(g, i, j);
    double d = (eb_covalent(g.z[i]) + eb_covalent(g.z[j])) + eb_code_shift(code);
    if (code == 4 && g.geom[i] == EB_TRIGONAL && g.geom[j] == EB_TRIGONAL) d = d - 0.05;
    return d;
}
// the angle class of i-a-k: the ring angle when the three lie on a 3-, 4- or 5-ring, else the class of a
__device__ __forceinline__ int eb_angle(const EbTopo& g, int a, int i, int k) {
    if (eb_bit(g.adj[i], k)) return 3;
    bool r4 = false, r5 = false;
#pragma unroll
    for (int w = 0; w < EB_W; ++w) {
        uint64_t m = g.adj[i][w] & g.adj[k][w];
        if (w == (a >> 6)) m &= ~(1ull << (a & 63));
        r4 |= m != 0;
    }
    if (r4) return 4;
    for (int w = 0; w < EB_W; ++w)
        for (uint64_t m = g.adj[i][w]; m; m &= m - 1) {
            const int x = (w << 6) + __ffsll((long long)m) - 1;
            if (x == a || x == k) continue;
#pragma unroll
            for (int v = 0; v < EB_W; ++v) {
                uint64_t c = g.adj[x][v] & g.adj[k][v];
                if (v == (a >> 6)) c &= ~(1ull << (a & 63));
                if (v == (i >> 6)) c &= ~(1ull << (i & 63));
                r5 |= c != 0;
            }
        }
    return r5 ? 5 : g.geom[a];
}

__global__ __launch_bounds__(EB_MAX_N) void embed_bounds_kernel(
    const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx, const int* __restrict__ nbr_code, const int* __restrict__ atom_off,
    int n_ligands, const int* __restrict__ z, const int* __restrict__ chiral_sign, float v_flat, float v_min, float v_max,
    int* __restrict__ counts, int* __restrict__ status, const int* __restrict__ quad_off, const long long* __restrict__ mat_off,
    float* bounds, int* __restrict__ geom_out, int* __restrict__ quads, float* __restrict__ quad_lo,
    float* __restrict__ quad_hi) {
    __shared__ uint64_t adj[EB_MAX_N][EB_W];
    __shared__ int lab[2][EB_MAX_N];
    __shared__ int sh[EB_MAX_N];
    __shared__ int sgeom[EB_MAX_N], smulti[EB_MAX_N], sz[EB_MAX_N];
    __shared__ float uk[EB_MAX_N], lk[EB_MAX_N];
    __shared__ int bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const bool write = quad_off != nullptr;
    if (n > EB_MAX_N || n < 0 || (write && status[b] != 0)) {          // block-uniform
        if (!write && t == 0) {
            status[b] = 3;
            counts[b] = 0;
        }
        return;
    }
    if (t == 0) bad = 0;
    const bool live = t < n;
    uint64_t r[EB_W] = {0, 0, 0, 0};
    bool hasA = false, hasD = false, hasT = false;
    int nD = 0;
    const int q0 = live ? nbr_ptr[a0 + t] : 0, q1 = live ? nbr_ptr[a0 + t + 1] : 0;
    for (int q = q0; q < q1; ++q) {
        const int o = nbr_idx[q] - a0, c = nbr_code[q];
        if (o >= 0 && o < n && o != t && !eb_regbit(r, o)) {
            eb_set(r, o);
            hasA |= c == 1;
            hasT |= c == 2;
            if (c == 3) { hasD = true; ++nD; }
        }
    }
#pragma unroll
    for (int w = 0; w < EB_W; ++w) adj[t][w] = r[w];
    const int zt = live ? z[a0 + t] : 0;
    const bool multi = hasA || hasD || hasT;
    sz[t] = zt;
    smulti[t] = multi ? 1 : 0;
    lab[0][t] = t;
    __syncthreads();
    const int deg = eb_popc(r);
    // ---- geometry class
    int gc = EB_TETRA;
    if (deg >= 4) gc = EB_TETRA;
    else if (deg <= 2 && (hasT || nD >= 2)) gc = EB_LINEAR;
    else if (multi) gc = EB_TRIGONAL;
    else if (zt == 7 || zt == 8) {
        bool conj = false;
#pragma unroll
        for (int w = 0; w < EB_W; ++w)
            for (uint64_t m = r[w]; m; m &= m - 1) conj |= smulti[(w << 6) + __ffsll((long long)m) - 1] != 0;
        if (conj) gc = EB_TRIGONAL;
    }
    sgeom[t] = gc;
    // ---- the signed-volume terms of atom t, counted (emit = false) or written at position p
    EbTopo g = {adj, sgeom, sz, nbr_ptr, nbr_idx, nbr_code, a0};
    const int cs = (live && chiral_sign != nullptr) ? chiral_sign[a0 + t] : 0;
    const bool stereo = live && (deg == 3 || deg == 4) && !multi && (zt != 7 || deg == 4) && (cs == 1 || cs == -1);
    auto quad_terms = [&](bool emit, int p) -> int {
        int cnt = 0;
        int nb[4] = {-1, -1, -1, -1};
        if (deg == 3 || deg == 4) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < EB_W; ++w)
                for (uint64_t m = r[w]; m; m &= m - 1) {
                    const int j = (w << 6) + __ffsll((long long)m) - 1;
                    if (c == 0) nb[0] = j; else if (c == 1) nb[1] = j; else if (c == 2) nb[2] = j; else nb[3] = j;
                    ++c;
                }
        }
        if (live && gc == EB_TRIGONAL && deg == 3) {
            if (emit) {
                int* qw = quads + 4 * (size_t)(p + cnt);
                qw[0] = t; qw[1] = nb[0]; qw[2] = nb[1]; qw[3] = nb[2];
                quad_lo[p + cnt] = -v_flat; quad_hi[p + cnt] = v_flat;
            }
            ++cnt;
        }
        if (live && (hasA || hasD))
            for (int q = q0; q < q1; ++q) {
                const int o = nbr_idx[q] - a0, c = nbr_code[q];
                if (o <= t || o >= n || (c != 1 && c != 3)) continue;
                if (q > q0 && nbr_idx[q - 1] == nbr_idx[q]) continue;      // (a repeated entry of a sorted list)
                for (int wi = 0; wi < EB_W; ++wi)
                    for (uint64_t mi = adj[t][wi]; mi; mi &= mi - 1) {
                        const int i = (wi << 6) + __ffsll((long long)mi) - 1;
                        if (i == o) continue;
                        for (int wj = 0; wj < EB_W; ++wj)
                            for (uint64_t mj = adj[o][wj]; mj; mj &= mj - 1) {
                                const int j = (wj << 6) + __ffsll((long long)mj) - 1;
                                if (j == t || j == i) continue;
                                if (emit) {
                                    int* qw = quads + 4 * (size_t)(p + cnt);
                                    qw[0] = i; qw[1] = t; qw[2] = o; qw[3] = j;
                                    quad_lo[p + cnt] = -v_flat; quad_hi[p + cnt] = v_flat;
                                }
                                ++cnt;
                            }
                    }
            }
        if (stereo) {
            if (emit) {
                int* qw = quads + 4 * (size_t)(p + cnt);
                qw[0] = deg == 3 ? t : nb[3]; qw[1] = nb[0]; qw[2] = nb[1]; qw[3] = nb[2];
                quad_lo[p + cnt] = cs > 0 ? v_min : -v_max; quad_hi[p + cnt] = cs > 0 ? v_max : -v_min;
            }
            ++cnt;
        }
        return cnt;
    };
    __syncthreads();                                                   // sgeom is complete
    const int nq = quad_terms(false, 0);
    int tot_q;
    const int pre_q = eb_scan(nq, sh, t, &tot_q);
    if (!write) {
        if (t == 0) {
            status[b] = 0;
            counts[b] = tot_q;
        }
        return;
    }
    const int oq = quad_off[b];
    if (quad_off[b + 1] - oq != tot_q) return;                         // never past the caller's slots (sized by the count pass)
    if (live) geom_out[a0 + t] = gc;
    quad_terms(true, oq + pre_q);
    if (n == 0) return;
    // ---- pairs one to four bonds apart, fragments
    uint64_t S1[EB_W], S2[EB_W], S3[EB_W], S4[EB_W];
#pragma unroll
    for (int w = 0; w < EB_W; ++w) S1[w] = r[w];
    if (live) eb_set(S1, t);
    auto grow = [&](const uint64_t* from, uint64_t* to) {
#pragma unroll
        for (int w = 0; w < EB_W; ++w) to[w] = from[w];
#pragma unroll
        for (int w = 0; w < EB_W; ++w)
            for (uint64_t m = from[w]; m; m &= m - 1) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
#pragma unroll
                for (int x = 0; x < EB_W; ++x) to[x] |= adj[j][x];
            }
    };
    grow(S1, S2);
    grow(S2, S3);
    grow(S3, S4);
    int cur = 0;
    for (int it = 0; it < n; ++it) {
        const int l = lab[cur][t];
        int nl = l;
#pragma unroll
        for (int w = 0; w < EB_W; ++w)
            for (uint64_t m = r[w]; m; m &= m - 1) nl = min(nl, lab[cur][(w << 6) + __ffsll((long long)m) - 1]);
        lab[cur ^ 1][t] = nl;
        cur ^= 1;
        if (!__syncthreads_or(nl != l)) break;
    }
    const int* frag = lab[cur];
    // ---- the bounds of the pairs (t, j), j > t
    float* M = bounds + mat_off[b];
    if (live) {
        M[(size_t)t * n + t] = 0.f;
        const double rt = (double)(zt >= 0 && zt < 54 ? eb_bondi[zt] : 2.00f);
        for (int j = t + 1; j < n; ++j) {
            double lo, up;
            if (eb_regbit(r, j)) {
                const double d = eb_d0(g, t, j);
                lo = d - 0.01; up = d + 0.01;
            } else if (eb_regbit(S2, j)) {
                lo = 1e300; up = -1e300;
                for (int w = 0; w < EB_W; ++w)
                    for (uint64_t m = adj[t][w] & adj[j][w]; m; m &= m - 1) {
                        const int a = (w << 6) + __ffsll((long long)m) - 1;
                        const double x = eb_d0(g, a, t), y = eb_d0(g, a, j);
                        const double c = eb_cos[eb_angle(g, a, t, j)];
                        const double d = sqrt((x * x + y * y) - ((2.0 * x) * y) * c);
                        lo = fmin(lo, d - 0.04); up = fmax(up, d + 0.04);
                    }
            } else if (eb_regbit(S3, j)) {
                lo = 1e300; up = -1e300;
                for (int wa = 0; wa < EB_W; ++wa)
                    for (uint64_t ma = adj[t][wa]; ma; ma &= ma - 1) {
                        const int a = (wa << 6) + __ffsll((long long)ma) - 1;
                        for (int wb = 0; wb < EB_W; ++wb)
                            for (uint64_t mb = adj[j][wb] & adj[a][wb]; mb; mb &= mb - 1) {
                                const int bb = (wb << 6) + __ffsll((long long)mb) - 1;
                                const double d1 = eb_d0(g, t, a), d2 = eb_d0(g, a, bb), d3 = eb_d0(g, bb, j);
                                const int k1 = eb_angle(g, a, t, bb), k2 = eb_angle(g, bb, a, j);
                                const double c1 = eb_cos[k1], s1 = eb_sin[k1], c2 = eb_cos[k2], s2 = eb_sin[k2];
                                const double xx = d2 - (d3 * c2 + d1 * c1);
                                const double ys = d3 * s2, yi = d1 * s1;
                                const double cis = sqrt(xx * xx + (ys - yi) * (ys - yi));
                                const double trans = sqrt(xx * xx + (ys + yi) * (ys + yi));
                                bool flat = false;                      // a planar six-ring: both centres TRIGONAL, a path t-x-y-j avoiding a, bb
                                if (sgeom[a] == EB_TRIGONAL && sgeom[bb] == EB_TRIGONAL)
                                    for (int wx = 0; wx < EB_W; ++wx)
                                        for (uint64_t mx = adj[t][wx]; mx; mx &= mx - 1) {
                                            const int x = (wx << 6) + __ffsll((long long)mx) - 1;
                                            if (x == a || x == bb) continue;
#pragma unroll
                                            for (int v = 0; v < EB_W; ++v) {
                                                uint64_t c = adj[x][v] & adj[j][v];
                                                if (v == (a >> 6)) c &= ~(1ull << (a & 63));
                                                if (v == (bb >> 6)) c &= ~(1ull << (bb & 63));
                                                flat |= c != 0;
                                            }
                                        }
                                lo = fmin(lo, cis - 0.06); up = fmax(up, (flat ? cis : trans) + 0.06);
                            }
                    }
            } else {
                const int zj = sz[j];
                const double rs = rt + (double)(zj >= 0 && zj < 54 ? eb_bondi[zj] : 2.00f);
                lo = eb_regbit(S4, j) ? rs * 0.8 : rs;
                up = frag[j] == frag[t] ? 1000.0 : 10.0;
            }
            M[(size_t)t * n + j] = (float)up;
            M[(size_t)j * n + t] = (float)lo;
        }
    }
    // ---- triangle smoothing in float32: passes over k ascending, uppers then lowers, each repeated until a whole pass changes
    //      nothing (a later k can lower a sum that an earlier k has used by a rounding; at the fixed point the triangle inequalities hold
    //      in float32 exactly); pair (i, j) belongs to thread (i % 16, j % 16) throughout
    const int ti = t >> 4, tj = t & 15;
    for (int pass = 0; pass < 2; ++pass)
        for (int rep = 0; rep < EB_SMOOTH_PASSES; ++rep) {
            bool changed = false;
            for (int k = 0; k < n; ++k) {
                __threadfence_block();
                __syncthreads();
                if (live) {
                    uk[t] = t == k ? 0.f : M[(size_t)min(t, k) * n + max(t, k)];
                    lk[t] = t == k ? 0.f : M[(size_t)max(t, k) * n + min(t, k)];
                }
                __syncthreads();
                for (int i0 = 0; i0 < n; i0 += 16) {
                    const int i = i0 + ti;
                    if (i >= n || i == k) continue;
                    for (int j0 = i0; j0 < n; j0 += 16) {
                        const int j = j0 + tj;
                        if (j <= i || j >= n || j == k) continue;
                        if (pass == 0) {
                            const size_t idx = (size_t)i * n + j;
                            const float s = uk[i] + uk[j];
                            if (s < M[idx]) { M[idx] = s; changed = true; }
                        } else {
                            const size_t idx = (size_t)j * n + i;
                            const float s = fmaxf(lk[i] - uk[j], lk[j] - uk[i]);
                            if (s > M[idx]) { M[idx] = s; changed = true; }
                        }
                    }
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    __threadfence_block();
    __syncthreads();
    bool mine = false;
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int i = i0 + ti;
        if (i >= n) continue;
        for (int j0 = i0; j0 < n; j0 += 16) {
            const int j = j0 + tj;
            if (j <= i || j >= n) continue;
            mine |= M[(size_t)j * n + i] > M[(size_t)i * n + j];
        }
    }
    if (mine) bad = 1;
    __syncthreads();
    if (t == 0 && bad) status[b] = 6;
}

// ------------------------------------------------------------------------------------------------ the embedding
__device__ __forceinline__ uint32_t eb_chain(uint32_t seed, uint32_t key, uint32_t conf, uint32_t tr) {
    uint32_t h = fb_hash32(seed + 0x9e3779b9u);
    h = fb_hash32((h ^ key) + 0x85ebca6bu);
    h = fb_hash32((h ^ conf) + 0xc2b2ae35u);
    return fb_hash32((h ^ tr) + 0x165667b1u);
}
__device__ __forceinline__ double eb_u01(uint32_t h4, uint32_t draw) {
    return (double)(fb_hash32((h4 ^ draw) + 0x27d4eb2fu) >> 8) * (1.0 / 16777216.0);
}

#define EB_NRED 6
// the sums (kinds 0) or maxima (kind 1) of v[0 .. cnt) over the atoms, in atom order, the same bits in every thread
template <int CNT, unsigned MAX_MASK>
__device__ __forceinline__ void eb_reduce(double (*red)[EB_MAX_N], int t, int n, double* v) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CNT; ++k) red[k][t] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
        double s = 0.0;
        if ((MAX_MASK >> k) & 1u) {
            for (int i = 0; i < n; ++i) s = fmax(s, red[k][i]);
        } else {
            for (int i = 0; i < n; ++i) s += red[k][i];
        }
        v[k] = s;
    }
}

__global__ __launch_bounds__(EB_MAX_N) void embed_conformers_kernel(
    const float* __restrict__ bounds, const long long* __restrict__ mat_off, const int* __restrict__ atom_off, int n_ligands, int n_atoms,
    int n_confs, const int* __restrict__ plan_status, const int* __restrict__ quad_off, const int* __restrict__ quads,
    const float* __restrict__ quad_lo, const float* __restrict__ quad_hi, const uint32_t* __restrict__ keys, uint32_t seed, int max_tries,
    int max_steps, int power_iters, float viol_tol_f, float v_tol_f, float w_v_f, float w4_f, float* __restrict__ coords,
    int* __restrict__ status, int* __restrict__ tries, int* __restrict__ steps_out, double* __restrict__ viol_out,
    double* __restrict__ energy_out, double* __restrict__ trace) {
    __shared__ float X[EB_MAX_N][4];
    __shared__ double red[EB_NRED][EB_MAX_N];
    __shared__ double vec[4][EB_MAX_N];
    __shared__ double vcur[EB_MAX_N];
    __shared__ double d0s[EB_MAX_N];
    const int b = blockIdx.x / n_confs, c = blockIdx.x % n_confs, t = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const size_t slot = (size_t)b * n_confs + c;
    const int st = plan_status[b];
    float* out = coords + ((size_t)c * n_atoms + a0) * 3;
    double* tr_out = trace != nullptr ? trace + slot * ((size_t)max_steps + 1) : nullptr;
    if (st != 0 || n <= 0 || n > EB_MAX_N) {                           // block-uniform: nothing to embed
        for (int i = t; i < 3 * max(n, 0); i += EB_MAX_N) out[i] = 0.f;
        if (t == 0) {
            status[slot] = st != 0 ? st : (n > EB_MAX_N ? 3 : 0);
            tries[slot] = 0; steps_out[slot] = 0; viol_out[slot] = 0.0; energy_out[slot] = 0.0;
        }
        return;
    }
    const bool live = t < n;
    const float* M = bounds + mat_off[b];
    const double viol_tol = (double)viol_tol_f, v_tol = (double)v_tol_f, w_v = (double)w_v_f, w4 = (double)w4_f;
    const uint32_t key = keys[b], un = (uint32_t)n;
    const int qa = quad_off[b], qb = quad_off[b + 1];
    const double dn = (double)n;

    // E_t (the pairs (t, j), j > t, the quads whose first atom is t, the fourth coordinate of t), dE/dx_t, the largest violation of
    // the three-dimensional distance of a pair (t, j), j > t, and the largest excess of a volume whose first atom is t, at the point X
    auto evaluate = [&](double* gr, double& Et, double& vt, double& vxt) {
        gr[0] = gr[1] = gr[2] = gr[3] = 0.0;
        Et = 0.0; vt = 0.0; vxt = 0.0;
        if (!live) return;
        const double x0 = (double)X[t][0], x1 = (double)X[t][1], x2 = (double)X[t][2], x3 = (double)X[t][3];
        for (int j = 0; j < n; ++j) {
            if (j == t) continue;
            const double e0 = x0 - (double)X[j][0], e1 = x1 - (double)X[j][1], e2 = x2 - (double)X[j][2], e3 = x3 - (double)X[j][3];
            const double d23 = e0 * e0 + e1 * e1 + e2 * e2;
            const double d2 = d23 + e3 * e3;
            const int lo_i = min(t, j), hi_i = max(t, j);
            const double u = (double)M[(size_t)lo_i * n + hi_i], l = (double)M[(size_t)hi_i * n + lo_i];
            const double u2 = u * u, l2 = l * l;
            double coef = 0.0, e = 0.0;
            if (d2 > u2) {
                const double a = d2 / u2 - 1.0;
                e = a * a;
                coef = 2.0 * a / u2;
            } else if (d2 < l2) {
                const double den = l2 + d2;
                const double q = 2.0 * l2 / den - 1.0;
                e = q * q;
                coef = 2.0 * q * (-2.0 * l2 / (den * den));
            }
            gr[0] += 2.0 * coef * e0; gr[1] += 2.0 * coef * e1; gr[2] += 2.0 * coef * e2; gr[3] += 2.0 * coef * e3;
            if (j > t) {
                Et += e;
                const double d3 = sqrt(d23);
                vt = fmax(vt, fmax(d3 - u, l - d3));
            }
        }
        for (int q = qa; q < qb; ++q) {
            const int p0 = quads[4 * (size_t)q], p1 = quads[4 * (size_t)q + 1], p2 = quads[4 * (size_t)q + 2], p3 = quads[4 * (size_t)q + 3];
            if (t != p0 && t != p1 && t != p2 && t != p3) continue;
            if ((unsigned)p0 >= un || (unsigned)p1 >= un || (unsigned)p2 >= un || (unsigned)p3 >= un) continue;
            const double ox = (double)X[p0][0], oy = (double)X[p0][1], oz = (double)X[p0][2];
            const double ax = (double)X[p1][0] - ox, ay = (double)X[p1][1] - oy, az = (double)X[p1][2] - oz;
            const double bx = (double)X[p2][0] - ox, by = (double)X[p2][1] - oy, bz = (double)X[p2][2] - oz;
            const double cx = (double)X[p3][0] - ox, cy = (double)X[p3][1] - oy, cz = (double)X[p3][2] - oz;
            const double bcx = by * cz - bz * cy, bcy = bz * cx - bx * cz, bcz = bx * cy - by * cx;
            const double V = ax * bcx + ay * bcy + az * bcz;
            const double lo = (double)quad_lo[q], hi = (double)quad_hi[q];
            const double rr = V - fmin(fmax(V, lo), hi);
            if (t == p0) {
                Et += w_v * rr * rr;
                vxt = fmax(vxt, fabs(rr));
            }
            if (rr == 0.0) continue;
            const double k = 2.0 * w_v * rr;
            const double cax = cy * az - cz * ay, cay = cz * ax - cx * az, caz = cx * ay - cy * ax;
            const double abx = ay * bz - az * by, aby = az * bx - ax * bz, abz = ax * by - ay * bx;
            if (t == p1) { gr[0] += k * bcx; gr[1] += k * bcy; gr[2] += k * bcz; }
            if (t == p2) { gr[0] += k * cax; gr[1] += k * cay; gr[2] += k * caz; }
            if (t == p3) { gr[0] += k * abx; gr[1] += k * aby; gr[2] += k * abz; }
            if (t == p0) { gr[0] -= k * (bcx + cax + abx); gr[1] -= k * (bcy + cay + aby); gr[2] -= k * (bcz + caz + abz); }
        }
        gr[3] += 2.0 * w4 * x3;
        Et += w4 * x3 * x3;
    };

    double best_viol = 0.0, best_E = 0.0;
    int best_steps = 0;
    bool have_best = false, done = false;
    int t_used = 0;
    for (int tr = 0; tr < max_tries && !done; ++tr) {
        const uint32_t h4 = eb_chain(seed, key, (uint32_t)c, (uint32_t)tr);
        auto dist2 = [&](int i, int j) -> double {                    // the squared random distance of the pair i != j
            const int lo_i = min(i, j), hi_i = max(i, j);
            const double u = (double)M[(size_t)lo_i * n + hi_i], l = (double)M[(size_t)hi_i * n + lo_i];
            const double d = l + eb_u01(h4, (uint32_t)(lo_i * n + hi_i)) * (u - l);
            return d * d;
        };
        // ---- d_i0^2 = mean_j d_ij^2 - (1 / n^2) sum_{j<k} d_jk^2
        double v[EB_NRED];
        double rs = 0.0, up = 0.0;
        if (live)
            for (int j = 0; j < n; ++j) {
                if (j == t) continue;
                const double q = dist2(t, j);
                rs += q;
                if (j > t) up += q;
            }
        v[0] = up;
        eb_reduce<1, 0u>(red, t, n, v);
        d0s[t] = live ? rs / dn - v[0] / (dn * dn) : 0.0;
        // ---- four eigenpairs of g_ij = (d_i0^2 + d_j0^2 - d_ij^2) / 2 by power iteration with deflation
        double lam[4] = {0.0, 0.0, 0.0, 0.0};
        double xc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double vi = live ? 2.0 * eb_u01(h4, (uint32_t)(n * n + a * n + t)) - 1.0 : 0.0;
            v[0] = vi * vi;
            eb_reduce<1, 0u>(red, t, n, v);
            double nrm = sqrt(v[0]);
            if (nrm > 0.0) vi = vi / nrm;
            double la = 0.0;
            for (int it = 0; it < power_iters; ++it) {
                __syncthreads();
                vcur[t] = vi;
                __syncthreads();
                double y = 0.0, dp[4] = {0.0, 0.0, 0.0, 0.0};
                if (live) {
                    const double dt0 = d0s[t];
                    for (int j = 0; j < n; ++j) {
                        const double gij = j == t ? dt0 : (dt0 + d0s[j] - dist2(t, j)) / 2.0;
                        y += gij * vcur[j];
                    }
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (p < a) {
                        for (int j = 0; j < n; ++j) dp[p] += vec[p][j] * vcur[j];
                        if (live) y = y - (lam[p] * dp[p]) * vec[p][t];
                    }
                v[0] = vi * y;
                v[1] = y * y;
                eb_reduce<2, 0u>(red, t, n, v);
                la = v[0];
                nrm = sqrt(v[1]);
                if (!(nrm > 0.0)) break;
                vi = y / nrm;
            }
            __syncthreads();
            vec[a][t] = live ? vi : 0.0;
            lam[a] = la;
            if (live) xc[a] = la > 0.0 ? sqrt(la) * vi : 2.0 * eb_u01(h4, (uint32_t)(n * n + (4 + a) * n + t)) - 1.0;
            __syncthreads();
        }
        float xf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { xf[k] = (float)xc[k]; X[t][k] = xf[k]; }
        __syncthreads();
        // ---- Polak-Ribiere+ conjugate gradients, a backtracking line search with quadratic interpolation, one evaluation per step
        double g[4], d[4], gn[4], Et, vt, vxt;
        evaluate(g, Et, vt, vxt);
        v[0] = Et; v[1] = vt; v[2] = vxt; v[3] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
        eb_reduce<4, 6u>(red, t, n, v);
        double E = v[0], viol = v[1], vex = v[2], gg = v[3];
        double gd = -gg;
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = -g[k];
        double alpha = 1.0 / fmax(1.0, sqrt(gg));
        int steps = 0, fails = 0, trial = 0;
        bool ok = false;
        if (tr_out != nullptr && t == 0) tr_out[0] = E;
        while (true) {
            ok = viol <= viol_tol && vex <= v_tol;
            if (ok || steps >= max_steps) break;
            if (!(gd < 0.0)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = -g[k];
                gd = -gg;
                if (gd == 0.0) break;
            }
            __syncthreads();                                           // every read of X by the last evaluation is over
#pragma unroll
            for (int k = 0; k < 4; ++k) X[t][k] = (float)((double)xf[k] + alpha * d[k]);
            __syncthreads();
            evaluate(gn, Et, vt, vxt);
            v[0] = Et; v[1] = vt; v[2] = vxt;
            v[3] = gn[0] * gn[0] + gn[1] * gn[1] + gn[2] * gn[2] + gn[3] * gn[3];
            v[4] = gn[0] * g[0] + gn[1] * g[1] + gn[2] * g[2] + gn[3] * g[3];
            v[5] = gn[0] * d[0] + gn[1] * d[1] + gn[2] * d[2] + gn[3] * d[3];
            eb_reduce<6, 6u>(red, t, n, v);
            ++steps;
            const double En = v[0];
            if (En <= E + 1e-4 * alpha * gd) {
                const double beta = fmax(0.0, (v[3] - v[4]) / gg);
                gd = -v[3] + beta * v[5];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    d[k] = -gn[k] + beta * d[k];
                    g[k] = gn[k];
                    xf[k] = X[t][k];
                }
                E = En; viol = v[1]; vex = v[2]; gg = v[3];
                if (trial == 0) alpha = alpha * 2.0;
                fails = 0; trial = 0;
            } else {
                const double den = 2.0 * (En - E - gd * alpha);
                const double an = den > 0.0 ? -gd * alpha * alpha / den : 0.5 * alpha;
                alpha = fmin(fmax(an, 0.1 * alpha), 0.5 * alpha);
                ++trial;
                if (trial >= EB_LS_MAX) {
                    if (fails) {
                        if (tr_out != nullptr && t == 0) tr_out[steps] = E;
                        break;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) d[k] = -g[k];
                    gd = -gg; fails = 1; trial = 0;
                }
            }
            if (tr_out != nullptr && t == 0) tr_out[steps] = E;
        }
        t_used = tr + 1;
        if (tr_out != nullptr) {                                       // (the trace is that of the last try made)
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            for (int i = steps + 1 + t; i <= max_steps; i += EB_MAX_N) tr_out[i] = qnan;
        }
        // ---- the try's result: the first three coordinates centred on the centroid and rounded to float32; E, the violations and
        //      the acceptance are those of the ROUNDED coordinates (the fourth coordinate dropped), so what is reported is what is returned
        v[0] = live ? (double)xf[0] : 0.0; v[1] = live ? (double)xf[1] : 0.0; v[2] = live ? (double)xf[2] : 0.0;
        eb_reduce<3, 0u>(red, t, n, v);
        const float c0 = live ? (float)((double)xf[0] - v[0] / dn) : 0.f, c1 = live ? (float)((double)xf[1] - v[1] / dn) : 0.f,
                    c2 = live ? (float)((double)xf[2] - v[2] / dn) : 0.f;
        __syncthreads();
        X[t][0] = c0; X[t][1] = c1; X[t][2] = c2; X[t][3] = 0.f;
        __syncthreads();
        evaluate(gn, Et, vt, vxt);
        v[0] = Et; v[1] = vt; v[2] = vxt;
        eb_reduce<3, 6u>(red, t, n, v);
        ok = v[1] <= viol_tol && v[2] <= v_tol;
        if (ok || !have_best || v[1] < best_viol) {
            if (live) { out[3 * t] = c0; out[3 * t + 1] = c1; out[3 * t + 2] = c2; }
            best_viol = v[1]; best_E = v[0]; best_steps = steps; have_best = true;
        }
        done = ok;
        __syncthreads();
    }
    if (t == 0) {
        status[slot] = done ? 0 : 1;
        tries[slot] = t_used; steps_out[slot] = best_steps; viol_out[slot] = best_viol; energy_out[slot] = best_E;
    }
}

extern "C" int fabind_embed_bounds(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* atom_off, int n_ligands,
                                   const int* z, const int* chiral_sign, float v_flat, float v_min, float v_max, int* counts, int* status,
                                   const int* quad_off, const long long* mat_off, float* bounds, int* geom, int* quads, float* quad_lo,
                                   float* quad_hi, hipStream_t stream) {
    if (n_ligands <= 0) return 0;
    FB_REQUIRE(nbr_ptr != nullptr && atom_off != nullptr && status != nullptr,
               "fabind_embed_bounds: nbr_ptr, atom_off and status are needed in both modes (z unless every ligand is empty)");
    FB_REQUIRE(quad_off != nullptr || counts != nullptr, "fabind_embed_bounds: count mode needs counts");
    FB_REQUIRE(quad_off == nullptr || mat_off != nullptr, "fabind_embed_bounds: write mode needs mat_off");
    FB_REQUIRE(v_flat >= 0.f && v_min >= 0.f && v_min <= v_max, "fabind_embed_bounds: v_flat >= 0 and 0 <= v_min <= v_max");
    hipLaunchKernelGGL(embed_bounds_kernel, dim3(n_ligands), dim3(EB_MAX_N), 0, stream, nbr_ptr, nbr_idx, nbr_code, atom_off, n_ligands, z,
                       chiral_sign, v_flat, v_min, v_max, counts, status, quad_off, mat_off, bounds, geom, quads, quad_lo, quad_hi);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_embed_conformers(const float* bounds, const long long* mat_off, const int* atom_off, int n_ligands, int n_atoms,
                                       int n_confs, const int* plan_status, const int* quad_off, const int* quads, const float* quad_lo,
                                       const float* quad_hi, const unsigned* keys, unsigned seed, int max_tries, int max_steps,
                                       int power_iters, float viol_tol, float v_tol, float w_v, float w4, float* coords, int* status,
                                       int* tries, int* steps, double* viol, double* energy, double* trace, hipStream_t stream) {
    if (n_ligands <= 0 || n_confs <= 0) return 0;
    FB_REQUIRE(mat_off != nullptr && atom_off != nullptr && plan_status != nullptr && quad_off != nullptr && keys != nullptr,
               "fabind_embed_conformers: mat_off, atom_off, plan_status, quad_off and keys are needed");
    FB_REQUIRE(status != nullptr && tries != nullptr && steps != nullptr && viol != nullptr && energy != nullptr,
               "fabind_embed_conformers: status, tries, steps, viol and energy are needed");
    FB_REQUIRE(n_atoms >= 0 && (n_atoms == 0 || coords != nullptr), "fabind_embed_conformers: coords is needed");
    FB_REQUIRE(max_tries >= 1 && max_tries <= 1024 && max_steps >= 0 && max_steps <= 1000000 && power_iters >= 1 && power_iters <= 100000,
               "fabind_embed_conformers: max_tries in [1, 1024], max_steps in [0, 1e6], power_iters in [1, 1e5]");
    FB_REQUIRE(viol_tol >= 0.f && v_tol >= 0.f && w_v >= 0.f && w4 >= 0.f, "fabind_embed_conformers: tolerances and weights >= 0");
    FB_REQUIRE((long long)n_ligands * (long long)n_confs < 2147483647ll, "fabind_embed_conformers: too many (ligand, conformer) blocks");
    hipLaunchKernelGGL(embed_conformers_kernel, dim3((unsigned)(n_ligands * n_confs)), dim3(EB_MAX_N), 0, stream, bounds, mat_off, atom_off,
                       n_ligands, n_atoms, n_confs, plan_status, quad_off, quads, quad_lo, quad_hi, keys, seed, max_tries, max_steps,
                       power_iters, viol_tol, v_tol, w_v, w4, coords, status, tries, steps, viol, energy, trace);
    FB_CHECK_LAUNCH();
    return 0;
}
