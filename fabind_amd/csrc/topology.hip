// Ligand LAS ("local atomic structure") constraint pairs from the bond list (reference FABind/fabind/utils/generation_utils.py:154-187
// get_LAS_distance_constraint_mask: RDKit adjacency, n_hops_adj(adj, 2), Chem.GetSymmSSSR -- per molecule on the host).
// LAS[i][j] = 1 (i != j) iff i, j are bonded, have a common neighbour, or lie on a common RELEVANT cycle: a cycle whose edge set is no
// GF(2) sum of strictly shorter cycles (the union of all minimum cycle bases).  DESIGN.md section 14.
//
// las_count_kernel: one work-group of four waves per ligand (n <= 256), everything in LDS.
//   0. wave w takes the roots r = w, w + 4, ...: a level-synchronous BFS fills row r of the hop-distance table D (uint8 [256][256],
//      0xFF = not reached; the one true distance of 255 -- the far end of a 256-atom chain -- shares that value and is never on a
//      cycle), notes the lowest atom of r's component, and flags every candidate length seen from r (below).
//   1. spanning forest: parent(x) = lowest-index neighbour one level closer to the lowest atom of x's component.  The non-tree bonds
//      ("chords") are numbered in ascending (lo, hi) order; more than 64: status 4, no ring pairs.  The cycle-space vector of a closed
//      walk is the XOR of the chord bits of its edges: one 64-bit word.
//   2. for every flagged length L ascending, until the basis holds as many vectors as there are chords (one work-group barrier per
//      length): wave w, root r: S_r(x) = chord vector of one shortest path r -> x (parent = lowest-index neighbour one level
//      closer) for the levels <= (L - 1) / 2, then the candidates of length L,
//      one per lane and step:  odd L = 2d + 1: a bond (p, q), D[r][p] = D[r][q] = d, vector S(p) ^ S(q) ^ chord(p, q);
//      even L = 2d: an atom p at d with two neighbours q1 < q2 at d - 1, vector S(q1) ^ S(q2) ^ chord(q1, p) ^ chord(q2, p).
//      A candidate is relevant iff its vector does not reduce to 0 against the echelon basis of the lengths < L.  For a relevant one
//      the wave marks row r: every j on a shortest path from r to either end t (D[r][j] + D[j][t] == D[r][t]), and p.  Row r lives
//      in the registers of lane r / 4 of this wave, which also writes it out: no row is shared between waves.  The relevant vectors
//      still independent of each other go to a per-wave list; after the barrier wave 0 reduces the four lists into the basis in a
//      fixed order.
//   3. lane i of wave w, atom x = 4 i + w: row x = ring row | neighbours | neighbours of neighbours, bit x cleared -> row_count,
//      mask_rows; the ring pair count.  LDS: 78 KB, two work-groups per CU.
//   A ligand of more than 256 atoms (status 3) gets the bonded / common-neighbour pairs only, tested pair by pair from the global lists.
// las_write_kernel: wave per row: the set bits (or the pair-by-pair test) are compacted in ascending j into the caller's slot
//   [row_off[i], row_off[i + 1]) -- row-major, the order of dense_to_sparse -- never past it.
// Integer arithmetic only; no atomics; plain vector stores; a ligand's result does not depend on the batch around it.
#include "common.h"
#include "fabind_hip.h"

#define LAS_MAX_N 256
#define LAS_W 4
#define LAS_MAX_CHORDS 64
#define LAS_MAX_ENT 640                                                // 2 * (256 + 64): more entries mean more than 64 chords
#define LAS_WAVES 4
#define LAS_THREADS 256

__device__ __forceinline__ void las_wave_sync() {                      // LDS hand-over between the lanes of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t las_cbit(uint8_t ch) { return ch == 0xFF ? 0ull : 1ull << (ch & 63); }

__device__ __forceinline__ int las_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// i and j (local ids, i != j) bonded or with a common neighbour, from the global neighbour lists
__device__ __forceinline__ bool las_two_hop(const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx, int n_entries, int a0, int n,
                                            int i, int j) {
    const int q0 = las_clamp(nbr_ptr[a0 + i], 0, n_entries), q1 = las_clamp(nbr_ptr[a0 + i + 1], 0, n_entries);
    for (int q = q0; q < q1; ++q) {
        const int y = nbr_idx[q] - a0;
        if ((unsigned)y >= (unsigned)n || y == i) continue;
        if (y == j) return true;
        const int p0 = las_clamp(nbr_ptr[a0 + y], 0, n_entries), p1 = las_clamp(nbr_ptr[a0 + y + 1], 0, n_entries);
        for (int p = p0; p < p1; ++p)
            if (nbr_idx[p] - a0 == j) return true;
    }
    return false;
}

struct LasShared {
    uint8_t D[LAS_MAX_N * LAS_MAX_N];
    uint64_t S[LAS_WAVES][LAS_MAX_N];
    uint64_t basis[LAS_MAX_CHORDS];
    uint64_t pend[LAS_WAVES][LAS_MAX_CHORDS];
    int npend[LAS_WAVES];
    int nbasis, mu;
    int red[LAS_WAVES];
    uint16_t lptr[LAS_MAX_N + 1];
    uint16_t ccnt[LAS_MAX_N], cbase[LAS_MAX_N];
    uint8_t lidx[LAS_MAX_ENT], lch[LAS_MAX_ENT];
    uint8_t croot[LAS_MAX_N], par[LAS_MAX_N];
    uint8_t lflag[LAS_MAX_N + 1];
};

// One candidate per lane (has = this lane holds one): relevance against the basis, marks of row r, the wave's pending list.
__device__ __forceinline__ void las_process(LasShared& sh, int wv, int ln, int n, const uint8_t* Drow, int nb, int& np, bool has,
                                            uint64_t v, int t1, int t2, int apex, uint64_t (&mark)[LAS_W], uint64_t (&done)[LAS_W]) {
    for (int i = 0; i < nb; ++i) {
        const uint64_t b = sh.basis[i];
        if ((v >> (63 - __clzll((long long)b))) & 1) v ^= b;
    }
    const bool rel = has && v != 0;
    uint64_t m = __ballot(rel);
    while (m) {                                                        // wave-uniform
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int ends[2] = {__shfl(t1, l, 64), __shfl(t2, l, 64)};
        const int ap = __shfl(apex, l, 64);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int t = ends[s] & (LAS_MAX_N - 1);
            bool seen = false;
#pragma unroll
            for (int w = 0; w < LAS_W; ++w)
                if (w == (t >> 6)) { seen = (done[w] >> (t & 63)) & 1; done[w] |= 1ull << (t & 63); }
            if (seen) continue;
            const int drt = Drow[t];
            const uint8_t* Dt = sh.D + t * LAS_MAX_N;                  // D is symmetric: row t read along j
#pragma unroll
            for (int w = 0; w < LAS_W; ++w) {
                if ((w << 6) >= n) break;                              // wave-uniform: no atoms in this word
                const int j = (w << 6) + ln;
                const bool hit = j < n && (int)Drow[j] + (int)Dt[j] == drt;
                mark[w] |= __ballot(hit);
            }
        }
        if (ap >= 0) {
#pragma unroll
            for (int w = 0; w < LAS_W; ++w)
                if (w == (ap >> 6)) mark[w] |= 1ull << (ap & 63);
        }
    }
    for (int i = 0; i < np; ++i) {
        const uint64_t b = sh.pend[wv][i];
        if ((v >> (63 - __clzll((long long)b))) & 1) v ^= b;
    }
    for (;;) {
        const uint64_t mm = __ballot(rel && v != 0);
        if (!mm || np >= LAS_MAX_CHORDS) break;
        const int l = __ffsll((long long)mm) - 1;
        const uint64_t b = (uint64_t)__shfl((unsigned long long)v, l, 64);
        if (ln == 0) sh.pend[wv][np] = b;
        ++np;
        if ((v >> (63 - __clzll((long long)b))) & 1) v ^= b;
    }
    las_wave_sync();
}

__global__ __launch_bounds__(LAS_THREADS) void las_count_kernel(const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx,
                                                                const int* __restrict__ atom_off, int n_entries,
                                                                int* __restrict__ row_count, uint32_t* __restrict__ mask_rows,
                                                                int* __restrict__ ring_pairs, int* __restrict__ status) {
    __shared__ LasShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    if (n <= 0) {
        if (tid == 0) { ring_pairs[b] = 0; status[b] = 0; }
        return;
    }
    if (n > LAS_MAX_N) {                                               // (a) and (b) only, pair by pair
        for (int i = wv; i < n; i += LAS_WAVES) {
            int cnt = 0;
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int j = c0 + ln;
                const bool hit = j < n && j != i && las_two_hop(nbr_ptr, nbr_idx, n_entries, a0, n, i, j);
                cnt += __popcll(__ballot(hit));
            }
            if (ln == 0) row_count[a0 + i] = cnt;
        }
        if (tid == 0) { ring_pairs[b] = 0; status[b] = 3; }
        return;
    }
    const int e0 = las_clamp(nbr_ptr[a0], 0, n_entries), ne = las_clamp(nbr_ptr[a0 + n], e0, n_entries) - e0;
    int st = ne <= LAS_MAX_ENT ? 0 : 4;                                // more entries than fit: more than 64 chords for certain
    uint64_t ring[LAS_W] = {0, 0, 0, 0};                               // the ring row of atom 4 * ln + wv: lane i keeps the wave's i-th root
    if (st == 0) {
        for (int i = tid; i <= n; i += LAS_THREADS) sh.lptr[i] = (uint16_t)las_clamp(nbr_ptr[a0 + i] - e0, 0, ne);
        for (int e = tid; e < ne; e += LAS_THREADS) sh.lidx[e] = (uint8_t)las_clamp(nbr_idx[e0 + e] - a0, 0, n - 1);
        for (int i = tid; i <= LAS_MAX_N; i += LAS_THREADS) sh.lflag[i] = 0;
        if (tid == 0) sh.nbasis = 0;
        __syncthreads();
        // ---- 0. hop distances, component roots, candidate lengths
        for (int r = wv; r < n; r += LAS_WAVES) {
            uint8_t* Drow = sh.D + r * LAS_MAX_N;
#pragma unroll
            for (int w = 0; w < LAS_W; ++w) Drow[(w << 6) + ln] = ((w << 6) + ln) == r ? 0 : 0xFF;
            las_wave_sync();
            int lowest = r;
            for (int k = 1; k < n; ++k) {
                uint64_t any = 0;
#pragma unroll
                for (int w = 0; w < LAS_W; ++w) {
                    if ((w << 6) >= n) break;
                    const int a = (w << 6) + ln;
                    bool nw = false;
                    if (a < n && a != r && Drow[a] == 0xFF)
                        for (int e = sh.lptr[a]; e < sh.lptr[a + 1] && !nw; ++e) nw = Drow[sh.lidx[e]] == k - 1;
                    const uint64_t mk = __ballot(nw);
                    if (mk && (w << 6) + __ffsll((long long)mk) - 1 < lowest) lowest = (w << 6) + __ffsll((long long)mk) - 1;
                    any |= mk;
                    if (nw) Drow[a] = (uint8_t)k;                      // (a lane that reads this k early still sees "not k - 1")
                }
                las_wave_sync();
                if (!any) break;
            }
            if (ln == 0) sh.croot[r] = (uint8_t)lowest;
#pragma unroll
            for (int w = 0; w < LAS_W; ++w) {
                const int a = (w << 6) + ln;
                if (a >= n) continue;
                const int d = Drow[a];
                if (d < 1 || d > LAS_MAX_N / 2) continue;
                int closer = 0;
                bool odd = false;
                for (int e = sh.lptr[a]; e < sh.lptr[a + 1]; ++e) {
                    const int q = sh.lidx[e], dq = Drow[q];
                    odd |= q > a && dq == d;
                    closer += dq == d - 1;
                }
                if (odd && 2 * d + 1 <= n) sh.lflag[2 * d + 1] = 1;    // (same-value stores from several lanes and waves)
                if (closer >= 2 && d >= 2 && 2 * d <= n) sh.lflag[2 * d] = 1;
            }
        }
        __syncthreads();
        // ---- 1. spanning forest and chord numbers
        if (tid < n) {
            const int x = tid, c = sh.croot[x];
            int p = x;
            if (x != c) {
                const uint8_t* Dc = sh.D + c * LAS_MAX_N;
                const int dx = Dc[x];
                for (int e = sh.lptr[x]; e < sh.lptr[x + 1]; ++e)
                    if ((int)Dc[sh.lidx[e]] + 1 == dx) { p = sh.lidx[e]; break; }
            }
            sh.par[x] = (uint8_t)p;
        }
        __syncthreads();
        if (tid < n) {
            const int x = tid;
            int c = 0;
            for (int e = sh.lptr[x]; e < sh.lptr[x + 1]; ++e) {
                const int y = sh.lidx[e];
                c += y > x && sh.par[x] != y && sh.par[y] != x;
            }
            sh.ccnt[x] = (uint16_t)c;
        }
        __syncthreads();
        if (tid < n) {
            int s = 0;
            for (int i = 0; i < tid; ++i) s += sh.ccnt[i];
            sh.cbase[tid] = (uint16_t)s;
            if (tid == n - 1) sh.mu = s + sh.ccnt[tid];
        }
        __syncthreads();
        if (sh.mu > LAS_MAX_CHORDS) st = 4;                            // work-group-uniform
    }
    if (st == 0) {
        if (tid < n) {
            const int x = tid;
            int k = sh.cbase[x];
            for (int e = sh.lptr[x]; e < sh.lptr[x + 1]; ++e) {
                const int y = sh.lidx[e];
                int id = 0xFF;
                if (y != x && sh.par[x] != y && sh.par[y] != x) {
                    if (y > x) id = k++;
                    else {
                        id = sh.cbase[y];
                        for (int f = sh.lptr[y]; f < sh.lptr[y + 1]; ++f) {
                            const int z = sh.lidx[f];
                            if (z == x) break;
                            id += z > y && sh.par[y] != z && sh.par[z] != y;
                        }
                    }
                }
                sh.lch[e] = (uint8_t)id;
            }
        }
        __syncthreads();
        // ---- 2. relevant cycles, lengths ascending
        int nb = 0;
        for (int L = 3; L <= n; ++L) {
            if (nb >= sh.mu) break;                                    // the basis spans the cycle space: nothing longer is relevant
            if (!sh.lflag[L]) continue;                                // work-group-uniform
            const int d = L >> 1, kmax = (L - 1) >> 1;
            const bool is_odd = L & 1;
            int np = 0;
            uint64_t* S = sh.S[wv];
            for (int r = wv; r < n; r += LAS_WAVES) {
                const uint8_t* Drow = sh.D + r * LAS_MAX_N;
                if (ln == 0) S[r] = 0;
                las_wave_sync();
                for (int k = 1; k <= kmax; ++k) {
                    uint64_t any = 0;
#pragma unroll
                    for (int w = 0; w < LAS_W; ++w) {
                        if ((w << 6) >= n) break;
                        const int a = (w << 6) + ln;
                        const bool at = a < n && Drow[a] == k;
                        if (at)
                            for (int e = sh.lptr[a]; e < sh.lptr[a + 1]; ++e) {
                                const int y = sh.lidx[e];
                                if (Drow[y] == k - 1) { S[a] = S[y] ^ las_cbit(sh.lch[e]); break; }
                            }
                        any |= __ballot(at);
                    }
                    las_wave_sync();
                    if (!any) break;
                }
                uint64_t mark[LAS_W] = {0, 0, 0, 0}, done[LAS_W] = {0, 0, 0, 0};
                for (int w = 0; (w << 6) < n; ++w) {
                    const int a = (w << 6) + ln;
                    const bool act = a < n && Drow[a] == d;
                    const int eend = act ? sh.lptr[a + 1] : 0;
                    int e1 = act ? sh.lptr[a] : 0, e2 = 0;
                    if (!is_odd) {                                     // first pair of closer neighbours
                        while (e1 < eend && Drow[sh.lidx[e1]] != d - 1) ++e1;
                        e2 = e1 + 1;
                        while (e2 < eend && Drow[sh.lidx[e2]] != d - 1) ++e2;
                    }
                    for (;;) {
                        bool has = false;
                        uint64_t v = 0;
                        int t1 = 0, t2 = 0, apex = -1;
                        if (is_odd) {
                            while (e1 < eend && !(sh.lidx[e1] > a && Drow[sh.lidx[e1]] == d)) ++e1;
                            if (e1 < eend) {
                                has = true;
                                t1 = a; t2 = sh.lidx[e1];
                                v = S[t1] ^ S[t2] ^ las_cbit(sh.lch[e1]);
                                ++e1;
                            }
                        } else if (e1 < eend && e2 < eend) {
                            has = true;
                            t1 = sh.lidx[e1]; t2 = sh.lidx[e2]; apex = a;
                            v = S[t1] ^ S[t2] ^ las_cbit(sh.lch[e1]) ^ las_cbit(sh.lch[e2]);
                            ++e2;
                            while (e2 < eend && Drow[sh.lidx[e2]] != d - 1) ++e2;
                            if (e2 >= eend) {
                                ++e1;
                                while (e1 < eend && Drow[sh.lidx[e1]] != d - 1) ++e1;
                                e2 = e1 + 1;
                                while (e2 < eend && Drow[sh.lidx[e2]] != d - 1) ++e2;
                            }
                        }
                        if (!__ballot(has)) break;                     // wave-uniform
                        las_process(sh, wv, ln, n, Drow, nb, np, has, v, t1, t2, apex, mark, done);
                    }
                }
                if (ln == (r >> 2)) {
#pragma unroll
                    for (int w = 0; w < LAS_W; ++w) ring[w] |= mark[w];
                }
            }
            if (ln == 0) sh.npend[wv] = np;
            __syncthreads();
            if (wv == 0) {                                             // the four lists into the basis, in a fixed order
                for (int ww = 0; ww < LAS_WAVES; ++ww)
                    for (int i = 0; i < sh.npend[ww]; ++i) {
                        uint64_t v = sh.pend[ww][i];
                        for (int k = 0; k < nb; ++k) {
                            const uint64_t bk = sh.basis[k];
                            if ((v >> (63 - __clzll((long long)bk))) & 1) v ^= bk;
                        }
                        if (v != 0 && nb < LAS_MAX_CHORDS) {
                            if (ln == 0) sh.basis[nb] = v;
                            ++nb;
                            las_wave_sync();
                        }
                    }
                if (ln == 0) sh.nbasis = nb;
            }
            __syncthreads();
            nb = sh.nbasis;
        }
    }
    // ---- 3. rows out
    int rp = 0;
    const int x = LAS_WAVES * ln + wv;
    if (x < n) {
        uint64_t row[LAS_W] = {0, 0, 0, 0};
        if (st == 0) {
#pragma unroll
            for (int w = 0; w < LAS_W; ++w) {
                row[w] = ring[w];
                if (w == (x >> 6)) row[w] &= ~(1ull << (x & 63));
                rp += __popcll(row[w]);
            }
        }
        const int q0 = las_clamp(nbr_ptr[a0 + x], 0, n_entries), q1 = las_clamp(nbr_ptr[a0 + x + 1], 0, n_entries);
        for (int q = q0; q < q1; ++q) {
            const int y = nbr_idx[q] - a0;
            if ((unsigned)y >= (unsigned)n) continue;
#pragma unroll
            for (int w = 0; w < LAS_W; ++w)
                if (w == (y >> 6)) row[w] |= 1ull << (y & 63);
            const int p0 = las_clamp(nbr_ptr[a0 + y], 0, n_entries), p1 = las_clamp(nbr_ptr[a0 + y + 1], 0, n_entries);
            for (int p = p0; p < p1; ++p) {
                const int z = nbr_idx[p] - a0;
                if ((unsigned)z >= (unsigned)n) continue;
#pragma unroll
                for (int w = 0; w < LAS_W; ++w)
                    if (w == (z >> 6)) row[w] |= 1ull << (z & 63);
            }
        }
        int cnt = 0;
        uint32_t* mr = mask_rows + (size_t)(a0 + x) * 8;
#pragma unroll
        for (int w = 0; w < LAS_W; ++w) {
            if (w == (x >> 6)) row[w] &= ~(1ull << (x & 63));
            cnt += __popcll(row[w]);
            mr[2 * w] = (uint32_t)row[w];
            mr[2 * w + 1] = (uint32_t)(row[w] >> 32);
        }
        row_count[a0 + x] = cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rp += __shfl_xor(rp, o, 64);
    if (ln == 0) sh.red[wv] = rp;
    __syncthreads();
    if (tid == 0) {
        ring_pairs[b] = (sh.red[0] + sh.red[1] + sh.red[2] + sh.red[3]) >> 1;
        status[b] = st;
    }
}

__global__ __launch_bounds__(LAS_THREADS) void las_write_kernel(const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx,
                                                                const int* __restrict__ atom_off, int n_entries,
                                                                const uint32_t* __restrict__ mask_rows, const int* __restrict__ row_off,
                                                                long n_pairs, long long* __restrict__ edge_index) {
    const int b = blockIdx.x, wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const uint64_t below = (1ull << ln) - 1;
    for (int i = wv; i < n; i += LAS_WAVES) {
        long pos = row_off[a0 + i];
        const long hi = row_off[a0 + i + 1];
        const long lim = hi < n_pairs ? hi : n_pairs;                  // never past the caller's slot (sized from the counts)
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int j = c0 + ln;
            uint64_t m;
            if (n <= LAS_MAX_N) {
                const uint32_t* mr = mask_rows + (size_t)(a0 + i) * 8 + (c0 >> 5);
                m = (uint64_t)mr[0] | ((uint64_t)mr[1] << 32);
            } else {
                m = __ballot(j < n && j != i && las_two_hop(nbr_ptr, nbr_idx, n_entries, a0, n, i, j));
            }
            const long p = pos + __popcll(m & below);
            if (((m >> ln) & 1) && j < n && p >= 0 && p < lim) {
                edge_index[p] = a0 + i;
                edge_index[n_pairs + p] = a0 + j;
            }
            pos += __popcll(m);
        }
    }
}

extern "C" int fabind_las_pairs(const int* nbr_ptr, const int* nbr_idx, const int* atom_off, int n_ligands, int n_entries,
                                int* row_count, unsigned* mask_rows, int* ring_pairs, int* status, const int* row_off, long n_pairs,
                                long long* edge_index, hipStream_t stream) {
    if (n_ligands <= 0) return 0;
    FB_REQUIRE(n_entries >= 0 && n_pairs >= 0, "fabind_las_pairs: n_entries >= 0 and n_pairs >= 0");
    FB_REQUIRE(nbr_ptr != nullptr && atom_off != nullptr && mask_rows != nullptr && (n_entries == 0 || nbr_idx != nullptr),
               "fabind_las_pairs: nbr_ptr, nbr_idx, atom_off and mask_rows are needed in both modes");
    if (edge_index == nullptr) {                                       // count mode
        FB_REQUIRE(row_count != nullptr && ring_pairs != nullptr && status != nullptr,
                   "fabind_las_pairs: count mode needs row_count, ring_pairs and status");
        hipLaunchKernelGGL(las_count_kernel, dim3(n_ligands), dim3(LAS_THREADS), 0, stream, nbr_ptr, nbr_idx, atom_off, n_entries,
                           row_count, mask_rows, ring_pairs, status);
        FB_CHECK_LAUNCH();
        return 0;
    }
    FB_REQUIRE(row_off != nullptr, "fabind_las_pairs: write mode needs row_off and edge_index");
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(las_write_kernel, dim3(n_ligands), dim3(LAS_THREADS), 0, stream, nbr_ptr, nbr_idx, atom_off, n_entries, mask_rows,
                       row_off, n_pairs, edge_index);
    FB_CHECK_LAUNCH();
    return 0;
}
