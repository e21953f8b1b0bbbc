// Ligand symmetry: label-preserving graph automorphisms and the symmetry-corrected RMSD / Smooth-L1 minimum over them
// (reference FABind_plus/fabind/utils/isomorphism.py:23-72 -- graph-tool subgraph_isomorphism(G, G, vertex_label, subgraph=False),
// run offline per molecule by tools/inject_isomorphism_to_data.py; utils/get_sym_rmsd.py:5-18 -- spyrmsd symmrmsd, per complex
// on the host under training.py:273-286; utils/permutation_loss.py:4-33 -- the per-ligand argmin of the permutation loss).
//
// sym_search_kernel: one wave per ligand (n <= 256 atoms).  The graph lives in LDS as adjacency bitsets (4 x u64 per row).
//   1. Colour refinement (1-WL) seeded by the labels: colour' = h(colour, sum_{j in N(i)} h(colour_j)) until the number of classes
//      stops growing.  The neighbour hash is commutative; a collision can only merge classes (weaker pruning, same result: every
//      candidate is checked exactly against the labels and the already-mapped atoms below).
//   2. Search order: the lowest-index unvisited atom adjacent to a visited one, else the lowest-index unvisited atom (a new
//      component).  For a ligand numbered so that every atom has a lower-index neighbour this is index order.
//   3. Depth-first search with an explicit stack in LDS (cand[d] = untried images of the atom at depth d).  An image v of atom u
//      is a candidate iff label and colour match, v is unused, v is adjacent to the image of every mapped neighbour of u, and
//      v has exactly as many mapped-image neighbours as u has mapped neighbours (so non-edges to mapped atoms are preserved too).
//      Every leaf is an automorphism; candidates are tried in ascending order.
//   The identity is always the first entry of a ligand's output (it is never lost to truncation); the search skips it when it
//   meets it.  Every candidate taken counts as one step; at `max_steps` the search stops with status 2.  At the (cap+1)-th
//   automorphism it stops with status 1 (count mode reports cap + 1, write mode keeps cap).  n > 256: status 3, identity only.
// sym_sort_kernel: write mode only -- the automorphisms of a ligand from search order into ascending lexicographic order
//   (rank = number of lexicographically smaller entries; entries are distinct).
// sym_score_kernel: one work-group per (ligand, pose); both coordinate sets staged in LDS; one wave per automorphism (k = wave,
//   wave + 4, ...), each lane a fixed strided set of atoms, a butterfly wave sum: every score is computed in a fixed order and
//   the minimum keeps the FIRST k that reaches it.  No float atomics: results are bit-reproducible.
#include "common.h"
#include "fabind_hip.h"
#include <limits.h>

#define SYM_MAX_N 256
#define SYM_W 4                                   // u64 words per adjacency row
#define SYM_SCORE_THREADS 256

__device__ __forceinline__ int sym_popc(const uint64_t* a, const uint64_t* b, int W) {
    int c = 0;
    for (int w = 0; w < W; ++w) c += __popcll(a[w] & b[w]);
    return c;
}

__device__ __forceinline__ int sym_count_classes(const uint32_t* col, int n) {
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        bool first = true;
        for (int j = 0; j < i && first; ++j) first = col[j] != col[i];
        c += first;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}

__global__ __launch_bounds__(64) void sym_search_kernel(const int* __restrict__ labels, const int* __restrict__ nbr_ptr,
                                                        const int* __restrict__ nbr_idx, const int* __restrict__ atom_off,
                                                        int cap, int max_steps, const int* __restrict__ flat_off,
                                                        int* __restrict__ out, int* __restrict__ count, int* __restrict__ status) {
    __shared__ uint64_t adj[SYM_MAX_N][SYM_W];
    __shared__ uint64_t cand[SYM_MAX_N][SYM_W];
    __shared__ uint32_t col[SYM_MAX_N], col2[SYM_MAX_N];
    __shared__ int lab[SYM_MAX_N], ord[SYM_MAX_N], img[SYM_MAX_N], amap[SYM_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    const bool write = out != nullptr;
    const int base = write ? flat_off[b] : 0, lim = write ? flat_off[b + 1] : 0;
    if (write && base + n <= lim)                 // the identity is entry 0 of every ligand
        for (int i = tid; i < n; i += 64) out[base + i] = i;
    if (n > SYM_MAX_N || n <= 0) {
        if (tid == 0) { count[b] = 1; status[b] = n > SYM_MAX_N ? 3 : 0; }
        return;
    }
    const int W = (n + 63) >> 6;
    for (int i = tid; i < n; i += 64) {
        uint64_t row[SYM_W] = {0, 0, 0, 0};
        for (int e = nbr_ptr[a0 + i]; e < nbr_ptr[a0 + i + 1]; ++e) {
            const int j = nbr_idx[e] - a0;
            if (j >= 0 && j < n && j != i) row[j >> 6] |= 1ull << (j & 63);
        }
#pragma unroll
        for (int w = 0; w < SYM_W; ++w) adj[i][w] = row[w];
        lab[i] = labels[a0 + i];
        col[i] = fb_hash32((uint32_t)labels[a0 + i] ^ 0x5bd1e995u);
    }
    __syncthreads();
    // 1. colour refinement: at most n rounds (each round that does not stop adds a class)
    int nc = sym_count_classes(col, n);
    for (int r = 0; r < n; ++r) {
        for (int i = tid; i < n; i += 64) {
            uint32_t s = 0;
            for (int w = 0; w < W; ++w)
                for (uint64_t m = adj[i][w]; m; m &= m - 1) s += fb_hash32(col[(w << 6) + __ffsll((long long)m) - 1] + 0x632be5abu);
            col2[i] = fb_hash32(col[i] * 0x9e3779b1u ^ fb_hash32(s));
        }
        __syncthreads();
        const int nc2 = sym_count_classes(col2, n);
        for (int i = tid; i < n; i += 64) col[i] = col2[i];
        __syncthreads();
        if (nc2 <= nc) break;
        nc = nc2;
    }
    if (tid != 0) return;
    // 2. search order
    uint64_t vis[SYM_W] = {0, 0, 0, 0}, fr[SYM_W] = {0, 0, 0, 0}, valid[SYM_W];
    for (int w = 0; w < SYM_W; ++w) {
        const int hi = n - (w << 6);
        valid[w] = hi >= 64 ? ~0ull : (hi <= 0 ? 0ull : ((1ull << hi) - 1));
    }
    for (int d = 0; d < n; ++d) {
        int u = -1;
        for (int w = 0; w < W && u < 0; ++w)
            if (fr[w]) u = (w << 6) + __ffsll((long long)fr[w]) - 1;
        for (int w = 0; w < W && u < 0; ++w) {
            const uint64_t m = valid[w] & ~vis[w];
            if (m) u = (w << 6) + __ffsll((long long)m) - 1;
        }
        ord[d] = u;
        img[d] = -1;
        vis[u >> 6] |= 1ull << (u & 63);
        for (int w = 0; w < W; ++w) fr[w] = (fr[w] | adj[u][w]) & ~vis[w];
    }
    // 3. depth-first search
    uint64_t used[SYM_W] = {0, 0, 0, 0}, mapped[SYM_W] = {0, 0, 0, 0};
    int d = 0, found = 1, st = 0;
    long long steps = 0;
    auto fill = [&](int dd) {
        const int u = ord[dd];
        uint64_t c[SYM_W];
        for (int w = 0; w < W; ++w) c[w] = valid[w] & ~used[w];
        int need = 0;
        for (int w = 0; w < W; ++w)
            for (uint64_t m = adj[u][w] & mapped[w]; m; m &= m - 1) {
                const int v = amap[(w << 6) + __ffsll((long long)m) - 1];
                for (int x = 0; x < W; ++x) c[x] &= adj[v][x];
                ++need;
            }
        for (int w = 0; w < W; ++w) {
            for (uint64_t m = c[w]; m; m &= m - 1) {
                const int v = (w << 6) + __ffsll((long long)m) - 1;
                if (lab[v] != lab[u] || col[v] != col[u] || sym_popc(adj[v], used, W) != need) c[w] &= ~(1ull << (v & 63));
            }
            cand[dd][w] = c[w];
        }
    };
    fill(0);
    while (true) {
        const int u = ord[d];
        if (img[d] >= 0) {                        // undo the previous choice at this depth
            const int v = img[d];
            used[v >> 6] &= ~(1ull << (v & 63));
            mapped[u >> 6] &= ~(1ull << (u & 63));
            img[d] = -1;
        }
        int v = -1;
        for (int w = 0; w < W && v < 0; ++w)
            if (cand[d][w]) v = (w << 6) + __ffsll((long long)cand[d][w]) - 1;
        if (v < 0) {
            if (d == 0) break;
            --d;
            continue;
        }
        if (steps >= (long long)max_steps) { st = 2; break; }
        ++steps;
        cand[d][v >> 6] &= ~(1ull << (v & 63));
        img[d] = v;
        amap[u] = v;
        used[v >> 6] |= 1ull << (v & 63);
        mapped[u >> 6] |= 1ull << (u & 63);
        if (d + 1 < n) {
            fill(++d);
            continue;
        }
        bool ident = true;                        // a leaf: amap is an automorphism
        for (int i = 0; i < n && ident; ++i) ident = amap[i] == i;
        if (ident) continue;
        if (found >= cap) { st = 1; if (!write) found = cap + 1; break; }
        if (write) {
            const int o = base + found * n;
            if (o + n > lim) { st = 1; break; }   // never past the caller's slot (sized from count mode)
            for (int i = 0; i < n; ++i) out[o + i] = amap[i];
        }
        ++found;
    }
    count[b] = found;
    status[b] = st;
}

__global__ __launch_bounds__(256) void sym_sort_kernel(const int* __restrict__ src, int* __restrict__ dst, const int* __restrict__ flat_off,
                                                       const int* __restrict__ count, const int* __restrict__ atom_off) {
    const int b = blockIdx.x;
    const int n = atom_off[b + 1] - atom_off[b], base = flat_off[b];
    const int K = min(count[b], n > 0 ? (flat_off[b + 1] - base) / n : 0);
    for (int k = threadIdx.x; k < K; k += 256) {
        const int* a = src + base + (size_t)k * n;
        int rank = 0;
        for (int q = 0; q < K; ++q) {
            const int* c = src + base + (size_t)q * n;
            int i = 0;
            while (i < n && c[i] == a[i]) ++i;
            rank += i < n && c[i] < a[i];
        }
        int* o = dst + base + (size_t)rank * n;
        for (int i = 0; i < n; ++i) o[i] = a[i];
    }
}

__device__ __forceinline__ float sym_sl1(float x) {
    const float a = fabsf(x);
    return a < 1.f ? 0.5f * x * x : a - 0.5f;
}

__global__ __launch_bounds__(SYM_SCORE_THREADS) void sym_score_kernel(const float* __restrict__ pred, int n_atoms, const float* __restrict__ ref,
                                                                      const int* __restrict__ atom_off, const int* __restrict__ flat_off,
                                                                      const int* __restrict__ auto_cnt, const int* __restrict__ flat,
                                                                      int n_lig, float* __restrict__ min_rmsd, int* __restrict__ arg_rmsd,
                                                                      float* __restrict__ min_sl1, int* __restrict__ arg_sl1,
                                                                      int* __restrict__ best_idx) {
    extern __shared__ float sm[];
    __shared__ float rv[4], lv[4];
    __shared__ int ra[4], la[4], kbest;
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    float* tx = sm;
    float* px = sm + 3 * n;
    const float* ps = pred + (size_t)s * n_atoms * 3;
    for (int i = tid; i < 3 * n; i += SYM_SCORE_THREADS) { tx[i] = ref[(size_t)a0 * 3 + i]; px[i] = ps[(size_t)a0 * 3 + i]; }
    __syncthreads();
    const int K = auto_cnt[b], nk = max(K, 1), base = K > 0 ? flat_off[b] : 0;
    float br = INFINITY, bl = INFINITY;
    int kr = INT_MAX, kl = INT_MAX;
    const float inv_n = 1.f / (float)max(n, 1), inv_3n = 1.f / (float)max(3 * n, 1);
    for (int k = wv; k < nk; k += 4) {
        float sr = 0.f, sl = 0.f;
        for (int i = ln; i < n; i += 64) {
            int j = K > 0 ? flat[base + (size_t)k * n + i] : i;
            j = (unsigned)j < (unsigned)n ? j : i;
            const float dx = px[3 * j] - tx[3 * i], dy = px[3 * j + 1] - tx[3 * i + 1], dz = px[3 * j + 2] - tx[3 * i + 2];
            sr += dx * dx + dy * dy + dz * dz;
            sl += sym_sl1(dx) + sym_sl1(dy) + sym_sl1(dz);
        }
        sr = wave_sum(sr);                        // butterfly: every lane holds the same sum
        sl = wave_sum(sl);
        const float r = sqrtf(sr * inv_n), l = sl * inv_3n;
        if (kr == INT_MAX || r < br) { br = r; kr = k; }
        if (kl == INT_MAX || l < bl) { bl = l; kl = k; }
    }
    if (ln == 0) { rv[wv] = br; ra[wv] = kr; lv[wv] = bl; la[wv] = kl; }
    __syncthreads();
    if (tid == 0) {
        float vr = INFINITY, vl = INFINITY;
        int ar = INT_MAX, al = INT_MAX;
        for (int w = 0; w < 4; ++w) {
            if (ra[w] != INT_MAX && (ar == INT_MAX || rv[w] < vr || (rv[w] == vr && ra[w] < ar))) { vr = rv[w]; ar = ra[w]; }
            if (la[w] != INT_MAX && (al == INT_MAX || lv[w] < vl || (lv[w] == vl && la[w] < al))) { vl = lv[w]; al = la[w]; }
        }
        const size_t o = (size_t)s * n_lig + b;
        min_rmsd[o] = vr; arg_rmsd[o] = ar;
        min_sl1[o] = vl; arg_sl1[o] = al;
        kbest = al;
    }
    if (best_idx == nullptr || s != 0) return;
    __syncthreads();
    for (int i = tid; i < n; i += SYM_SCORE_THREADS) {
        int j = K > 0 ? flat[base + (size_t)kbest * n + i] : i;
        j = (unsigned)j < (unsigned)n ? j : i;
        best_idx[a0 + i] = a0 + j;
    }
}

extern "C" int fabind_sym_automorphisms(const int* labels, const int* nbr_ptr, const int* nbr_idx, const int* atom_off, int n_ligands,
                                        int cap, int max_steps, const int* flat_off, int* scratch, int* flat, int* count, int* status,
                                        hipStream_t stream) {
    if (n_ligands <= 0) return 0;
    FB_REQUIRE(cap >= 1 && max_steps >= 0, "fabind_sym_automorphisms: cap >= 1, max_steps >= 0");
    FB_REQUIRE((flat == nullptr) == (scratch == nullptr) && (flat == nullptr || flat_off != nullptr),
               "fabind_sym_automorphisms: write mode needs flat_off, scratch and flat");
    hipLaunchKernelGGL(sym_search_kernel, dim3(n_ligands), dim3(64), 0, stream, labels, nbr_ptr, nbr_idx, atom_off, cap, max_steps,
                       flat_off, scratch, count, status);
    FB_CHECK_LAUNCH();
    if (flat == nullptr) return 0;
    hipLaunchKernelGGL(sym_sort_kernel, dim3(n_ligands), dim3(256), 0, stream, scratch, flat, flat_off, count, atom_off);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_sym_score(const float* pred, int n_pose, int n_atoms, const float* ref, const int* atom_off, const int* flat_off,
                                const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* min_rmsd, int* arg_rmsd,
                                float* min_sl1, int* arg_sl1, int* best_idx, hipStream_t stream) {
    if (n_ligands <= 0 || n_pose <= 0) return 0;
    FB_REQUIRE(max_atoms >= 0 && max_atoms <= 2048, "fabind_sym_score: at most 2048 atoms per ligand");
    FB_REQUIRE(n_pose <= 65535, "fabind_sym_score: at most 65535 poses");
    const size_t lds = (size_t)6 * max(max_atoms, 1) * sizeof(float);
    hipLaunchKernelGGL(sym_score_kernel, dim3(n_ligands, n_pose), dim3(SYM_SCORE_THREADS), lds, stream, pred, n_atoms, ref, atom_off,
                       flat_off, auto_cnt, flat, n_ligands, min_rmsd, arg_rmsd, min_sl1, arg_sl1, best_idx);
    FB_CHECK_LAUNCH();
    return 0;
}
