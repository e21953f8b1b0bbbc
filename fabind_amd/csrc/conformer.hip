// Train-time ligand augmentation: rotatable bonds from the bond list, torsion noise and the uniform random rotation
// (reference FABind_plus/fabind/utils/utils.py:155-190 get_torsions -- RDKit SMARTS "[!$(*#*)&!D1]-&!@[!$(*#*)&!D1]";
// :285-304 --train-ligand-torsion-noise: SetDihedralRad per rotatable bond, CanonicalizeConformer, uniform_random_rotation;
// :45-81 uniform_random_rotation; :307-311 random_rotation of the start conformer -- all per sample on the host, in dataloader workers).
//
// torsion_find_kernel: one wave per entry e = (j -> k) of the symmetrised neighbour lists.  Entries with j > k, a code other than
//   SINGLE (4), an end of heavy-atom degree < 2 or an end that has a TRIPLE (2) bond leave at once.  Otherwise the ligand's adjacency
//   goes to LDS as bitsets (4 x u64 per row) and the wave flood-fills from k without crossing j-k: visited / frontier are four
//   wave-uniform u64 words, lane L answers for atoms L, L + 64, L + 128, L + 192 ("has an unvisited atom of mine a neighbour on the
//   frontier"), a ballot per word collects the next frontier and the loop ends when every ballot is empty.  j reached: a ring bond,
//   dropped.  Otherwise the visited set is the moving side.  i / l = lowest-index neighbour of j other than k / of k other than j.
// torsion_count_kernel: one wave per ligand: count[b] = rotatable entries of its atoms; status 3 for n > 256 (zero torsions).
// torsion_write_kernel: one wave per ligand: the found entries, already in ascending (j, k) order in the neighbour lists (sorted by
//   owner, then by neighbour), are compacted into the caller's slot (ballot + popcount), never past it.
// conformer_perturb_kernel: one work-group of one wave per (ligand, copy); the ligand's coordinates live in LDS (n <= 256; a larger
//   ligand has no torsions and is rotated straight from global memory).  The torsions are applied one after another: all lanes read the
//   four atoms of `quad` (LDS broadcast), compute the dihedral (IUPAC sign: atan2(b2/|b2| . (n1 x n2), n1 . n2), n1 = b1 x b2,
//   n2 = b2 x b3, b1 = pj - pi, b2 = pk - pj, b3 = pl - pk) and rotate the atoms of `side` -- k itself excepted: the axis atoms never
//   move -- about the axis j -> k through pj by target - current (Rodrigues), or by target when `relative`.
//   COLLINEAR: the dihedral counts as degenerate (current = 0) when |n1|^2 <= 1e-8 |b1|^2 |b2|^2 or |n2|^2 <= 1e-8 |b2|^2 |b3|^2,
//   i.e. the sine of a bond angle is at most 1e-4 (this also covers coincident atoms); a zero-length axis skips the torsion.
//   Then M = -(H R) of uniform_random_rotation from (x1, x2, x3) and out = (x - mean) M [+ mean M unless `centre`].
//   Draws: u(seed, key[b], copy, draw) = top 24 bits of four chained fb_hash32 rounds, in [0, 1); draw t < T_b is torsion t's target
//   2 pi u, then x2, x3, x1 (the reference's order) at T_b, T_b + 1, T_b + 2.  Sums: each lane adds its atoms in ascending order, then
//   the butterfly wave_sum -- a fixed order, repeats are bit-identical.  No atomics, no inline assembly.
#include "common.h"
#include "fabind_hip.h"

#define CF_MAX_N 256
#define CF_W 4
#define CF_TWO_PI 6.28318530717958647692f

__device__ __forceinline__ float cf_uniform(uint32_t seed, uint32_t key, uint32_t copy, uint32_t draw) {
    uint32_t h = fb_hash32(seed + 0x9e3779b9u);
    h = fb_hash32((h ^ key) + 0x85ebca6bu);
    h = fb_hash32((h ^ copy) + 0xc2b2ae35u);
    h = fb_hash32((h ^ draw) + 0x27d4eb2fu);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ int cf_first(const uint64_t* r) {           // lowest set bit of a 256-bit row, -1 if none
    for (int w = 0; w < CF_W; ++w)
        if (r[w]) return (w << 6) + __ffsll((long long)r[w]) - 1;
    return -1;
}

__global__ __launch_bounds__(64) void torsion_find_kernel(const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx,
                                                          const int* __restrict__ nbr_code, const int* __restrict__ nbr_own,
                                                          const int* __restrict__ atom_off, int n_ligands, int* __restrict__ flag,
                                                          int* __restrict__ sq, uint32_t* __restrict__ ss) {
    __shared__ uint64_t adj[CF_MAX_N][CF_W];
    __shared__ uint64_t trip[CF_W];
    const int e = blockIdx.x, ln = threadIdx.x;
    const int gj = nbr_own[e], gk = nbr_idx[e];
    int lo = 0, hi = n_ligands;                                        // the last ligand whose first atom is <= gj
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (atom_off[mid] <= gj) lo = mid; else hi = mid;
    }
    const int a0 = atom_off[lo], n = atom_off[lo + 1] - a0;
    const int j = gj - a0, k = gk - a0;
    if (nbr_code[e] != 4 || j < 0 || j >= k || k >= n || n > CF_MAX_N) {   // wave-uniform
        if (ln == 0) flag[e] = 0;
        return;
    }
#pragma unroll
    for (int w = 0; w < CF_W; ++w) {
        const int i = (w << 6) + ln;
        uint64_t row[CF_W] = {0, 0, 0, 0};
        bool tr = false;
        if (i < n) {
            for (int q = nbr_ptr[a0 + i]; q < nbr_ptr[a0 + i + 1]; ++q) {
                const int o = nbr_idx[q] - a0;
                if (o >= 0 && o < n && o != i) {
                    row[o >> 6] |= 1ull << (o & 63);
                    tr |= nbr_code[q] == 2;
                }
            }
#pragma unroll
            for (int x = 0; x < CF_W; ++x) adj[i][x] = row[x];
        }
        const uint64_t m = __ballot(tr);
        if (ln == 0) trip[w] = m;
    }
    __syncthreads();
    uint64_t rj[CF_W], rk[CF_W];
    int dj = 0, dk = 0;
#pragma unroll
    for (int w = 0; w < CF_W; ++w) {
        rj[w] = adj[j][w];
        rk[w] = adj[k][w];
        dj += __popcll(rj[w]);
        dk += __popcll(rk[w]);
    }
    const bool tj = (trip[j >> 6] >> (j & 63)) & 1, tk = (trip[k >> 6] >> (k & 63)) & 1;
    if (dj < 2 || dk < 2 || tj || tk) {
        if (ln == 0) flag[e] = 0;
        return;
    }
    uint64_t V[CF_W] = {0, 0, 0, 0}, F[CF_W] = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < CF_W; ++w) {                                   // (static indices: the words stay in registers)
        if (w == (k >> 6)) { rj[w] &= ~(1ull << (k & 63)); V[w] = F[w] = 1ull << (k & 63); }
        if (w == (j >> 6)) rk[w] &= ~(1ull << (j & 63));
    }
    for (int it = 0; it < n; ++it) {                                   // every round that goes on visits at least one new atom
        uint64_t nf[CF_W];
#pragma unroll
        for (int w = 0; w < CF_W; ++w) {
            const int a = (w << 6) + ln;
            bool nw = false;
            if (a < n && !((V[w] >> ln) & 1)) {
                uint64_t hit = 0;
#pragma unroll
                for (int x = 0; x < CF_W; ++x) hit |= (a == j ? rj[x] : adj[a][x]) & F[x];
                nw = hit != 0;
            }
            nf[w] = __ballot(nw);
        }
        if (!(nf[0] | nf[1] | nf[2] | nf[3])) break;
#pragma unroll
        for (int w = 0; w < CF_W; ++w) { V[w] |= nf[w]; F[w] = nf[w]; }
    }
    uint64_t vj = 0;
#pragma unroll
    for (int w = 0; w < CF_W; ++w)
        if (w == (j >> 6)) vj = V[w];
    if ((vj >> (j & 63)) & 1) {                                        // j reached without the bond: j-k is on a cycle
        if (ln == 0) flag[e] = 0;
        return;
    }
    if (ln == 0) {
        flag[e] = 1;
        int* q = sq + (size_t)e * 4;
        q[0] = cf_first(rj); q[1] = j; q[2] = k; q[3] = cf_first(rk);
    }
    if (ln < 8) {
        const uint64_t v = ln < 2 ? V[0] : ln < 4 ? V[1] : ln < 6 ? V[2] : V[3];
        ss[(size_t)e * 8 + ln] = (uint32_t)(v >> ((ln & 1) * 32));
    }
}

__global__ __launch_bounds__(64) void torsion_count_kernel(const int* __restrict__ nbr_ptr, const int* __restrict__ atom_off,
                                                           const int* __restrict__ flag, int* __restrict__ count, int* __restrict__ status) {
    const int b = blockIdx.x, ln = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    int c = 0;
    if (n > 0 && n <= CF_MAX_N)
        for (int e = nbr_ptr[a0] + ln; e < nbr_ptr[a0 + n]; e += 64) c += flag[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (ln == 0) { count[b] = c; status[b] = n > CF_MAX_N ? 3 : 0; }
}

__global__ __launch_bounds__(64) void torsion_write_kernel(const int* __restrict__ nbr_ptr, const int* __restrict__ atom_off,
                                                           const int* __restrict__ flag, const int* __restrict__ sq,
                                                           const uint32_t* __restrict__ ss, const int* __restrict__ tor_off,
                                                           int* __restrict__ quad, uint32_t* __restrict__ side) {
    const int b = blockIdx.x, ln = threadIdx.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    if (n <= 0 || n > CF_MAX_N) return;
    int pos = tor_off[b];
    const int lim = tor_off[b + 1], e1 = nbr_ptr[a0 + n];
    for (int e0 = nbr_ptr[a0]; e0 < e1; e0 += 64) {                    // wave-uniform bounds: every lane reaches the ballot
        const int e = e0 + ln;
        const bool f = e < e1 && flag[e] != 0;
        const uint64_t m = __ballot(f);
        const int p = pos + __popcll(m & ((1ull << ln) - 1));
        if (f && p < lim) {                                            // never past the caller's slot (sized from the counts)
#pragma unroll
            for (int x = 0; x < 4; ++x) quad[(size_t)p * 4 + x] = sq[(size_t)e * 4 + x];
#pragma unroll
            for (int x = 0; x < 8; ++x) side[(size_t)p * 8 + x] = ss[(size_t)e * 8 + x];
        }
        pos += __popcll(m);
    }
}

__global__ __launch_bounds__(64) void conformer_perturb_kernel(const float* __restrict__ x, const int* __restrict__ atom_off, int n_atoms,
                                                               const int* __restrict__ tor_off, const int* __restrict__ quad,
                                                               const uint32_t* __restrict__ side, const float* __restrict__ angles,
                                                               int t_total, const float* __restrict__ uniforms,
                                                               const int* __restrict__ keys, uint32_t seed, int relative, int rotate,
                                                               int centre, float* __restrict__ out) {
    __shared__ float sx[CF_MAX_N * 3];
    const int b = blockIdx.x, s = blockIdx.y, ln = threadIdx.x, B = gridDim.x;
    const int a0 = atom_off[b], n = atom_off[b + 1] - a0;
    if (n <= 0) return;
    const float* xb = x + (size_t)a0 * 3;
    float* ob = out + ((size_t)s * n_atoms + a0) * 3;
    const bool staged = n <= CF_MAX_N;
    const int t0 = tor_off != nullptr ? tor_off[b] : 0;
    const int T = tor_off != nullptr && staged ? tor_off[b + 1] - t0 : 0;
    const uint32_t key = keys != nullptr ? (uint32_t)keys[b] : (uint32_t)b;
    if (staged) {
        for (int i = ln; i < 3 * n; i += 64) sx[i] = xb[i];
        __syncthreads();
    }
    for (int t = 0; t < T; ++t) {
        const int* q = quad + (size_t)(t0 + t) * 4;
        const int qi = q[0], qj = q[1], qk = q[2], ql = q[3];
        if ((unsigned)qi >= (unsigned)n || (unsigned)qj >= (unsigned)n || (unsigned)qk >= (unsigned)n || (unsigned)ql >= (unsigned)n)
            continue;                                                  // wave-uniform: a plan of another batch moves nothing out of range
        const float pjx = sx[3 * qj], pjy = sx[3 * qj + 1], pjz = sx[3 * qj + 2];
        const float b1x = pjx - sx[3 * qi], b1y = pjy - sx[3 * qi + 1], b1z = pjz - sx[3 * qi + 2];
        const float b2x = sx[3 * qk] - pjx, b2y = sx[3 * qk + 1] - pjy, b2z = sx[3 * qk + 2] - pjz;
        const float b3x = sx[3 * ql] - sx[3 * qk], b3y = sx[3 * ql + 1] - sx[3 * qk + 1], b3z = sx[3 * ql + 2] - sx[3 * qk + 2];
        __syncthreads();                                               // every lane holds the four atoms before any atom moves
        const float l2 = b2x * b2x + b2y * b2y + b2z * b2z;
        if (l2 == 0.f) continue;                                       // wave-uniform
        const float target = angles != nullptr ? angles[(size_t)s * t_total + t0 + t] : CF_TWO_PI * cf_uniform(seed, key, s, t);
        float theta = target;
        if (!relative) {
            const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
            const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
            const float l1 = b1x * b1x + b1y * b1y + b1z * b1z, l3 = b3x * b3x + b3y * b3y + b3z * b3z;
            const float m1 = n1x * n1x + n1y * n1y + n1z * n1z, m2 = n2x * n2x + n2y * n2y + n2z * n2z;
            float cur = 0.f;
            if (m1 > 1e-8f * l1 * l2 && m2 > 1e-8f * l2 * l3) {
                const float cx = n1y * n2z - n1z * n2y, cy = n1z * n2x - n1x * n2z, cz = n1x * n2y - n1y * n2x;
                const float yv = (cx * b2x + cy * b2y + cz * b2z) / sqrtf(l2);
                const float xv = n1x * n2x + n1y * n2y + n1z * n2z;
                cur = atan2f(yv, xv);
            }
            theta = target - cur;
        }
        float sn, cs;
        sincosf(theta, &sn, &cs);
        const float inv = 1.0f / sqrtf(l2);
        const float ux = b2x * inv, uy = b2y * inv, uz = b2z * inv;
        const uint32_t* sd = side + (size_t)(t0 + t) * 8;
#pragma unroll
        for (int w = 0; w < CF_W; ++w) {
            const int a = (w << 6) + ln;
            if (a < n && a != qk && ((sd[a >> 5] >> (a & 31)) & 1u)) {
                const float vx = sx[3 * a] - pjx, vy = sx[3 * a + 1] - pjy, vz = sx[3 * a + 2] - pjz;
                const float d = (ux * vx + uy * vy + uz * vz) * (1.0f - cs);
                const float wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
                sx[3 * a] = pjx + (vx * cs + wx * sn + ux * d);
                sx[3 * a + 1] = pjy + (vy * cs + wy * sn + uy * d);
                sx[3 * a + 2] = pjz + (vz * cs + wz * sn + uz * d);
            }
        }
        __syncthreads();
    }
    const float* src = staged ? sx : xb;
    float mx = 0.f, my = 0.f, mz = 0.f;
    for (int i = ln; i < n; i += 64) { mx += src[3 * i]; my += src[3 * i + 1]; mz += src[3 * i + 2]; }
    mx = wave_sum(mx); my = wave_sum(my); mz = wave_sum(mz);
    const float fn = (float)n;
    mx /= fn; my /= fn; mz /= fn;
    float M[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
    if (rotate) {
        float x1, x2, x3;
        if (uniforms != nullptr) {
            const float* u = uniforms + ((size_t)s * B + b) * 3;
            x1 = u[0]; x2 = u[1]; x3 = u[2];
        } else {
            x2 = cf_uniform(seed, key, s, T);
            x3 = cf_uniform(seed, key, s, T + 1);
            x1 = cf_uniform(seed, key, s, T + 2);
        }
        float s1, c1, s2, c2;
        sincosf(CF_TWO_PI * x1, &s1, &c1);
        sincosf(CF_TWO_PI * x2, &s2, &c2);
        const float r3 = sqrtf(x3);
        const float v[3] = {c2 * r3, s2 * r3, sqrtf(1.0f - x3)};
        const float R[3][3] = {{c1, -s1, 0.f}, {s1, c1, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int m = 0; m < 3; ++m) acc += ((r == m ? 1.0f : 0.0f) - 2.0f * v[r] * v[m]) * R[m][c];
                M[r][c] = -acc;
            }
    }
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (!centre) {
        ox = mx * M[0][0] + my * M[1][0] + mz * M[2][0];
        oy = mx * M[0][1] + my * M[1][1] + mz * M[2][1];
        oz = mx * M[0][2] + my * M[1][2] + mz * M[2][2];
    }
    for (int i = ln; i < n; i += 64) {
        const float dx = src[3 * i] - mx, dy = src[3 * i + 1] - my, dz = src[3 * i + 2] - mz;
        ob[3 * i] = (dx * M[0][0] + dy * M[1][0] + dz * M[2][0]) + ox;
        ob[3 * i + 1] = (dx * M[0][1] + dy * M[1][1] + dz * M[2][1]) + oy;
        ob[3 * i + 2] = (dx * M[0][2] + dy * M[1][2] + dz * M[2][2]) + oz;
    }
}

extern "C" int fabind_torsion_plan(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* nbr_own, const int* atom_off,
                                   int n_ligands, int n_entries, int* flag, int* scratch_quad, unsigned* scratch_side, int* count,
                                   int* status, const int* tor_off, int* quad, unsigned* side, hipStream_t stream) {
    if (n_ligands <= 0) return 0;
    FB_REQUIRE(n_entries >= 0, "fabind_torsion_plan: n_entries >= 0");
    FB_REQUIRE(n_entries == 0 || (flag != nullptr && scratch_quad != nullptr && scratch_side != nullptr),
               "fabind_torsion_plan: flag, scratch_quad and scratch_side are needed in both modes");
    if (quad == nullptr) {                                             // count mode
        FB_REQUIRE(count != nullptr && status != nullptr, "fabind_torsion_plan: count mode needs count and status");
        if (n_entries > 0) {
            hipLaunchKernelGGL(torsion_find_kernel, dim3(n_entries), dim3(64), 0, stream, nbr_ptr, nbr_idx, nbr_code, nbr_own, atom_off,
                               n_ligands, flag, scratch_quad, scratch_side);
            FB_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(torsion_count_kernel, dim3(n_ligands), dim3(64), 0, stream, nbr_ptr, atom_off, flag, count, status);
        FB_CHECK_LAUNCH();
        return 0;
    }
    FB_REQUIRE(tor_off != nullptr && side != nullptr, "fabind_torsion_plan: write mode needs tor_off, quad and side");
    if (n_entries == 0) return 0;
    hipLaunchKernelGGL(torsion_write_kernel, dim3(n_ligands), dim3(64), 0, stream, nbr_ptr, atom_off, flag, scratch_quad, scratch_side,
                       tor_off, quad, side);
    FB_CHECK_LAUNCH();
    return 0;
}

extern "C" int fabind_conformer_perturb(const float* x, const int* atom_off, int n_ligands, int n_atoms, int n_copies, const int* tor_off,
                                        const int* quad, const unsigned* side, const float* angles, int t_total, const float* uniforms,
                                        const int* keys, unsigned seed, int relative, int rotate, int centre, float* out,
                                        hipStream_t stream) {
    if (n_ligands <= 0 || n_copies <= 0) return 0;
    FB_REQUIRE(n_copies <= 65535, "fabind_conformer_perturb: at most 65535 copies");
    FB_REQUIRE(tor_off == nullptr || t_total == 0 || (quad != nullptr && side != nullptr),
               "fabind_conformer_perturb: a torsion plan needs quad and side");
    hipLaunchKernelGGL(conformer_perturb_kernel, dim3(n_ligands, n_copies), dim3(64), 0, stream, x, atom_off, n_atoms, tor_off, quad, side,
                       angles, t_total, uniforms, keys, (uint32_t)seed, relative, rotate, centre, out);
    FB_CHECK_LAUNCH();
    return 0;
}
