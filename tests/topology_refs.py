"""Numpy / plain-Python restatement of fabind_amd.topology (csrc/topology.hip): the LAS ("local atomic structure") pair mask of a
ligand from its bond list -- bonded, two bonds apart, or on a common RELEVANT cycle (a cycle whose edge set is no GF(2) sum of
strictly shorter cycles; the union of all minimum cycle bases) -- restated step by step as DESIGN.md section 14 words it, plus a
brute-force definition for small graphs (every simple cycle, Gaussian elimination over edge-incidence vectors) and the hand-written
molecules the tests share."""
import itertools

import numpy as np

MAX_ATOMS = 256
MAX_CHORDS = 64


# ------------------------------------------------------------------------------------------------ graphs
def adjacency(n, bonds):
    """Neighbour sets of the undirected simple graph: repeated rows and both directions collapse, self-loops are dropped."""
    nb = [set() for _ in range(n)]
    for a, b in np.asarray(bonds, np.int64).reshape(-1, 2):
        a, b = int(a), int(b)
        if a != b:
            nb[a].add(b)
            nb[b].add(a)
    return nb


def two_hop_mask(n, nb):
    """(a) bonded or (b) a common neighbour; zero diagonal."""
    A = np.zeros((n, n), np.int64)
    for a in range(n):
        for b in nb[a]:
            A[a, b] = 1
    M = ((A + A @ A) > 0).astype(np.int64)
    M[np.arange(n), np.arange(n)] = 0
    return M


def hop_distances(n, nb):
    """All-pairs hop distance by a BFS from every atom; -1 = not reachable."""
    D = -np.ones((n, n), np.int64)
    for r in range(n):
        D[r, r] = 0
        front, d = [r], 0
        while front:
            d += 1
            nxt = []
            for u in front:
                for v in nb[u]:
                    if D[r, v] < 0:
                        D[r, v] = d
                        nxt.append(v)
            front = nxt
    return D


def _reduce(v, basis):
    """v against an echelon basis kept in insertion order: [(vector, its highest bit)]."""
    for b, piv in basis:
        if (v >> piv) & 1:
            v ^= b
    return v


# ------------------------------------------------------------------------------------------------ restatement of section 2
def ring_mask(n, nb):
    """-> (R int64 [n, n], status).  R[i][j] = 1 iff i != j lie on a common relevant cycle.  status 3: more than 256 atoms,
    4: more than 64 chords (R is zero then)."""
    R = np.zeros((n, n), np.int64)
    if n > MAX_ATOMS:
        return R, 3
    nbs = [sorted(s) for s in nb]
    D = hop_distances(n, nb)
    # 1. spanning forest: the BFS tree from the lowest atom of every component, parent = lowest-index neighbour one level closer
    par = [-1] * n
    for x in range(n):
        c = int(np.nonzero(D[x] >= 0)[0][0])
        if x != c:
            par[x] = min(y for y in nbs[x] if D[c, y] == D[c, x] - 1)
    chords = sorted((a, b) for a in range(n) for b in nbs[a] if a < b and par[a] != b and par[b] != a)
    if len(chords) > MAX_CHORDS:
        return R, 4
    cid = {e: k for k, e in enumerate(chords)}
    cb = lambda a, b: (1 << cid[(min(a, b), max(a, b))]) if (min(a, b), max(a, b)) in cid else 0
    # 2./3. candidates at every root
    cands = {}                                                     # length -> [(root, vector, ends, apex or None)]
    for r in range(n):
        S = {r: 0}
        for x in sorted((x for x in range(n) if D[r, x] > 0), key=lambda x: (D[r, x], x)):
            y = min(y for y in nbs[x] if D[r, y] == D[r, x] - 1)
            S[x] = S[y] ^ cb(y, x)
        for p in range(n):
            d = D[r, p]
            if d < 1:
                continue
            for q in nbs[p]:
                if q > p and D[r, q] == d:
                    cands.setdefault(2 * d + 1, []).append((r, S[p] ^ S[q] ^ cb(p, q), (p, q), None))
            if d >= 2:
                cl = [q for q in nbs[p] if D[r, q] == d - 1]
                for q1, q2 in itertools.combinations(cl, 2):
                    cands.setdefault(2 * d, []).append((r, S[q1] ^ S[q2] ^ cb(q1, p) ^ cb(q2, p), (q1, q2), p))
    # 4./5. lengths ascending
    basis = []
    for L in sorted(cands):
        rel = [c for c in cands[L] if _reduce(c[1], basis)]
        for r, _, ends, apex in rel:
            for t in ends:
                for j in range(n):
                    if D[r, j] >= 0 and D[j, t] >= 0 and D[r, j] + D[j, t] == D[r, t]:
                        R[r, j] = 1
            if apex is not None:
                R[r, apex] = 1
        for _, v, _, _ in rel:
            v = _reduce(v, basis)
            if v:
                basis.append((v, v.bit_length() - 1))
    R[np.arange(n), np.arange(n)] = 0
    return R, 0


def las_mask(n, bonds):
    """-> (mask int64 [n, n], ring_pairs, status): the whole definition for one ligand; bonds [E, 2] local ids."""
    nb = adjacency(n, bonds)
    R, status = ring_mask(n, nb)
    M = ((two_hop_mask(n, nb) + R) > 0).astype(np.int64)
    return M, int(np.triu(R | R.T, 1).sum()), status


def pairs_of(mask):
    """dense_to_sparse of a mask: int64 [2, El], row-major."""
    i, j = np.nonzero(mask)
    return np.stack([i, j]).astype(np.int64)


def las_pairs(bond_index, atom_off):
    """A batch: bond_index [2, E] global ids, atom_off [B + 1] -> (edge_index int64 [2, El] global, off, ring_pairs, status)."""
    bi = np.asarray(bond_index, np.int64).reshape(2, -1)
    ao = np.asarray(atom_off, np.int64)
    ei, off, rp, st = [], [0], [], []
    for b in range(len(ao) - 1):
        a0, a1 = int(ao[b]), int(ao[b + 1])
        sel = (bi[0] >= a0) & (bi[0] < a1)
        M, r, s = las_mask(a1 - a0, bi[:, sel].T - a0)
        p = pairs_of(M) + a0
        ei.append(p)
        off.append(off[-1] + p.shape[1])
        rp.append(r)
        st.append(s)
    ei = np.concatenate(ei, 1) if ei else np.zeros((2, 0), np.int64)
    return ei, np.asarray(off, np.int32), np.asarray(rp, np.int32), np.asarray(st, np.int32)


# ------------------------------------------------------------------------------------------------ brute force
def simple_cycles(n, nb, limit=200000):
    """Every simple cycle once, as a vertex list starting at its lowest vertex; None when there are more than `limit`."""
    out = []
    for s in range(n):
        stack = [(s, [s], {s})]
        while stack:
            u, path, seen = stack.pop()
            for v in nb[u]:
                if v == s and len(path) >= 3 and path[1] < path[-1]:
                    out.append(path)
                    if len(out) > limit:
                        return None
                elif v > s and v not in seen:
                    stack.append((v, path + [v], seen | {v}))
    return out


def brute_rings(n, nb, limit=200000):
    """The relevant cycles by definition: a cycle is kept iff its edge-incidence vector is not in the GF(2) span of ALL strictly
    shorter cycles.  -> list of vertex lists, or None above `limit` simple cycles."""
    cyc = simple_cycles(n, nb, limit)
    if cyc is None:
        return None
    eid = {}
    for a in range(n):
        for b in nb[a]:
            if a < b:
                eid[(a, b)] = len(eid)

    def vec(c):
        v = 0
        for a, b in zip(c, c[1:] + c[:1]):
            v |= 1 << eid[(min(a, b), max(a, b))]
        return v
    by_len = {}
    for c in cyc:
        by_len.setdefault(len(c), []).append((c, vec(c)))
    basis, rings = [], []
    for L in sorted(by_len):
        rings += [c for c, v in by_len[L] if _reduce(v, basis)]
        for _, v in by_len[L]:
            v = _reduce(v, basis)
            if v:
                basis.append((v, v.bit_length() - 1))
    return rings


def mask_from_rings(n, nb, rings):
    """The mask the definition gives once the ring list is known (the arithmetic of the reference's function)."""
    M = two_hop_mask(n, nb)
    R = np.zeros((n, n), np.int64)
    for ring in rings:
        for i in ring:
            for j in ring:
                if i != j:
                    R[i, j] = 1
    return ((M + R) > 0).astype(np.int64), int(np.triu(R, 1).sum())


def brute_las_mask(n, bonds):
    nb = adjacency(n, bonds)
    return mask_from_rings(n, nb, brute_rings(n, nb))


# ------------------------------------------------------------------------------------------------ shapes
def chain(n, first=0):
    return [(first + i, first + i + 1) for i in range(n - 1)]


def ring(n, first=0):
    return chain(n, first) + [(first + n - 1, first)]


def ladder(k):
    """2 x k ladder: rails 0..k-1 and k..2k-1, a rung at every position: 2k atoms, 3k - 2 bonds, k - 1 chords."""
    return chain(k) + chain(k, k) + [(i, k + i) for i in range(k)]


def hand_molecules():
    """name -> (n, bonds, rings written out by hand, ring pairs of the issue's table)."""
    six = list(range(6))
    out = {"benzene": (6, ring(6), [six], 15)}
    # naphthalene: two 6-rings sharing the bond 0-5
    out["naphthalene"] = (10, ring(6) + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 0)], [six, [0, 5, 6, 7, 8, 9]], 29)
    # norbornane: bridgeheads 0 and 3, bridges 1-2, 4-5 and the one-atom bridge 6; the 6-ring 0-1-2-3-4-5 is the sum of the 5-rings
    out["norbornane"] = (7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 6), (6, 3)], [[0, 1, 2, 3, 6], [0, 5, 4, 3, 6]], 17)
    # bicyclo[2.2.2]octane: bridgeheads 0 and 1, bridges 2-3, 4-5, 6-7; three 6-rings
    b222 = [(0, 2), (2, 3), (3, 1), (0, 4), (4, 5), (5, 1), (0, 6), (6, 7), (7, 1)]
    out["bicyclo222octane"] = (8, b222, [[0, 2, 3, 1, 5, 4], [0, 2, 3, 1, 7, 6], [0, 4, 5, 1, 7, 6]], 28)
    # cubane: bottom face 0-1-2-3, top face 4-5-6-7, verticals; six 4-rings
    cube = ring(4) + ring(4, 4) + [(i, i + 4) for i in range(4)]
    out["cubane"] = (8, cube, [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [3, 0, 4, 7]], 24)
    # a 6-ring with a cyclopropane fused on every bond: atom 6 + i bridges the bond i - (i + 1) % 6
    tri = [(i, 6 + i) for i in range(6)] + [((i + 1) % 6, 6 + i) for i in range(6)]
    out["hexa_cyclopropa_6ring"] = (12, ring(6) + tri, [six] + [[i, (i + 1) % 6, 6 + i] for i in range(6)], 27)
    out["biphenyl"] = (12, ring(6) + ring(6, 6) + [(0, 6)], [six, list(range(6, 12))], 30)
    # spiro[4.4]nonane: two 5-rings sharing atom 0
    out["spiro_pair"] = (9, ring(5) + [(0, 5), (5, 6), (6, 7), (7, 8), (8, 0)], [[0, 1, 2, 3, 4], [0, 5, 6, 7, 8]], 20)
    out["ring14"] = (14, ring(14), [list(range(14))], 91)
    return out


def random_graph(rng, n, extra, connected=True, max_degree=4):
    """A seeded random simple graph: a random spanning tree (or, not connected, a forest of two trees) plus up to `extra` further
    edges, degree <= max_degree, atoms renumbered at random."""
    deg = [0] * n
    edges = set()
    split = int(rng.integers(1, n)) if (not connected and n >= 2) else n
    for x in range(1, n):
        if x == split:
            continue                                               # x starts the second tree
        lo = 0 if x < split else split
        cand = [y for y in range(lo, x) if deg[y] < max_degree]
        if not cand:
            continue
        y = int(rng.choice(cand))
        edges.add((y, x))
        deg[y] += 1
        deg[x] += 1
    for _ in range(extra):
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and (min(a, b), max(a, b)) not in edges and deg[a] < max_degree and deg[b] < max_degree:
            edges.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    perm = rng.permutation(n)
    return [(int(perm[a]), int(perm[b])) for a, b in sorted(edges)]


def random_ring_system(rng, n):
    """A seeded drug-like graph of exactly n atoms: rings of 3 to 7 atoms fused on a bond, joined spiro at an atom or hung on a
    single bond, bridges across a ring, and chain atoms, degree <= 4, atoms renumbered at random.  -> bonds."""
    bonds, deg, m = ring(6), [2] * 6, 6

    def add(a, b):
        bonds.append((a, b))
        deg[a] += 1
        deg[b] += 1
    while m < n:
        kind, room = int(rng.integers(0, 5)), n - m
        if kind == 0 and room >= 1:                                    # fuse a ring of k atoms on a bond (k - 2 new atoms)
            a, b = bonds[int(rng.integers(0, len(bonds)))]
            k = int(rng.integers(3, 8))
            if deg[a] < 4 and deg[b] < 4 and k - 2 <= room:
                new = list(range(m, m + k - 2))
                deg += [0] * len(new)
                for u, v in zip([a] + new, new + [b]):
                    add(u, v)
                m += len(new)
        elif kind == 1 and room >= 2:                                  # spiro ring at an atom
            a = int(rng.integers(0, m))
            k = int(rng.integers(3, 7))
            if deg[a] <= 2 and k - 1 <= room:
                new = list(range(m, m + k - 1))
                deg += [0] * len(new)
                for u, v in zip([a] + new, new + [a]):
                    add(u, v)
                m += len(new)
        elif kind == 2 and room >= 5:                                  # a ring on a single bond
            a = int(rng.integers(0, m))
            k = int(rng.integers(5, 7))
            if deg[a] < 4 and k <= room:
                deg += [0] * k
                for u, v in ring(k, m):
                    add(u, v)
                add(a, m)
                m += k
        elif kind == 3:                                                # one-atom bridge between two atoms at distance 2 or more
            a, b = (int(v) for v in rng.integers(0, m, 2))
            if a != b and deg[a] < 4 and deg[b] < 4 and (min(a, b), max(a, b)) not in {(min(u, v), max(u, v)) for u, v in bonds}:
                deg.append(0)
                add(a, m)
                add(m, b)
                m += 1
        else:                                                          # a chain atom
            a = int(rng.integers(0, m))
            if deg[a] < 4:
                deg.append(0)
                add(a, m)
                m += 1
    return renumber(bonds, rng.permutation(n))


def renumber(bonds, perm):
    """bonds with atom a renamed perm[a]."""
    return [(int(perm[a]), int(perm[b])) for a, b in bonds]
