"""Numpy restatement of fabind_amd.conformer (csrc/conformer.hip), float64 by default and float32 on request: the torsion plan
(depth-first bridges + component masks -- another algorithm than the kernel's flood fill per candidate), the dihedral setter, the
rotation M = -(H R) of the reference's uniform_random_rotation (utils/utils.py:45-81) and the hash-based draws; plus the
hand-written molecules, chains and the plain-text V2000 reader the tests share."""
import numpy as np

AROMATIC, TRIPLE, DOUBLE, SINGLE, OTHER = 1, 2, 3, 4, 5
MAX_ATOMS = 256
DIST_SEED = 2024          # the seed of the GPU distribution test; tests/test_conformer_refs_cpu.py checks it on the restated draws
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ draws
def hash32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def uniform(seed, key, copy, draw):
    """u(seed, key, copy, draw) of csrc/conformer.hip::cf_uniform: the top 24 bits of four chained hash rounds, in [0, 1)."""
    seed, key, copy, draw = int(seed), int(key), int(copy), int(draw)
    h = hash32((seed & M32) + 0x9e3779b9)
    h = hash32((h ^ (key & M32)) + 0x85ebca6b)
    h = hash32((h ^ (copy & M32)) + 0xc2b2ae35)
    h = hash32((h ^ (draw & M32)) + 0x27d4eb2f)
    return (h >> 8) / 16777216.0


def drawn_inputs(seed, keys, n_copies, tor_counts):
    """(angles [S, T_total], uniforms [S, B, 3] = (x1, x2, x3)) the kernel draws: torsion t of ligand b is draw t, then x2, x3, x1."""
    B, T = len(tor_counts), int(sum(tor_counts))
    ang, uni = np.zeros((n_copies, T), np.float32), np.zeros((n_copies, B, 3), np.float32)
    for s in range(n_copies):
        t0 = 0
        for b, tb in enumerate(tor_counts):
            for t in range(tb):
                ang[s, t0 + t] = np.float32(6.28318530717958647692) * np.float32(uniform(seed, keys[b], s, t))
            uni[s, b, 1], uni[s, b, 2], uni[s, b, 0] = (uniform(seed, keys[b], s, tb + d) for d in range(3))
            t0 += tb
    return ang, uni


# ------------------------------------------------------------------------------------------------ plan
def _adjacency(n, bonds, codes):
    nb = [set() for _ in range(n)]
    code = {}
    for (a, b), c in zip(np.asarray(bonds, np.int64).reshape(-1, 2), np.asarray(codes, np.int64).reshape(-1)):
        a, b = int(a), int(b)
        if a == b:
            continue
        nb[a].add(b)
        nb[b].add(a)
        k = (min(a, b), max(a, b))
        code[k] = min(code.get(k, 1 << 30), int(c))
    return nb, code


def _bridges(n, nb):
    """Bridges of an undirected simple graph (iterative depth-first search, low-link)."""
    disc, low, out, t = [-1] * n, [0] * n, set(), 0
    for r in range(n):
        if disc[r] >= 0:
            continue
        disc[r] = low[r] = t
        t += 1
        stack = [(r, -1, iter(sorted(nb[r])))]
        while stack:
            u, p, it = stack[-1]
            adv = False
            for v in it:
                if v == p:
                    continue
                if disc[v] >= 0:
                    low[u] = min(low[u], disc[v])
                else:
                    disc[v] = low[v] = t
                    t += 1
                    stack.append((v, u, iter(sorted(nb[v]))))
                    adv = True
                    break
            if not adv:
                stack.pop()
                if p >= 0:
                    low[p] = min(low[p], low[u])
                    if low[u] > disc[p]:
                        out.add((min(u, p), max(u, p)))
    return out


def plan(n, bonds, codes):
    """-> (quad int32 [T, 4], side uint32 [T, 8], status).  bonds [E, 2] local ids (any direction, duplicates allowed)."""
    if n > MAX_ATOMS:
        return np.zeros((0, 4), np.int32), np.zeros((0, 8), np.uint32), 3
    nb, code = _adjacency(n, bonds, codes)
    triple = [any(code[(min(a, b), max(a, b))] == TRIPLE for b in nb[a]) for a in range(n)]
    br = _bridges(n, nb)
    quads, sides = [], []
    for (j, k) in sorted(code):
        if code[(j, k)] != SINGLE or len(nb[j]) < 2 or len(nb[k]) < 2 or triple[j] or triple[k] or (j, k) not in br:
            continue
        seen, todo = {k}, [k]
        while todo:
            u = todo.pop()
            for v in nb[u]:
                if v not in seen and not (u == k and v == j):
                    seen.add(v)
                    todo.append(v)
        assert j not in seen
        w = np.zeros(8, np.uint32)
        for a in seen:
            w[a >> 5] |= np.uint32(1 << (a & 31))
        quads.append((min(nb[j] - {k}), j, k, min(nb[k] - {j})))
        sides.append(w)
    return (np.asarray(quads, np.int32).reshape(-1, 4), np.asarray(sides, np.uint32).reshape(-1, 8), 0)


def side_atoms(words):
    return [a for a in range(256) if (int(words[a >> 5]) >> (a & 31)) & 1]


def batch_plan(mols):
    """The restated TorsionPlan of a list of molecules (dicts with n, bonds, codes): quad, side, off, status."""
    qs, ss, off, st = [], [], [0], []
    for m in mols:
        q, s, status = plan(m["n"], m["bonds"], m["codes"])
        qs.append(q); ss.append(s); st.append(status); off.append(off[-1] + len(q))
    return np.concatenate(qs), np.concatenate(ss), np.asarray(off, np.int32), np.asarray(st, np.int32)


# ------------------------------------------------------------------------------------------------ geometry
def dihedral(p, q, dt=np.float64):
    """IUPAC dihedral of atoms q = (i, j, k, l) of p [n, 3], in dtype dt; (angle, degenerate)."""
    p = np.asarray(p, dt)
    b1, b2, b3 = p[q[1]] - p[q[0]], p[q[2]] - p[q[1]], p[q[3]] - p[q[2]]
    n1, n2 = np.cross(b1, b2).astype(dt), np.cross(b2, b3).astype(dt)
    l1, l2, l3 = dt(b1 @ b1), dt(b2 @ b2), dt(b3 @ b3)
    if not (dt(n1 @ n1) > dt(1e-8) * l1 * l2 and dt(n2 @ n2) > dt(1e-8) * l2 * l3):
        return dt(0), True
    y = dt(np.cross(n1, n2).astype(dt) @ b2) / np.sqrt(l2)
    return dt(np.arctan2(y, dt(n1 @ n2))), False


def rotation_matrix(x1, x2, x3, dt=np.float64):
    """M = -(H R) exactly as utils/utils.py:58-78 builds it from the three uniforms."""
    tp = dt(2 * np.pi)
    x1, x2, x3 = dt(x1), dt(x2), dt(x3)
    R = np.eye(3, dtype=dt)
    R[0, 0] = R[1, 1] = np.cos(tp * x1)
    R[0, 1] = -np.sin(tp * x1)
    R[1, 0] = np.sin(tp * x1)
    v = np.array([np.cos(tp * x2) * np.sqrt(x3), np.sin(tp * x2) * np.sqrt(x3), np.sqrt(dt(1) - x3)], dtype=dt)
    H = np.eye(3, dtype=dt) - dt(2) * np.outer(v, v)
    return (-(H @ R)).astype(dt)


def perturb_one(x, quad, side, angles, uni, relative=False, rotate=True, centre=True, dt=np.float64):
    """One ligand, one copy.  x [n, 3]; quad [T, 4] / side [T, 8]; angles [T] target dihedrals; uni = (x1, x2, x3)."""
    p = np.array(x, dtype=dt)
    n = len(p)
    for t in range(len(quad)):
        q = [int(v) for v in quad[t]]
        axis = p[q[2]] - p[q[1]]
        l2 = dt(axis @ axis)
        if l2 == 0:
            continue
        theta = dt(angles[t])
        if not relative:
            theta = dt(theta - dihedral(p, q, dt)[0])
        u = (axis / np.sqrt(l2)).astype(dt)
        cs, sn = dt(np.cos(theta)), dt(np.sin(theta))
        idx = [a for a in side_atoms(side[t]) if a < n and a != q[2]]
        if idx:
            v = p[idx] - p[q[1]]
            d = (v @ u)[:, None].astype(dt) * (dt(1) - cs)
            p[idx] = (p[q[1]] + (v * cs + np.cross(u[None, :], v).astype(dt) * sn + u[None, :] * d)).astype(dt)
    mean = p.mean(axis=0, dtype=dt)
    M = rotation_matrix(uni[0], uni[1], uni[2], dt) if rotate else np.eye(3, dtype=dt)
    out = (p - mean) @ M
    if not centre:
        out = out + mean @ M
    return out.astype(dt)


def perturb(x, atom_off, quad, side, off, angles, uniforms, relative=False, rotate=True, centre=True, dt=np.float64):
    """The whole call: x [N, 3]; angles [S, T_total]; uniforms [S, B, 3] -> [S, N, 3] in dtype dt."""
    S, B = len(uniforms), len(atom_off) - 1
    out = np.zeros((S, len(x), 3), dt)
    for s in range(S):
        for b in range(B):
            a0, a1, t0, t1 = atom_off[b], atom_off[b + 1], off[b], off[b + 1]
            if a1 > a0:
                out[s, a0:a1] = perturb_one(x[a0:a1], quad[t0:t1], side[t0:t1], angles[s, t0:t1], uniforms[s, b], relative, rotate,
                                            centre, dt)
    return out


# ------------------------------------------------------------------------------------------------ molecules
def mol(n, bonds, codes=None, name=""):
    bonds = np.asarray(bonds, np.int64).reshape(-1, 2)
    codes = np.full(len(bonds), SINGLE, np.int64) if codes is None else np.asarray(codes, np.int64)
    return dict(n=n, bonds=bonds, codes=codes, name=name)


def chain(n):
    return mol(n, [(i, i + 1) for i in range(n - 1)], name="chain%d" % n)


def hand_molecules():
    """name -> (molecule, the expected rotatable bonds as {(j, k): sorted side atoms}), known by inspection."""
    S, D, T, A = SINGLE, DOUBLE, TRIPLE, AROMATIC
    ring6 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5)]
    out = {
        "ethane": (chain(2), {}),
        "propane": (chain(3), {}),
        "butane": (chain(4), {(1, 2): [2, 3]}),
        # HC#C-CH2-CH2-CH3: C1#C2, C2-C3 (C2 has a triple bond), C3-C4 rotatable, C4-C5 (C5 terminal)
        "pent-1-yne": (mol(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [T, S, S, S]), {(2, 3): [3, 4]}),
        "but-1-yne": (mol(4, [(0, 1), (1, 2), (2, 3)], [T, S, S]), {}),
        "but-2-ene": (mol(4, [(0, 1), (1, 2), (2, 3)], [S, D, S]), {}),
        "cyclohexane": (mol(6, ring6), {}),
        "decalin": (mol(10, ring6 + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 0)]), {}),
        "ethylcyclohexane": (mol(8, ring6 + [(0, 6), (6, 7)]), {(0, 6): [6, 7]}),
        "biphenyl": (mol(12, ring6 + [(6, 7), (7, 8), (8, 9), (9, 10), (10, 11), (6, 11), (0, 6)], [A] * 6 + [A] * 6 + [S]),
                     {(0, 6): [6, 7, 8, 9, 10, 11]}),
        # CH3-C(=O)-NH-CH3, heavy atoms C0 C1 O2 N3 C4
        "N-methylacetamide": (mol(5, [(0, 1), (1, 2), (1, 3), (3, 4)], [S, D, S, S]), {(1, 3): [3, 4]}),
        # butane + pentane in one ligand (disconnected): atoms 0-3 and 4-8
        "two-fragment": (mol(9, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7), (7, 8)]), {(1, 2): [2, 3], (5, 6): [6, 7, 8], (6, 7): [7, 8]}),
    }
    for k, (m, _) in out.items():
        m["name"] = k
    return out


def embed(m, seed=0):
    """Coordinates for a molecule graph: a seeded depth-first placement with 1.5 A bonds, bond angles near 110 degrees and random
    dihedrals (rings are not closed geometrically: the tests use distances of the INPUT as their truth, not chemistry)."""
    rng = np.random.RandomState(seed)
    n = m["n"]
    nb, _ = _adjacency(n, m["bonds"], m["codes"])
    x, placed, parent = np.zeros((n, 3)), [False] * n, [-1] * n
    for r in range(n):
        if placed[r]:
            continue
        x[r] = rng.randn(3) * 3.0
        placed[r] = True
        stack = [r]
        while stack:
            u = stack.pop()
            for v in sorted(nb[u]):
                if placed[v]:
                    continue
                if parent[u] < 0:
                    d = rng.randn(3)
                else:
                    back = x[parent[u]] - x[u]
                    back /= np.linalg.norm(back)
                    perp = np.cross(back, rng.randn(3))
                    perp /= np.linalg.norm(perp)
                    ang = np.deg2rad(110.0 + rng.uniform(-8, 8))
                    d = np.cos(ang) * back + np.sin(ang) * perp
                x[v] = x[u] + 1.5 * d / np.linalg.norm(d)
                placed[v], parent[v] = True, u
                stack.append(v)
    return x.astype(np.float32)


def pack(mols, coords=None):
    """A list of molecules as one batch: (x [N, 3] float32, bond_index [2, E] global int64, codes [E], atom_off [B + 1])."""
    off = np.concatenate([[0], np.cumsum([m["n"] for m in mols])]).astype(np.int64)
    bi = np.concatenate([m["bonds"] + off[i] for i, m in enumerate(mols)] + [np.zeros((0, 2), np.int64)]).T
    codes = np.concatenate([m["codes"] for m in mols] + [np.zeros(0, np.int64)])
    if coords is None:
        coords = [m["x"] if "x" in m else embed(m, seed=17 + i) for i, m in enumerate(mols)]
    x = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in coords] + [np.zeros((0, 3), np.float32)])
    return x, bi, codes, off.astype(np.int32)


# ------------------------------------------------------------------------------------------------ V2000
V2000_CODE = {1: SINGLE, 2: DOUBLE, 3: TRIPLE, 4: AROMATIC}


def parse_v2000(text):
    """Heavy atoms of the first molecule of an SDF / MOL file (fixed-column V2000 counts, atom and bond blocks) -> (symbols,
    coords [n, 3] float64, bonds [E, 2] local ids among the heavy atoms, codes [E])."""
    lines = text.splitlines()
    na, nbd = int(lines[3][0:3]), int(lines[3][3:6])
    sym, xyz = [], []
    for ln in lines[4:4 + na]:
        xyz.append([float(ln[0:10]), float(ln[10:20]), float(ln[20:30])])
        sym.append(ln[31:34].strip())
    heavy = [i for i, s in enumerate(sym) if s not in ("H", "D")]
    new = {old: i for i, old in enumerate(heavy)}
    bonds, codes = [], []
    for ln in lines[4 + na:4 + na + nbd]:
        a, b, t = int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])
        if a in new and b in new:
            bonds.append((new[a], new[b]))
            codes.append(V2000_CODE.get(t, OTHER))
    return [sym[i] for i in heavy], np.asarray(xyz)[heavy], np.asarray(bonds, np.int64).reshape(-1, 2), np.asarray(codes, np.int64)


def fixture_molecules(g):
    """The ligands of tests/golden/conformer_ligands.npz as molecule dicts (with their crystal coordinates under 'x')."""
    out = []
    for name in [str(s) for s in g["names"]]:
        m = mol(len(g[name + "_z"]), g[name + "_bonds"], g[name + "_codes"], name)
        m["x"] = g[name + "_xyz"].astype(np.float32)
        out.append(m)
    return out


def bonded_and_13_pairs(m):
    nb, _ = _adjacency(m["n"], m["bonds"], m["codes"])
    pairs = set()
    for a in range(m["n"]):
        for b in nb[a]:
            pairs.add((min(a, b), max(a, b)))
            for c in nb[b]:
                if c != a:
                    pairs.add((min(a, c), max(a, c)))
    return np.asarray(sorted(pairs), np.int64).reshape(-1, 2)


def rigid_fragments(m, quad):
    """Atom labels of the rigid fragments: the components once every rotatable bond of `quad` is removed."""
    nb, _ = _adjacency(m["n"], m["bonds"], m["codes"])
    cut = {(int(q[1]), int(q[2])) for q in quad}
    lab, c = [-1] * m["n"], 0
    for r in range(m["n"]):
        if lab[r] >= 0:
            continue
        lab[r], todo = c, [r]
        while todo:
            u = todo.pop()
            for v in nb[u]:
                if lab[v] < 0 and (min(u, v), max(u, v)) not in cut:
                    lab[v] = c
                    todo.append(v)
        c += 1
    return np.asarray(lab)
