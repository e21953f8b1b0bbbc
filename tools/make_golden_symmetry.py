"""Writes tests/golden/symmetry_graphs.npz: hand-built ligand graphs, their label-preserving automorphisms, random poses and the
float64 minima the symmetry kernels must reproduce (tests/test_symmetry_cpu.py, tests/test_gpu_symmetry.py).

Graphs are label + bond arrays built here (no RDKit): chains, benzene, neopentane, a bis-CF3 biphenyl, cyclohexane, a salt of two
identical nitrate ions, a single atom, C60 with all labels equal, and drug-like graphs of 60-150 heavy atoms (two of them with
their atoms renumbered at random, so the search order is not the index order).  Labels come from
fabind_amd.symmetry.reference_atom_labels (the reference's atomGetnum).  Expected automorphism sets: networkx GraphMatcher(G, G,
node_match=label equality), sorted lexicographically.  Poses: S = 10 per ligand over a batch of 64 ligands; expected min RMSD,
min Smooth-L1 (beta 1) and their argmins in float64, every pose redrawn until the best score leads the runner-up by 1e-4 relative.

usage (CPU, networkx needed): python tools/make_golden_symmetry.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fabind_amd.symmetry import reference_atom_labels  # noqa: E402

AR, TR, DB, SG = 1, 2, 3, 4
S_POSES, B_LIG = 10, 64


class Mol:
    def __init__(self):
        self.z, self.bonds = [], []

    def atom(self, z, to=None, code=SG):
        self.z.append(z)
        i = len(self.z) - 1
        if to is not None:
            self.bonds.append((to, i, code))
        return i

    def bond(self, i, j, code=SG):
        self.bonds.append((i, j, code))

    def ring(self, size, z=6, code=AR, to=None, to_code=SG):
        first = self.atom(z, to, to_code)
        ids = [first] + [self.atom(z, None) for _ in range(size - 1)]
        for a, b in zip(ids, ids[1:] + ids[:1]):
            self.bond(a, b, code)
        return ids

    def cf3(self, to):
        c = self.atom(6, to)
        for _ in range(3):
            self.atom(9, c)
        return c

    def graph(self):
        e = np.array([(i, j) for i, j, _ in self.bonds], dtype=np.int64).reshape(-1, 2).T
        c = [k for _, _, k in self.bonds]
        lab = reference_atom_labels(self.z, e, c).numpy()
        return lab.astype(np.int32), e.astype(np.int32)


def chain(labels):
    n = len(labels)
    return np.asarray(labels, dtype=np.int32), np.array([np.arange(n - 1), np.arange(1, n)], dtype=np.int32).reshape(2, -1)


def benzene():
    m = Mol()
    m.ring(6)
    return m.graph()


def cyclohexane():
    m = Mol()
    m.ring(6, code=SG)
    return m.graph()


def neopentane():
    m = Mol()
    c = m.atom(6)
    for _ in range(4):
        m.atom(6, c)
    return m.graph()


def bis_cf3_biphenyl():
    m = Mol()
    r1 = m.ring(6)
    r2 = m.ring(6, to=r1[0])
    m.cf3(r1[3])
    m.cf3(r2[3])
    return m.graph()


def nitrate_salt():
    m = Mol()
    for _ in range(2):
        n = m.atom(7)
        m.atom(8, n, DB)
        m.atom(8, n)
        m.atom(8, n)
    return m.graph()


def single_atom():
    return np.array([600], dtype=np.int32), np.zeros((2, 0), dtype=np.int32)


def c60():
    import networkx as nx
    ico = nx.icosahedral_graph()
    ends = {}
    for u, v in ico.edges():
        for a, b in ((u, v), (v, u)):
            ends[(a, b)] = len(ends)
    g = nx.Graph()
    for (a, b), i in ends.items():
        g.add_edge(i, ends[(b, a)])
        for w in ico.neighbors(a):
            if w != b and ico.has_edge(b, w):
                g.add_edge(i, ends[(a, w)])
    order = list(nx.bfs_tree(g, 0))
    ren = {v: i for i, v in enumerate(order)}
    e = np.array([(ren[u], ren[v]) for u, v in g.edges()], dtype=np.int32).T
    assert g.number_of_nodes() == 60 and e.shape[1] == 90
    return np.full(60, 600, dtype=np.int32), e


def druglike(n_target, seed):
    """Rings (aromatic 6 / 5, saturated 6) joined by short chains, with CF3 / methyl / hydroxyl / carbonyl / amide / halogen
    substituents -- mixed labels, a few symmetric groups."""
    rng = np.random.default_rng(seed)
    m = Mol()
    m.ring(6)
    n_cf3 = 0
    while len(m.z) < n_target - 8:
        attach = int(rng.integers(len(m.z)))
        kind = rng.choice(["ring6", "ring5", "sat6", "chain", "cf3", "me", "oh", "co", "amide", "hal"],
                          p=[0.14, 0.08, 0.06, 0.18, 0.06, 0.14, 0.08, 0.08, 0.1, 0.08])
        deg = sum(1 for i, j, _ in m.bonds if attach in (i, j))
        if deg >= 3 or m.z[attach] in (9, 17) or (m.z[attach] == 8 and deg >= 2):
            continue
        if kind == "ring6":
            m.ring(6, to=attach)
        elif kind == "ring5":
            r = m.ring(5, to=attach)
            m.z[r[2]] = 7
        elif kind == "sat6":
            r = m.ring(6, code=SG, to=attach)
            m.z[r[3]] = 7
        elif kind == "chain":
            a = attach
            for _ in range(int(rng.integers(1, 4))):
                a = m.atom(int(rng.choice([6, 6, 6, 7, 8])), a)
        elif kind == "cf3" and n_cf3 < 2:
            m.cf3(attach)
            n_cf3 += 1
        elif kind == "me":
            m.atom(6, attach)
        elif kind == "oh":
            m.atom(8, attach)
        elif kind == "co":
            m.atom(8, attach, DB)
        elif kind == "amide":
            c = m.atom(6, attach)
            m.atom(8, c, DB)
            m.atom(7, c)
        elif kind == "hal":
            m.atom(int(rng.choice([9, 17])), attach)
    return m.graph()


def shuffled(g, seed):
    lab, e = g
    p = np.random.default_rng(seed).permutation(len(lab))       # new id of old atom i = p[i]
    lab2 = np.empty_like(lab)
    lab2[p] = lab
    return lab2, p[e].astype(np.int32)


def automorphisms_networkx(lab, e):
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
    g = nx.Graph()
    g.add_nodes_from((i, {"l": int(x)}) for i, x in enumerate(lab))
    g.add_edges_from(map(tuple, e.T.tolist()))
    gm = GraphMatcher(g, g, node_match=lambda a, b: a["l"] == b["l"])
    autos = sorted(tuple(m[i] for i in range(len(lab))) for m in gm.isomorphisms_iter())
    return np.array(autos, dtype=np.int32).reshape(len(autos), len(lab))


def sl1(x):
    a = np.abs(x)
    return np.where(a < 1.0, 0.5 * x * x, a - 0.5)


def scores(pred, true, autos):
    d = pred[autos].astype(np.float64) - true.astype(np.float64)[None]        # [K, n, 3]
    n = true.shape[0]
    return np.sqrt((d ** 2).sum(-1).sum(-1) / n), sl1(d).sum(-1).sum(-1) / (3 * n)


def tie_free(v):
    if len(v) < 2:
        return True
    s = np.sort(v)
    return s[1] - s[0] > 1e-4 * abs(s[0])


def main(out):
    graphs = [("chain_mixed", chain([604, 608, 608, 804])), ("chain_equal", chain([600] * 7)), ("benzene", benzene()),
              ("neopentane", neopentane()), ("bis_cf3_biphenyl", bis_cf3_biphenyl()), ("cyclohexane", cyclohexane()),
              ("nitrate_salt", nitrate_salt()), ("single_atom", single_atom()), ("c60", c60())]
    for i, n in enumerate((68, 98, 128, 156)):
        g = druglike(n, 100 + i)
        graphs.append(("druglike_%d" % len(g[0]), g))
    graphs.append((graphs[-3][0] + "_shuffled", shuffled(graphs[-3][1], 7)))
    graphs.append((graphs[-2][0] + "_shuffled", shuffled(graphs[-2][1], 8)))
    res = {"names": np.array([g[0] for g in graphs])}
    for gi, (name, (lab, e)) in enumerate(graphs):
        a = automorphisms_networkx(lab, e)
        print("%-22s n=%3d bonds=%3d K=%d" % (name, len(lab), e.shape[1], len(a)))
        res["g%d_labels" % gi], res["g%d_bonds" % gi], res["g%d_autos" % gi] = lab, e, a
    rng = np.random.default_rng(2026)
    gid = np.arange(B_LIG) % len(graphs)
    trues, preds = [], []
    exp = {k: np.zeros((S_POSES, B_LIG), dtype=t) for k, t in (("rmsd", np.float64), ("sl1", np.float64), ("arg_rmsd", np.int32),
                                                                 ("arg_sl1", np.int32))}
    for b, g in enumerate(gid):
        autos = res["g%d_autos" % g]
        n = autos.shape[1]
        true = (3.0 * rng.standard_normal((n, 3))).astype(np.float32)
        ps = np.zeros((S_POSES, n, 3), dtype=np.float32)
        for s in range(S_POSES):
            while True:
                k = int(rng.integers(len(autos)))
                p = np.empty((n, 3), dtype=np.float32)
                p[autos[k]] = true + (0.8 * rng.standard_normal((n, 3))).astype(np.float32)     # pred[a_k[i]] ~ true[i]
                r, l1 = scores(p, true, autos)
                if tie_free(r) and tie_free(l1):
                    break
            ps[s] = p
            exp["rmsd"][s, b], exp["arg_rmsd"][s, b] = r.min(), int(np.argmin(r))
            exp["sl1"][s, b], exp["arg_sl1"][s, b] = l1.min(), int(np.argmin(l1))
        trues.append(true)
        preds.append(ps)
    res["batch_graph"] = gid.astype(np.int32)
    res["true"] = np.concatenate(trues, 0)
    res["pred"] = np.concatenate(preds, 1)
    for k, v in exp.items():
        res["exp_" + k] = v
    np.savez_compressed(out, **res)
    print("wrote %s (%d bytes, %d atoms in the pose batch)" % (out, os.path.getsize(out), res["true"].shape[0]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "symmetry_graphs.npz"))
