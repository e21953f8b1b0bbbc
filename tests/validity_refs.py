"""Float64 numpy restatement of fabind_amd.validity (csrc/pose_check.hip) on the same float32 inputs and the same definitions, by other
means: breadth-first hop counts instead of set unions, a flood fill for the aromatic systems, `numpy.linalg.eigh` planes,
`numpy.linalg.det` volumes; plus the molecules, poses, pockets and error bounds the tests share.

Bounds (U = 2^-24, the unit roundoff of float32): the kernel works in float64 on the float32 coordinates, so a
finite statistic differs from this restatement by float64 rounding and by ONE rounding to float32 at the store:
* ratios (bond, angle, clash) and ca_dist: 4 U |v| -- U for the store, the rest covers the float64 terms and leaves a factor;
* flatness: 2 U |v| + 1e-7 A -- two backward-stable eigen-solvers on a covariance of norm <= 200 A^2 agree on the normal to
  50 eps64 200 / gap; with atoms within 5 A of the centroid and gap >= 1e-4 A^2 (asserted on every group of every test pose) that is
  5.5e-8 A;
* chirality: 2 U |v| + 1e-9 -- the determinant of float64 differences below 10 A carries at most 1e-13 A^3 against |V0| >= 1 A^3."""
import numpy as np

import conformer_refs as R

U = 2.0 ** -24
MAX_ATOMS = 256
BONDI = {5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 34: 1.90, 35: 1.85, 53: 1.98}
STATS = ("bond_lo", "bond_hi", "angle_lo", "angle_hi", "clash", "flat_aromatic", "flat_double", "chirality", "ca_dist")
BOND, ANGLE, CLASH, AROMATIC_FLAT, DOUBLE_FLAT, CHIRALITY, PROTEIN, NONFINITE, UNCHECKED = 1, 2, 4, 8, 16, 32, 64, 128, 256
DEFAULTS = dict(bond_tol=(0.75, 1.25), angle_tol=(0.75, 1.25), clash_min=0.7, flat_max=0.25, ca_min=None)
OFFSET = np.array([50.0, -50.0, 50.0])
POCKET_COUNTS = (65, 0, 1, 63, 64, 3, 2, 0, 4)      # residues per complex of `world_molecules`: a complex without any between others
CA_MIN = 5.0
MIN_GAP = 1e-4


def bound(col, v):
    v = abs(float(v))
    if col in (5, 6):
        return 2 * U * v + 1e-7
    if col == 7:
        return 2 * U * v + 1e-9
    return 4 * U * v


def threshold_gaps(stats, bond_tol=(0.75, 1.25), angle_tol=(0.75, 1.25), clash_min=0.7, flat_max=0.25, ca_min=None):
    """[(column, value, threshold)] of every comparison `flags` makes on finite statistics."""
    t = [(0, bond_tol[0]), (1, bond_tol[1]), (2, angle_tol[0]), (3, angle_tol[1]), (4, clash_min), (5, flat_max), (6, flat_max), (7, 0.0)]
    if ca_min is not None:
        t.append((8, ca_min))
    return [(c, stats[c], thr) for c, thr in t if np.isfinite(stats[c])]


# ------------------------------------------------------------------------------------------------ plan
def hops(n, nb):
    """h [n, n]: the bond count of the shortest path, 0 on the diagonal, -1 for another fragment (breadth-first from every atom)."""
    h = np.full((n, n), -1, np.int64)
    for s in range(n):
        h[s, s] = 0
        todo = [s]
        while todo:
            nxt = []
            for u in todo:
                for v in nb[u]:
                    if h[s, v] < 0:
                        h[s, v] = h[s, u] + 1
                        nxt.append(v)
            todo = nxt
    return h


def pair_classes(h):
    """0 exempt (self, h = 3), 1 bonded, 2 angle, 3 clash (h >= 4 or another fragment)."""
    c = np.where(h == 1, 1, np.where(h == 2, 2, np.where((h >= 4) | (h < 0), 3, 0)))
    np.fill_diagonal(c, 0)
    return c.astype(np.int64)


def _components(n, edges):
    lab = list(range(n))
    nb = [set() for _ in range(n)]
    for a, b in edges:
        nb[a].add(b); nb[b].add(a)
    seen, out = set(), []
    for r in range(n):
        if r in seen or not nb[r]:
            continue
        comp, todo = {r}, [r]
        while todo:
            u = todo.pop()
            for v in nb[u]:
                if v not in comp:
                    comp.add(v); todo.append(v)
        seen |= comp
        out.append(sorted(comp))
    return out


def signed_volume(x32, c, nbrs):
    """float32 differences, float64 determinant; neighbours ascending."""
    o = x32[c] if len(nbrs) == 3 else x32[nbrs[3]]
    m = np.stack([x32[nbrs[k]] - o for k in range(3)]).astype(np.float64)      # (float32 - float32 is a float32)
    return float(np.linalg.det(m))


def _parity_odd(p):
    return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) % 2 == 1


def plan(m, z, x0, radii=None, min_volume=1.0, autos=None):
    """One ligand.  m: molecule dict (n, bonds, codes); z [n]; x0 float32 [n, 3]; autos: a list of permutations (index arrays), the
    complete automorphism set, or None.  -> dict(status, cls [n, n], pairs [(i, j, kind, d0)], groups [(kind, [atoms])],
    centres [(c, n1, n2, n3, n4 or -1, v0)], radii float32 [n])."""
    n = m["n"]
    x32 = np.asarray(x0, np.float32).reshape(n, 3)
    rad = (np.asarray([BONDI.get(int(a), 2.00) for a in z], np.float32) if radii is None else np.asarray(radii, np.float32)).reshape(n)
    empty = dict(cls=np.zeros((n, n), np.int64), pairs=[], groups=[], centres=[], radii=rad)
    if n > MAX_ATOMS:
        return dict(status=3, **empty)
    nb, code = R._adjacency(n, m["bonds"], m["codes"])
    cls = pair_classes(hops(n, nb))
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            if cls[i, j] in (1, 2):
                d = (x32[i] - x32[j]).astype(np.float64)
                pairs.append((i, j, int(cls[i, j]), float(np.sqrt((d * d).sum()))))
    if any(p[3] == 0.0 for p in pairs):
        return dict(status=5, **empty)
    keyed = []
    for comp in _components(n, [k for k, c in code.items() if c == R.AROMATIC]):
        if len(comp) >= 4:
            keyed.append(((comp[0], 0, 0), (0, comp)))
    for (j, k), c in code.items():
        if c == R.DOUBLE and all(int(z[a]) in (6, 7, 8) and len(nb[a]) <= 3 for a in (j, k)):
            atoms = sorted({j, k} | nb[j] | nb[k])
            if len(atoms) >= 4:
                keyed.append(((j, 1, k), (1, atoms)))
    groups = [g for _, g in sorted(keyed, key=lambda t: t[0])]
    centres = []
    for c in range(n):
        nbrs = sorted(nb[c])
        if len(nbrs) not in (3, 4) or any(code[(min(c, v), max(c, v))] in (R.AROMATIC, R.DOUBLE, R.TRIPLE) for v in nbrs):
            continue
        if int(z[c]) == 7 and len(nbrs) != 4:
            continue
        v0 = signed_volume(x32, c, nbrs)
        if abs(v0) < min_volume:
            continue
        if autos is not None and any(int(a[c]) == c and _parity_odd([nbrs.index(int(a[v])) for v in nbrs]) for a in autos):
            continue
        centres.append(tuple([c] + nbrs + [-1] * (4 - len(nbrs)) + [v0]))
    return dict(status=0, cls=cls, pairs=pairs, groups=groups, centres=centres, radii=rad)


def pack_cls(cls):
    """[n, n] codes -> uint32 [n, 16] words of the device layout."""
    n = len(cls)
    w = np.zeros((n, 16), np.uint64)
    for i in range(n):
        for j in np.nonzero(cls[i])[0]:
            w[i, j >> 4] |= np.uint64(int(cls[i, j]) << (2 * (int(j) & 15)))
    return w.astype(np.uint32)


def batch_plan(plans):
    """The ValidityPlan fields of a list of `plan` results, as numpy arrays in the device layout."""
    B = len(plans)
    offs = np.zeros((4, B + 1), np.int32)
    cls, rad, ij, kind, d0, grp, gat, cen, v0, status = [], [], [], [], [], [], [], [], [], []
    for b, p in enumerate(plans):
        status.append(p["status"])
        n = len(p["radii"])
        cls.append(pack_cls(p["cls"]) if n <= MAX_ATOMS else np.zeros((n, 16), np.uint32))
        rad.append(p["radii"])
        pos = 0
        for i, j, k, d in p["pairs"]:
            ij.append((i, j)); kind.append(k); d0.append(d)
        for k, atoms in p["groups"]:
            grp.append((k, pos, len(atoms))); gat += atoms; pos += len(atoms)
        for c in p["centres"]:
            cen.append(c[:5]); v0.append(c[5])
        offs[:, b + 1] = offs[:, b] + [len(p["pairs"]), len(p["groups"]), pos, len(p["centres"])]
    cat = lambda a, shape, dt: np.asarray(a, dt).reshape(shape)
    return dict(status=cat(status, (B,), np.int32), cls=np.concatenate(cls + [np.zeros((0, 16), np.uint32)]),
                radii=np.concatenate(rad + [np.zeros(0, np.float32)]), offs=offs, pair_ij=cat(ij, (-1, 2), np.int32),
                pair_kind=cat(kind, (-1,), np.int32), pair_d0=cat(d0, (-1,), np.float64), group=cat(grp, (-1, 3), np.int32),
                group_atoms=cat(gat, (-1,), np.int32), centre=cat(cen, (-1, 5), np.int32), centre_v0=cat(v0, (-1,), np.float64))


# ------------------------------------------------------------------------------------------------ the checks
def plane_fit(p):
    """(largest distance from the least-squares plane, gap between the two smallest eigenvalues of the covariance) of p [k, 3]."""
    q = p - p.mean(0)
    w, v = np.linalg.eigh(q.T @ q)
    return float(np.abs(q @ v[:, 0]).max()), float(w[1] - w[0])


def stats(pl, pose, pocket=None):
    """The nine statistics of one pose (float32 [n, 3]) of a ligand with plan `pl`, in float64; NaN rows as the kernel reports them."""
    if pl["status"] != 0 or not np.isfinite(pose).all():
        return np.full(9, np.nan)
    x = np.asarray(pose, np.float32).astype(np.float64)
    n = len(x)
    out = np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, 0.0, 0.0, np.inf, np.inf])
    for i, j, k, d0 in pl["pairs"]:
        q = np.sqrt(((x[i] - x[j]) ** 2).sum()) / d0
        lo = 0 if k == 1 else 2
        out[lo], out[lo + 1] = min(out[lo], q), max(out[lo + 1], q)
    rad = pl["radii"].astype(np.float64)
    ii, jj = np.nonzero(np.triu(pl["cls"] == 3, 1))
    if len(ii):
        out[4] = (np.sqrt(((x[ii] - x[jj]) ** 2).sum(1)) / (rad[ii] + rad[jj])).min()
    for k, atoms in pl["groups"]:
        out[5 + k] = max(out[5 + k], plane_fit(x[atoms])[0])
    for c in pl["centres"]:
        nbrs = [v for v in c[1:5] if v >= 0]
        o = x[c[0]] if len(nbrs) == 3 else x[nbrs[3]]
        out[7] = min(out[7], np.linalg.det(np.stack([x[nbrs[k]] - o for k in range(3)])) / c[5])
    if pocket is not None and len(pocket) and n:
        pk = np.asarray(pocket, np.float32).astype(np.float64)
        out[8] = np.sqrt(((x[:, None, :] - pk[None, :, :]) ** 2).sum(-1)).min()
    return out


def min_gap(pl, pose):
    x = np.asarray(pose, np.float32).astype(np.float64)
    return min([plane_fit(x[atoms])[1] for _, atoms in pl["groups"]] + [np.inf])


def flags(pl, pose, st, bond_tol=(0.75, 1.25), angle_tol=(0.75, 1.25), clash_min=0.7, flat_max=0.25, ca_min=None):
    if pl["status"] != 0:
        return UNCHECKED
    if not np.isfinite(pose).all():
        return NONFINITE
    f = 0
    f |= BOND * bool(st[0] < bond_tol[0] or st[1] > bond_tol[1])
    f |= ANGLE * bool(st[2] < angle_tol[0] or st[3] > angle_tol[1])
    f |= CLASH * bool(st[4] < clash_min)
    f |= AROMATIC_FLAT * bool(st[5] > flat_max)
    f |= DOUBLE_FLAT * bool(st[6] > flat_max)
    f |= CHIRALITY * bool(st[7] <= 0)
    f |= PROTEIN * bool(ca_min is not None and st[8] < ca_min)
    return int(f)


# ------------------------------------------------------------------------------------------------ consumers
def select_valid(rmsd, cdis, conf, valid, top_n):
    """Per complex: the `top_n` most confident valid samples (sample order on ties), filled with the most confident invalid ones;
    -> (min rmsd [B], min centroid distance [B], the picks [top_n, B])."""
    S, B = rmsd.shape
    r, c, picks = np.zeros(B), np.zeros(B), np.zeros((top_n, B), np.int64)
    for b in range(B):
        order = sorted(range(S), key=lambda s: (not valid[s, b], -conf[s, b], s))[:top_n]
        picks[:, b] = order
        r[b], c[b] = rmsd[order, b].min(), cdis[order, b].min()
    return r, c, picks


# ------------------------------------------------------------------------------------------------ molecules, poses, pockets
HAND_Z = {"N-methylacetamide": [6, 6, 8, 7, 6]}


def hand(name):
    m = R.hand_molecules()[name][0]
    return m, np.asarray(HAND_Z.get(name, [6] * m["n"]), np.int64)


def isopentane():
    """2-methylbutane with a tetrahedral C0: swapping the methyls 1 <-> 2 fixes C0 and is an odd permutation of its neighbours."""
    m = R.mol(5, [(0, 1), (0, 2), (0, 3), (3, 4)], name="isopentane")
    a = 1.5 / np.sqrt(3.0)
    m["x"] = np.array([[0, 0, 0], [a, a, a], [a, -a, -a], [-a, a, -a], [-a - 1.2, a + 0.9, -a]], np.float32)
    return m, np.full(5, 6, np.int64)


def automorphisms(m, z):
    """Every label-preserving automorphism of a SMALL molecule, by backtracking."""
    n = m["n"]
    nb, _ = R._adjacency(n, m["bonds"], m["codes"])
    lab = [(int(z[i]), len(nb[i])) for i in range(n)]
    out, a = [], [-1] * n

    def go(i):
        if i == n:
            out.append(np.asarray(a, np.int64))
            return
        for c in range(n):
            if c in a[:i] or lab[c] != lab[i]:
                continue
            if all((a[j] in nb[c]) == (j in nb[i]) for j in range(i)):
                a[i] = c
                go(i + 1)
                a[i] = -1
    go(0)
    return out


def world_molecules(g):
    """The molecules of the statistics tests: the four crystal ligands, three hand molecules (embedded), an empty ligand and a chain
    beyond the atom limit.  -> [(molecule with 'x', z)]."""
    out = [(m, np.asarray(g[m["name"] + "_z"], np.int64)) for m in R.fixture_molecules(g)]
    for k, name in enumerate(("two-fragment", "N-methylacetamide", "biphenyl")):
        m, z = hand(name)
        m["x"] = R.embed(m, seed=40 + k)
        out.append((m, z))
    out.insert(5, (dict(R.mol(0, [], name="empty"), x=np.zeros((0, 3), np.float32)), np.zeros(0, np.int64)))
    big = R.chain(257)
    big["x"] = R.embed(big, seed=50)
    out.append((big, np.full(257, 6, np.int64)))
    return out


N_POSES = 9
POSE_KINDS = ("crystal", "torsion", "stretch", "mirror", "noise0.05", "noise0.5", "aromatic-push", "overlay", "torsion2")


def make_poses(m, pl, seed):
    """The nine test poses of one ligand, float32 [9, n, 3], offset into the protein frame: the start pose, torsion changes, one bond
    stretched by 1.3 (one side translated), the mirror image -x, Gaussian noise of 0.05 A and 0.5 A, one aromatic atom pushed 0.5 A out
    of its plane, one fragment translated onto another, another torsion change.  A kind a ligand has no use for (no rotatable bond, no
    aromatic group, one fragment) falls back to 0.02 A noise with its own seed."""
    rng = np.random.RandomState(seed)
    n = m["n"]
    x = np.asarray(m["x"], np.float64).reshape(n, 3)
    out = np.zeros((N_POSES, n, 3))
    if n == 0 or n > MAX_ATOMS:
        return (out + OFFSET).astype(np.float32)
    quad, side, _ = R.plan(n, m["bonds"], m["codes"])
    nb, _ = R._adjacency(n, m["bonds"], m["codes"])
    fallback = lambda: x + 0.02 * rng.randn(n, 3)

    def torsion():
        if not len(quad):
            return fallback()
        return R.perturb_one(x, quad, side, rng.uniform(-1.5, 1.5, len(quad)), (0, 0, 0), relative=True, rotate=False, centre=False)
    out[0] = x
    out[1] = torsion()
    if len(quad):
        j, k = int(quad[0][1]), int(quad[0][2])
        y = x.copy()
        mv = [a for a in R.side_atoms(side[0]) if a < n]
        y[mv] += 0.3 * (x[k] - x[j])
        out[2] = y
    else:
        out[2] = fallback()
    out[3] = x * np.array([-1.0, 1.0, 1.0])
    out[4] = x + 0.05 * rng.randn(n, 3)
    out[5] = x + 0.5 * rng.randn(n, 3)
    aro = [atoms for k, atoms in pl["groups"] if k == 0]
    if aro:
        q = x[aro[0]] - x[aro[0]].mean(0)
        normal = np.linalg.eigh(q.T @ q)[1][:, 0]
        y = x.copy()
        y[aro[0][0]] += 0.5 * normal
        out[6] = y
    else:
        out[6] = fallback()
    lab = R.rigid_fragments(m, np.zeros((0, 4), np.int64))
    if lab.max() > 0:
        y = x.copy()
        a, b = np.nonzero(lab == 0)[0], np.nonzero(lab == 1)[0]
        y[b] += x[a].mean(0) - x[b].mean(0) + 0.1
        out[7] = y
    else:
        out[7] = fallback()
    out[8] = torsion()
    out = out + OFFSET
    return out.astype(np.float32)


def make_pocket(mols, counts, seed):
    """C-alpha clouds: complex b gets counts[b] points 4-14 A from the centroid of its start pose (in the protein frame).
    -> (xyz float32 [R, 3], batch int64 [R])."""
    rng = np.random.RandomState(seed)
    xyz, batch = [], []
    for b, ((m, _), c) in enumerate(zip(mols, counts)):
        centre = (np.asarray(m["x"], np.float64).mean(0) if m["n"] else np.zeros(3)) + OFFSET
        d = rng.randn(c, 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-30
        xyz.append(centre + d * rng.uniform(4.0, 14.0, (c, 1)))
        batch += [b] * c
    return np.concatenate(xyz + [np.zeros((0, 3))]).astype(np.float32), np.asarray(batch, np.int64)


def check_consumers(dev):
    """`select_valid_by_confidence` and `valid_sampling_metrics` on `dev` against the restatement: ties in the confidence, a complex
    with no valid pose, one with fewer valid poses than top_n, one with all valid."""
    import torch
    from fabind_amd.plus import metrics as M
    rng = np.random.RandomState(9)
    S, B = 7, 6
    rmsd = rng.uniform(0.3, 6.0, (S, B)).astype(np.float32)
    cdis = rng.uniform(0.1, 4.0, (S, B)).astype(np.float32)
    conf = np.round(rng.uniform(0, 1, (S, B)) * 4).astype(np.float32) / 4        # many ties
    valid = rng.rand(S, B) < 0.5
    valid[:, 1] = False
    valid[:, 2] = False
    valid[3, 2] = True
    valid[:, 4] = True
    t = lambda a: torch.as_tensor(a).to(dev)
    for top_n in (1, 3, S):
        r, c = M.select_valid_by_confidence(t(rmsd), t(cdis), t(conf), t(valid), top_n)
        rr, cc, picks = select_valid(rmsd, cdis, conf, valid, top_n)
        np.testing.assert_array_equal(r.cpu().numpy(), rr.astype(np.float32))
        np.testing.assert_array_equal(c.cpu().numpy(), cc.astype(np.float32))
        got = M.valid_sampling_metrics(t(rmsd), t(cdis), t(conf), t(valid), top_n)
        want = {}
        for x, p in ((rr, "rmsd"), (cc, "centroid_dis")):
            want.update({p + "_mean": x.mean(), p + "_2A": (x < 2).mean(), p + "_5A": (x < 5).mean(), p + "_25": np.quantile(x, 0.25),
                         p + "_50": np.quantile(x, 0.5), p + "_75": np.quantile(x, 0.75)})
        top1 = select_valid(rmsd, cdis, conf, np.ones_like(valid), 1)[2][0]
        want["valid_share"] = valid.mean()
        want["top1_valid_share"] = valid[top1, np.arange(B)].mean()
        want["rmsd_lt2_and_valid"] = np.mean([any(valid[s, b] and rmsd[s, b] < 2 for s in picks[:, b]) for b in range(B)])
        assert sorted(got) == sorted(want)
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-6 * max(1.0, abs(want[k])), (top_n, k, got[k], want[k])
    # with every pose valid the choice is select_by_confidence's
    a = M.select_valid_by_confidence(t(rmsd), t(cdis), t(conf), t(np.ones_like(valid)), 2)
    b = M.select_by_confidence(t(rmsd), t(cdis), t(conf), 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
