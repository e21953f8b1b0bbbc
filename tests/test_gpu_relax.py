"""GPU: fabind_amd.relax.relax_poses (csrc/pose_relax.hip) -- sampled poses relaxed out of protein and internal clashes over the
ligand's torsions and one rigid motion -- against the numpy restatement of tests/relax_refs.py (pinned on the CPU by
tests/test_relax_refs_cpu.py, its results on the committed cases recorded in tests/golden/relax_cases.npz) and against invariants that
hold by construction.

Bounds, written down before the device was consulted (u = 2^-24):
* molecule: `pass_bound` + `rmsd_bound` of tests/test_gpu_conformer_fit.py (two float32 torsion passes with the same angles, rigidly
  aligned, and the float32 store), with rho the largest distance from the origin of the frames involved.  A bonded or 1-3 pair lies in
  one rigid fragment or has one atom on the axis that moves the other, so its distance is the start conformer's up to the position error
  of its two atoms: the same bound.
* energies: the kernel evaluates E on its float32 pose in the frame of the target's centroid and stores float32(pose + centroid); the
  restatement evaluates E on the stored coordinates.  The store moves every component by at most u rho (rho the largest stored
  component), so each of the three sums moves by at most u rho |d sum / dX|_1 to first order; the second order is at most
  3 (u rho)^2 per term for n + 8 m terms (m pairs within reach + 0.01 A; a pair's distance is 1-Lipschitz and its curvature 1 / d with
  d >= reach / 8 assumed); the sums themselves are float64 sums of at most a few thousand terms in another order: 2^-40 relative.
  `energy_bound` = 1.001 u rho L1 + 3 (u rho)^2 (n + 8 m) + 2^-40 sum.
* restatement: the device's final E within 4 x the yardstick max |E32 - E64| of the float32-pose restatement on the committed cases.
Every test prints its largest fraction of its bound before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import conformer_refs as R
import contact_refs as C
import fit_refs as F
import relax_refs as X
import validity_refs as V
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
FIELDS = ("coords", "angles", "energy0", "energy", "iters", "stop", "trace")


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _radius(*clouds):
    return max([float(np.abs(c).max()) * np.sqrt(3.0) for c in clouds if len(c)] + [0.0])


def pass_bound(T, rho):
    return 2.0 * U * rho * (100.0 * T + 16.0)


def rmsd_bound(rho, rmsd):
    return 4.0 * U * (rho + rmsd)


def rigid_bound(rho_in, rho_out):
    return 16.0 * U * (rho_in + rho_out)


def energy_bound(rho, l1, n, m, value):
    return 1.001 * U * rho * l1 + 3.0 * (U * rho) ** 2 * (n + 8 * m) + 2.0 ** -40 * abs(value)


class _Batch:
    """A list of complexes on the device: ligands (molecule, z, start conformer) with their torsion and validity plans, proteins with
    their grid, and the restated plans next to them."""

    def __init__(self, mols, zs, xs, prots):
        from fabind_amd import conformer, validity
        self.mols, self.zs, self.prots = mols, zs, prots
        self.x, bi, codes, self.off = R.pack(mols, coords=xs)
        self.bi, self.codes = bi, codes
        self.tp = conformer.rotatable_bonds(_t(bi), _t(codes), self.off, on_overflow="truncate")
        self.vp = validity.validity_plan(_t(bi), _t(codes), _t(np.concatenate(zs + [np.zeros(0, np.int64)])), _t(self.x), self.off,
                                         on_overflow="skip")
        self.poff = np.concatenate([[0], np.cumsum([len(p[1]) for p in prots])]).astype(np.int32)
        pxyz = np.concatenate([p[0] for p in prots] + [np.zeros((0, 3), np.float32)]).astype(np.float32)
        pz = np.concatenate([p[1] for p in prots] + [np.zeros(0, np.int64)])
        self.grid = validity.protein_grid(_t(pxyz), _t(pz), self.poff, on_overflow="skip")
        self.quad, self.side, self.toff, _ = R.batch_plan(mols)
        self.T = np.diff(self.toff)
        self.B, self.N = len(mols), len(self.x)
        self.vplans = [V.plan(m, z, self.x[self.sl(b)]) for b, (m, z) in enumerate(zip(mols, zs))]
        self.kept = [C.kept(p[0], p[1])[:2] for p in prots]
        self.gstatus = [0 if np.isfinite(p[0]).all() else 6 for p in prots]

    def sl(self, b):
        return slice(self.off[b], self.off[b + 1])

    def tl(self, b):
        return slice(self.toff[b], self.toff[b + 1])

    def relax(self, y, **kw):
        from fabind_amd import relax
        kw.setdefault("on_overflow", "truncate")
        kw.setdefault("return_trace", True)
        return relax.relax_poses(_t(self.x), _t(y), self.tp, self.vp, self.grid, **kw)

    def energy_of(self, b, coords, y, **kw):
        """The restatement's three sums on given coordinates, and per sum (|d sum / dX|_1, pairs within reach + 0.01 A)."""
        vpl = self.vplans[b]
        args = (coords, y, vpl["cls"], vpl["radii"], self.kept[b][0], self.kept[b][1], vpl["status"], self.gstatus[b])
        sums, _ = X.energy_of(*args, **kw)
        l1 = [X.energy_of(*args, **dict(kw, w_fit=float(k == 0), w_prot=float(k == 1), w_intra=float(k == 2)))[1] for k in range(3)]
        near, _ = X.energy_of(coords, y, vpl["cls"], vpl["radii"] + np.float32(0.01), self.kept[b][0], self.kept[b][1] + np.float32(0.01),
                              vpl["status"], self.gstatus[b], **kw)
        n = len(coords)
        pairs = n * len(self.kept[b][0]) + n * n                         # (an upper count of the pairs: the bound only has to hold)
        return sums, l1, [0, pairs if near[1] > 0 else 0, pairs if near[2] > 0 else 0]


def host(out):
    return {f: getattr(out, f).cpu().numpy() for f in FIELDS + ("status",) if getattr(out, f) is not None}


# ------------------------------------------------------------------------------------------------ the two worlds
class _Cases:
    """The 14 complexes of relax_refs.complexes with their three targets each; the committed cases start at the recorded angles."""

    def __init__(self):
        g = load_npz("conformer_ligands")
        self.gold = load_npz("relax_cases")
        self.cx = X.complexes(g)
        self.b = _Batch([c["mol"] for c in self.cx], [c["z"] for c in self.cx], [c["mol"]["x"] for c in self.cx],
                        [(c["prot_xyz"], c["prot_z"]) for c in self.cx])
        S = X.TARGETS_PER_MOLECULE
        self.y = np.zeros((S, self.b.N, 3), np.float32)
        self.a0 = np.zeros((S, int(self.b.toff[-1])), np.float32)
        for k, c in enumerate(self.cx):
            for s in range(S):
                self.y[s, self.b.sl(k)] = X.make_target(c, X.target_seed(k, s))
        for i, (k, s) in enumerate(self.gold["cases"]):
            self.a0[s, self.b.tl(k)] = self.gold["angles0"][self.gold["angle_off"][i]:self.gold["angle_off"][i + 1]]
        self.out = self.b.relax(self.y, angles0=self.a0)
        self.h = host(self.out)


SHAPE_CHAINS = (1, 2, 3, 8, 32, 60, 61, 62, 63, 64, 65, 256, 257)
KINDS = ("inside", "surface", "coincident", "outside+x", "pocket-a", "outside+y", "pocket-b", "outside+z-corner", "beyond")


class _Shapes:
    """Chains of 1 .. 257 atoms (T = 0, 57, 58, 59 and beyond), an empty ligand, two recorded ligands (the second against a protein with
    a NaN coordinate), the first again in a frame offset by 50 A, and a butane with two coincident bonded atoms (validity status 5);
    proteins of 0, 1 and 600 heavy atoms with hydrogens interleaved, each with its pocket carved; nine targets each (KINDS).  The start
    conformers sit on a grid of 1 / 64 A and the "inside" target is the conformer shifted by whole angstroms."""

    def __init__(self):
        g = load_npz("conformer_ligands")
        fx = R.fixture_molecules(g)[:2]
        mols = [R.chain(n) for n in SHAPE_CHAINS] + [R.mol(0, [], name="empty")] + fx + [dict(fx[0], name=fx[0]["name"] + "+50"),
                                                                                          dict(R.chain(4), name="coincident")]
        zs, xs, prots, ys = [], [], [], []
        for k, m in enumerate(mols):
            z = X.atomic_numbers(dict(m, name=m["name"].split("+")[0]), g)
            # coordinates on a grid of 1 / 64 A: with n a power of two the centred conformer is exact in float32 (test 5)
            x = (np.round(np.asarray(m["x"] if "x" in m else R.embed(m, seed=100 + k), np.float64).reshape(-1, 3) * 64.0) / 64.0).astype(np.float32)
            if m["name"] == "coincident":
                x[1] = x[0]
            q, sd, _ = R.plan(m["n"], m["bonds"], m["codes"])
            shift = (50.0, -50.0, 50.0) if m["name"].endswith("+50") else (-7.5, -3.0, 0.0)
            nprot = 0 if k == 0 else 1 if k == 1 else 600
            pxyz, pz = C.synthetic_protein(max(nprot, 1), seed=400 + k, hydrogens=0.5 if nprot > 1 else 0.0, origin=shift)
            poses = C.poses_for(x, pxyz, pz, seed=500 + k)
            if m["n"]:                                                   # "inside": the conformer shifted by whole angstroms, exactly
                poses[0] = x + np.round(poses[0].astype(np.float64).mean(0) - x.astype(np.float64).mean(0)).astype(np.float32)
            rl = V.plan(m, z, x)["radii"]
            if nprot > 1 and m["n"]:
                pxyz, pz = X.carve(pxyz, pz, poses[0], rl)
            if nprot == 1 and m["n"]:
                pxyz = (poses[0][:1] + np.float32([2.5, 0.0, 0.0])).astype(np.float32)
            if nprot == 0:
                pxyz, pz = pxyz[:0], pz[:0]
            if m["n"]:
                c = dict(mol=dict(m, quad=q, side=sd), placed=poses[0])
                poses[4], poses[6] = X.make_target(c, 900 + k), X.make_target(c, 950 + k)
            if m["name"] == fx[1]["name"]:                               # the second recorded ligand: a protein the grid refuses
                pxyz = pxyz.copy()
                pxyz[3, 1] = np.nan
            zs.append(z); xs.append(x); prots.append((pxyz, pz)); ys.append(poses)
        self.b = _Batch(mols, zs, xs, prots)
        self.y = np.concatenate(ys, 1).astype(np.float32)
        self.out = self.b.relax(self.y)
        self.h = host(self.out)
        self.start = self.b.relax(self.y, max_iters=0)
        self.h0 = host(self.start)


@pytest.fixture(scope="module")
def cases():
    return _Cases()


@pytest.fixture(scope="module")
def shapes():
    return _Shapes()


def _worlds(cases, shapes):
    return (("cases", cases), ("shapes", shapes))


# ------------------------------------------------------------------------------------------------ 1. still the molecule
def test_coords_are_the_start_conformer_under_the_returned_angles(cases, shapes):
    from fabind_amd import conformer
    worst, worst_d = 0.0, 0.0
    for name, w in _worlds(cases, shapes):
        b, h = w.b, w.h
        S = h["coords"].shape[0]
        assert np.abs(h["angles"]).max(initial=0) <= np.float32(np.pi) and np.isfinite(h["angles"]).all() and np.isfinite(h["coords"]).all()
        pert = conformer.perturb_conformers(_t(b.x), b.tp, n_copies=S, angles=w.out.angles, relative=True, random_rotation=False,
                                            centre=False).cpu().numpy().astype(np.float64)
        for k, m in enumerate(b.mols):
            if not m["n"]:
                continue
            x0 = b.x[b.sl(k)].astype(np.float64)
            pairs = R.bonded_and_13_pairs(m)
            d0 = np.linalg.norm(x0[pairs[:, 0]] - x0[pairs[:, 1]], axis=1) if len(pairs) else np.zeros(0)
            for s in range(S):
                c, p = h["coords"][s, b.sl(k)].astype(np.float64), pert[s, b.sl(k)]
                rho = _radius(x0, c - c.mean(0), p)
                bound = pass_bound(b.T[k], rho) + rmsd_bound(_radius(c), 0.0)
                got = F.rmsd(F.rigid_image(p, c), c)
                worst = max(worst, got / bound)
                assert got <= bound, (name, s, m["name"], got, bound)
                if len(pairs):
                    dd = np.abs(np.linalg.norm(c[pairs[:, 0]] - c[pairs[:, 1]], axis=1) - d0).max()
                    worst_d = max(worst_d, dd / bound)
                    assert dd <= bound, (name, s, m["name"], dd, bound)
                if (h["status"][k] & 7) != 0:
                    assert not h["angles"][s, b.tl(k)].any()
    print("molecule: largest fraction of the bound %.4f (aligned RMSD), %.4f (bonded and 1-3 distances)" % (worst, worst_d))


# ------------------------------------------------------------------------------------------------ 2. energies and trace
def test_energies_are_those_of_the_stored_coordinates(cases, shapes):
    worst = 0.0
    for name, w in _worlds(cases, shapes):
        b = w.b
        runs = [(w.h, "energy")] + ([(w.h0, "energy")] if name == "shapes" else [])
        for h, field in runs:
            S = h["coords"].shape[0]
            for k, m in enumerate(b.mols):
                for s in range(S):
                    got = h[field][s, k]
                    if not m["n"]:
                        assert (got == 0).all() and (h["energy0"][s, k] == 0).all()
                        continue
                    c, y = h["coords"][s, b.sl(k)].astype(np.float64), w.y[s, b.sl(k)].astype(np.float64)
                    if (h["status"][k] & 7) == 3:
                        assert np.isnan(got[1:]).all() and np.isnan(h["energy0"][s, k, 1:]).all() and got[0] == h["energy0"][s, k, 0]
                        want = ((c - y) ** 2).sum()
                        assert abs(got[0] - want) <= energy_bound(np.abs(c).max(), 2 * np.abs(c - y).sum(), m["n"], 0, want)
                        continue
                    sums, l1, near = b.energy_of(k, c, y)
                    rho = float(np.abs(c).max())
                    for j in range(3):
                        bound = energy_bound(rho, l1[j], m["n"], near[j], sums[j])
                        if j and sums[j] == 0.0 and near[j] == 0:               # no pair within reach + 0.01 A: exactly zero
                            assert got[j] == 0.0, (name, s, m["name"], j, got[j])
                            continue
                        worst = max(worst, abs(got[j] - sums[j]) / bound)
                        assert abs(got[j] - sums[j]) <= bound, (name, field, s, m["name"], j, got[j], sums[j], bound)
    # the run with max_iters = 0 stores the start pose: its energy is the energy0 of every run, bit for bit
    assert np.array_equal(shapes.h0["energy"], shapes.h0["energy0"], equal_nan=True)
    assert np.array_equal(shapes.h0["energy0"], shapes.h["energy0"], equal_nan=True)
    assert not shapes.h0["iters"].any() and (shapes.h0["stop"] == X.STOP_CAP).all()
    print("energies: largest fraction of energy_bound %.4f" % worst)


def test_trace_decreases_strictly_and_energy_never_rises(cases, shapes):
    seen = set()
    for name, w in _worlds(cases, shapes):
        h, b = w.h, w.b
        S = h["coords"].shape[0]
        assert h["trace"].shape == (S, b.B, 100) and h["trace"].dtype == np.float64
        for k, m in enumerate(b.mols):
            for s in range(S):
                tr, it = h["trace"][s, k], int(h["iters"][s, k])
                assert np.isfinite(tr[:it]).all() and np.isnan(tr[it:]).all(), (name, s, m["name"])
                assert (np.diff(tr[:it]) < 0).all(), (name, s, m["name"], tr[:it])
                assert h["stop"][s, k] in (X.STOP_CONVERGED, X.STOP_CAP, X.STOP_REJECTED)
                seen.add(int(h["stop"][s, k]))
                if (h["status"][k] & 7) == 3 or not m["n"]:
                    assert it == 0
                    continue
                e0, e1 = X.total(h["energy0"][s, k]), X.total(h["energy"][s, k])
                assert e1 <= e0, (name, s, m["name"], e0, e1)
                if it:
                    assert tr[0] < e0 and tr[it - 1] == e1, (name, s, m["name"])
                else:
                    assert e1 == e0
    print("stop codes seen:", sorted(seen))
    assert {X.STOP_CONVERGED, X.STOP_CAP} <= seen


# ------------------------------------------------------------------------------------------------ 3. against the restatement
def test_final_energy_within_four_times_the_float32_yardstick(cases):
    gold, h = cases.gold, cases.h
    assert len(gold["cases"]) >= 24 and (gold["d32"] <= 1e-3).all()
    yard = float(np.abs(gold["E32"] - gold["E64"]).max())
    assert 0 < yard <= 1e-4                                              # (recorded: 4.4e-5; tests/test_relax_refs_cpu.py recomputes it)
    worst = 0.0
    for i, (k, s) in enumerate(gold["cases"]):
        dev = X.total(h["energy"][s, k])
        off = abs(dev - gold["E64"][i])
        c64 = gold["coords64"][gold["atom_off"][i]:gold["atom_off"][i + 1]]
        print("case %2d %d %-18s float64 %.6f in %3d, float32 restatement off by %.2e, device off by %.2e in %3d, %.2e A from the float64 pose" % (
            k, s, cases.cx[k]["name"], gold["E64"][i], gold["iters64"][i], abs(gold["E32"][i] - gold["E64"][i]), off, h["iters"][s, k],
            F.rmsd(h["coords"][s, cases.b.sl(k)], c64)))
        worst = max(worst, off)
    print("restatement: yardstick %.3e, largest device deviation %.3e, fraction of 4 x yardstick %.3f" % (yard, worst, worst / (4 * yard)))
    for i, (k, s) in enumerate(gold["cases"]):
        assert abs(X.total(h["energy"][s, k]) - gold["E64"][i]) <= 4.0 * yard, (cases.cx[k]["name"], s)


# ------------------------------------------------------------------------------------------------ 4. effect
def test_relaxed_poses_pass_both_clash_checks(cases):
    from fabind_amd import validity
    gold, b = cases.gold, cases.b
    clean = (gold["prot1"] >= 0.75 + 1e-3) & (gold["clash1"] >= 0.70 + 1e-3)
    flagged = (gold["prot0"] < 0.75) | (gold["clash0"] < 0.70)
    assert (clean & flagged).sum() >= 12
    prot = validity.check_poses_protein(cases.out.coords, b.vp, b.grid)
    own = validity.check_poses(cases.out.coords, b.vp)
    pf, of = prot.flags.cpu().numpy(), own.flags.cpu().numpy()
    before = validity.check_poses_protein(_t(cases.y), b.vp, b.grid).flags.cpu().numpy()
    n = 0
    for i, (k, s) in enumerate(gold["cases"]):
        if clean[i]:
            n += 1
            assert not pf[k, s] & validity.PROTEIN_CLASH, (cases.cx[k]["name"], s, prot.stats[k, s])
            assert not of[k, s] & validity.CLASH, (cases.cx[k]["name"], s, own.stats[k, s])
    print("effect: %d cases checked; PROTEIN_CLASH among all %d poses: %d at the targets, %d after" % (
        n, pf.size, int((before & validity.PROTEIN_CLASH != 0).sum()), int((pf & validity.PROTEIN_CLASH != 0).sum())))
    ov0 = validity.check_poses_protein(_t(cases.y), b.vp, b.grid).stats[:, :, 2].mean().item()
    print("overlap (reported): mean %.4f at the targets, %.4f after" % (ov0, prot.stats[:, :, 2].mean().item()))


# ------------------------------------------------------------------------------------------------ 5. nothing to do
def test_no_protein_in_reach_and_an_unperturbed_target(shapes):
    b, h = shapes.b, shapes.h
    far = [KINDS.index("beyond"), KINDS.index("outside+z-corner")]
    for k, m in enumerate(b.mols):
        if not m["n"] or (h["status"][k] & 7) == 3:
            continue
        for s in far:
            assert h["energy0"][s, k, 1] == 0.0 and h["energy"][s, k, 1] == 0.0, (m["name"], s)
    assert (h["energy0"][:, 0, 1] == 0.0).all() and (h["energy"][:, 0, 1] == 0.0).all()          # the protein of 0 kept atoms
    assert h["status"][0] == 0 and len(b.kept[0][0]) == 0
    # the unperturbed placement with the intra term off, for n a power of two (the centroids and the centred coordinates are then exact,
    # the cross-covariance is symmetric bit for bit and Horn's quaternion is the identity): E == 0 at the start, no iteration, and coords
    # is the Horn image, which is the target
    out = host(b.relax(shapes.y[:1], w_intra=0.0))
    worst, n = 0.0, 0
    for k, m in enumerate(b.mols):
        if not m["n"] or m["n"] & (m["n"] - 1) or (h["status"][k] & 7) == 3:
            continue
        y = shapes.y[0, b.sl(k)].astype(np.float64)
        if X.prot_clash(y, b.vplans[k]["radii"], *b.kept[k]) < 0.81:     # (the chain of 2 atoms sits 2.5 A from its one protein atom)
            continue
        n += 1
        assert out["iters"][0, k] == 0 and out["stop"][0, k] == X.STOP_CONVERGED, (m["name"], out["iters"][0, k], out["energy0"][0, k])
        assert (out["energy"][0, k, :2] == 0).all() and not out["angles"][0, b.tl(k)].any()      # (the intra sum is reported, with weight 0)
        c = out["coords"][0, b.sl(k)].astype(np.float64)
        want = F.rigid_image(b.x[b.sl(k)].astype(np.float64), y)
        bound = rigid_bound(_radius(b.x[b.sl(k)] - b.x[b.sl(k)].mean(0)), _radius(want))
        worst = max(worst, np.abs(c - want).max() / bound)
        assert np.abs(c - want).max() <= bound, (m["name"],)
    assert n >= 6                                                        # chains of 1, 8, 32, 64 and 256 atoms and the coincident butane
    print("nothing to do: %d ligands, largest fraction of rigid_bound %.4f" % (n, worst))


# ------------------------------------------------------------------------------------------------ 6. bit identity
def _same(a, b, what):
    for f in FIELDS:
        bits = torch.int32 if a[f].element_size() == 4 else torch.int64
        assert torch.equal(a[f].reshape(-1).view(bits), b[f].reshape(-1).view(bits)), (what, f)


def test_same_bits_alone_in_any_batch_among_any_poses_and_on_a_repeat(cases):
    w = cases
    cx = w.cx
    for k, s in ((9, 2), (7, 1), (1, 0)):                                # a recorded ligand, the chain of 20 atoms, biphenyl
        def run(order, S, at):
            sub = [cx[i] for i in order]
            bb = _Batch([c["mol"] for c in sub], [c["z"] for c in sub], [c["mol"]["x"] for c in sub], [(c["prot_xyz"], c["prot_z"]) for c in sub])
            pos = order.index(k)
            y = np.zeros((S, bb.N, 3), np.float32)
            a0 = np.zeros((S, int(bb.toff[-1])), np.float32)
            for j, i in enumerate(order):
                for t in range(S):
                    y[t, bb.sl(j)] = X.make_target(cx[i], X.target_seed(i, (t + j) % 3))
            y[at, bb.sl(pos)] = w.y[s, w.b.sl(k)]
            a0[at, bb.tl(pos)] = w.a0[s, w.b.tl(k)]
            o = bb.relax(y, angles0=a0)
            return dict(coords=o.coords[at, bb.sl(pos)], angles=o.angles[at, bb.tl(pos)], energy0=o.energy0[at, pos], energy=o.energy[at, pos],
                        iters=o.iters[at, pos], stop=o.stop[at, pos], trace=o.trace[at, pos])
        alone = run([k], 1, 0)
        for order, S, at in (([0, 12, k, 5], 1, 0), ([8, k, 3], 3, 2), ([k], 3, 2), ([k], 1, 0)):
            _same(alone, run(order, S, at), (cx[k]["name"], order, S))
        big = w.out                                                     # ... and inside the batch of the other tests
        assert torch.equal(alone["coords"], big.coords[s, w.b.sl(k)]) and torch.equal(alone["energy"], big.energy[s, k])
        assert int(alone["iters"]) >= 1


def test_nonfinite_target_ends_that_pose_alone(cases):
    w, b = cases, cases.b
    k = 9
    y = np.repeat(w.y[2:3], 8, 0).copy()
    a0 = np.repeat(w.a0[2:3], 8, 0)
    y[5, b.off[k] + 3, 1] = np.nan
    out = b.relax(y, angles0=a0)
    h = host(out)
    assert h["stop"][5, k] == X.STOP_NONFINITE and h["iters"][5, k] == 0
    assert np.isnan(h["coords"][5, b.sl(k)]).all() and np.isnan(h["angles"][5, b.tl(k)]).all()
    assert np.isnan(h["energy"][5, k]).all() and np.isnan(h["energy0"][5, k]).all() and np.isnan(h["trace"][5, k]).all()
    for f in FIELDS:                                                    # every other (complex, pose): the bits of the run without it
        got, want = getattr(out, f).clone(), getattr(w.out, f)[2:3].expand(8, *getattr(w.out, f).shape[1:]).clone()
        if f == "coords":
            got[5, b.sl(k)] = 0; want[5, b.sl(k)] = 0
        elif f == "angles":
            got[5, b.tl(k)] = 0; want[5, b.tl(k)] = 0
        else:
            got[5, k] = 0; want[5, k] = 0
        bits = torch.int32 if got.element_size() == 4 else torch.int64
        assert torch.equal(got.reshape(-1).view(bits), want.reshape(-1).view(bits)), f
    assert torch.equal(out.status, w.out.status)


def test_c_abi_writes_everything_inside_and_nothing_outside(shapes):
    from fabind_amd import _lib
    w, b = shapes, shapes.b
    S, B, N, Tt, MI, PAD = 2, b.B, b.N, int(b.toff[-1]), 5, 64
    lib = _lib.load()
    x, y = _t(b.x), _t(w.y[3:5])

    def band(numel, dtype):
        fill = float("nan") if dtype.is_floating_point else -777
        buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device=DEV)
        buf[:PAD] = 12345
        buf[PAD + numel:] = 12345
        return buf
    sizes = dict(coords=(S * N * 3, torch.float32), angles=(S * Tt, torch.float32), energy0=(S * B * 3, torch.float64),
                 energy=(S * B * 3, torch.float64), iters=(S * B, torch.int32), stop=(S * B, torch.int32), status=(B, torch.int32),
                 trace=(S * B * MI, torch.float64))
    bufs = {k: band(n, dt) for k, (n, dt) in sizes.items()}
    p = lambda k: bufs[k].data_ptr() + PAD * bufs[k].element_size()
    g, vp, tp = b.grid, b.vp, b.tp
    f = ctypes.c_float
    rc = lib.fabind_pose_relax(x.data_ptr(), y.data_ptr(), None, tp.atom_off.data_ptr(), B, N, S, tp.off.data_ptr(), tp.quad.data_ptr(),
                               tp.side.data_ptr(), Tt, int(np.diff(b.off).max()), int(b.T.max()), vp.status.data_ptr(), vp.cls.data_ptr(),
                               vp.radii.data_ptr(), g.status.data_ptr(), g.origin.data_ptr(), g.dims.data_ptr(), g.cell_off.data_ptr(),
                               g.atom_off.data_ptr(), g.cell_ptr.data_ptr(), g.xyz.data_ptr(), g.radii.data_ptr(), f(g.edge), f(0.8 * 4.0),
                               f(1.0), f(100.0), f(100.0), f(0.8), f(0.75), MI, f(1e-6), p("coords"), p("angles"), p("energy0"), p("energy"),
                               p("iters"), p("stop"), p("status"), p("trace"), _lib.stream())
    assert rc == 0, lib.fabind_last_error()
    torch.cuda.synchronize()
    big = b.relax(w.y[3:5], max_iters=MI)
    for k, (n, dt) in sizes.items():
        inner = bufs[k][PAD:PAD + n]
        assert bool((bufs[k][:PAD] == 12345).all()) and bool((bufs[k][PAD + n:] == 12345).all()), k
        bits = torch.int32 if inner.element_size() == 4 else torch.int64
        assert torch.equal(inner.view(bits), getattr(big, k).reshape(-1).view(bits)), k     # every slot written: the wrapper's bits
        if k in ("iters", "stop", "status"):
            assert not bool((inner == -777).any()), k
    it = bufs["iters"][PAD:PAD + S * B].view(S, B)
    tr = bufs["trace"][PAD:PAD + S * B * MI].view(S, B, MI)
    assert bool((torch.isnan(tr) == ~(torch.arange(MI, device=DEV)[None, None, :] < it[:, :, None])).all())
    zero = band(S * B * MI, torch.float64)
    zero[PAD:PAD + S * B * MI] = 0.0                                    # prefilled with zeros: every slot must change to E or NaN
    args = [x.data_ptr(), y.data_ptr(), None, tp.atom_off.data_ptr(), B, N, S, tp.off.data_ptr(), tp.quad.data_ptr(), tp.side.data_ptr(), Tt,
            int(np.diff(b.off).max()), int(b.T.max()), vp.status.data_ptr(), vp.cls.data_ptr(), vp.radii.data_ptr(), g.status.data_ptr(),
            g.origin.data_ptr(), g.dims.data_ptr(), g.cell_off.data_ptr(), g.atom_off.data_ptr(), g.cell_ptr.data_ptr(), g.xyz.data_ptr(),
            g.radii.data_ptr(), f(g.edge), f(0.8 * 4.0), f(1.0), f(100.0), f(100.0), f(0.8), f(0.75), MI, f(1e-6), p("coords"), p("angles"),
            p("energy0"), p("energy"), p("iters"), p("stop"), p("status"), zero.data_ptr() + PAD * 8, _lib.stream()]
    assert lib.fabind_pose_relax(*args) == 0
    torch.cuda.synchronize()
    assert not bool((zero[PAD:PAD + S * B * MI] == 0.0).any())
    # refused before a launch: too many poses, a reach beyond the cell edge, a negative weight
    for pos, val in ((6, 65536), (25, f(g.edge * 1.01)), (27, f(-1.0))):
        bad = list(args)
        bad[pos] = val
        assert lib.fabind_pose_relax(*bad) != 0


# ------------------------------------------------------------------------------------------------ 7. statuses, refusals, wrapper
def test_statuses_and_the_terms_they_switch_off(shapes):
    from fabind_amd import relax
    b, h = shapes.b, shapes.h
    names = [m["name"] for m in b.mols]
    want = []
    for k, m in enumerate(b.mols):
        code = 3 if m["n"] > 256 else 4 if b.T[k] > 58 else 0
        want.append(code | (relax.NO_INTRA if b.vplans[k]["status"] != 0 else 0) | (relax.NO_PROTEIN if b.gstatus[k] != 0 else 0))
    assert h["status"].tolist() == want, (names, h["status"].tolist(), want)
    assert want[names.index("chain257")] == 3 | relax.NO_INTRA and want[names.index("coincident")] == relax.NO_INTRA
    assert want.count(relax.NO_PROTEIN) == 1 and [w & 7 for w in want].count(4) == 5
    assert b.vp.status.cpu().numpy()[names.index("coincident")] == 5 and b.grid.status.cpu().numpy()[want.index(relax.NO_PROTEIN)] == 6
    k3 = names.index("chain257")
    worst = 0.0
    for s in range(len(KINDS)):                                          # status 3: the Horn image of the start conformer
        xx, y = b.x[b.sl(k3)].astype(np.float64), shapes.y[s, b.sl(k3)].astype(np.float64)
        imgs = F.rigid_image(xx, y)
        bound = rigid_bound(_radius(xx - xx.mean(0)), _radius(imgs))
        worst = max(worst, np.abs(h["coords"][s, b.sl(k3)] - imgs).max() / bound)
        assert np.abs(h["coords"][s, b.sl(k3)] - imgs).max() <= bound
    print("status 3: largest fraction of rigid_bound %.4f" % worst)
    lowered = 0
    for k in [i for i, v in enumerate(want) if (v & 7) == 4]:           # status 4: the rigid relaxation lowers E
        for s in range(len(KINDS)):
            e0, e1 = X.total(h["energy0"][s, k]), X.total(h["energy"][s, k])
            lowered += e1 < e0 and h["iters"][s, k] >= 1
            assert not h["angles"][s, b.tl(k)].any() and e1 <= e0
    assert lowered >= 10
    kp = want.index(relax.NO_PROTEIN)
    assert (h["energy"][:, kp, 1] == 0).all() and (h["energy0"][:, kp, 1] == 0).all()
    assert (h["energy"][:, names.index("coincident"), 2] == 0).all()
    with pytest.raises(RuntimeError, match=r"status 4 \(more than 58 torsions\).*ligand %d: status 3 \(more than 256 atoms\)" % k3):
        b.relax(shapes.y, on_overflow="raise")


def test_argument_errors_come_before_any_launch(shapes, monkeypatch):
    import dataclasses
    from fabind_amd import _lib, relax, validity
    b = shapes.b
    x, y = _t(b.x), _t(shapes.y[:2])
    small = validity.protein_grid(_t(np.zeros((1, 3), np.float32)), _t(np.array([6])), np.array([0, 1] + [1] * (b.B - 1), np.int32), edge=2.0)

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("native call %s after a bad argument" % name)
    monkeypatch.setattr(_lib, "load", lambda: _NoLaunch())
    bad_tp = dataclasses.replace(b.tp, quad=b.tp.quad[:-1])
    bad_vp = dataclasses.replace(b.vp, cls=b.vp.cls[:-1])
    bad_grid = dataclasses.replace(b.grid, cell_ptr=b.grid.cell_ptr[:-1].contiguous())
    f64_vp = dataclasses.replace(b.vp, radii=b.vp.radii.double())
    i64_grid = dataclasses.replace(b.grid, cell_ptr=b.grid.cell_ptr.long())
    for exc, kw in ((ValueError, dict(conformer=x[:, :2])), (ValueError, dict(target=y[:, :-1])), (ValueError, dict(target=y[0, :, :2])),
                    (ValueError, dict(torsion_plan=None)), (ValueError, dict(validity_plan=None)), (ValueError, dict(grid=None)),
                    (ValueError, dict(torsion_plan=bad_tp)), (ValueError, dict(validity_plan=bad_vp)), (ValueError, dict(grid=bad_grid)),
                    (ValueError, dict(grid=small)), (ValueError, dict(validity_plan=f64_vp)), (ValueError, dict(grid=i64_grid)),
                    (ValueError, dict(out=torch.empty(2, b.N, 3, dtype=torch.float64, device=DEV))), (ValueError, dict(on_overflow="ignore")), (ValueError, dict(max_iters=-1)),
                    (ValueError, dict(tol=-1.0)), (ValueError, dict(tol=float("nan"))), (ValueError, dict(w_prot=-1.0)),
                    (ValueError, dict(c_prot=float("inf"))), (ValueError, dict(c_prot=2.0)), (ValueError, dict(angles0=torch.zeros(2, 3, device=DEV))),
                    (ValueError, dict(angles0=torch.zeros(2, int(b.toff[-1]), dtype=torch.float64)[:, :-1])),
                    (ValueError, dict(out=torch.empty(2, b.N, 3))), (ValueError, dict(out=torch.empty(3, b.N, 3, device=DEV))),
                    (RuntimeError, dict(conformer=x.cpu())), (RuntimeError, dict(target=y.cpu())), (RuntimeError, dict(on_overflow="raise"))):
        args = dict(conformer=x, target=y, torsion_plan=b.tp, validity_plan=b.vp, grid=b.grid, on_overflow="truncate")
        args.update(kw)
        with pytest.raises(exc):
            relax.relax_poses(**args)


def test_wrapper_fits_and_then_relaxes(cases):
    from fabind_amd import conformer, relax
    from fabind_amd.utils.post_optim_utils import relax_compound_coords_batched
    w, b = cases, cases.b
    cb = _t(np.repeat(np.arange(b.B), np.diff(b.off)))
    fit = conformer.fit_conformers(_t(b.x), _t(w.y), b.tp, on_overflow="truncate")
    want = relax.relax_poses(_t(b.x), _t(w.y), b.tp, b.vp, b.grid, angles0=fit.angles, on_overflow="truncate")
    x, e, e0 = relax_compound_coords_batched(_t(b.x), _t(w.y), cb, b.tp, b.vp, b.grid)
    assert torch.equal(x, want.coords) and torch.equal(e, want.energy) and torch.equal(e0, want.energy0)
    x1, e1, _ = relax_compound_coords_batched(_t(b.x), _t(w.y[0]), cb, b.tp, b.vp, b.grid)
    assert tuple(x1.shape) == (b.N, 3) and tuple(e1.shape) == (b.B, 3) and torch.equal(x1, want.coords[0]) and torch.equal(e1, want.energy[0])
    with pytest.raises(ValueError):
        relax_compound_coords_batched(_t(b.x), _t(w.y), cb, b.tp, None, b.grid)
    with pytest.raises(ValueError):
        relax_compound_coords_batched(_t(b.x), _t(w.y), cb[:-1], b.tp, b.vp, b.grid)
    with pytest.raises(RuntimeError, match="HIP device"):
        relax_compound_coords_batched(_t(b.x), torch.as_tensor(w.y), cb, b.tp, b.vp, b.grid)
    out = torch.full((3 * b.N * 3 + 128,), -777.0, device=DEV)
    view = out[64:64 + 3 * b.N * 3].view(3, b.N, 3)
    o = relax.relax_poses(_t(b.x), _t(w.y), b.tp, b.vp, b.grid, angles0=_t(w.a0), out=view)
    assert o.coords.data_ptr() == view.data_ptr() and torch.equal(view, w.out.coords)
    assert bool((out[:64] == -777.0).all()) and bool((out[-64:] == -777.0).all())
