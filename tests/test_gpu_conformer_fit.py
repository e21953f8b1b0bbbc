"""GPU: fabind_amd.conformer.fit_conformers (csrc/conformer_fit.hip) -- the start conformer fitted to target poses over its torsions and
one rigid motion -- against the float64 numpy restatement of tests/fit_refs.py (pinned on the CPU by tests/test_fit_refs_cpu.py) and
against invariants that hold by construction.

Bounds (u = 2^-24, the unit roundoff of float32; rho = the largest distance of an atom from the origin of the frame the arithmetic runs
in; derivations in DESIGN.md section 16):
* `pass_bound`: two float32 torsion passes with the same angles differ, after the best rigid alignment, by an RMSD of at most
  2 u rho (100 T + 16): about 100 roundings of size u rho per Rodrigues update (difference, dot, cross, three sums, sincos, the unit
  axis), T updates per atom at most, 16 for centring, the rigid transform and the stores; internal coordinates carry no lever arm.
* `rmsd_bound`: 4 u (rho + rmsd) for an RMSD recomputed from stored float32 coordinates.
* `rigid_bound`: 16 u (rho_conformer + rho_output) per coordinate for the rigid image of a non-degenerate ligand.
Every test prints its largest fraction of its bound before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import conformer_refs as R
import fit_refs as F
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _molecules():
    g = load_npz("conformer_ligands")
    hand = [m for _, (m, _) in sorted(R.hand_molecules().items())]
    chains = [R.chain(n) for n in (1, 2, 3, 4, 60, 61, 62, 63, 64, 65, 256, 257)]
    return hand + R.fixture_molecules(g) + [R.mol(0, [], name="empty")] + chains


def _plan(mols, on_overflow="truncate"):
    from fabind_amd import conformer
    x, bi, codes, off = R.pack(mols)
    return conformer.rotatable_bonds(_t(bi), _t(codes), off, on_overflow=on_overflow), x, off


def _radius(*clouds):
    return max([float(np.abs(c).max()) * np.sqrt(3.0) for c in clouds if len(c)] + [0.0])


def pass_bound(T, rho):
    return 2.0 * U * rho * (100.0 * T + 16.0)


def rmsd_bound(rho, rmsd):
    return 4.0 * U * (rho + rmsd)


def rigid_bound(rho_in, rho_out):
    return 16.0 * U * (rho_in + rho_out)


class _World:
    """One batch of every molecule, its plan (device and restated), targets of three kinds and the device's answers, made once."""

    def __init__(self):
        from fabind_amd import conformer
        self.mols = _molecules()
        self.plan, self.x, self.off = _plan(self.mols)
        self.quad, self.side, self.toff, self.pstatus = R.batch_plan(self.mols)
        self.B, self.N = len(self.mols), len(self.x)
        self.T = np.diff(self.toff)
        self.fitted = [b for b, m in enumerate(self.mols) if 1 <= self.T[b] <= F.MAX_TORSIONS and m["n"] <= F.MAX_ATOMS]
        rng = np.random.RandomState(31)
        # three targets per kind: "recover" = torsions changed by +-0.3 rad, rotated and shifted; "noisy" = +-0.5 rad plus 0.3 A noise
        self.targets, self.exact = {}, {}
        for kind, amp, noise in (("recover", 0.3, 0.0), ("noisy", 0.5, 0.3)):
            y = np.zeros((3, self.N, 3))
            for s in range(3):
                for b, m in enumerate(self.mols):
                    if m["n"]:
                        mm = dict(x=self.x[self.off[b]:self.off[b + 1]].astype(np.float64), quad=self.lq(b), side=self.ls(b))
                        y[s, self.off[b]:self.off[b + 1]] = F.make_target(mm, rng, amp, noise)[0]
            self.targets[kind], self.exact[kind] = y.astype(np.float32), y
        self.fit = {k: conformer.fit_conformers(_t(self.x), _t(y), self.plan, return_trace=True, on_overflow="truncate")
                    for k, y in self.targets.items()}
        self.host = {k: {f: getattr(v, f).cpu().numpy() for f in ("coords", "angles", "rmsd0", "rmsd", "iters", "stop", "status", "trace")}
                     for k, v in self.fit.items()}
        self._ref = {}

    def lq(self, b):
        return self.quad[self.toff[b]:self.toff[b + 1]]

    def ls(self, b):
        return self.side[self.toff[b]:self.toff[b + 1]]

    def sl(self, b):
        return slice(self.off[b], self.off[b + 1])

    def ref(self, kind, s, b, dt=np.float64, exact=False):
        """The restatement on the same float32 inputs (exact: on the target before it was rounded to float32), once per case."""
        key = (kind, s, b, dt, exact)
        if key not in self._ref:
            y = (self.exact if exact else self.targets)[kind][s, self.sl(b)]
            self._ref[key] = F.fit_one(self.x[self.sl(b)], y, self.lq(b), self.ls(b), dt=dt)
        return self._ref[key]


@pytest.fixture(scope="module")
def world():
    return _World()


# ------------------------------------------------------------------------------------------------ 1. invariant of the answer
def test_coords_are_the_start_conformer_under_the_returned_angles(world):
    """coords == perturb_conformers(conformer, plan, angles, relative) up to a rigid motion: the local geometry is the start conformer's."""
    from fabind_amd import conformer
    w = world
    worst = 0.0
    for kind, fit in w.fit.items():
        h = w.host[kind]
        assert np.abs(h["angles"]).max() <= np.float32(np.pi) and np.isfinite(h["angles"]).all() and np.isfinite(h["coords"]).all()
        pert = conformer.perturb_conformers(_t(w.x), w.plan, n_copies=3, angles=fit.angles, relative=True, random_rotation=False,
                                            centre=False).cpu().numpy().astype(np.float64)
        for s in range(3):
            for b, m in enumerate(w.mols):
                if not m["n"]:
                    continue
                c, p = h["coords"][s, w.sl(b)].astype(np.float64), pert[s, w.sl(b)]
                rho = _radius(w.x[w.sl(b)], c - c.mean(0), p)
                bound = pass_bound(w.T[b], rho) + rmsd_bound(_radius(c), 0.0)
                got = F.rmsd(F.rigid_image(p, c), c)
                worst = max(worst, got / bound)
                assert got <= bound, (kind, s, m["name"], got, bound)
                if b not in w.fitted:
                    assert not h["angles"][s, w.toff[b]:w.toff[b + 1]].any()
    print("invariant: largest fraction of pass_bound %.4f" % worst)


def test_rmsd_and_rmsd0_are_those_of_the_coordinates(world):
    w = world
    worst = 0.0
    for kind in w.fit:
        h = w.host[kind]
        for s in range(3):
            for b, m in enumerate(w.mols):
                if not m["n"]:
                    assert h["rmsd"][s, b] == 0 and h["rmsd0"][s, b] == 0 and h["iters"][s, b] == 0
                    continue
                y = w.targets[kind][s, w.sl(b)].astype(np.float64)
                c = h["coords"][s, w.sl(b)].astype(np.float64)
                r = F.rmsd(c, y)
                r0 = F.rmsd(F.rigid_image(w.x[w.sl(b)], y), y)
                rho = _radius(c, y, w.x[w.sl(b)])
                for got, want in ((h["rmsd"][s, b], r), (h["rmsd0"][s, b], r0)):
                    bound = rmsd_bound(rho, want)
                    worst = max(worst, abs(got - want) / bound)
                    assert abs(got - want) <= bound, (kind, s, m["name"], got, want, bound)
    print("rmsd / rmsd0: largest fraction of rmsd_bound %.4f" % worst)


# ------------------------------------------------------------------------------------------------ 2. trace
def test_trace_decreases_strictly(world):
    w = world
    seen = set()
    for kind in w.fit:
        h = w.host[kind]
        assert h["trace"].shape == (3, w.B, 50) and h["trace"].dtype == np.float64
        for s in range(3):
            for b, m in enumerate(w.mols):
                tr, it = h["trace"][s, b], int(h["iters"][s, b])
                assert np.isfinite(tr[:it]).all() and np.isnan(tr[it:]).all(), (kind, s, m["name"])
                assert (np.diff(tr[:it]) < 0).all(), (kind, s, m["name"], tr[:it])
                assert h["rmsd"][s, b] <= h["rmsd0"][s, b]
                assert h["stop"][s, b] in (F.STOP_CONVERGED, F.STOP_CAP, F.STOP_REJECTED)
                seen.add(int(h["stop"][s, b]))
                if it:
                    n = m["n"]
                    assert tr[0] < float(h["rmsd0"][s, b]) ** 2 * n * (1 + 4 * U) and abs(np.sqrt(tr[it - 1] / n) - h["rmsd"][s, b]) <= U * h["rmsd"][s, b]
                if b not in w.fitted or m["n"] <= 2:
                    assert it == 0 and h["stop"][s, b] == F.STOP_CONVERGED
                else:
                    assert 1 <= it <= 50
    print("stop codes seen:", sorted(seen))


def test_iteration_cap_is_a_stop_code(world):
    from fabind_amd import conformer
    w = world
    fit = conformer.fit_conformers(_t(w.x), _t(w.targets["noisy"][:1]), w.plan, max_iters=2, return_trace=True, on_overflow="truncate")
    it, st = fit.iters.cpu().numpy()[0], fit.stop.cpu().numpy()[0]
    assert fit.trace.shape == (1, w.B, 2) and it.max() == 2
    assert ((it == 2) <= (st != F.STOP_REJECTED)).all() and (st[it == 2] == F.STOP_CAP).sum() >= 1
    full = w.host["noisy"]
    two = fit.trace.cpu().numpy()[0]
    assert np.array_equal(two, full["trace"][0, :, :2], equal_nan=True)               # the first steps do not depend on the cap


# ------------------------------------------------------------------------------------------------ 3. recovery
def test_recovers_a_pose_the_conformer_can_reach(world):
    """The float64 restatement gets the target as it was made; the device gets its float32 rounding (half an ulp at 16 A is 5e-7 A per
    coordinate: the rounded target itself is not reachable to 1e-6 A) and has to end below 1e-4 A of that."""
    w = world
    h = w.host["recover"]
    cases = [(s, b) for s in range(3) for b in w.fitted]
    ok, worst = 0, 0.0
    for s, b in cases:
        r = w.ref("recover", s, b, exact=True)
        print("recover %-18s pose %d: float64 %.2e in %2d, device %.2e in %2d" % (w.mols[b]["name"], s, r["rmsd"], r["iters"], h["rmsd"][s, b], h["iters"][s, b]))
        if r["rmsd"] < 1e-6:
            ok += 1
            worst = max(worst, float(h["rmsd"][s, b]))
    assert ok >= 0.9 * len(cases), (ok, len(cases))
    print("recovery: %d of %d cases qualify, largest device rmsd %.3e (gate 1e-4)" % (ok, len(cases), worst))
    for s, b in cases:
        if w.ref("recover", s, b, exact=True)["rmsd"] < 1e-6:
            assert h["rmsd"][s, b] < 1e-4, (w.mols[b]["name"], s, h["rmsd"][s, b])


# ------------------------------------------------------------------------------------------------ 4. noisy targets
def test_noisy_targets_within_four_times_the_float32_deviation(world):
    w = world
    h = w.host["noisy"]
    cases = [(s, b) for s in range(3) for b in w.fitted]
    rows = []
    for s, b in cases:
        r64, r32 = w.ref("noisy", s, b), w.ref("noisy", s, b, np.float32)
        rows.append((s, b, r64["rmsd"], abs(r32["rmsd"] - r64["rmsd"]), abs(float(h["rmsd"][s, b]) - r64["rmsd"])))
        print("noisy %-18s pose %d: float64 %.6f, float32 restatement off by %.2e, device off by %.2e (rigid only %.4f)" % (
            w.mols[b]["name"], s, r64["rmsd"], rows[-1][3], rows[-1][4], h["rmsd0"][s, b]))
    kept = [r for r in rows if r[3] <= 1e-3]
    assert len(kept) >= 0.9 * len(rows), (len(kept), len(rows))
    yard = max(r[3] for r in kept)
    worst = max(r[4] for r in kept)
    print("noisy: %d of %d cases kept, float32 yardstick %.3e, largest device deviation %.3e, fraction of 4 x yardstick %.3f" % (
        len(kept), len(rows), yard, worst, worst / (4 * yard)))
    assert 0 < yard <= 1e-5                                              # (recorded: 3.0e-6 A; test_fit_refs_cpu.py pins the float32 path at 2e-6 A on its list)
    for s, b, _, _, dev in kept:
        assert dev <= 4.0 * yard, (w.mols[b]["name"], s, dev, yard)


# ------------------------------------------------------------------------------------------------ 5. rigid only
def _check_rigid(coords, x, y, name):
    want = F.rigid_image(x, y)
    bound = rigid_bound(_radius(x - x.mean(0)), _radius(want))
    got = float(np.abs(coords - want).max())
    assert got <= bound, (name, got, bound)
    return got / bound


def test_rigid_fit_without_a_plan_and_past_the_limits(world):
    from fabind_amd import conformer
    w = world
    worst = 0.0
    cb = _t(np.repeat(np.arange(w.B), np.diff(w.off)))
    small = np.array([m["n"] <= 256 for m in w.mols])
    for S in (1, 3):
        y = w.targets["noisy"][:S]
        fit = conformer.fit_conformers(_t(w.x), _t(y[0] if S == 1 else y), None, atom_off=w.off, on_overflow="truncate")
        assert tuple(fit.angles.shape) == (S, 0) and tuple(fit.coords.shape) == (S, w.N, 3) and fit.trace is None
        st = fit.status.cpu().numpy()
        assert not st[small].any() and (st[~small] == 3).all()
        assert not fit.iters.any() and not fit.stop.any() and torch.equal(fit.rmsd, fit.rmsd0)
        c = fit.coords.cpu().numpy().astype(np.float64)
        for s in range(S):
            for b, m in enumerate(w.mols):
                if m["n"]:
                    worst = max(worst, _check_rigid(c[s, w.sl(b)], w.x[w.sl(b)].astype(np.float64), y[s, w.sl(b)].astype(np.float64), m["name"]))
        same = conformer.fit_conformers(_t(w.x), _t(y), None, compound_batch=cb, on_overflow="truncate")
        assert torch.equal(same.coords, fit.coords) and torch.equal(same.rmsd, fit.rmsd)
    with pytest.raises(RuntimeError, match=r"ligand %d: status 3 \(more than 256 atoms\)" % (w.B - 1)):
        conformer.fit_conformers(_t(w.x), _t(w.targets["noisy"]), None, atom_off=w.off)
    # with the plan: no torsions, more than 58 torsions, more than 256 atoms
    h = w.host["noisy"]
    want_status = [3 if m["n"] > 256 else 4 if w.T[b] > 58 else 0 for b, m in enumerate(w.mols)]
    assert h["status"].tolist() == want_status and want_status.count(4) == 5 and want_status.count(3) == 1
    for s in range(3):
        for b, m in enumerate(w.mols):
            if m["n"] and b not in w.fitted:
                worst = max(worst, _check_rigid(h["coords"][s, w.sl(b)].astype(np.float64), w.x[w.sl(b)].astype(np.float64),
                                                w.targets["noisy"][s, w.sl(b)].astype(np.float64), m["name"]))
                assert h["iters"][s, b] == 0 and h["rmsd"][s, b] == h["rmsd0"][s, b]
                assert not h["angles"][s, w.toff[b]:w.toff[b + 1]].any()
    print("rigid only: largest fraction of rigid_bound %.4f" % worst)
    names = [r"ligand %d: status 4 \(more than 58 torsions\)" % b for b, v in enumerate(want_status) if v == 4]
    with pytest.raises(RuntimeError, match=".*".join(names) + r".*ligand %d: status 3 \(more than 256 atoms\)" % (w.B - 1)):
        conformer.fit_conformers(_t(w.x), _t(w.targets["noisy"]), w.plan)


def test_rigid_fit_of_degenerate_clouds_is_proper():
    """Planar, collinear and mirrored targets, n = 1, 2, 3: the image is that of the float64 quaternion fit, a proper rotation."""
    from fabind_amd import conformer
    rng = np.random.RandomState(3)
    xs, ys = [], []
    for n, kind in ((1, "any"), (2, "any"), (3, "any"), (7, "planar"), (6, "collinear"), (9, "mirror"), (40, "mirror")):
        x = rng.randn(n, 3) * 3
        if kind == "planar":
            x[:, 2] = 0.5
        if kind == "collinear":
            x = np.outer(np.arange(n) * 1.3, rng.randn(3)) + 1.0
        y = x @ F.random_rotation(rng).T + rng.uniform(-20, 20, 3)
        if kind == "mirror":
            y = y * np.array([1.0, 1.0, -1.0])                          # the best orthogonal map is a reflection: det of the covariance < 0
        xs.append(x.astype(np.float32)); ys.append(y.astype(np.float32))
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    x, y = np.concatenate(xs), np.concatenate(ys)
    fit = conformer.fit_conformers(_t(x), _t(y), None, atom_off=off)
    c = fit.coords.cpu().numpy()[0].astype(np.float64)
    for b in range(len(xs)):
        sl = slice(off[b], off[b + 1])
        _check_rigid(c[sl], xs[b].astype(np.float64), ys[b].astype(np.float64), b)
        if len(xs[b]) >= 4:
            vol = lambda z: np.linalg.det(z[1:4] - z[0])
            assert abs(vol(c[sl]) - vol(xs[b].astype(np.float64))) <= 1e-3 * max(1.0, abs(vol(xs[b].astype(np.float64))))      # handedness kept
    assert np.all(fit.rmsd.cpu().numpy()[0, :5] < 1e-5) and np.all(fit.rmsd.cpu().numpy()[0, 5:] > 0.1)


# ------------------------------------------------------------------------------------------------ 6. bit identity
def test_same_bits_alone_in_any_batch_and_among_any_poses(world):
    from fabind_amd import conformer
    w = world
    fields = ("coords", "angles", "rmsd0", "rmsd", "iters", "stop", "trace")
    for b in (w.fitted[3], w.fitted[-1], w.fitted[-4]):                  # a hand molecule, the 61-atom chain (58 torsions), a recorded ligand
        m = w.mols[b]
        y = w.targets["noisy"][2, w.sl(b)]

        def run(mols, pos, S, s):
            p, x, off = _plan(mols)
            sl = slice(off[pos], off[pos + 1])
            x[sl] = w.x[w.sl(b)]
            tg = np.random.RandomState(S + len(mols)).randn(S, len(x), 3).astype(np.float32) * 4
            for i, mm in enumerate(mols):                                # the other ligands get targets of their own
                tg[:, off[i]:off[i + 1]] += x[off[i]:off[i + 1]]
            tg[s, sl] = y
            f = conformer.fit_conformers(_t(x), _t(tg), p, return_trace=True, on_overflow="truncate")
            tl = slice(int(p.off[pos]), int(p.off[pos + 1]))
            return dict(coords=f.coords[s, sl], angles=f.angles[s, tl], rmsd0=f.rmsd0[s, pos], rmsd=f.rmsd[s, pos], iters=f.iters[s, pos],
                        stop=f.stop[s, pos], trace=f.trace[s, pos])
        alone = run([m], 0, 1, 0)
        others = [run([w.mols[0], R.chain(64), m, w.mols[14]], 2, 1, 0), run([R.chain(257), m, R.chain(2)], 1, 3, 2), run([m], 0, 3, 2),
                  run([m], 0, 1, 0)]
        for o in others:
            for f in fields:
                bits = torch.int32 if alone[f].element_size() == 4 else torch.int64
                assert torch.equal(alone[f].reshape(-1).view(bits), o[f].reshape(-1).view(bits)), (m["name"], f)
        big = w.fit["noisy"]                                            # ... and inside the big batch of the other tests
        assert torch.equal(alone["coords"], big.coords[2, w.sl(b)]) and torch.equal(alone["rmsd"], big.rmsd[2, b])
        assert int(alone["iters"]) >= 1


# ------------------------------------------------------------------------------------------------ 7. memory
def test_c_abi_writes_everything_inside_and_nothing_outside(world):
    from fabind_amd import _lib
    w = world
    S, B, N, Tt, MI, PAD = 2, w.B, w.N, int(w.toff[-1]), 5, 64
    lib = _lib.load()
    x, y = _t(w.x), _t(w.targets["noisy"][:S])
    aoff = _t(w.off, torch.int32)

    def band(numel, dtype):
        fill = float("nan") if dtype.is_floating_point else -777
        buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device=DEV)
        buf[:PAD] = 12345
        buf[PAD + numel:] = 12345
        return buf
    sizes = dict(coords=(S * N * 3, torch.float32), angles=(S * Tt, torch.float32), rmsd0=(S * B, torch.float32), rmsd=(S * B, torch.float32),
                 iters=(S * B, torch.int32), stop=(S * B, torch.int32), status=(B, torch.int32), trace=(S * B * MI, torch.float64))
    bufs = {k: band(n, dt) for k, (n, dt) in sizes.items()}
    p = lambda k: bufs[k].data_ptr() + PAD * bufs[k].element_size()
    rc = lib.fabind_conformer_fit(x.data_ptr(), y.data_ptr(), aoff.data_ptr(), B, N, S, w.plan.off.data_ptr(), w.plan.quad.data_ptr(),
                                  w.plan.side.data_ptr(), Tt, int(np.diff(w.off).max()), int(w.T.max()), MI, ctypes.c_float(1e-6),
                                  p("coords"), p("angles"), p("rmsd0"), p("rmsd"), p("iters"), p("stop"), p("status"), p("trace"), _lib.stream())
    assert rc == 0, lib.fabind_last_error()
    torch.cuda.synchronize()
    for k, (n, dt) in sizes.items():
        inner = bufs[k][PAD:PAD + n]
        assert bool((bufs[k][:PAD] == 12345).all()) and bool((bufs[k][PAD + n:] == 12345).all()), k
        if k == "trace":
            continue
        assert not bool(torch.isnan(inner).any()) if dt.is_floating_point else not bool((inner == -777).any()), k
    e = [b for b, m in enumerate(w.mols) if m["n"] == 0][0]
    assert bufs["rmsd"][PAD:PAD + S * B].view(S, B)[:, e].tolist() == [0.0, 0.0] and bufs["iters"][PAD:PAD + S * B].view(S, B)[:, e].tolist() == [0, 0]
    it = bufs["iters"][PAD:PAD + S * B].view(S, B)
    tr = bufs["trace"][PAD:PAD + S * B * MI].view(S, B, MI)
    written = torch.arange(MI, device=DEV)[None, None, :] < it[:, :, None]
    assert bool((torch.isnan(tr) == ~written).all())                    # E where a step was accepted, a written NaN behind it
    trace_only_nan = band(S * B * MI, torch.float64)
    trace_only_nan[PAD:PAD + S * B * MI] = 0.0                          # prefilled with zeros: every slot must change to E or NaN
    rc = lib.fabind_conformer_fit(x.data_ptr(), y.data_ptr(), aoff.data_ptr(), B, N, S, w.plan.off.data_ptr(), w.plan.quad.data_ptr(),
                                  w.plan.side.data_ptr(), Tt, int(np.diff(w.off).max()), int(w.T.max()), MI, ctypes.c_float(1e-6),
                                  p("coords"), p("angles"), p("rmsd0"), p("rmsd"), p("iters"), p("stop"), p("status"),
                                  trace_only_nan.data_ptr() + PAD * 8, _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not bool((trace_only_nan[PAD:PAD + S * B * MI] == 0.0).any())
    # the limits are refused before a launch
    assert lib.fabind_conformer_fit(x.data_ptr(), y.data_ptr(), aoff.data_ptr(), B, N, 65536, None, None, None, 0, 256, 0, MI,
                                    ctypes.c_float(1e-6), p("coords"), None, p("rmsd0"), p("rmsd"), p("iters"), p("stop"), p("status"), None,
                                    _lib.stream()) != 0


# ------------------------------------------------------------------------------------------------ 8. wrapper and arguments
def test_wrapper_returns_what_fit_conformers_returns(world):
    from fabind_amd import conformer
    from fabind_amd.utils.post_optim_utils import torsion_fit_compound_coords_batched
    w = world
    cb = _t(np.repeat(np.arange(w.B), np.diff(w.off)))
    big = w.fit["noisy"]
    x, r, r0 = torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"]), cb, w.plan)
    assert torch.equal(x, big.coords) and torch.equal(r, big.rmsd) and torch.equal(r0, big.rmsd0)
    x1, r1, r01 = torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"][0]), cb, w.plan)
    assert tuple(x1.shape) == (w.N, 3) and tuple(r1.shape) == (w.B,)
    assert torch.equal(x1, big.coords[0]) and torch.equal(r1, big.rmsd[0]) and torch.equal(r01, big.rmsd0[0])
    with pytest.raises(RuntimeError, match="more than 58 torsions"):
        torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"]), cb, w.plan, on_overflow="raise")
    with pytest.raises(ValueError):
        torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"]), cb[:-1], w.plan)
    with pytest.raises(ValueError):
        torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"]), torch.flip(cb, [0]), w.plan)
    with pytest.raises(ValueError):
        torsion_fit_compound_coords_batched(_t(w.x), _t(w.targets["noisy"]), cb, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        torsion_fit_compound_coords_batched(_t(w.x), torch.as_tensor(w.targets["noisy"]), cb, w.plan)
    out = torch.full((3 * w.N * 3 + 128,), -777.0, device=DEV)
    view = out[64:64 + 3 * w.N * 3].view(3, w.N, 3)
    f = conformer.fit_conformers(_t(w.x), _t(w.targets["noisy"]), w.plan, on_overflow="truncate", out=view)
    assert f.coords.data_ptr() == view.data_ptr() and torch.equal(view, big.coords)
    assert bool((out[:64] == -777.0).all()) and bool((out[-64:] == -777.0).all())


def test_argument_errors_come_before_any_launch(world, monkeypatch):
    from fabind_amd import _lib, conformer
    w = world
    x, y = _t(w.x), _t(w.targets["noisy"])

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("native call %s after a bad argument" % name)
    monkeypatch.setattr(_lib, "load", lambda: _NoLaunch())
    bad_plan = conformer.TorsionPlan(quad=w.plan.quad[:-1], side=w.plan.side, off=w.plan.off, status=w.plan.status, atom_off=w.plan.atom_off)
    for exc, kw in ((ValueError, dict(conformer=x[:, :2])), (ValueError, dict(target=y[:, :-1])), (ValueError, dict(target=y[0, :, :2])),
                    (ValueError, dict(plan=None)), (ValueError, dict(plan=bad_plan)), (ValueError, dict(on_overflow="ignore")),
                    (ValueError, dict(max_iters=-1)), (ValueError, dict(tol=-1.0)), (ValueError, dict(tol=float("nan"))),
                    (ValueError, dict(atom_off=w.off[:-1])), (ValueError, dict(out=torch.empty(3, w.N, 3))),
                    (ValueError, dict(out=torch.empty(2, w.N, 3, device=DEV))), (RuntimeError, dict(conformer=x.cpu())),
                    (RuntimeError, dict(target=y.cpu())), (RuntimeError, dict(on_overflow="raise"))):
        args = dict(conformer=x, target=y, plan=w.plan, on_overflow="truncate")
        args.update(kw)
        with pytest.raises(exc):
            conformer.fit_conformers(**args)
