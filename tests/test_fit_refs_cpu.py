"""CPU: the numpy restatement of the torsion-space fit (tests/fit_refs.py) pinned against independent definitions -- the rigid fit against
known transforms and the SVD route, the Jacobian against central finite differences, the trace against its construction -- and the
recovery experiment behind the defaults of fabind_amd.conformer.fit_conformers, with its case lists fixed by seed."""
import os
import re

import numpy as np
import pytest

import conformer_refs as R
import fit_refs as F
from helpers import load_npz


def _cases():
    return F.molecules_with_torsions(load_npz("conformer_ligands"))


# ------------------------------------------------------------------------------------------------ rigid fit
def test_jacobi_equals_eigh():
    rng = np.random.RandomState(0)
    mats = [rng.randn(4, 4) for _ in range(40)] + [np.zeros((4, 4)), np.eye(4), np.diag([1.0, 1.0, -2.0, 0.0])]
    mats.append(np.outer([1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]))    # rank one: a triple eigenvalue
    for A in mats:
        A = A + A.T
        w, v = F.jacobi_eigh4(A)
        scale = max(1.0, np.abs(A).max())
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(A)).max() <= 1e-13 * scale
        assert np.abs(A @ v - v * w).max() <= 1e-13 * scale and np.abs(v.T @ v - np.eye(4)).max() <= 1e-14


@pytest.mark.parametrize("shape", ["cloud", "planar", "collinear", "n1", "n2", "n3"])
def test_rigid_fit_recovers_a_known_transform(shape):
    rng = np.random.RandomState(len(shape))
    for _ in range(10):
        n = dict(n1=1, n2=2, n3=3).get(shape, 11)
        P = rng.randn(n, 3) * 4
        if shape == "planar":
            P[:, 1] = -0.7
        if shape == "collinear":
            P = np.outer(rng.randn(n), rng.randn(3)) + rng.randn(3)
        Rm, t = F.random_rotation(rng), rng.uniform(-30, 30, 3)
        assert abs(np.linalg.det(Rm) - 1.0) <= 1e-13
        Y = P @ Rm.T + t
        got_R, cp, cy = F.horn(P, Y)
        assert abs(np.linalg.det(got_R) - 1.0) <= 1e-13 and np.abs(got_R @ got_R.T - np.eye(3)).max() <= 1e-13
        assert np.abs(F.rigid_image(P, Y) - Y).max() <= 1e-12 * 40
        if shape == "cloud":
            assert np.abs(got_R - Rm).max() <= 1e-12                     # unique only for a cloud that spans space


def test_rotation_is_proper_when_the_covariance_has_a_negative_determinant():
    rng = np.random.RandomState(7)
    for _ in range(10):
        P = rng.randn(9, 3) * 3
        Y = (P @ F.random_rotation(rng).T) * np.array([1.0, -1.0, 1.0]) + rng.randn(3) + 0.05 * rng.randn(9, 3)
        S = (P - P.mean(0)).T @ (Y - Y.mean(0))
        assert np.linalg.det(S) < 0
        Rm, _, _ = F.horn(P, Y)
        assert abs(np.linalg.det(Rm) - 1.0) <= 1e-13
        img = F.rigid_image(P, Y)
        assert np.abs(img - F.kabsch_svd(P, Y)).max() <= 1e-10          # the SVD route with its sign case agrees
        for _ in range(20):                                             # no other proper rotation does better
            other = (P - P.mean(0)) @ F.random_rotation(rng).T + Y.mean(0)
            assert ((img - Y) ** 2).sum() <= ((other - Y) ** 2).sum()


# ------------------------------------------------------------------------------------------------ pose and Jacobian
def test_torsion_pass_is_that_of_perturb_one():
    rng = np.random.RandomState(1)
    for m in _cases():
        a = rng.uniform(-np.pi, np.pi, len(m["quad"]))
        want = R.perturb_one(m["x"], m["quad"], m["side"], a, (0, 0, 0), relative=True, rotate=False, centre=False)
        assert np.abs(F.apply_torsions(m["x"], m["quad"], m["side"], a) - want).max() <= 1e-12


def test_jacobian_equals_central_differences():
    """Column t against (P(a + h e_t) - P(a - h e_t)) / 2h with P the torsion pass followed by the FIXED rigid motion of pose(a) --
    modulo the six rigid columns: changing a torsion whose fixed side a later torsion moves also shifts the whole ligand, and `pose`
    fits that motion away; the rigid columns against the same differences of a translation / a rotation about the centroid."""
    rng = np.random.RandomState(2)
    h = 1e-6
    for m in _cases():
        q, s, T = m["quad"], m["side"], len(m["quad"])
        a = rng.uniform(-1, 1, T)
        y = F.make_target(m, rng, 0.5, 0.3)[0]
        p = F.apply_torsions(m["x"], q, s, a)
        Rm, cp, cy = F.horn(p, y)
        X = (p - cp) @ Rm.T + cy
        J = F.jacobian(X, q, s).reshape(len(X), 3, T + 6)
        move = lambda z: (z - cp) @ Rm.T + cy
        rigid = J.reshape(-1, T + 6)[:, T:]
        exact = 0
        for t in range(T):
            e = np.zeros(T)
            e[t] = h
            fd = (move(F.apply_torsions(m["x"], q, s, a + e)) - move(F.apply_torsions(m["x"], q, s, a - e))) / (2 * h)
            diff = (fd - J[:, :, t]).reshape(-1)
            exact += np.abs(diff).max() <= 1e-7 * max(1.0, np.abs(X - X.mean(0)).max())
            rest = diff - rigid @ np.linalg.lstsq(rigid, diff, rcond=None)[0]
            assert np.abs(rest).max() <= 1e-7 * max(1.0, np.abs(X - X.mean(0)).max()), (m["name"], t)
        assert exact >= 1                                                # (the last torsion of the plan needs no rigid part)
        c = X.mean(0)
        for d in range(3):
            e = np.zeros(3)
            e[d] = 1.0
            assert np.abs(J[:, :, T + d] - e).max() == 0
            rot = lambda v: (X - c) + np.cross(v[None, :], X - c) + c          # first order in |v|: linear, any step serves
            fd = (rot(e) - rot(-e)) / 2.0
            assert np.abs(J[:, :, T + 3 + d] - fd).max() <= 1e-12 * max(1.0, np.abs(X).max())
        k_rows = [int(qq[2]) for qq in q]
        assert all(not J[k, :, t].any() for t, k in enumerate(k_rows))     # k is on the axis: it never moves


def test_wrap():
    a = np.array([0.0, np.pi, -np.pi, 3 * np.pi, -3 * np.pi, 7.0, -7.0, 2 * np.pi])
    w = F.wrap(a)
    assert (w > -np.pi).all() and (w <= np.pi).all() and np.abs(np.exp(1j * w) - np.exp(1j * a)).max() <= 1e-15
    assert w[1] == np.pi and w[2] == np.pi


# ------------------------------------------------------------------------------------------------ the fit
def _experiment(amp, seed, noise=0.0, draws=4):
    rng = np.random.RandomState(seed)
    rows = []
    for m in _cases():
        for d in range(draws):
            y, clean, _ = F.make_target(m, rng, amp, noise)
            r64 = F.fit_one(m["x"], y, m["quad"], m["side"])
            r32 = F.fit_one(m["x"], y, m["quad"], m["side"], dt=np.float32)
            rows.append(dict(name=m["name"], y=y, clean=clean, x=m["x"], r64=r64, r32=r32))
    assert len(rows) == 52
    return rows


def _check_common(rows):
    for r in rows:
        for f in (r["r64"], r["r32"]):
            tr = f["trace"]
            assert all(b < a for a, b in zip(tr, tr[1:])) and len(tr) == f["iters"] <= 50         # strictly decreasing, no tolerance
            assert f["rmsd"] <= f["rmsd0"] and f["stop"] in (F.STOP_CONVERGED, F.STOP_CAP, F.STOP_REJECTED) and f["status"] == 0
            assert np.abs(f["angles"]).max() <= np.pi
            if tr:
                assert tr[0] < f["rmsd0"] ** 2 * len(r["x"]) and abs(np.sqrt(tr[-1] / len(r["x"])) - f["rmsd"]) <= 1e-12


def _steps_to(r, n, gate=1e-6):
    """Accepted steps until the RMSD is below `gate` (the steps after that sit at the rounding floor)."""
    return 1 + next(i for i, e in enumerate(r["trace"]) if np.sqrt(e / n) < gate)


# float32 moves the RMSD of a recovered case by its rounding floor: half an ulp of a coordinate of up to 16 A is 2^-24 * 8 = 4.8e-7 A,
# as a vector sqrt(3) times that, once for the centred conformer and once for the pose: 2e-6 A.  Past 0.3 rad the float32 run stops a
# few accepted steps short of the float64 one at that floor, which the measured 4.7e-6 / 6.3e-6 A show; the bounds are 3 and 4 floors.
@pytest.mark.parametrize("amp,seed,least,iters,to_gate,f32", [(0.3, 1, 52, 15, 7, 2e-6), (1.0, 1, 47, 30, None, 6e-6),
                                                             (np.pi, 1, 42, 30, None, 8e-6)])
def test_recovery_of_reachable_poses(amp, seed, least, iters, to_gate, f32):
    """The start conformer with every torsion changed by a uniform angle in +-amp, rotated and shifted: 52 of 52 cases come back to
    below 1e-6 A at 0.3 rad -- within 7 accepted steps, at most 13 in all, the rest at the rounding floor --, 47 at 1.0 rad, 43 at pi
    (asserted: the 42 of the first experiment); the rest stop in local minima, as a local method does.  Rounding the coordinates to
    float32 moves the RMSD of a recovered case by 1.7e-6 A at 0.3 rad, 4.7e-6 A at 1.0 rad and 6.3e-6 A at pi at most."""
    rows = _experiment(amp, seed)
    _check_common(rows)
    good = [r for r in rows if r["r64"]["rmsd"] < 1e-6]
    dev = max(abs(r["r32"]["rmsd"] - r["r64"]["rmsd"]) for r in good)
    steps = max(_steps_to(r["r64"], len(r["x"])) for r in good)
    print("amp %.2f: %d of %d recovered, below 1e-6 A within %d accepted steps, at most %d in all, float32 moves the rmsd by at most %.2e" % (
        amp, len(good), len(rows), steps, max(r["r64"]["iters"] for r in good), dev))
    assert len(good) >= least and max(r["r64"]["iters"] for r in good) <= iters
    assert to_gate is None or steps <= to_gate
    assert dev <= f32
    for r in good:
        assert F.rmsd(r["r64"]["coords"], r["y"]) < 1e-6                 # the coordinates, not only the reported number


def test_noisy_targets_are_fitted_better_than_rigidly():
    """+-0.5 rad plus Gaussian noise of 0.3 A per coordinate: the median RMSD of the fitted pose to the NOISE-FREE pose is 0.27 A; the
    noisy target itself sits at 0.52 A and the rigid fit of the start conformer at 0.40 A.  No case ends in another minimum under
    float32 coordinates (1e-3 A), and they move the final RMSD to the target by 8.7e-7 A at most: asserted below 2e-6 A, the rounding
    floor derived above -- this deviation is the yardstick of the GPU test of the noisy targets, so it is pinned here."""
    rows = _experiment(0.5, 2, noise=0.3)
    _check_common(rows)
    fit = np.median([F.rmsd(r["r64"]["coords"], r["clean"]) for r in rows])
    noisy = np.median([F.rmsd(r["y"], r["clean"]) for r in rows])
    rigid = np.median([F.rmsd(F.rigid_image(r["x"], r["y"]), r["clean"]) for r in rows])
    devs = [abs(r["r32"]["rmsd"] - r["r64"]["rmsd"]) for r in rows]
    print("noisy: fitted %.3f, target %.3f, rigid %.3f; float32 moves the rmsd by at most %.2e" % (fit, noisy, rigid, max(devs)))
    assert fit < 0.30 and 0.49 < noisy < 0.55 and 0.38 < rigid < 0.43
    assert all(d <= 1e-3 for d in devs)                                 # no other minimum
    assert max(devs) <= 2e-6                                            # the figure itself
    for r in rows:
        assert r["r64"]["rmsd"] < F.rmsd(F.rigid_image(r["x"], r["y"]), r["y"])


def test_limits_and_degenerate_ligands():
    rng = np.random.RandomState(4)
    for n, status in ((1, 0), (2, 0), (3, 0), (61, 0), (62, F.STATUS_TORSIONS), (257, F.STATUS_ATOMS)):
        m = R.chain(n)
        q, s, _ = R.plan(n, m["bonds"], m["codes"])                      # (no torsions for more than 256 atoms)
        x = R.embed(m, seed=n).astype(np.float64)
        y = x @ F.random_rotation(rng).T + 5.0
        r = F.fit_one(x, y, q, s, max_iters=3)
        assert r["status"] == status and r["rmsd"] <= r["rmsd0"] < 1e-9
        if status or n <= 3:
            assert r["iters"] == 0 and not r["angles"].any() and np.abs(r["coords"] - y).max() < 1e-9
    r = F.fit_one(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4), np.int32), np.zeros((0, 8), np.uint32))
    assert r["rmsd"] == 0 and r["iters"] == 0


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_stays_19_and_the_prototype_is_there():
    from fabind_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fabind_hip.h")).read()
    assert re.search(r"#define\s+FABIND_ABI_VERSION\s+19\b", hdr) and _lib.ABI_VERSION == 19
    m = re.search(r"\bint\s+fabind_conformer_fit\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S)
    assert m and m.group(1).strip().endswith("hipStream_t stream")
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["fabind_conformer_fit"]) == 23
    assert "conformer_fit.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "conformer_fit.hip"))
    src = open(os.path.join(build.CSRC, "conformer_fit.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", src) and "asm" not in re.sub(r"//[^\n]*", "", src)
    from fabind_amd import conformer
    from fabind_amd.utils import post_optim_utils
    assert callable(conformer.fit_conformers) and callable(post_optim_utils.torsion_fit_compound_coords_batched)
    assert conformer.MAX_FIT_TORSIONS == F.MAX_TORSIONS and conformer.MAX_ATOMS == F.MAX_ATOMS
    assert set(conformer.STOP) == {F.STOP_CONVERGED, F.STOP_CAP, F.STOP_REJECTED} and {3, 4} <= set(conformer.STATUS)
