"""CPU: pins tests/relax_refs.py, the numpy restatement that tests/test_gpu_relax.py compares fabind_amd.relax.relax_poses with -- the
gradient against central finite differences of E, the normal matrix, the energy pieces against contact_refs.close_pairs and by hand,
the trace, the host experiment behind the defaults on the committed case list, the recorded results of tests/golden/relax_cases.npz,
the margins of the GPU inputs -- and the header, binding and build-list entries of the new entry point."""
import os
import re

import numpy as np
import pytest

import contact_refs as C
import fit_refs as F
import relax_refs as X
from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def res():
    return X.Results(load_npz("conformer_ligands"))


@pytest.fixture(scope="module")
def gold():
    return load_npz("relax_cases")


def _state(res, k, s):
    """A pose of case (k, s) with both clash terms active: the start of the relaxation (the Horn fit under the fit's angles)."""
    c = res.cx[k]
    m = c["mol"]
    y, fit, _ = res.run(k, s)
    y64 = y.astype(np.float64)
    cy = y64.mean(0)
    x0c = np.asarray(m["x"], np.float64) - np.asarray(m["x"], np.float64).mean(0)
    a = fit["angles"].astype(np.float32).astype(np.float64)
    q, cp, cyc = X.horn_quat(F.apply_torsions(x0c, m["quad"], m["side"], a), y64 - cy)
    t = cyc - F.quaternion_rotation(q) @ cp
    P, rp = c["kept"][0].astype(np.float64) - cy, c["kept"][1]
    return dict(m=m, x0c=x0c, yc=y64 - cy, a=a, q=q, t=t, P=P, rp=rp, rl=c["vplan"]["radii"], clash=c["vplan"]["cls"] == 3)


def _E(st, theta, c):
    T = len(st["a"])
    q, t = X.rigid_step(st["q"], st["t"], c, theta[T:T + 3], theta[T + 3:])
    Xp = X.pose(st["x0c"], st["m"]["quad"], st["m"]["side"], st["a"] + theta[:T], q, t)
    return X.total(X.terms(Xp, st["yc"], st["P"], st["rp"], st["rl"], st["clash"])[0])


@pytest.mark.parametrize("k,s", [(10, 1), (7, 1), (1, 0), (8, 1)])
def test_gradient_is_that_of_E_and_H_is_positive_semidefinite(res, k, s):
    st = _state(res, k, s)
    Xp = X.pose(st["x0c"], st["m"]["quad"], st["m"]["side"], st["a"], st["q"], st["t"])
    sums, A, b = X.terms(Xp, st["yc"], st["P"], st["rp"], st["rl"], st["clash"])
    assert sums[1] > 0 and sums[2] > 0                                   # both clash terms are active at this pose
    H, g = X.normal_equations(Xp, A, b, st["m"]["quad"], st["m"]["side"])
    c = Xp.mean(0)
    M = len(g)
    fd = np.zeros(M)
    for j in range(M):
        e = np.zeros(M)
        e[j] = 1e-6
        fd[j] = (_E(st, e, c) - _E(st, -e, c)) / 2e-6
    scale = np.abs(fd).max()
    print("case (%d, %d): |grad| max %.3e, largest deviation of -2 g from central differences %.3e" % (k, s, scale, np.abs(fd + 2 * g).max()))
    assert np.abs(fd + 2.0 * g).max() <= 1e-6 * scale                    # (central differences with h = 1e-6: h^2 E''' and 2^-52 E / h)
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-12 * np.abs(H).max()
    for Ai in A:                                                         # every A_i is positive semi-definite on its own
        assert np.linalg.eigvalsh(Ai).min() >= -1e-12 * np.abs(Ai).max()


def test_energy_pieces_against_close_pairs_and_by_hand(res):
    w = X._w({})
    for k, s in ((10, 1), (8, 1), (13, 2)):
        c = res.cx[k]
        y, fit, _ = res.run(k, s)
        pose = fit["coords"].astype(np.float32)
        rl, (px, pr) = c["vplan"]["radii"].astype(np.float64), c["kept"]
        sums, l1 = X.energy_of(pose, y, c["vplan"]["cls"], c["vplan"]["radii"], px, pr)
        i, j, d2 = C.close_pairs(pose, px, w["c_prot"] * (rl.max() + pr.max()))
        rho = np.maximum(0.0, w["c_prot"] * (rl[i] + pr[j].astype(np.float64)) - np.sqrt(d2))
        assert len(i) and abs(sums[1] - (rho ** 2).sum()) <= 1e-9 * max(1.0, sums[1])     # (the frame shift costs 2^-53 x 60 A per distance)
        ii, jj = np.nonzero(np.triu(c["vplan"]["cls"] == 3, 1))
        d = np.linalg.norm(pose[ii].astype(np.float64) - pose[jj].astype(np.float64), axis=1)
        assert abs(sums[2] - (np.maximum(0.0, w["c_intra"] * (rl[ii] + rl[jj]) - d) ** 2).sum()) <= 1e-9 * max(1.0, sums[2])
        assert abs(sums[0] - ((pose.astype(np.float64) - y.astype(np.float64)) ** 2).sum()) <= 1e-9 * max(1.0, sums[0]) and l1 > 0
    # one atom against one atom: X = 0, P = (2, 0, 0), both carbon: reach = 0.8 x 3.4 = 2.72, rho = 0.72, n = (-1, 0, 0)
    sums, A, b = X.terms(np.zeros((1, 3)), np.zeros((1, 3)), np.array([[2.0, 0.0, 0.0]]), np.float32([1.7]), np.float32([1.7]), None)
    reach = float(w["c_prot"]) * (float(np.float32(1.7)) * 2)
    assert sums[0] == 0 and sums[2] == 0 and abs(sums[1] - (reach - 2.0) ** 2) <= 1e-15 and abs(sums[1] - 0.72 ** 2) <= 1e-6
    assert np.allclose(A[0], np.diag([1.0 + 100.0, 1.0, 1.0]), atol=1e-12) and np.allclose(b[0], [-100.0 * (reach - 2.0), 0.0, 0.0], atol=1e-12)
    # two ligand atoms of a clash pair 2 A apart: reach 0.75 x 3.4 = 2.55; the gradient is exact, A the majorant 2 w n n^T on both
    cl = np.array([[False, True], [True, False]])
    sums, A, b = X.terms(np.array([[0.0, 0, 0], [0.0, 2.0, 0]]), np.array([[0.0, 0, 0], [0.0, 2.0, 0]]), None, None, np.float32([1.7, 1.7]), cl)
    ri = 0.75 * 2 * float(np.float32(1.7)) - 2.0
    assert abs(sums[2] - ri ** 2) <= 1e-15 and np.allclose(b, [[0, -100.0 * ri, 0], [0, 100.0 * ri, 0]], atol=1e-12)
    assert np.allclose(A[0], np.diag([1.0, 201.0, 1.0])) and np.allclose(A[1], A[0])
    # a pair at distance 0 has its energy and no direction; a pair at the reach is inactive
    sums, A, b = X.terms(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), np.float32([1.7]), np.float32([1.7]), None)
    assert abs(sums[1] - reach ** 2) <= 1e-15 and np.array_equal(A[0], np.eye(3)) and not b.any()
    sums, _, _ = X.terms(np.zeros((1, 3)), np.zeros((1, 3)), np.array([[reach, 0.0, 0.0]]), np.float32([1.7]), np.float32([1.7]), None)
    assert sums[1] == 0.0


def test_rigid_step_and_limits():
    rng = np.random.RandomState(5)
    q = rng.randn(4); q /= np.linalg.norm(q)
    t, c, tau, om = rng.randn(3), rng.randn(3), rng.randn(3) * 0.1, rng.randn(3) * 0.2
    p = rng.randn(7, 3)
    X0 = p @ F.quaternion_rotation(q).T + t
    q2, t2 = X.rigid_step(q, t, c, tau, om)
    Re = F.quaternion_rotation(X.quat_exp(om))
    assert np.allclose(p @ F.quaternion_rotation(q2).T + t2, (X0 - c) @ Re.T + c + tau, atol=1e-13) and abs(q2 @ q2 - 1) < 1e-15
    h = 1e-6                                                              # the rotation columns of the Jacobian: e_d x (X - c)
    qh, th = X.rigid_step(q, t, c, np.zeros(3), np.array([h, 0, 0]))
    assert np.allclose((p @ F.quaternion_rotation(qh).T + th - X0) / h, np.cross([1.0, 0, 0], X0 - c), atol=1e-5)
    # the limits: more than 256 atoms -> the Horn image, more than 58 torsions -> rigid; a NaN target -> NaN and stop code 3
    import conformer_refs as R
    big = R.embed(R.chain(257), seed=1).astype(np.float64)
    y = big @ F.random_rotation(rng).T + 3.0
    o = X.relax_one(big, y, np.zeros((0, 4), int), np.zeros((0, 8), int), None, np.full(257, 1.7, np.float32), vstatus=3)
    assert o["status"] == X.STATUS_ATOMS | X.NO_INTRA and o["iters"] == 0 and np.isnan(o["energy"][1:]).all() and o["energy"][0] < 1e-20
    o = X.relax_one(big[:5], np.full((5, 3), np.nan), np.zeros((0, 4), int), np.zeros((0, 8), int), np.zeros((5, 5)), np.full(5, 1.7, np.float32))
    assert o["stop"] == X.STOP_NONFINITE and np.isnan(o["coords"]).all() and np.isnan(o["energy"]).all()


def test_committed_cases_meet_the_conditions_and_match_the_recorded_results(res, gold):
    assert [tuple(c) for c in gold["cases"]] == list(X.CASES) and len(X.CASES) >= 24
    rows = [res.row(k, s) for k, s in X.CASES]
    seen = set()
    for i, ((k, s), r) in enumerate(zip(X.CASES, rows)):
        _, fit, o64 = res.run(k, s)
        _, _, o32 = res.run(k, s, np.float32)
        assert r["d32"] <= 1e-3, (k, s, r["d32"])                        # the float32-pose restatement ends at the float64 one
        for o in (o64, o32):
            tr = np.asarray(o["trace"])
            assert len(tr) == o["iters"] >= 1 and (np.diff(tr) < 0).all() and tr[0] < X.total(o["energy0"]) and tr[-1] == X.total(o["energy"])
            seen.add(o["stop"])
        a0 = gold["angles0"][gold["angle_off"][i]:gold["angle_off"][i + 1]]
        assert np.abs(a0 - fit["angles"].astype(np.float32)).max(initial=0) <= 1e-5
        assert abs(gold["E64"][i] - r["E64"]) <= 1e-6 * max(1.0, r["E64"]), (k, s, gold["E64"][i], r["E64"])
        assert F.rmsd(gold["coords64"][gold["atom_off"][i]:gold["atom_off"][i + 1]], o64["coords"]) <= 1e-5
        for f in ("prot0", "prot1", "clash0", "clash1"):
            assert gold[f][i] == r[f] or abs(gold[f][i] - r[f]) <= 1e-6, (k, s, f)
    yard = max(abs(r["E64"] - r["E32"]) for r in rows)
    gyard = float(np.abs(gold["E32"] - gold["E64"]).max())
    print("yardstick max |E32 - E64|: %.3e now, %.3e recorded; largest d32 %.2e A; stop codes %s" % (yard, gyard, max(r["d32"] for r in rows), sorted(seen)))
    assert 0 < yard <= 1e-4 and 0 < gyard <= 1e-4 and (gold["d32"] <= 1e-3).all()
    # the margins of the GPU effect test: at least 12 cases start flagged and end clear of both thresholds by 1e-3
    eff = [r for r in rows if r["flagged0"] and r["clean1"]]
    geff = ((gold["prot1"] >= 0.751) & (gold["clash1"] >= 0.701) & ((gold["prot0"] < 0.75) | (gold["clash0"] < 0.70))).sum()
    print("effect: %d of %d cases start flagged and end clean (%d recorded)" % (len(eff), len(rows), geff))
    assert len(eff) >= 12 and geff == len(eff)


# the host experiment behind the defaults, protein term only, on the committed case list: (w_prot, c_prot) -> targets with
# prot_clash < 0.75 before, after, and the median RMSD to the target (A)
TABLE = {(10.0, 0.80): (18, 7, 0.142), (100.0, 0.80): (18, 0, 0.160), (100.0, 0.85): (18, 0, 0.276), (1000.0, 0.80): (18, 0, 0.163)}


@pytest.mark.parametrize("w_prot,c_prot", sorted(TABLE))
def test_the_experiment_behind_the_defaults(res, w_prot, c_prot):
    before = after = 0
    rm = []
    for k, s in X.CASES:
        c = res.cx[k]
        y, fit, o = res.run(k, s, w_prot=w_prot, c_prot=c_prot, w_intra=0.0)
        before += X.prot_clash(fit["coords"], c["vplan"]["radii"], *c["kept"]) < 0.75
        after += X.prot_clash(o["coords"], c["vplan"]["radii"], *c["kept"]) < 0.75
        rm.append(F.rmsd(o["coords"], y))
        assert o["iters"] <= 100
    print("w_prot %g c_prot %g: %d -> %d of %d, median RMSD %.3f A" % (w_prot, c_prot, before, after, len(X.CASES), np.median(rm)))
    want = TABLE[(w_prot, c_prot)]
    assert (before, after) == want[:2] and abs(np.median(rm) - want[2]) <= 2e-3


def test_header_binding_and_build_list_name_the_entry_point():
    from fabind_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    assert re.search(r"\bint\s+fabind_pose_relax\s*\(", hdr) and "csrc/pose_relax.hip" in hdr
    assert "fabind_pose_relax" in _lib.SIGNATURES and len(_lib.SIGNATURES["fabind_pose_relax"]) == 42
    assert "pose_relax.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pose_relax.hip"))
    src = open(os.path.join(build.CSRC, "pose_relax.hip")).read()
    assert 'extern "C" int fabind_pose_relax(' in src and "atomicAdd" not in src and "asm" not in src.replace("assume", "")
    users = [f for f in ("kernels.py", "relax.py") if ".fabind_pose_relax(" in open(os.path.join(ROOT, "fabind_amd", f)).read()]
    assert users == ["kernels.py"]
