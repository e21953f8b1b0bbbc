"""CPU: the numpy restatement of fabind_amd.validity (tests/validity_refs.py) pinned on molecules whose answers are known by
inspection and on the four crystal ligands of tests/golden/conformer_ligands.npz; the margins the GPU flag test relies on; the
consumers of plus/metrics.py (plain torch) against their restatement; the new entry points in header, binding and build list."""
import os
import re

import numpy as np
import pytest
import torch

import conformer_refs as R
import validity_refs as V
from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crystal():
    g = load_npz("conformer_ligands")
    out = []
    for m in R.fixture_molecules(g):
        z = np.asarray(g[m["name"] + "_z"], np.int64)
        out.append((m, z, V.plan(m, z, m["x"])))
    return out


def test_crystal_ligands_pass_every_check(crystal):
    """The figures a numpy run with these definitions gave on the crystal poses: lowest clash ratio 0.878, largest aromatic deviation
    0.044 A, largest qualifying double-bond deviation 0.093 A, smallest kept stereo-centre volume 2.29 A^3."""
    st = np.stack([V.stats(pl, m["x"]) for m, _, pl in crystal])
    for (m, _, pl), s in zip(crystal, st):
        assert pl["status"] == 0 and V.flags(pl, m["x"], s) == 0, m["name"]
        np.testing.assert_allclose(s[:4], 1.0, rtol=0, atol=2 * V.U)      # d0 comes from float32 differences, the pose's from float64
        assert s[7] == pytest.approx(1.0, abs=8 * V.U) and s[8] == np.inf
    assert st[:, 4].min() == pytest.approx(0.878, abs=5e-4)
    assert st[:, 5].max() == pytest.approx(0.044, abs=5e-4)
    assert st[:, 6].max() == pytest.approx(0.093, abs=5e-4)
    vols = [abs(c[5]) for _, _, pl in crystal for c in pl["centres"]]
    assert min(vols) == pytest.approx(2.29, abs=5e-3)


def test_sulfonyl_and_phosphoryl_double_bonds_are_no_planar_groups(crystal):
    excluded = 0
    for m, z, pl in crystal:
        nb, code = R._adjacency(m["n"], m["bonds"], m["codes"])
        doubles = [k for k, c in code.items() if c == R.DOUBLE]
        hetero = [k for k in doubles if any(int(z[a]) in (15, 16) for a in k)]
        crowded = [k for k in doubles if k not in hetero and any(len(nb[a]) > 3 for a in k)]
        excluded += len(hetero)
        assert len([1 for k, _ in pl["groups"] if k == 1]) == len(doubles) - len(hetero) - len(crowded), m["name"]
    assert excluded >= 2


def test_hand_molecules():
    plans = {}
    for name in R.hand_molecules():
        m, z = V.hand(name)
        plans[name] = (m, V.plan(m, z, R.embed(m, seed=3)))
    groups = lambda name: plans[name][1]["groups"]
    assert groups("biphenyl") == [(0, [0, 1, 2, 3, 4, 5]), (0, [6, 7, 8, 9, 10, 11])]
    assert groups("but-2-ene") == [(1, [0, 1, 2, 3])]
    assert groups("N-methylacetamide") == [(1, [0, 1, 2, 3])]
    assert groups("cyclohexane") == [] and groups("decalin") == []
    # hop classes by inspection: butane 0-1-2-3
    np.testing.assert_array_equal(plans["butane"][1]["cls"], [[0, 1, 2, 0], [1, 0, 1, 2], [2, 1, 0, 1], [0, 2, 1, 0]])
    # pentane chain of the two-fragment ligand (atoms 4..8): 4-8 are four bonds apart; every cross-fragment pair is a clash pair
    cls = plans["two-fragment"][1]["cls"]
    assert cls[4, 8] == 3 and cls[4, 7] == 0 and cls[4, 6] == 2 and cls[4, 5] == 1
    assert (cls[:4, 4:] == 3).all() and (cls[4:, :4] == 3).all() and (cls == cls.T).all()
    # cyclohexane: the ring makes 0-3 three bonds apart both ways, nothing further
    assert (plans["cyclohexane"][1]["cls"] == 3).sum() == 0
    # ratio pairs are exactly the bonded and 1-3 pairs the conformer tests use
    for name, (m, pl) in plans.items():
        assert [(i, j) for i, j, _, _ in pl["pairs"]] == [tuple(p) for p in R.bonded_and_13_pairs(m)], name
    # no stereo centres in these: every atom has at most three neighbours and the embedding is not tetrahedral by design
    assert plans["butane"][1]["centres"] == []


def test_limits():
    m = R.chain(257)
    assert V.plan(m, [6] * 257, R.embed(m, 1))["status"] == 3
    m = R.chain(256)
    assert V.plan(m, [6] * 256, R.embed(m, 1))["status"] == 0
    m = R.chain(3)
    x = R.embed(m, 1)
    x[2] = x[0]                                                        # a 1-3 pair at distance 0
    assert V.plan(m, [6] * 3, x)["status"] == 5
    pl = V.plan(R.mol(0, []), [], np.zeros((0, 3), np.float32))
    st = V.stats(pl, np.zeros((0, 3), np.float32))
    np.testing.assert_array_equal(st, [np.inf, -np.inf, np.inf, -np.inf, np.inf, 0, 0, np.inf, np.inf])
    assert V.flags(pl, np.zeros((0, 3)), st) == 0


def test_radii_table_and_override():
    m = R.chain(4)
    z = [6, 16, 53, 99]
    np.testing.assert_array_equal(V.plan(m, z, R.embed(m, 1))["radii"], np.asarray([1.70, 1.80, 1.98, 2.00], np.float32))
    np.testing.assert_array_equal(V.plan(m, z, R.embed(m, 1), radii=[1, 2, 3, 4])["radii"], np.asarray([1, 2, 3, 4], np.float32))


def test_mirror_image_inverts_every_centre_and_keeps_every_distance(crystal):
    for m, _, pl in crystal:
        x = m["x"].astype(np.float64)
        a, b = V.stats(pl, m["x"]), V.stats(pl, (x * [-1.0, 1.0, 1.0]).astype(np.float32))
        assert len(pl["centres"]) >= 2
        assert b[7] == pytest.approx(-1.0, abs=1e-12)
        np.testing.assert_allclose(np.delete(b, 7), np.delete(a, 7), rtol=1e-12, atol=1e-12)
        assert V.flags(pl, m["x"], b) == V.CHIRALITY


def test_isopropyl_centre_needs_the_automorphisms_to_be_dropped():
    m, z = V.isopentane()
    autos = V.automorphisms(m, z)
    assert len(autos) == 2
    kept = V.plan(m, z, m["x"])["centres"]
    assert [c[:5] for c in kept] == [(0, 1, 2, 3, -1)] and abs(kept[0][5]) > 2.0
    assert V.plan(m, z, m["x"], autos=autos)["centres"] == []
    # the identity alone drops nothing; a small min_volume keeps flat centres out either way
    assert len(V.plan(m, z, m["x"], autos=autos[:1])["centres"]) == 1
    assert V.plan(m, z, m["x"], min_volume=3.0)["centres"] == []


def test_test_poses_keep_their_distance_from_every_threshold():
    """What the GPU flag test relies on: over every molecule and pose of the statistics world no statistic lies within 16 bounds of a
    threshold, with and without the C-alpha check, and every planar group has the eigenvalue gap the flatness bound assumes."""
    g = load_npz("conformer_ligands")
    mols = V.world_molecules(g)
    pocket, pbatch = V.make_pocket(mols, V.POCKET_COUNTS, seed=5)
    seen = 0
    closest = np.inf
    for b, (m, z) in enumerate(mols):
        pl = V.plan(m, z, m["x"])
        poses = V.make_poses(m, pl, seed=100 + b)
        for s in range(V.N_POSES):
            st = V.stats(pl, poses[s], pocket[pbatch == b])
            if pl["status"] != 0:
                assert np.isnan(st).all()
                continue
            assert V.min_gap(pl, poses[s]) >= V.MIN_GAP, (m["name"], s)
            for col, v, thr in V.threshold_gaps(st, ca_min=V.CA_MIN):
                frac = abs(v - thr) / (16 * max(V.bound(col, v), V.bound(col, thr)))
                closest = min(closest, frac)
                assert frac > 1.0, (m["name"], V.POSE_KINDS[s], V.STATS[col], v, thr)
                seen += 1
    print("closest statistic: %.3g x 16 bounds from its threshold over %d comparisons" % (closest, seen))
    assert seen > 300


def test_test_poses_raise_the_flags_they_were_built_for():
    g = load_npz("conformer_ligands")
    mols = V.world_molecules(g)
    hit = {k: 0 for k in V.POSE_KINDS}
    for b, (m, z) in enumerate(mols[:5]):
        pl = V.plan(m, z, m["x"])
        poses = V.make_poses(m, pl, seed=100 + b)
        f = [V.flags(pl, poses[s], V.stats(pl, poses[s])) for s in range(V.N_POSES)]
        if b < 4:
            assert f[0] == 0, m["name"]
            assert f[1] & ~V.CLASH == 0 and f[8] & ~V.CLASH == 0        # a torsion change keeps everything but may clash
            assert f[2] & V.BOND and f[3] == V.CHIRALITY and f[4] == 0
            assert f[5] & (V.BOND | V.ANGLE)
        if any(k == 0 for k, _ in pl["groups"]):
            assert f[6] & V.AROMATIC_FLAT
            hit["aromatic-push"] += 1
        if m["name"] == "two-fragment":
            assert f[7] & V.CLASH
            hit["overlay"] += 1
    assert hit["aromatic-push"] >= 2 and hit["overlay"] == 1


def test_select_valid_restatement_by_hand():
    rmsd = np.array([[1.0], [2.0], [3.0], [4.0]])
    conf = np.array([[0.9], [0.8], [0.8], [0.1]])
    valid = np.array([[False], [False], [True], [True]])
    r, c, picks = V.select_valid(rmsd, rmsd * 10, conf, valid, 3)
    assert picks[:, 0].tolist() == [2, 3, 0] and r[0] == 1.0 and c[0] == 10.0


def test_consumers_on_the_host():
    V.check_consumers(torch.device("cpu"))


def test_entry_points_are_declared_bound_and_built():
    from fabind_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    assert "#define FABIND_ABI_VERSION 19" in hdr and _lib.ABI_VERSION == 19
    for nm in ("fabind_validity_plan", "fabind_pose_check"):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % nm, hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[nm]), nm
    assert "pose_check.hip" in build.SOURCES
    from fabind_amd import validity
    assert validity.STATS == V.STATS and validity.MAX_ATOMS == V.MAX_ATOMS
    assert [validity.FLAGS[k] for k in ("BOND", "ANGLE", "CLASH", "AROMATIC_FLAT", "DOUBLE_FLAT", "CHIRALITY", "PROTEIN", "NONFINITE",
                                        "UNCHECKED")] == [1, 2, 4, 8, 16, 32, 64, 128, 256]
