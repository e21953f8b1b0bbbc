"""CPU: the restatement tests/embed_refs.py of fabind_amd.embed (csrc/embed.hip) -- the distance-geometry rules against their own
properties, against the crystal ligands of tests/golden/conformer_ligands.npz (the external check), and the host experiment behind the
defaults of `embed_conformers` (DESIGN.md section 20 records the figures this file prints)."""
import os
import re

import numpy as np
import pytest

import conformer_refs as C
import embed_refs as E
from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(16)
SMALL = ("ethane", "propane", "butane", "cyclopropane", "cyclobutane", "cyclopentane", "benzene", "biphenyl", "naphthalene", "norbornane",
         "spiro", "acetamide", "acetonitrile", "sulfone", "two-fragment")


def crystal():
    g = load_npz("conformer_ligands")
    return [(m, np.asarray(g[m["name"] + "_z"], np.int64)) for m in C.fixture_molecules(g)]


def all_cases():
    """name -> (molecule, z): the hand molecules and the four crystal ligands, in a fixed order (the index is the ligand's key)."""
    out = dict(E.hand_molecules())
    for m, z in crystal():
        out[m["name"]] = (m, z)
    return out


@pytest.fixture(scope="module")
def plans():
    return {k: E.bounds(m, z) for k, (m, z) in all_cases().items()}


def test_statuses_and_shapes(plans):
    assert plans["chain257"]["status"] == 3 and plans["chain257"]["bounds"].size == 0
    for k, p in plans.items():
        if k != "chain257":
            assert p["status"] == 0, k
            assert p["bounds"].shape == (p["n"], p["n"]) and p["bounds"].dtype == np.float32
            assert p["quads"].shape[1] == 4 and len(p["quad_lo"]) == len(p["quads"]) == len(p["quad_hi"])
    assert plans["empty"]["n"] == 0 and plans["atom"]["bounds"].tolist() == [[0.0]]
    assert len(plans["propane"]["quads"]) == 0


def test_geometry_classes_and_rule_values(plans):
    assert plans["acetonitrile"]["geom"].tolist() == [E.TETRA, E.LINEAR, E.LINEAR]
    assert plans["acetamide"]["geom"].tolist() == [E.TETRA, E.TRIGONAL, E.TRIGONAL, E.TRIGONAL]      # the conjugated N is TRIGONAL
    assert plans["sulfone"]["geom"].tolist() == [E.TETRA, E.TETRA, E.TRIGONAL, E.TRIGONAL, E.TETRA]  # a 4-neighbour S stays TETRA
    assert set(plans["benzene"]["geom"].tolist()) == {E.TRIGONAL}
    U, L = E.unpack_bounds(E.bounds(*E.hand_molecules()["butane"], smooth=False)["bounds"])
    assert U[0, 1] == np.float32(1.51) and L[0, 1] == np.float32(1.49)
    d13 = np.sqrt(1.5 * 1.5 + 1.5 * 1.5 - 2 * 1.5 * 1.5 * (-1.0 / 3.0))
    assert abs(U[0, 2] - (d13 + 0.04)) < 1e-6 and abs(L[0, 2] - (d13 - 0.04)) < 1e-6
    assert 2.4 < L[0, 3] < 2.7 and 3.8 < U[0, 3] < 4.0                                              # cis - 0.06, trans + 0.06
    U, L = E.unpack_bounds(E.bounds(*E.hand_molecules()["cyclopropane"], smooth=False)["bounds"])
    assert U[0, 2] == np.float32(1.51)                                                               # a 3-ring has no 1-3 pair
    U, L = E.unpack_bounds(E.bounds(*E.hand_molecules()["cyclobutane"], smooth=False)["bounds"])
    assert abs(U[0, 2] - (1.5 * np.sqrt(2.0) + 0.04)) < 1e-6                                         # 90 degrees
    U, L = E.unpack_bounds(E.bounds(*E.hand_molecules()["benzene"], smooth=False)["bounds"])
    assert abs(U[0, 3] - L[0, 3] - 0.12) < 1e-6 and abs(0.5 * (U[0, 3] + L[0, 3]) - 2 * 1.39) < 1e-6  # para: cis for both, flat ring
    U, L = E.unpack_bounds(E.bounds(*E.hand_molecules()["two-fragment"], smooth=False)["bounds"])
    assert U[0, 5] == np.float32(10.0) and L[0, 5] == np.float32(3.4) and U[4, 8] == np.float32(1000.0)
    assert L[4, 8] == np.float32(np.float64(np.float32(1.7)) * 2 * 0.8)                              # four bonds apart


def test_bounds_are_consistent_smoothed_and_idempotent(plans):
    for k in SMALL + ("chain64", "6ckl", "6g3c"):
        p = plans[k]
        U, L = E.unpack_bounds(p["bounds"])
        n = p["n"]
        off = ~np.eye(n, dtype=bool)
        assert (L[off] <= U[off]).all() and (L[off] > 0).all(), k
        if n <= 30:
            for i in range(n):                                          # every triple, in float32 exactly (smoothing runs to its fixed point)
                for j in range(n):
                    if i != j:
                        assert (U[i, j] <= (U[i] + U[:, j]).astype(np.float32)).all(), (k, i, j)
                        assert (L[i, j] >= (L[i] - U[:, j]).astype(np.float32)).all(), (k, i, j)
        passes = []
        U2, L2 = E.smooth_bounds(U, L, passes)
        np.testing.assert_array_equal(U2, U, err_msg=k)
        np.testing.assert_array_equal(L2, L, err_msg=k)
        assert passes == [1, 1]
    for k, p in plans.items():
        if p["status"] == 0 and p["n"] > 1:
            passes = []
            E.smooth_bounds(*E.unpack_bounds(E.bounds(*all_cases()[k], smooth=False)["bounds"]), passes)
            assert max(passes) < E.SMOOTH_PASSES, (k, passes)          # every case reaches the fixed point before the cap


def test_a_renumbered_molecule_gives_the_renumbered_bounds():
    rng = np.random.RandomState(5)
    cases = all_cases()
    for k in ("biphenyl", "norbornane", "acetamide", "two-fragment", "6g3c", "6efk"):
        m, z = cases[k]
        n = m["n"]
        perm = rng.permutation(n)                                       # new id of old atom a = perm[a]
        m2 = C.mol(n, perm[m["bonds"]], m["codes"], k)
        z2 = np.zeros(n, np.int64)
        z2[perm] = np.asarray(z)
        raw, raw2 = E.bounds(m, z, smooth=False), E.bounds(m2, z2, smooth=False)
        for a, b in zip(E.unpack_bounds(raw["bounds"]), E.unpack_bounds(raw2["bounds"])):
            np.testing.assert_array_equal(a, b[np.ix_(perm, perm)], err_msg=k)                       # the rules: the same bits
        np.testing.assert_array_equal(raw["geom"], raw2["geom"][perm])
        sm, sm2 = E.bounds(m, z), E.bounds(m2, z2)
        for a, b in zip(E.unpack_bounds(sm["bounds"]), E.unpack_bounds(sm2["bounds"])):
            # smoothing sums the same path in another order of k: at most 2 (n - 1) 2^-24 of the longest path's sum
            assert (np.abs(a - b[np.ix_(perm, perm)]) <= 2 * n * 2.0 ** -24 * np.abs(a).max()).all(), k


def test_external_check_against_the_crystal_ligands():
    """The rules against deposited coordinates: at least 90 % of the bonded pairs within 0.15 A of d0, at least 90 % of the 1-3 pairs
    within 0.30 A of the rule's distance, no pair four or more bonds apart more than 0.3 A below its smoothed lower bound."""
    nb_ok = nb_all = na_ok = na_all = 0
    worst_b = worst_a = worst_far = 0.0
    for m, z in crystal():
        x = m["x"].astype(np.float64)
        d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
        nb, _ = E.adjacency(m)
        h = E.hop_matrix(m["n"], nb)
        Ur, Lr = E.unpack_bounds(E.bounds(m, z, smooth=False)["bounds"])
        mid = 0.5 * (Ur.astype(np.float64) + Lr.astype(np.float64))
        iu = np.triu_indices(m["n"], 1)
        b, a = h[iu] == 1, h[iu] == 2
        nb_ok += int((np.abs(d[iu] - mid[iu])[b] <= 0.15).sum()); nb_all += int(b.sum())
        na_ok += int((np.abs(d[iu] - mid[iu])[a] <= 0.30).sum()); na_all += int(a.sum())
        worst_b = max(worst_b, float(np.abs(d[iu] - mid[iu])[b].max()))
        worst_a = max(worst_a, float(np.abs(d[iu] - mid[iu])[a].max()))
        _, L = E.unpack_bounds(E.bounds(m, z)["bounds"])
        far = h[iu] >= 4
        worst_far = max(worst_far, float((L[iu].astype(np.float64) - d[iu])[far].max()))
        assert d[iu][far].min() >= 2.8, m["name"]
    print("\ncrystal check: bonds %d / %d = %.1f %% within 0.15 A (worst %.2f), 1-3 pairs %d / %d = %.1f %% within 0.30 A (worst %.2f), "
          "largest lower-bound violation four or more bonds apart %.2f A"
          % (nb_ok, nb_all, 100.0 * nb_ok / nb_all, worst_b, na_ok, na_all, 100.0 * na_ok / na_all, worst_a, worst_far))
    assert nb_all == 145 and na_all == 209
    assert nb_ok >= 0.9 * nb_all
    assert na_ok >= 0.9 * na_all
    assert worst_far <= 0.3


def test_draws_are_the_hash_chain_of_the_conformer_kernel():
    u = E.draws(3, 7, 2, 1, np.arange(5))
    for i in range(5):
        h = C.hash32((3 & E.M32) + 0x9e3779b9)
        h = C.hash32((h ^ 7) + 0x85ebca6b)
        h = C.hash32((h ^ 2) + 0xc2b2ae35)
        h = C.hash32((h ^ 1) + 0x165667b1)
        h = C.hash32((h ^ i) + 0x27d4eb2f)
        assert u[i] == (h >> 8) / 16777216.0
    assert (E.draws(3, 7, 2, 1, np.arange(64)) != E.draws(3, 7, 3, 1, np.arange(64))).any()


def test_gradient_of_E_is_exact():
    m, z = all_cases()["6g3c"]
    p = E.bounds(m, z, E.chiral_signs(m, z, m["x"]))
    U, L = E.unpack_bounds(p["bounds"])
    q = p["quads"].astype(np.int64)
    x = E.initial_coords(p, 1, 2, 0, 0, 20)
    E0, g, _, _ = E.evaluate(x, U, L, q, p["quad_lo"], p["quad_hi"], 0.1, 0.1)
    rng = np.random.RandomState(0)
    for _ in range(6):
        d = rng.randn(*x.shape)
        h = 1e-6
        num = (E.evaluate(x + h * d, U, L, q, p["quad_lo"], p["quad_hi"], 0.1, 0.1)[0]
               - E.evaluate(x - h * d, U, L, q, p["quad_lo"], p["quad_hi"], 0.1, 0.1)[0]) / (2 * h)
        assert abs(num - float((g * d).sum())) <= 1e-5 * max(1.0, abs(num))


def test_host_experiment_every_case_embeds_at_the_defaults(plans):
    """The experiment behind the defaults: 16 seeds per hand molecule and crystal ligand reach status 0 within max_tries at viol_tol =
    0.1 A; at 0.05 A norbornane never does (its 1-3 bounds across the bridge disagree by 0.11 A), so 0.1 is the smallest of 0.05 /
    0.1 / 0.2 at which all succeed.  Prints the table of tries and steps that DESIGN.md section 20 records."""
    rows = []
    for key, (k, p) in enumerate(plans.items()):
        if p["status"] != 0 or p["n"] == 0:
            continue
        res = [E.embed(p, seed=s, key=key) for s in SEEDS]
        assert all(r["status"] == 0 for r in res), (k, [r["status"] for r in res])
        assert all(np.isfinite(r["coords"]).all() and r["viol"] <= E.DEFAULTS["viol_tol"] for r in res), k
        tries, steps = [r["tries"] for r in res], [r["steps"] for r in res]
        rows.append("%-13s n %3d  tries mean %.2f max %d  steps median %d max %d" % (k, p["n"], np.mean(tries), max(tries), np.median(steps),
                                                                                    max(steps)))
    print("\n" + "\n".join(rows))
    r = [E.embed(plans["norbornane"], seed=s, key=0, viol_tol=0.05, max_tries=2) for s in range(4)]
    assert all(x["status"] == 1 for x in r)


def test_stereo_terms_give_the_asked_hand():
    for m, z in crystal():
        cs = E.chiral_signs(m, z, m["x"])
        if not np.any(cs):
            continue
        for sign in (1, -1):
            p = E.bounds(m, z, sign * cs)
            r = E.embed(p, seed=4, key=1)
            assert r["status"] == 0, m["name"]
            got = E.chiral_signs(m, z, r["coords"])
            np.testing.assert_array_equal(got[cs != 0], (sign * cs)[cs != 0], err_msg=m["name"])
    assert sum(int(np.any(E.chiral_signs(m, z, m["x"]))) for m, z in crystal()) >= 2


def test_molecule_from_sdf_reads_v2000():
    from fabind_amd.embed import molecule_from_sdf
    text = "\n".join(["acetamide", "  test", "", "  5  4  0  0  0  0  0  0  0  0999 V2000",
                      "    0.0000    0.0000    0.0000 C   0  0", "    1.5000    0.0000    0.0000 C   0  0",
                      "    2.1000    1.1000    0.0000 O   0  0", "    2.2000   -1.1000    0.0000 N   0  0",
                      "   -0.5000    0.9000    0.0000 H   0  0", "  1  2  1  0", "  2  3  2  0", "  2  4  1  0", "  1  5  1  0", "M  END", "$$$$"])
    mol = molecule_from_sdf(text)
    assert mol["atomic_numbers"].tolist() == [6, 6, 8, 7] and mol["bonds"].tolist() == [[0, 1], [1, 2], [1, 3]]
    assert mol["bond_codes"].tolist() == [C.SINGLE, C.DOUBLE, C.SINGLE] and mol["coords"].shape == (4, 3)
    assert mol["coords"][2].tolist() == [np.float32(2.1), np.float32(1.1), 0.0]
    sym, xyz, bonds, codes = C.parse_v2000(text)
    assert bonds.tolist() == mol["bonds"].tolist() and codes.tolist() == mol["bond_codes"].tolist()
    with pytest.raises(ValueError):
        molecule_from_sdf("x\n\n\n  9  9  0  0  0  0  0  0  0  0999 V2000\n")


def test_c_abi_is_additive_and_has_one_call_site():
    from fabind_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    assert "#define FABIND_ABI_VERSION 19" in hdr and _lib.ABI_VERSION == 19
    src = open(os.path.join(ROOT, "fabind_amd", "csrc", "embed.hip")).read()
    for nm, nargs in (("fabind_embed_bounds", 20), ("fabind_embed_conformers", 28)):
        assert re.search(r"\bint\s+%s\s*\(" % nm, hdr) and len(_lib.SIGNATURES[nm]) == nargs
        assert 'extern "C" int %s(' % nm in src
        users = [f for f in sorted(os.listdir(os.path.join(ROOT, "fabind_amd"))) if f.endswith(".py")
                 and ".%s(" % nm in open(os.path.join(ROOT, "fabind_amd", f)).read()]
        assert users == ["kernels.py"], (nm, users)
    assert "atomicAdd" not in src and "asm" not in src.replace("assume", "")
    from fabind_amd.build import SOURCES
    assert "embed.hip" in SOURCES
