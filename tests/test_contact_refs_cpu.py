"""CPU: the float64 restatement of tests/contact_refs.py (what tests/test_gpu_protein_contacts.py holds the device to) against scipy's
cKDTree and hand cases, the PDB reader, the binding's tables, and the margins of the GPU inputs: no pair within 1e-6 A of the cutoff, no
lattice point with |d^2 - R^2| < 1e-9 A^2, no pair ratio within 1e-9 of clash_min, every flagged statistic at least 16 bounds from its
threshold -- so counts, pairs and flags must be equal exactly on the device."""
import os
import re

import numpy as np
import pytest

import contact_refs as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_set_equals_ckdtree_on_random_proteins():
    from scipy.spatial import cKDTree
    for seed, n, cutoff in ((1, 300, 5.0), (2, 800, 4.0), (3, 50, 2.5)):
        pxyz, pz = C.synthetic_protein(n, seed=seed, hydrogens=0.3)
        kx, _, _ = C.kept(pxyz, pz)
        rng = np.random.RandomState(seed)
        pose = (kx[rng.randint(0, len(kx), size=20)] + rng.uniform(-3, 3, size=(20, 3))).astype(np.float32)
        i, j, d2 = C.close_pairs(pose, kx, cutoff)
        got = set(zip(i.tolist(), j.tolist()))
        tree = cKDTree(kx.astype(np.float64))
        want = {(a, b) for a, near in enumerate(tree.query_ball_point(pose.astype(np.float64), cutoff)) for b in near}
        d = np.sqrt(((pose[:, None].astype(np.float64) - kx[None].astype(np.float64)) ** 2).sum(-1))
        assert np.abs(d - cutoff).min() > 1e-9                          # (no pair on the boundary: < and <= agree)
        assert got == want and len(got) > 20
        assert (d2 < cutoff * cutoff).all()


def test_one_atom_against_one_atom_at_a_known_distance():
    lig, prot = np.array([[0.0, 0.0, 0.0]], np.float32), np.array([[3.0, 4.0, 0.0], [0.25, 0.0, 0.0]], np.float32)
    r = C.contacts(lig, [1.7], prot, [8, 1])                           # the hydrogen at 0.25 A takes no part
    assert r["stats"][1] == np.inf and r["counts"][0] == 0 and r["pair"].tolist() == [-1, -1]     # d = 5 is not < cutoff
    r = C.contacts(lig, [1.7], prot, [8, 1], cutoff=5.5)
    assert r["stats"][1] == 5.0 and r["stats"][0] == 5.0 / (np.float64(np.float32(1.7)) + np.float64(np.float32(1.52)))
    assert r["pair"].tolist() == [0, 0] and r["flags"] == 0 and r["counts"][0] == 0
    r = C.contacts(lig, [1.7], np.array([[1.5, 0.0, 0.0]], np.float32), [6], cutoff=5.0)
    assert abs(r["stats"][0] - 1.5 / 3.4) < 1e-7 and r["counts"][0] == 1 and r["flags"] & C.CLASH
    r = C.contacts(lig, [1.7], lig, [6])                               # coincident: ratio 0
    assert r["stats"][0] == 0.0 and r["stats"][1] == 0.0 and r["stats"][2] == 1.0 and r["flags"] == C.CLASH | C.OVERLAP


def test_lattice_counts_of_two_overlapping_spheres_by_hand():
    # radius 1.25 A at scale 0.8 = 1.0 A, spacing 0.5: a sphere at the origin holds the k with |k|^2 <= 4: 1 + 6 + 12 + 8 + 6 = 33 points
    r = C.contacts(np.zeros((1, 3), np.float32), [1.25], np.zeros((0, 3), np.float32), [])
    assert r["counts"].tolist() == [0, 33, 0] and r["stats"][2] == 0.0 and r["stats"][0] == np.inf
    # a second ligand sphere at (1, 0, 0), k-centre (2, 0, 0): the union counts each point once.  Shared points: |k|^2 <= 4 and
    # |k - (2, 0, 0)|^2 <= 4, i.e. kx = 1 with ky^2 + kz^2 <= 3 (9 points), kx = 0 and kx = 2 with ky = kz = 0 (2 points): 11
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    r = C.contacts(two, [1.25, 1.25], np.zeros((0, 3), np.float32), [])
    assert r["counts"][1] == 33 + 33 - 11
    # the ligand sphere at the origin against a protein sphere at (1, 0, 0): 11 of its 33 points are protein points
    r = C.contacts(two[:1], [1.25], two[1:], [6], prot_r=[1.25])
    assert r["counts"].tolist() == [1, 33, 11] and r["stats"][2] == 11 / 33 and r["flags"] == C.CLASH | C.OVERLAP
    assert r["stats"][0] == 1.0 / 2.5 and r["pair"].tolist() == [0, 0]


def test_minimum_ties_go_to_the_lowest_ids():
    lig = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    prot = np.array([[0.5, 9, 9], [2, 0, 0], [-2, 0, 0], [12, 0, 0], [0, 0, 2]], np.float32)
    r = C.contacts(lig, [1.7, 1.7], prot, [1, 6, 6, 6, 6])
    assert r["pair"].tolist() == [0, 1] and r["counts"][0] == 4        # protein ids count the hydrogen


def test_grid_faces_negative_coordinates_and_minus_zero():
    x = np.array([[-0.0, 0.0, 5.0], [-5.0, -1e-30, 4.9999995], [10.0, -5.0000005, -10.0], [-2.5, 2.5, 0.0], [0.0, 0.0, 0.0]], np.float32)
    c = C.cell_index(x, 5.0)
    assert c.tolist() == [[0, 0, 1], [-1, -1, 0], [2, -2, -2], [-1, 0, 0], [0, 0, 0]]
    g = C.grid(x, [6, 7, 8, 6, 1])
    assert g["status"] == 0 and g["origin"].tolist() == [-1, -2, -2] and g["dims"].tolist() == [4, 3, 4]
    lin = lambda cx, cy, cz: ((cz + 2) * 3 + (cy + 2)) * 4 + (cx + 1)
    assert g["atom_id"].tolist() == [i for _, i in sorted((lin(*c[i]), i) for i in range(4))]
    assert g["cell_ptr"][-1] == 4 and len(g["cell_ptr"]) == 49 and (np.diff(g["cell_ptr"]) >= 0).all()
    assert g["radii"].tolist() == C.bondi([6, 7, 8, 6])[g["atom_id"]].tolist()
    two = C.grid(np.array([[1, 1, 1], [2, 2, 2], [1.5, 1, 1]], np.float32), [6, 1, 8])       # one cell, ids ascending, hydrogen dropped
    assert two["atom_id"].tolist() == [0, 2] and two["dims"].tolist() == [1, 1, 1] and two["cell_ptr"].tolist() == [0, 2]
    assert C.grid(np.array([[0, 0, np.inf]], np.float32), [6])["status"] == 6
    assert C.grid(np.array([[0, 0, 0], [0, 0, 5.3e6]], np.float32), [6, 6])["status"] == 7    # 1 x 1 x (2^20 + ...) cells
    assert C.grid(np.array([[0, 0, 0], [0, 0, 5.2e6]], np.float32), [6, 6])["status"] == 0
    assert C.grid(np.zeros((0, 3), np.float32), [])["cell_ptr"].tolist() == [0]
    b = C.batch_grid([two, C.grid(np.zeros((0, 3), np.float32), []), two])
    assert b["cell_off"].tolist() == [0, 1, 1, 2] and b["atom_off"].tolist() == [0, 2, 2, 4] and b["cell_ptr"].tolist() == [0, 2, 4]


PDB = """\
HEADER    HAND-WRITTEN
ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00  0.00           N
ATOM      2  CA  ALA A   1      11.639   6.071  -5.147  1.00  0.00           C
ATOM      3  HA  ALA A   1      12.000   7.000  -5.000  1.00  0.00           H
ATOM      4  CB AALA A   1      12.000   5.000  -4.000  0.50  0.00           C
ATOM      5  CB BALA A   1      12.100   5.100  -4.100  0.50  0.00           C
ATOM      6  OXT ALA A   1     -10.500-100.250   0.000  1.00  0.00
ATOM      7 HG21 VAL A   2       1.000   2.000   3.000  1.00  0.00
HETATM    8 CA    CA A 101       1.500   2.500   3.500  1.00  0.00          CA
HETATM    9 ZN    ZN A 102       4.000   5.000   6.000  1.00  0.00
HETATM   10  O   HOH A 201       7.000   8.000   9.000  1.00  0.00           O
HETATM   11  C1  LIG A 301       0.000   0.000   0.000  1.00  0.00           C
ENDMDL
ATOM     12  N   ALA A   1       0.000   0.000   0.000  1.00  0.00           N
"""


def test_pdb_reader_on_a_hand_written_block():
    from fabind_amd.validity import protein_atoms_from_pdb
    xyz, z, het = protein_atoms_from_pdb(PDB)
    assert xyz.dtype == np.float32 and z.dtype == np.int32 and het.dtype == bool
    assert z.tolist() == [7, 6, 6, 8, 20, 30, 6] and het.tolist() == [False] * 4 + [True] * 3
    assert xyz[0].tolist() == [np.float32(11.104), np.float32(6.134), np.float32(-6.504)]
    assert xyz[3].tolist() == [-10.5, -100.25, 0.0] and xyz[2].tolist() == [12.0, 5.0, -4.0]
    xyz, z, het = protein_atoms_from_pdb(PDB, keep_water=True, keep_hydrogens=True)
    assert z.tolist() == [7, 6, 1, 6, 8, 1, 20, 30, 8, 6]
    e = protein_atoms_from_pdb("")
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2].shape == (0,)


def test_the_binding_mirrors_the_header_and_the_source_is_built():
    from fabind_amd import _lib, build, validity
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fabind_hip.h")).read(), flags=re.S)
    for nm in ("fabind_protein_grid", "fabind_pose_protein_check"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % nm, hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[nm]), nm
    assert "protein_contacts.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "protein_contacts.hip"))
    assert _lib.ABI_VERSION == 19
    assert validity.PROTEIN_FLAGS == dict(PROTEIN_CLASH=C.CLASH, PROTEIN_OVERLAP=C.OVERLAP, NONFINITE=C.NONFINITE, UNCHECKED=C.UNCHECKED)
    assert "PROTEIN_CLASH" not in validity.FLAGS and "prot_clash" not in validity.STATS and len(validity.FLAGS) == 9
    assert validity.MAX_CELLS == C.MAX_CELLS and validity.CELL_CLAMP == int(C.CLAMP)


def test_no_cpu_fallback():
    import torch
    from fabind_amd import validity
    with pytest.raises(RuntimeError, match="HIP device only"):
        validity.protein_grid(torch.zeros(1, 3), torch.ones(1), [0, 1])
    with pytest.raises(RuntimeError, match="HIP device only"):
        validity.check_poses_protein(torch.zeros(1, 3), None, None)


def test_margins_of_the_gpu_inputs():
    """The restatement on every (complex, pose) the GPU statistics test uses: the margins that make its exact comparisons fair, and that
    the poses reach what they are there for."""
    kinds = {k: [] for k in C.POSE_KINDS}
    for case in C.stat_cases():
        r_lig = C.bondi(case["z"])
        for kind, pose in zip(C.POSE_KINDS, case["poses"]):
            r = C.contacts(pose, r_lig, case["prot_xyz"], case["prot_z"])
            what = (case["name"], kind)
            assert r["margins"]["cutoff"] >= 1e-6, what
            assert r["margins"]["lattice"] >= 1e-9, what
            assert r["margins"]["close"] >= 1e-9, what
            v = r["stats"]
            if np.isfinite(v[0]):
                assert abs(v[0] - np.float32(0.75)) >= 16 * C.bound(0, v[0]), what
            assert abs(v[2] - np.float32(0.075)) >= 16 * C.bound(2, v[2]), what
            kinds[kind].append(r)
    assert all(r["flags"] == C.CLASH | C.OVERLAP for r in kinds["inside"])
    assert all(r["stats"][0] == 0.0 and r["stats"][1] == 0.0 for r in kinds["coincident"])
    assert all(r["stats"][0] == np.inf and r["pair"].tolist() == [-1, -1] and r["flags"] == 0 and r["counts"][1] > 0 for r in kinds["beyond"])
    assert all(r["stats"][0] == np.inf for r in kinds["outside+z-corner"])
    faces = [r for k in C.POSE_KINDS if k.startswith("outside") and "corner" not in k for r in kinds[k]]
    assert sum(np.isfinite(r["stats"][0]) for r in faces) >= len(faces) // 2          # outside the box, yet pairs within the cutoff
    assert any(r["flags"] == 0 and np.isfinite(r["stats"][0]) for r in kinds["surface"] + faces)
