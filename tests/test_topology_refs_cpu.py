"""CPU: the numpy restatement of fabind_amd.topology (tests/topology_refs.py) against the brute-force definition (every simple cycle,
Gaussian elimination against all strictly shorter ones), against the reference's own get_LAS_distance_constraint_mask as recorded
in tests/golden/las_molecules.npz (tests/make_las_golden.py), and on the invariants of the definition -- the GPU tests then compare
the kernel with the restatement.  Everything is integer: every comparison is exact."""
import os
import re

import numpy as np
import pytest

import topology_refs as T
from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ring pairs of the hand molecules as the design prototype gave them
RING_PAIRS = {"benzene": 15, "naphthalene": 29, "norbornane": 17, "bicyclo222octane": 28, "cubane": 24, "hexa_cyclopropa_6ring": 27,
              "biphenyl": 30, "spiro_pair": 20, "ring14": 91}


def test_hand_molecule_table_is_complete():
    assert set(T.hand_molecules()) == set(RING_PAIRS)


@pytest.mark.parametrize("name", sorted(RING_PAIRS))
def test_hand_molecules_equal_brute_force_and_hand_rings(name):
    n, bonds, rings, _ = T.hand_molecules()[name]
    mask, ring_pairs, status = T.las_mask(n, bonds)
    assert status == 0
    assert ring_pairs == RING_PAIRS[name]                              # the literal counts
    bmask, bpairs = T.brute_las_mask(n, bonds)
    assert np.array_equal(mask, bmask) and ring_pairs == bpairs
    hmask, hpairs = T.mask_from_rings(n, T.adjacency(n, bonds), rings)
    assert np.array_equal(mask, hmask) and ring_pairs == hpairs
    got = sorted(tuple(sorted(r)) for r in T.brute_rings(n, T.adjacency(n, bonds)))
    assert got == sorted(tuple(sorted(r)) for r in rings)              # the brute force finds exactly the hand-written rings


@pytest.mark.parametrize("connected", [True, False])
def test_random_graphs_equal_brute_force(connected):
    rng = np.random.default_rng(20240 + connected)
    cyclic = 0
    for it in range(200):
        n = int(rng.integers(3, 11))
        bonds = T.random_graph(rng, n, int(rng.integers(0, 6)), connected=connected)
        assert len(bonds) <= n + 4 and max(np.bincount(np.asarray(bonds).reshape(-1), minlength=n)) <= 4
        mask, ring_pairs, status = T.las_mask(n, bonds)
        bmask, bpairs = T.brute_las_mask(n, bonds)
        assert status == 0 and np.array_equal(mask, bmask) and ring_pairs == bpairs, (n, bonds)
        cyclic += ring_pairs > 0
    assert cyclic >= 100                                               # the sample is not mostly trees


def test_random_ring_systems_equal_brute_force():
    rng = np.random.default_rng(31)
    for _ in range(40):
        n = int(rng.integers(8, 17))
        bonds = T.random_ring_system(rng, n)
        mask, ring_pairs, status = T.las_mask(n, bonds)
        bmask, bpairs = T.brute_las_mask(n, bonds)
        assert status == 0 and ring_pairs > 0 and np.array_equal(mask, bmask) and ring_pairs == bpairs, (n, bonds)


def test_restatement_equals_the_reference_function_on_every_recorded_molecule():
    g = load_npz("las_molecules")
    assert len(g["names"]) == 13 and sorted(set(g["ring_source"].tolist())) == ["brute", "hand"]
    for name in g["names"]:
        n, bonds = int(g[name + "_n"]), g[name + "_bonds"]
        mask, _, status = T.las_mask(n, bonds)
        assert status == 0 and np.array_equal(mask, g[name + "_mask"].astype(np.int64)), name


def _all_graphs():
    g = load_npz("las_molecules")
    out = [(str(name), int(g[name + "_n"]), [tuple(int(v) for v in b) for b in g[name + "_bonds"]]) for name in g["names"]]
    out += [("ladder5", 10, T.ladder(5)), ("two_fragments", 11, T.ring(5) + T.ring(6, 5)), ("chain7", 7, T.chain(7))]
    return out


def test_symmetric_with_zero_diagonal():
    for name, n, bonds in _all_graphs():
        mask, _, _ = T.las_mask(n, bonds)
        assert np.array_equal(mask, mask.T) and not mask.diagonal().any(), name
        assert set(np.unique(mask)) <= {0, 1}


def test_invariant_under_renumbering():
    rng = np.random.default_rng(7)
    for name, n, bonds in _all_graphs():
        mask, ring_pairs, _ = T.las_mask(n, bonds)
        for _ in range(5):
            perm = rng.permutation(n)
            pmask, ppairs, _ = T.las_mask(n, T.renumber(bonds, perm))
            assert ppairs == ring_pairs, name
            assert np.array_equal(pmask[np.ix_(perm, perm)], mask), name   # atom a became perm[a]


def test_bond_list_forms_and_pairs_order():
    n, bonds, _, _ = T.hand_molecules()["naphthalene"]
    mask, _, _ = T.las_mask(n, bonds)
    rev = [(b, a) for a, b in bonds]
    for form in (rev, bonds + rev, bonds + bonds + rev, bonds + [(3, 3)]):
        assert np.array_equal(T.las_mask(n, form)[0], mask)
    p = T.pairs_of(mask)
    key = p[0] * n + p[1]
    assert (np.diff(key) > 0).all() and p.shape[1] == mask.sum()
    ei, off, rp, st = T.las_pairs(np.asarray(bonds).T + 4, [0, 4, 4 + n])
    assert off.tolist() == [0, 0, p.shape[1]] and np.array_equal(ei, p + 4) and rp.tolist() == [0, 29] and st.tolist() == [0, 0]


def test_caps():
    assert T.las_mask(257, T.ring(257))[2] == 3
    m, rp, st = T.las_mask(257, T.ring(257))
    assert rp == 0 and m.sum() == 4 * 257                              # (a) and (b) only
    assert T.las_mask(130, T.ladder(65))[2] == 0                       # 64 chords
    m, rp, st = T.las_mask(132, T.ladder(66))                          # 65 chords
    assert st == 4 and rp == 0 and np.array_equal(m, T.two_hop_mask(132, T.adjacency(132, T.ladder(66))))


def test_entry_point_is_declared_bound_and_exported():
    from fabind_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fabind_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+fabind_las_pairs\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m and "hipStream_t" in m.group(1).split(",")[-1]
    assert "fabind_las_pairs" in _lib.SIGNATURES
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["fabind_las_pairs"])
    assert "topology.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "topology.hip"))
    lib = _lib.load()
    assert hasattr(lib, "fabind_las_pairs")
    assert lib.fabind_abi_version() == 19 and _lib.ABI_VERSION == 19


def test_device_only_and_argument_checks():
    import torch
    from fabind_amd import data, topology
    with pytest.raises(RuntimeError, match="HIP device only"):
        topology.las_pairs(torch.zeros(2, 3, dtype=torch.int64), [0, 4])
    with pytest.raises(ValueError, match="on_overflow"):
        topology.las_pairs(torch.zeros(2, 3, dtype=torch.int64), [0, 4], on_overflow="ignore")
    s = dict(protein_node_xyz=np.zeros((3, 3)), protein_esm2_feat=np.zeros((3, 4)), coords=np.zeros((2, 3)),
             compound_node_features=np.zeros((2, 5)), rdkit_coords=np.zeros((2, 3)), input_atom_edge_list=np.array([[0, 1]]))
    with_las = dict(s, LAS_edge_index=np.array([[0, 1], [1, 0]]))
    with pytest.raises(ValueError, match="LAS_edge_index"):
        data.pack_samples([s, with_las], pin=False)
    assert data.pack_samples([s, s], pin=False)[2].get("derive_las") is True
    assert "derive_las" not in data.pack_samples([with_las, with_las], pin=False)[2]
