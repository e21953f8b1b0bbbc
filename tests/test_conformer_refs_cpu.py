"""CPU: the numpy restatement of fabind_amd.conformer (tests/conformer_refs.py) on molecules whose answer is known by inspection,
on the reference's example ligands (tests/golden/conformer_ligands.npz, tests/make_conformer_golden.py) and against the reference's
own uniform_random_rotation as recorded in that fixture -- the GPU tests then compare the kernels with the restatement."""
import numpy as np
import pytest
import torch

import conformer_refs as R
from helpers import load_npz

from fabind_amd import conformer

DIST_SEED = R.DIST_SEED


def _as_dict(m):
    q, s, st = R.plan(m["n"], m["bonds"], m["codes"])
    assert st == 0
    return {(int(a[1]), int(a[2])): R.side_atoms(w) for a, w in zip(q, s)}, q


@pytest.mark.parametrize("name", sorted(R.hand_molecules()))
def test_hand_molecules(name):
    m, want = R.hand_molecules()[name]
    got, q = _as_dict(m)
    assert got == want
    assert [tuple(a[1:3]) for a in q] == sorted(want)                  # ascending (j, k)
    for bonds, codes in ((m["bonds"][:, ::-1], m["codes"]), (np.concatenate([m["bonds"], m["bonds"][:, ::-1]]), np.tile(m["codes"], 2)),
                         (np.concatenate([m["bonds"], m["bonds"]]), np.tile(m["codes"], 2))):
        q2, s2, _ = R.plan(m["n"], bonds, codes)
        assert np.array_equal(q2, q) and np.array_equal(s2, R.plan(m["n"], m["bonds"], m["codes"])[1])


def test_quads_take_the_lowest_other_neighbour():
    # isobutyl-like: 0-1, 1-2, 1-3, 3-4, 4-5: bonds 1-3 and 3-4 rotate; i of (1,3) = 0 (not 2), l = 4
    q, s, _ = R.plan(6, [(0, 1), (1, 2), (1, 3), (3, 4), (4, 5)], [4] * 5)
    assert q.tolist() == [[0, 1, 3, 4], [1, 3, 4, 5]]
    assert R.side_atoms(s[0]) == [3, 4, 5] and R.side_atoms(s[1]) == [4, 5]


def test_chains_and_the_atom_cap():
    for n in (1, 2, 3, 4, 63, 64, 65, 128, 129, 256):
        q, s, st = R.plan(**{k: R.chain(n)[k] for k in ("n", "bonds", "codes")})
        assert st == 0 and len(q) == max(n - 3, 0)
        for a, w in zip(q, s):
            assert a.tolist() == [a[1] - 1, a[1], a[1] + 1, a[1] + 2] and R.side_atoms(w) == list(range(a[2], n))
    q, s, st = R.plan(**{k: R.chain(257)[k] for k in ("n", "bonds", "codes")})
    assert st == 3 and len(q) == 0


def test_fixture_ligands_satisfy_the_plan_properties():
    g = load_npz("conformer_ligands")
    total = 0
    for m in R.fixture_molecules(g):
        nb, _ = R._adjacency(m["n"], m["bonds"], m["codes"])
        q, s, st = R.plan(m["n"], m["bonds"], m["codes"])
        assert st == 0
        for a, w in zip(q, s):
            i, j, k, l = (int(v) for v in a)
            side = set(R.side_atoms(w))
            assert j not in side and k in side and i in nb[j] and l in nb[k] and i not in side and l in side
            comp, todo = {j}, [j]                                      # the component of the bond, by a search of its own
            while todo:
                u = todo.pop()
                for v in nb[u]:
                    if v not in comp:
                        comp.add(v)
                        todo.append(v)
            other, todo = {j}, [j]                                     # j's side without the bond
            while todo:
                u = todo.pop()
                for v in nb[u]:
                    if v not in other and not (u == j and v == k):
                        other.add(v)
                        todo.append(v)
            assert k not in other                                      # no ring bond is listed
            assert side | other == comp and not (side & other)
            total += 1
    assert total == 6 + 26 + 5 + 20


def test_rotation_is_the_references_to_round_off():
    """The restated M against the reference's uniform_random_rotation outputs recorded for seeded numpy draws."""
    g = load_npz("conformer_ligands")
    none_q, none_s = np.zeros((0, 4), np.int32), np.zeros((0, 8), np.uint32)
    for x, u, y in zip(g["rot_x"], g["rot_u"], g["rot_y"]):
        got = R.perturb_one(x, none_q, none_s, [], u, centre=False)
        assert np.abs(got - y).max() <= 1e-13 * max(1.0, np.abs(y).max())
        M = R.rotation_matrix(*u)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(M) - 1.0) < 1e-14
        Mt = conformer.random_rotation_matrix(torch.from_numpy(u)).numpy()
        assert np.abs(Mt - M).max() < 1e-14
    M32 = conformer.random_rotation_matrix(torch.tensor(g["rot_u"], dtype=torch.float32))
    assert M32.shape == (len(g["rot_u"]), 3, 3) and M32.dtype == torch.float32


def test_dihedral_setter_sets_every_dihedral():
    g = load_npz("conformer_ligands")
    rng = np.random.RandomState(0)
    for m in R.fixture_molecules(g) + [dict(R.chain(40), x=R.embed(R.chain(40), 3))]:
        q, s, _ = R.plan(m["n"], m["bonds"], m["codes"])
        ang = rng.uniform(0, 2 * np.pi, len(q))
        x = m["x"].astype(np.float64)
        y = R.perturb_one(x, q, s, ang, (0.3, 0.6, 0.2))
        for a, t in zip(q, ang):
            d, deg = R.dihedral(y, a)
            assert not deg and abs((d - t + np.pi) % (2 * np.pi) - np.pi) < 1e-9
        pr = R.bonded_and_13_pairs(m)
        dist = lambda z: np.linalg.norm(z[pr[:, 0]] - z[pr[:, 1]], axis=1)
        assert np.abs(dist(y) - dist(x)).max() < 1e-9 and np.abs(y.mean(0)).max() < 1e-9
        rel = R.perturb_one(x, q, s, ang, (0.3, 0.6, 0.2), relative=True)
        for a, t in zip(q, ang):                                       # relative: every dihedral moves BY its angle
            assert abs((R.dihedral(rel, a)[0] - R.dihedral(x, a)[0] - t + np.pi) % (2 * np.pi) - np.pi) < 1e-9
    # a positive rotation about j -> k raises the IUPAC dihedral: cis butane (0) set to +90 degrees, checked by value
    x = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [1.0, 0.0, 1.5]])
    assert abs(R.dihedral(x, (0, 1, 2, 3))[0]) < 1e-12
    q, s, _ = R.plan(4, R.chain(4)["bonds"], R.chain(4)["codes"])
    y = R.perturb_one(x, q, s, [np.pi / 2], (0, 0, 0), rotate=False, centre=False)
    assert np.allclose(y[3], [0.0, 1.0, 1.5]) and np.allclose(y[:3], x[:3])     # right-handed about +z


def test_degenerate_dihedral_counts_as_zero():
    x = np.array([[0.0, 0.0, -1.5], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [1.0, 0.0, 2.0]])           # i, j, k collinear
    assert R.dihedral(x, (0, 1, 2, 3)) == (0.0, True)
    q, s, _ = R.plan(4, R.chain(4)["bonds"], R.chain(4)["codes"])
    y = R.perturb_one(x, q, s, [np.pi / 2], (0, 0, 0), rotate=False, centre=False)
    assert np.allclose(y[3], [0.0, 1.0, 2.0])


def test_draws_are_uniform_for_the_committed_seed():
    """4096 copies of a 4-atom chain under DIST_SEED, on the restated draws: the bounds of the GPU distribution test (5 sigma)."""
    S = 4096
    ang, uni = R.drawn_inputs(DIST_SEED, [0], S, [1])
    assert ang.min() >= 0 and ang.max() < 2 * np.pi + 1e-6 and uni.min() >= 0 and uni.max() < 1
    d0 = np.array([1.0, 0.0, 0.0])
    dirs = np.stack([d0 @ R.rotation_matrix(*uni[s, 0].astype(np.float64)) for s in range(S)])
    assert np.abs(dirs.mean(0)).max() < 0.045 and abs((dirs[:, 2] ** 2).mean() - 1.0 / 3.0) < 0.03
    assert abs(np.exp(1j * ang[:, 0].astype(np.float64)).mean()) < 4 / np.sqrt(S)
    # keys and copies decorrelate: another key gives other numbers, the same arguments the same
    assert R.uniform(1, 2, 3, 4) == R.uniform(1, 2, 3, 4) and R.uniform(1, 2, 3, 4) != R.uniform(1, 3, 3, 4)
    assert R.uniform(0, 0, 0, 0) != 0.0


def test_public_module_argument_checks():
    with pytest.raises(RuntimeError, match="HIP device"):
        conformer.rotatable_bonds(torch.zeros(2, 0, dtype=torch.long), [], [0, 3])
    with pytest.raises(RuntimeError, match="HIP device"):
        conformer.perturb_conformers(torch.zeros(3, 3), None, torsion_noise=False, atom_off=[0, 3])
    with pytest.raises(ValueError, match="bond_codes"):
        from fabind_amd.data import pack_samples
        s = dict(protein_node_xyz=np.zeros((4, 3)), protein_esm2_feat=np.zeros((4, 2)), coords=np.zeros((3, 3)),
                 compound_node_features=np.zeros((3, 2)), rdkit_coords=np.zeros((3, 3)), input_atom_edge_list=np.array([[0, 1], [1, 2]]),
                 LAS_edge_index=np.array([[0, 1], [1, 0]]))
        pack_samples([s, dict(s, bond_codes=[4, 4])], pin=False)      # all samples or none
