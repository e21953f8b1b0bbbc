"""GPU: fabind_amd.topology (csrc/topology.hip) -- the LAS pairs of a batch of ligands from their bond lists -- against the numpy
restatement of tests/topology_refs.py (checked on the CPU against the brute-force definition and the reference's own function by
tests/test_topology_refs_cpu.py), and its use by fabind_amd.data.build_batch and the post-optimisation.  Everything is integer:
every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import topology_refs as T
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _t(a, dtype=torch.int64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _fixture():
    g = load_npz("las_molecules")
    return tuple((str(name), int(g[name + "_n"]), tuple(tuple(int(v) for v in b) for b in g[name + "_bonds"]),
                  g[name + "_mask"].astype(np.int64)) for name in g["names"])


@functools.lru_cache(maxsize=None)
def _want(n, bonds):
    """(pairs int64 [2, El] local ids, ring_pairs, status) of one ligand by the restatement; computed once per graph."""
    mask, ring_pairs, status = T.las_mask(n, list(bonds))
    return T.pairs_of(mask), ring_pairs, status


def _pack(mols):
    """mols: [(n, bonds)] -> (bond_index [2, E] global ids, atom_off)."""
    off = np.concatenate([[0], np.cumsum([n for n, _ in mols])]).astype(np.int64)
    bi = [np.asarray(b, np.int64).reshape(-1, 2).T + off[k] for k, (_, b) in enumerate(mols)]
    return (np.concatenate(bi, 1) if bi else np.zeros((2, 0), np.int64)), off


def _run(mols, on_overflow="raise"):
    from fabind_amd import topology
    bi, off = _pack(mols)
    return topology.las_pairs(_t(bi), off, on_overflow=on_overflow)


def _assert_equal(p, mols):
    """Device result == restatement, ligand by ligand; returns the per-ligand pair blocks (local ids)."""
    off = np.concatenate([[0], np.cumsum([n for n, _ in mols])]).astype(np.int64)
    ei, po = p.edge_index.cpu().numpy(), p.off.cpu().numpy()
    assert p.edge_index.dtype == torch.int64 and p.off.dtype == torch.int32 and p.status.dtype == torch.int32
    assert ei.shape == (2, int(po[-1])) and po[0] == 0 and len(po) == len(mols) + 1
    assert np.array_equal(p.atom_off.cpu().numpy(), off)
    blocks = []
    for k, (n, bonds) in enumerate(mols):
        want, ring_pairs, status = _want(n, tuple(tuple(b) for b in bonds))
        got = ei[:, po[k]:po[k + 1]] - off[k]
        assert np.array_equal(got, want), (k, n)
        assert int(p.ring_pairs[k]) == ring_pairs and int(p.status[k]) == status, (k, n)
        blocks.append(got)
    return blocks


def _mols():
    return [(n, bonds) for _, n, bonds, _ in _fixture()]


# ------------------------------------------------------------------------------------------------ 1. the fixture molecules
def test_every_fixture_molecule_alone_in_a_batch_and_reversed():
    mols = _mols()
    alone = [_assert_equal(_run([m]), [m])[0] for m in mols]
    fwd = _assert_equal(_run(mols), mols)
    rev = _assert_equal(_run(mols[::-1]), mols[::-1])[::-1]
    for a, f, r in zip(alone, fwd, rev):
        assert np.array_equal(a, f) and np.array_equal(a, r)           # the same bits alone and in any batch


def test_las_mask_equals_the_recorded_reference_mask():
    from fabind_amd import topology
    for name, n, bonds, mask in _fixture():
        got = topology.las_mask(_t(np.asarray(bonds).T), n)
        assert got.dtype == torch.int64 and got.shape == (n, n)
        assert np.array_equal(got.cpu().numpy(), mask), name


def test_pairs_come_in_dense_to_sparse_order():
    mols = _mols()
    p = _run(mols)
    ei = p.edge_index.cpu().numpy()
    key = ei[0] * (int(p.atom_off[-1]) + 1) + ei[1]
    assert (np.diff(key) > 0).all()                                    # row-major and strictly increasing over the whole batch
    assert (ei[0] != ei[1]).all()
    lig = np.searchsorted(p.atom_off.cpu().numpy(), ei, side="right") - 1
    assert np.array_equal(lig[0], lig[1])                              # no pair crosses ligands
    assert np.array_equal(np.bincount(lig[0], minlength=len(mols)), np.diff(p.off.cpu().numpy()))


def test_random_graphs_and_ring_systems_in_one_batch():
    rng = np.random.default_rng(77)
    mols = []
    for it in range(150):                                              # the small graphs the CPU test holds against the brute force
        n = int(rng.integers(3, 11))
        mols.append((n, tuple(T.random_graph(rng, n, int(rng.integers(0, 6)), connected=it % 3 != 0))))
    for _ in range(24):                                                # fused / spiro / bridged systems of drug-like size
        n = int(rng.integers(20, 61))
        mols.append((n, tuple(T.random_ring_system(rng, n))))
    p = _run(mols)
    _assert_equal(p, mols)
    assert int((p.ring_pairs > 0).sum()) >= 100


# ------------------------------------------------------------------------------------------------ 2. edge shapes
def test_empty_batch():
    from fabind_amd import topology
    p = topology.las_pairs(torch.zeros(2, 0, dtype=torch.int64, device=DEV), [0])
    assert p.edge_index.shape == (2, 0) and p.off.tolist() == [0] and p.status.numel() == 0 and p.ring_pairs.numel() == 0


def test_small_and_degenerate_ligands():
    tree = [(0, 1), (1, 2), (1, 3), (3, 4), (3, 5), (5, 6)]
    two = T.ring(5) + T.ring(6, 5)                                     # two fragments in one ligand
    mols = [(1, []), (6, T.ring(6)), (0, []), (2, [(0, 1)]), (7, tree), (11, two), (0, []), (3, [])]
    p = _run(mols)
    _assert_equal(p, mols)
    assert p.ring_pairs.tolist() == [0, 15, 0, 0, 0, 25, 0, 0]
    assert np.diff(p.off.cpu().numpy()).tolist() == [0, 30, 0, 2, 2 * (6 + 7), 20 + 30, 0, 0]


def test_bond_list_forms_give_the_same_pairs():
    from fabind_amd import topology
    n, bonds, _, _ = T.hand_molecules()["hexa_cyclopropa_6ring"]
    b = np.asarray(bonds, np.int64).T
    want = _want(n, tuple(tuple(x) for x in bonds))[0]
    loops = np.array([[3, 7], [3, 7]])
    for form in (b, b[::-1], np.concatenate([b, b[::-1]], 1), np.concatenate([b, b, b[::-1]], 1), np.concatenate([loops, b], 1)):
        assert np.array_equal(topology.las_pairs(_t(form), [0, n]).edge_index.cpu().numpy(), want)


def test_argument_errors():
    from fabind_amd import topology
    with pytest.raises(ValueError, match="two different ligands"):
        topology.las_pairs(_t([[0, 2], [1, 3]]), [0, 3, 5])
    with pytest.raises(ValueError, match="outside"):
        topology.las_pairs(_t([[0], [5]]), [0, 5])
    with pytest.raises(RuntimeError, match="HIP device only"):
        topology.las_pairs(torch.zeros(2, 1, dtype=torch.int64), [0, 2])


# ------------------------------------------------------------------------------------------------ 3. bitset and table edges
def test_chains_and_rings_at_the_word_edges():
    mols = [(n, T.chain(n)) for n in (63, 64, 65)] + [(n, T.ring(n)) for n in (63, 64, 65)]
    p = _run(mols)
    _assert_equal(p, mols)
    assert p.ring_pairs.tolist() == [0, 0, 0] + [n * (n - 1) // 2 for n in (63, 64, 65)]


def test_rings_of_255_and_256_atoms_and_a_chain_of_256():
    mols = [(255, T.ring(255)), (256, T.ring(256)), (256, T.chain(256))]
    p = _run(mols)
    _assert_equal(p, mols)
    assert p.ring_pairs.tolist() == [255 * 254 // 2, 256 * 255 // 2, 0]
    assert np.diff(p.off.cpu().numpy()).tolist() == [255 * 254, 256 * 255, 2 * 255 + 2 * 254]


def test_more_than_256_atoms():
    mols = [(6, T.ring(6)), (257, T.ring(257)), (5, T.ring(5))]
    with pytest.raises(RuntimeError, match=r"ligand 1: status 3 \(more than 256 atoms\)"):
        _run(mols)
    p = _run(mols, on_overflow="truncate")
    _assert_equal(p, mols)                                             # the restatement: (a) and (b) only for the large one
    assert p.status.tolist() == [0, 3, 0] and p.ring_pairs.tolist() == [15, 0, 10]
    assert int(p.off[2] - p.off[1]) == 4 * 257


def test_chord_cap():
    mols = [(2 * k, T.ladder(k)) for k in (64, 65)]                    # 63 and 64 chords
    p = _run(mols)
    _assert_equal(p, mols)
    assert p.status.tolist() == [0, 0] and p.ring_pairs.tolist() == [63 * 6 - 62, 64 * 6 - 63]   # 4-rings sharing a rung
    over = [(6, T.ring(6)), (132, T.ladder(66))]                       # 65 chords
    with pytest.raises(RuntimeError, match=r"ligand 1: status 4 \(more than 64 non-tree bonds\)"):
        _run(over)
    q = _run(over, on_overflow="truncate")
    _assert_equal(q, over)
    assert q.status.tolist() == [0, 4] and q.ring_pairs.tolist() == [15, 0]
    dense = [(40, [(i, j) for i in range(40) for j in range(i + 1, 40)])]            # more neighbour entries than the kernel stages
    r = _run(dense, on_overflow="truncate")
    _assert_equal(r, dense)
    assert r.status.tolist() == [4] and int(r.off[-1]) == 40 * 39


# ------------------------------------------------------------------------------------------------ 4. renumbering
def test_mask_permutes_with_a_renumbering():
    from fabind_amd import topology
    rng = np.random.default_rng(11)
    # a fused / bridged system: naphthalene with a cyclopropane on the fusion bond and a norbornane hung on atom 2
    n0, b0, _, _ = T.hand_molecules()["naphthalene"]
    n1, b1, _, _ = T.hand_molecules()["norbornane"]
    bonds = list(b0) + [(0, 10), (5, 10)] + [(a + 11, b + 11) for a, b in b1] + [(2, 11)]
    n = n0 + 1 + n1
    base = topology.las_mask(_t(np.asarray(bonds).T), n).cpu().numpy()
    assert np.array_equal(base, T.las_mask(n, bonds)[0])
    for _ in range(4):
        perm = rng.permutation(n)
        got = topology.las_mask(_t(np.asarray(T.renumber(bonds, perm)).T), n).cpu().numpy()
        assert np.array_equal(got[np.ix_(perm, perm)], base)


# ------------------------------------------------------------------------------------------------ 5. memory discipline
def test_nothing_is_written_past_the_end_and_the_passes_agree():
    from fabind_amd import kernels as K, topology
    mols = _mols() + [(257, T.ring(257)), (64, T.ring(64))]
    bi, off = _pack(mols)
    N, B, PAD, SENT = int(off[-1]), len(mols), 64, -77
    aoff = _t(off, torch.int32)
    nptr, nidx = topology._neighbour_lists(_t(bi), N)

    def run():
        rc = torch.full((N + PAD,), SENT, dtype=torch.int32, device=DEV)
        mr = torch.full((N + PAD, 8), SENT, dtype=torch.int32, device=DEV)
        rp = torch.full((B + PAD,), SENT, dtype=torch.int32, device=DEV)
        st = torch.full((B + PAD,), SENT, dtype=torch.int32, device=DEV)
        K.las_pairs(nptr, nidx, aoff, B, rc, mr, rp, st)
        for buf, used in ((rc, N), (mr, N), (rp, B), (st, B)):
            assert bool((buf[used:] == SENT).all())
        assert bool((rc[:N] >= 0).all()) and bool((st[:B] != SENT).all())
        row_off = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
        row_off[1:] = torch.cumsum(rc[:N], 0)
        El = int(row_off[-1])
        out = torch.full((2 * El + PAD,), SENT, dtype=torch.int64, device=DEV)
        K.las_pairs(nptr, nidx, aoff, B, rc, mr, rp, st, row_off, El, out)
        assert bool((out[2 * El:] == SENT).all())                      # nothing past the end
        assert bool((out[:2 * El] != SENT).all())                      # the count pass and the write pass agree: every slot is filled
        return out[:2 * El].view(2, El), rc[:N], mr[:N], rp[:B], st[:B]
    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)                                       # a repeat run is bit-identical
    p = topology.las_pairs(_t(bi), off, on_overflow="truncate")
    assert torch.equal(p.edge_index, first[0]) and torch.equal(p.ring_pairs, first[3]) and torch.equal(p.status, first[4])
    _assert_equal(p, mols)


# ------------------------------------------------------------------------------------------------ 6. the batch builder and a consumer
def _samples(with_las):
    g = torch.Generator().manual_seed(5)
    fix = {name: (n, bonds) for name, n, bonds, _ in _fixture()}
    out = []
    for L, name in ((60, "naphthalene"), (45, "6g3c"), (50, "spiro_pair")):
        n, bonds = fix[name]
        prot = torch.randn(L, 3, generator=g) * 8.0
        lig = torch.randn(n, 3, generator=g) * 2.0 + torch.tensor([3.0, 0.0, 0.0])
        s = dict(protein_node_xyz=prot, protein_esm2_feat=torch.randn(L, 16, generator=g), coords=lig,
                 compound_node_features=torch.randn(n, 8, generator=g), input_atom_edge_list=np.asarray(bonds, np.int64),
                 rdkit_coords=lig - lig.mean(0), pdb=name)
        if with_las:
            s["LAS_edge_index"] = _run([(n, bonds)]).edge_index.cpu().numpy()
        out.append(s)
    return out


def test_build_batch_derives_the_pairs_when_no_sample_carries_them():
    from fabind_amd.data import DeviceFeeder, build_batch
    derived, given = build_batch(_samples(False), DEV), build_batch(_samples(True), DEV)
    fields = 0
    stores = lambda b: list(b._stores.items()) + [("", b._glob)]
    assert [k for k, _ in stores(derived)] == [k for k, _ in stores(given)]
    for (key, sd), (_, sg) in zip(stores(derived), stores(given)):
        assert sorted(sd.keys()) == sorted(sg.keys()), key
        for f in sd.keys():
            if torch.is_tensor(sd[f]):
                assert sd[f].dtype == sg[f].dtype and torch.equal(sd[f], sg[f]), (key, f)
                fields += 1
            else:
                assert sd[f] == sg[f], (key, f)
    assert fields >= 35
    n_las = derived["compound", "LAS", "compound"].edge_index.shape[1]
    assert n_las == sum(_want(n, bonds)[0].shape[1] for n, bonds in (m[1:3] for m in _fixture() if m[0] in ("naphthalene", "6g3c", "spiro_pair")))
    mixed = _samples(True)
    del mixed[1]["LAS_edge_index"]
    with pytest.raises(ValueError, match="LAS_edge_index"):
        build_batch(mixed, DEV)
    fed = list(DeviceFeeder([_samples(False)], DEV))                   # the side-stream path
    assert torch.equal(fed[0]["complex", "LAS", "complex"].edge_index, given["complex", "LAS", "complex"].edge_index)


def test_post_optimisation_takes_the_pairs():
    from fabind_amd.utils.post_optim_utils import post_optimize_compound_coords_batched
    mols = [m for m in _mols() if m[0] <= 29][:6]
    p = _run(mols)
    g = torch.Generator().manual_seed(9)
    N = int(p.atom_off[-1])
    ref = (torch.randn(N, 3, generator=g) * 2.0).to(DEV)
    pred = ref + 0.3 * torch.randn(N, 3, generator=g).to(DEV)
    cb = torch.repeat_interleave(torch.arange(len(mols)), torch.as_tensor([n for n, _ in mols])).to(DEV)
    a = post_optimize_compound_coords_batched(ref, pred, cb, total_epoch=20, LAS_edge_index=p.edge_index)
    plain = torch.as_tensor(p.edge_index.cpu().numpy().copy()).to(DEV)
    b = post_optimize_compound_coords_batched(ref, pred, cb, total_epoch=20, LAS_edge_index=plain)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.isfinite(a[0]).all()
