"""GPU: pairwise symmetry-corrected RMSD and leader clustering of sampled poses (fabind_amd/poses.py, csrc/pose_cluster.hip) against the
float64 restatements of tests/pose_cluster_refs.py.

Distances: |D_dev - D64| <= (1.5 n + 4) 2^-24 D64 elementwise -- the worst case of a float32 sum of 3 n non-negative terms in any order,
the divide and the root (derived in pose_cluster_refs.bound, not measured); every case prints its largest fraction of the bound before
it asserts (`pytest -s`; DESIGN.md section 15 records it).  Clustering is integer work: equality.  The native calls of this file write
into NaN- / sentinel-prefilled buffers with a guard band behind each output."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import pose_cluster_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64


def _table(autos_list, status=None):
    """`symmetry.Automorphisms` of hand-given lists: one [K_b, n_b] array per ligand."""
    from fabind_amd.symmetry import Automorphisms
    n = [a.shape[1] for a in autos_list]
    off = np.concatenate([[0], np.cumsum([a.size for a in autos_list])])
    flat = np.concatenate([a.reshape(-1) for a in autos_list]) if autos_list else np.zeros(0)
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)          # noqa: E731
    return Automorphisms(flat=i32(flat), off=i32(off), count=i32([len(a) for a in autos_list]),
                         status=i32(status if status is not None else [0] * len(n)), atom_off=i32(np.concatenate([[0], np.cumsum(n)])))


def _cb(A):
    n = torch.diff(A.atom_off).long()
    return torch.repeat_interleave(torch.arange(n.numel(), device=DEV), n)


def _stack(pose_list):
    """[S, n_b, 3] arrays of equal S -> [S, N, 3] on the device."""
    return torch.from_numpy(np.concatenate(pose_list, axis=1)).to(DEV)


def _guarded_pair(poses, A, use=None):
    """fabind_pose_pair_rmsd straight through the C ABI into a NaN-prefilled buffer with a sentinel band behind it."""
    from fabind_amd import _lib
    S, N = poses.shape[0], poses.shape[1]
    B = A.atom_off.numel() - 1
    buf = torch.full((B * S * S + GUARD,), float("nan"), device=DEV)
    buf[B * S * S:] = -7.0
    use = torch.where(A.status == 0, A.count, torch.zeros_like(A.count)) if use is None else use
    flat = A.flat if A.flat.numel() else torch.zeros(1, dtype=torch.int32, device=DEV)
    max_atoms = int(torch.diff(A.atom_off).max())
    rc = _lib.load().fabind_pose_pair_rmsd(poses.data_ptr(), S, N, A.atom_off.data_ptr(), A.off.data_ptr(), use.data_ptr(), flat.data_ptr(),
                                           B, max_atoms, buf.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, buf[:B * S * S].reshape(B, S, S), buf[B * S * S:]


def _assert_structure(D):
    assert torch.equal(D, D.transpose(1, 2))                                             # bit-symmetric
    diag = torch.diagonal(D, dim1=1, dim2=2)
    assert torch.equal(diag.contiguous().view(torch.int32), torch.zeros_like(diag, dtype=torch.int32))   # +0.0, not -0.0
    assert not bool(torch.isnan(D).any())


def _assert_bound(name, D_dev, D64, n):
    got = D_dev.double().cpu().numpy()
    err, bnd = np.abs(got - D64), R.bound(D64, n)
    frac = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    print("pose_pair_rmsd %-28s n %3d S %3d  max err / bound = %.3f" % (name, n, len(D64), frac))
    assert (err <= bnd).all(), (name, frac)
    return frac


@pytest.mark.parametrize("name", list(R.cases()))
def test_distances_against_float64(name):
    from fabind_amd.poses import pairwise_rmsd
    poses, autos, D64 = R.cases()[name]
    A = _table([autos])
    x = torch.from_numpy(poses).to(DEV)
    rc, D, guard = _guarded_pair(x, A)
    assert rc == 0 and bool((guard == -7.0).all())
    _assert_structure(D)
    _assert_bound(name, D[0], D64, poses.shape[1])
    D2 = pairwise_rmsd(x, _cb(A), A)
    assert D2.shape == D.shape and torch.equal(D2, D)                                    # the public path, and a repeat run: same bits
    sub = [0, len(poses) - 1] if len(poses) > 2 else [0, 1]                              # two poses of the S: the same bits at S = 2
    Ds = pairwise_rmsd(x[sub], _cb(A), A)
    assert torch.equal(Ds, D[:, sub][:, :, sub])


def test_mixed_batch_equals_every_ligand_alone_and_an_empty_ligand_is_zero():
    from fabind_amd.poses import pairwise_rmsd
    rng = np.random.default_rng(11)
    S = 37                                                                               # two tiles, the second partial
    names = ["benzene", "chain_mixed", "c60", "druglike_95", "single_atom", "bis_cf3_biphenyl", "neopentane", "druglike_123"]
    autos = [R.fixture_autos(nm) for nm in names]
    autos.insert(3, np.zeros((1, 0), dtype=np.int64))                                    # n_b = 0 between two non-empty ligands
    poses = [R.random_poses(rng, S, a.shape[1], a) for a in autos]
    A = _table(autos)
    x = _stack(poses)
    rc, D, guard = _guarded_pair(x, A)
    assert rc == 0 and bool((guard == -7.0).all())
    _assert_structure(D)
    assert not bool(D[3].any())
    D2 = pairwise_rmsd(x, _cb(A), A)
    assert torch.equal(D2, D)
    for b, a in enumerate(autos):
        n = a.shape[1]
        if n == 0:
            continue
        D64 = R.pair_rmsd_ref(poses[b], a)
        _assert_bound("batch[%d]" % b, D[b], D64, n)
        Ab = _table([a])
        alone = pairwise_rmsd(torch.from_numpy(poses[b]).to(DEV), _cb(Ab), Ab)
        assert torch.equal(alone[0], D[b]), b                                            # alone = in the batch, bit for bit
    pick = [3, 5, 20, 36]                                                                # a pose subset across both tiles: the same bits
    assert torch.equal(pairwise_rmsd(x[pick], _cb(A), A), D[:, pick][:, :, pick])


def test_plain_rmsd_forms_agree():
    """autos=None = an identity-only table = a ligand whose search was cut at `cap` (status 1) = plain RMSD."""
    from fabind_amd.poses import pairwise_rmsd
    from fabind_amd.symmetry import ligand_automorphisms
    rng = np.random.default_rng(3)
    S = 6
    # 12 isolated equal atoms (12! automorphisms: cut at cap) beside benzene
    lab = torch.full((18,), 600, dtype=torch.int32, device=DEV)
    ring = [(12 + i, 12 + (i + 1) % 6) for i in range(6)]
    bonds = torch.tensor(ring, dtype=torch.int64, device=DEV).T
    off = torch.tensor([0, 12, 18], dtype=torch.int32, device=DEV)
    A = ligand_automorphisms(lab, bonds, off, cap=50, on_overflow="truncate")
    assert A.status.tolist() == [1, 0] and A.count.tolist() == [50, 12]
    poses = [R.random_poses(rng, S, 12), R.random_poses(rng, S, 6, R.fixture_autos("benzene"))]
    x = _stack(poses)
    cb = _cb(A)
    D = pairwise_rmsd(x, cb, A)
    plain = pairwise_rmsd(x, cb)                                                         # autos=None
    ident = _table([np.arange(12).reshape(1, 12), np.arange(6).reshape(1, 6)])
    assert torch.equal(pairwise_rmsd(x, cb, ident), plain)                               # K = 1
    assert torch.equal(D[0], plain[0])                                                   # the truncated set is not used
    _assert_bound("truncated -> plain", D[0], R.pair_rmsd_ref(poses[0], np.arange(12).reshape(1, 12)), 12)
    _assert_bound("benzene beside it", D[1], R.pair_rmsd_ref(poses[1], R.fixture_autos("benzene")), 6)
    assert bool((D[1] <= plain[1]).all()) and bool((D[1] < plain[1]).any())
    bad = replace(A, status=torch.tensor([0, 2], dtype=torch.int32, device=DEV))         # a failed ligand: plain RMSD, as symmetric_rmsd
    assert torch.equal(pairwise_rmsd(x, cb, bad)[1], plain[1])


def test_columns_agree_with_symmetric_rmsd():
    from fabind_amd.poses import pairwise_rmsd
    from fabind_amd.symmetry import symmetric_rmsd
    rng = np.random.default_rng(4)
    names = ["benzene", "c60", "druglike_61", "chain_equal", "druglike_95"]
    autos = [R.fixture_autos(nm) for nm in names]
    S = 7
    poses = [R.random_poses(rng, S, a.shape[1], a) for a in autos]
    A = _table(autos)
    x, cb = _stack(poses), _cb(A)
    D = pairwise_rmsd(x, cb, A)
    D64 = [R.pair_rmsd_ref(poses[b], a) for b, a in enumerate(autos)]
    for t in range(S):
        r, corrected = symmetric_rmsd(x, x[t], cb, A)                                    # [S, B]
        assert bool(corrected.all())
        for b, a in enumerate(autos):
            bnd = R.bound(D64[b][:, t], a.shape[1])
            col = r[:, b].double().cpu().numpy()
            off_diag = np.arange(S) != t
            assert (np.abs(col - D64[b][:, t])[off_diag] <= bnd[off_diag]).all()         # the existing kernel inside the same bound
            assert (np.abs(col - D[b, :, t].double().cpu().numpy())[off_diag] <= 2 * bnd[off_diag]).all(), (t, b)


def _guarded_cluster(D, conf, thr):
    from fabind_amd import _lib
    B, S = D.shape[0], D.shape[1]
    bufs = [torch.full((S * B + GUARD,), -77, dtype=torch.int32, device=DEV) for _ in range(3)] + \
           [torch.full((B + GUARD,), -77, dtype=torch.int32, device=DEV)]
    rc = _lib.load().fabind_pose_cluster(D.data_ptr(), conf.data_ptr(), S, B, float(thr), *[b.data_ptr() for b in bufs], _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for b, used in zip(bufs, (S * B, S * B, S * B, B)):
        assert bool((b[used:] == -77).all())
    return [b[:S * B].reshape(S, B) for b in bufs[:3]] + [bufs[3][:B]]


def _assert_clusters(got, D, conf, thr):
    """got: (cluster_id, leader, size [S, B], n_clusters [B]) on the device; D [B, S, S], conf [S, B] on the device."""
    Dh, ch = D.cpu().numpy(), conf.cpu().numpy()
    cid, leader, size, ncl = (g.cpu().numpy() for g in got)
    for b in range(Dh.shape[0]):
        w = R.leader_cluster_ref(Dh[b], ch[:, b], thr)
        assert ncl[b] == w[3], b
        assert np.array_equal(cid[:, b], w[0]) and np.array_equal(leader[:, b], w[1]) and np.array_equal(size[:, b], w[2]), b


@pytest.mark.parametrize("S", [2, 64, 65, 257])
def test_clustering_equals_the_restatement_on_the_device_distances(S):
    from fabind_amd.poses import cluster_from_distances, pairwise_rmsd
    rng = np.random.default_rng(S)
    autos = [R.fixture_autos("benzene"), R.fixture_autos("chain_mixed"), R.fixture_autos("nitrate_salt")]
    # every other pose is a noisy copy of one conformer (about 1.2 A apart), the rest lie anywhere: distances on both sides of 2 A
    poses = [R.random_poses(rng, S, a.shape[1], a) for a in autos]
    A = _table(autos)
    x, cb = _stack(poses), _cb(A)
    D = pairwise_rmsd(x, cb, A)
    B = 3
    conf = torch.from_numpy(rng.normal(size=(S, B)).astype(np.float32)).to(DEV)
    for thr in (2.0, 0.0, float("inf"), 1.0):
        got = _guarded_cluster(D, conf, thr)
        _assert_clusters(got, D, conf, thr)
        pc = cluster_from_distances(D, conf, thr)
        assert all(torch.equal(a, b) for a, b in zip((pc.cluster_id, pc.leader, pc.size, pc.n_clusters), got))
        if thr == 0.0:                                                                   # S singletons, in confidence order
            assert pc.n_clusters.tolist() == [S] * B and bool((pc.size == 1).all())
            assert torch.equal(pc.leader.long(), torch.argsort(conf, dim=0, descending=True, stable=True))
        if thr == float("inf"):                                                          # one cluster
            assert pc.n_clusters.tolist() == [1] * B and pc.size[0].tolist() == [S] * B and not bool(pc.cluster_id.any())
    # ties, +-inf and NaN confidences
    tied = torch.round(conf)
    _assert_clusters(_guarded_cluster(D, tied, 2.0), D, tied, 2.0)
    odd = conf.clone()
    odd[::3, 0] = float("nan")
    odd[0, 1], odd[S - 1, 1] = float("-inf"), float("inf")
    odd[:, 2] = float("nan")
    for thr in (2.0, 0.0):
        _assert_clusters(_guarded_cluster(D, odd, thr), D, odd, thr)
    # a NaN row (and column) of D joins nothing
    Dn = D.clone()
    Dn[:, S // 2, :] = float("nan")
    Dn[:, :, S // 2] = float("nan")
    got = _guarded_cluster(Dn, conf, float("inf"))
    _assert_clusters(got, Dn, conf, float("inf"))
    assert got[3].tolist() == [2] * B


def test_one_pose_and_no_ligand_launch_nothing():
    from fabind_amd.poses import cluster_poses, pairwise_rmsd
    A = _table([R.fixture_autos("benzene"), R.fixture_autos("chain_mixed")])
    cb = _cb(A)
    x = torch.randn(1, 10, 3, device=DEV)
    pc, D = cluster_poses(x, torch.randn(1, 2, device=DEV), cb, A)
    assert D.shape == (2, 1, 1) and not bool(D.any())
    assert pc.cluster_id.tolist() == [[0, 0]] and pc.leader.tolist() == [[0, 0]] and pc.size.tolist() == [[1, 1]] and pc.n_clusters.tolist() == [1, 1]
    assert all(t.dtype == torch.int32 for t in (pc.cluster_id, pc.leader, pc.size, pc.n_clusters))
    none = _table([])
    pc, D = cluster_poses(torch.zeros(4, 0, 3, device=DEV), torch.zeros(4, 0, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV), none)
    assert D.shape == (0, 4, 4) and pc.cluster_id.shape == (4, 0) and pc.n_clusters.shape == (0,)
    assert pairwise_rmsd(torch.zeros(4, 0, 3, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)).shape == (0, 4, 4)


def test_planted_modes_end_to_end():
    from fabind_amd.poses import cluster_poses
    for name, (poses, mode, D64, autos, conf) in R.mode_cases().items():
        assert (np.abs(D64 - R.THRESHOLD) >= R.MARGIN).all(), name                       # the margin condition first
        A = _table([autos])
        c = torch.from_numpy(conf).to(DEV).reshape(-1, 1)
        pc, D = cluster_poses(torch.from_numpy(poses).to(DEV), c, _cb(A), A, threshold=R.THRESHOLD)
        _assert_bound("modes " + name, D[0], D64, poses.shape[1])
        w = R.leader_cluster_ref(D64, conf, R.THRESHOLD)                                 # the restatement on the FLOAT64 distances
        assert int(pc.n_clusters[0]) == w[3] == mode.max() + 1, name
        cid = pc.cluster_id[:, 0].cpu().numpy()
        assert np.array_equal(cid, w[0]) and np.array_equal(pc.leader[:, 0].cpu().numpy(), w[1]), name
        assert np.array_equal(pc.size[:, 0].cpu().numpy(), w[2]), name
        assert ((cid[:, None] == cid[None, :]) == (mode[:, None] == mode[None, :])).all(), name     # the planted partition


def test_distinct_selection_against_select_by_confidence():
    from fabind_amd.plus.metrics import distinct_sampling_metrics, sampling_metrics, select_by_confidence, select_distinct_by_confidence
    from fabind_amd.poses import cluster_poses
    cases = R.mode_cases()
    names = ["benzene", "druglike_61"]                                                   # 16 and 20 poses: cut both to 16
    S = 16
    autos = [cases[nm][3] for nm in names]
    A = _table(autos)
    x = _stack([cases[nm][0][:S] for nm in names])
    g = torch.Generator().manual_seed(0)
    conf, rmsd, cdis = (torch.rand(S, 2, generator=g).to(DEV) * sc for sc in (1.0, 8.0, 6.0))
    pc, D = cluster_poses(x, conf, _cb(A), A)
    r1, c1, p1 = select_distinct_by_confidence(rmsd, cdis, conf, pc, top_n=1)
    w1 = select_by_confidence(rmsd, cdis, conf, top_n=1)
    assert torch.equal(r1, w1[0]) and torch.equal(c1, w1[1]) and torch.equal(p1[0], conf.argmax(0))
    pc0, _ = cluster_poses(x, conf, _cb(A), A, threshold=0.0)                            # singletons: the plain top-N for every N
    for top_n in range(1, S + 1):
        r, c, p = select_distinct_by_confidence(rmsd, cdis, conf, pc0, top_n=top_n)
        w = select_by_confidence(rmsd, cdis, conf, top_n=top_n)
        assert torch.equal(r, w[0]) and torch.equal(c, w[1]), top_n
    assert torch.equal(p, torch.argsort(conf, dim=0, descending=True, stable=True))
    m0, w0 = distinct_sampling_metrics(rmsd, cdis, conf, pc0, top_n=5), sampling_metrics(rmsd, cdis, conf, top_n=5)
    assert all(m0[k] == w0[k] for k in w0) and m0["n_clusters_mean"] == S and m0["top_cluster_share"] == 1 / S
    m = distinct_sampling_metrics(rmsd, cdis, conf, pc, top_n=5)
    ncl = pc.n_clusters.double().mean().item()
    assert m["n_clusters_mean"] == ncl and 1 < ncl < S and m["top_cluster_share"] == (pc.size[0].double().mean() / S).item()
    r5, _, p5 = select_distinct_by_confidence(rmsd, cdis, conf, pc, top_n=5)
    for b in range(2):                                                                   # fewer clusters than top_n: -1 padding, its own minima
        k = int(pc.n_clusters[b])
        lead = pc.leader[:min(k, 5), b].long()
        assert p5[:, b].tolist() == lead.tolist() + [-1] * (5 - len(lead)) and r5[b] == rmsd[lead, b].min()


def test_refusals_launch_nothing():
    from fabind_amd import _lib
    from fabind_amd.poses import cluster_from_distances, pairwise_rmsd
    A = _table([R.chain_autos(3)])
    cb = _cb(A)
    x = torch.zeros(513, 3, 3, device=DEV)
    with pytest.raises((ValueError, RuntimeError), match="512"):
        pairwise_rmsd(x, cb, A)
    with pytest.raises((ValueError, RuntimeError), match="512"):
        cluster_from_distances(torch.zeros(1, 513, 513, device=DEV), torch.zeros(513, 1, device=DEV))
    rc, D, guard = _guarded_pair(x, A)                                                   # the library's own refusal: nothing written
    assert rc != 0 and b"512" in _lib.load().fabind_last_error() and bool(torch.isnan(D).all()) and bool((guard == -7.0).all())
    big = torch.tensor([0, 2049], dtype=torch.int32, device=DEV)
    out = torch.full((4,), float("nan"), device=DEV)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = _lib.load().fabind_pose_pair_rmsd(torch.zeros(2, 2049, 3, device=DEV).data_ptr(), 2, 2049, big.data_ptr(), z.data_ptr(), z.data_ptr(),
                                           z.data_ptr(), 1, 2049, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"2048" in _lib.load().fabind_last_error() and bool(torch.isnan(out).all())
    ids = torch.full((513 + GUARD,), -77, dtype=torch.int32, device=DEV)
    rc = _lib.load().fabind_pose_cluster(torch.zeros(513 * 513, device=DEV).data_ptr(), torch.zeros(513, device=DEV).data_ptr(), 513, 1, 2.0,
                                         ids.data_ptr(), ids.data_ptr(), ids.data_ptr(), ids.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((ids == -77).all())
    with pytest.raises(ValueError, match="compound_batch"):                              # a mismatched compound_batch
        pairwise_rmsd(torch.zeros(3, 3, 3, device=DEV), torch.tensor([0, 0, 1], device=DEV), A)
    with pytest.raises(ValueError, match="compound_batch"):
        pairwise_rmsd(torch.zeros(3, 3, 3, device=DEV), torch.tensor([0, 0], device=DEV), A)
    with pytest.raises(ValueError, match="non-decreasing"):
        pairwise_rmsd(torch.zeros(3, 3, 3, device=DEV), torch.tensor([1, 0, 1], device=DEV))
