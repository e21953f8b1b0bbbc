"""CPU: the float64 restatements of tests/pose_cluster_refs.py against independent definitions (the minimum over ALL label- and
bond-preserving permutations, enumerated with itertools), the invariants of leader clustering, the margin condition of every planted-mode
case the GPU test clusters, and the contract of fabind_amd/poses.py that needs no device."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import pose_cluster_refs as R
from helpers import load_npz


def _enumerated_autos(labels, bonds):
    n = len(labels)
    adj = np.zeros((n, n), dtype=bool)
    for i, j in np.asarray(bonds).reshape(2, -1).T:
        adj[i, j] = adj[j, i] = True
    out = []
    for p in itertools.permutations(range(n)):
        p = np.array(p)
        if (labels[p] == labels).all() and (adj[np.ix_(p, p)] == adj).all():
            out.append(p)
    return np.array(out)


@pytest.mark.parametrize("name", ["chain_mixed", "chain_equal", "benzene", "neopentane", "cyclohexane", "single_atom"])
def test_pair_rmsd_ref_is_the_minimum_over_all_structure_preserving_permutations(name):
    g = load_npz("symmetry_graphs")
    gi = [str(s) for s in g["names"]].index(name)
    labels, bonds, autos = g["g%d_labels" % gi], g["g%d_bonds" % gi], g["g%d_autos" % gi]
    n = len(labels)
    assert n <= 7
    mine = _enumerated_autos(labels, bonds)
    assert sorted(map(tuple, mine)) == sorted(map(tuple, autos))                       # the fixture's list is the whole group
    rng = np.random.default_rng(gi)
    x = R.random_poses(rng, 5, n, autos).astype(np.float64)
    D = R.pair_rmsd_ref(x, autos)
    for s in range(5):
        for t in range(5):
            want = 0.0 if s == t else min(np.sqrt(((x[s][p] - x[t]) ** 2).sum(-1).mean()) for p in mine)
            assert abs(D[s, t] - want) <= 1e-12 * max(want, 1.0), (name, s, t)
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    plain = R.pair_rmsd_ref(x, np.arange(n).reshape(1, n))
    assert (D <= plain + 1e-15).all() and (len(autos) < 12 or (D < plain - 1e-6).any())


def test_hand_built_tables_are_automorphisms():
    for n in (3, 63, 64, 65):
        a = R.ring_autos(n)
        assert a.shape == (2 * n, n) and len({tuple(r) for r in a}) == 2 * n and (np.sort(a, 1) == np.arange(n)).all()
        assert (a[0] == np.arange(n)).all() and all(tuple(a[k]) < tuple(a[k + 1]) for k in range(2 * n - 1))
        ring = {frozenset((i, (i + 1) % n)) for i in range(n)}
        assert all({frozenset((r[i], r[(i + 1) % n])) for i in range(n)} == ring for r in a)
    assert R.chain_autos(1).tolist() == [[0]] and R.chain_autos(2).tolist() == [[0, 1], [1, 0]]
    assert R.chain_autos(256).shape == (2, 256)


def _check_invariants(D, conf, thr):
    cid, leader, size, k = R.leader_cluster_ref(D, conf, thr)
    S = len(conf)
    assert (cid >= 0).all() and set(cid) == set(range(k))                                # a partition into k non-empty clusters
    assert (leader[k:] == -1).all() and (size[k:] == 0).all() and size[:k].sum() == S
    assert [int((cid == c).sum()) for c in range(k)] == size[:k].tolist()
    for c in range(k):
        assert cid[leader[c]] == c
        for t in np.nonzero(cid == c)[0]:
            assert t == leader[c] or D[leader[c], t] < thr                               # members within thr of their leader
    for c in range(k):
        for e in range(c + 1, k):
            assert not D[leader[c], leader[e]] < thr                                     # leaders pairwise >= thr
    key = [(np.isnan(conf[p]), -conf[p] if not np.isnan(conf[p]) else 0.0, p) for p in leader[:k]]
    assert key == sorted(key)                                                            # leaders in confidence order
    return cid, leader, size, k


def test_leader_clustering_invariants():
    rng = np.random.default_rng(5)
    for S in (1, 2, 7, 40):
        x = rng.normal(scale=2.0, size=(S, 4, 3))
        D = R.pair_rmsd_ref(x, np.arange(4).reshape(1, 4))
        conf = rng.normal(size=S)
        for thr in (0.0, 1.5, 2.5, 4.0, np.inf):
            cid, leader, size, k = _check_invariants(D, conf, thr)
            if thr == 0.0:
                assert k == S and leader.tolist() == np.argsort(-conf, kind="stable").tolist()
            if thr == np.inf:
                assert k == 1 and size[0] == S and leader[0] == int(np.argmax(conf))
        tied = np.round(conf)                                                            # ties keep pose order
        _check_invariants(D, tied, 2.5)
        assert R.leader_cluster_ref(D, np.zeros(S), 0.0)[1].tolist() == list(range(S))
        odd = conf.copy()
        odd[::3] = np.nan
        if S > 1:
            odd[1] = np.inf
        cid, leader, size, k = _check_invariants(D, odd, 2.5)
        assert S == 1 or leader[0] == 1                                                  # +inf first, NaN never ahead of a number
        assert R.leader_cluster_ref(D, odd, 0.0)[1][-len(odd[::3]):].tolist() == list(range(0, S, 3))
        Dn = D.copy()
        Dn[0, :] = Dn[:, 0] = np.nan                                                     # a NaN row joins nothing
        cid, _, size, _ = _check_invariants(Dn, conf, np.inf)
        assert size[cid[0]] == 1


def test_planted_modes_keep_their_margin():
    for name, (poses, mode, D, autos, conf) in R.mode_cases().items():
        assert np.array_equal(D, R.pair_rmsd_ref(poses, autos)), name
        assert (np.abs(D - R.THRESHOLD) >= R.MARGIN).all(), name
        n = poses.shape[1]
        assert (R.bound(D, n) < np.abs(D - R.THRESHOLD) / 10).all()                      # the float32 error cannot cross the threshold
        same = mode[:, None] == mode[None, :]
        assert (D[same] < R.THRESHOLD).all() and (D[~same] > R.THRESHOLD).all(), name
        cid, leader, size, k = R.leader_cluster_ref(D, conf, R.THRESHOLD)
        assert k == mode.max() + 1 and ((cid[:, None] == cid[None, :]) == same).all(), name
        if name in ("benzene", "c60"):                                                   # every atom moves: plain RMSD splits the modes
            assert R.leader_cluster_ref(R.pair_rmsd_ref(poses, np.arange(n).reshape(1, n)), conf, R.THRESHOLD)[3] > k, name


def test_distance_cases_cover_the_shapes():
    c = R.cases()
    ns = {v[0].shape[1] for v in c.values()}
    Ss = {v[0].shape[0] for v in c.values()}
    Ks = {len(v[1]) for v in c.values()}
    assert {1, 2, 63, 64, 65, 256, 257} <= ns and {2, 3, 63, 64, 65, 257} <= Ss and {1, 2, 12, 24, 120} <= Ks
    for name, (poses, autos, D) in c.items():
        assert poses.dtype == np.float32 and np.isfinite(D).all() and (D[~np.eye(len(D), dtype=bool)] > 0).all(), name


def test_poses_module_refuses_cpu_tensors_and_is_declared():
    from fabind_amd import _lib, build, poses
    x, cb, conf = torch.zeros(3, 4, 3), torch.zeros(4, dtype=torch.long), torch.zeros(3, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        poses.pairwise_rmsd(x, cb)
    with pytest.raises(RuntimeError, match="HIP device only"):
        poses.cluster_from_distances(torch.zeros(1, 3, 3), conf)
    with pytest.raises(RuntimeError, match="HIP device only"):
        poses.cluster_poses(x, conf, cb)
    assert "pose_cluster.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pose_cluster.hip"))
    hdr = open(os.path.join(build.INCLUDE, "fabind_hip.h")).read()
    for nm in ("fabind_pose_pair_rmsd", "fabind_pose_cluster"):
        assert nm in _lib.SIGNATURES and re.search(r"\bint\s+%s\s*\(" % nm, hdr)
    assert _lib.ABI_VERSION == 19 and "#define FABIND_ABI_VERSION 19" in hdr             # additive: the version stays


def test_distinct_selection_on_a_hand_worked_case():
    """Two modes, the less populated one ranked first.  Poses 0..5, confidences 0.9 (pose 4), 0.8 (pose 1), ...: mode A = {4, 2},
    mode B = {1, 0, 3, 5}.  Clusters in confidence order: A (leader 4, size 2), B (leader 1, size 4)."""
    from fabind_amd.plus.metrics import distinct_sampling_metrics, select_by_confidence, select_distinct_by_confidence
    from fabind_amd.poses import PoseClusters
    conf = torch.tensor([[0.5], [0.8], [0.7], [0.3], [0.9], [0.1]])
    rmsd = torch.tensor([[1.0], [1.2], [6.1], [0.9], [6.0], [1.1]])
    cdis = torch.tensor([[0.4], [0.5], [5.0], [0.2], [5.5], [0.3]])
    D = np.full((6, 6), 7.0)
    for grp in ((4, 2), (1, 0, 3, 5)):
        for i in grp:
            for j in grp:
                D[i, j] = 0.0 if i == j else 0.5
    cid, leader, size, k = R.leader_cluster_ref(D, conf[:, 0].numpy(), 2.0)
    assert k == 2 and leader[:2].tolist() == [4, 1] and size[:2].tolist() == [2, 4] and cid.tolist() == [1, 1, 0, 1, 0, 1]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32).reshape(-1, 1)                   # noqa: E731
    cl = PoseClusters(i32(cid), i32(leader), i32(size), torch.tensor([k], dtype=torch.int32))
    r1, c1, p1 = select_distinct_by_confidence(rmsd, cdis, conf, cl, top_n=1)
    assert (r1.item(), c1.item(), p1.tolist()) == (6.0, 5.5, [[4]])
    assert select_by_confidence(rmsd, cdis, conf, 1)[0].item() == 6.0
    r2, c2, p2 = select_distinct_by_confidence(rmsd, cdis, conf, cl, top_n=2)           # the second DISTINCT pose is mode B's leader
    assert (round(r2.item(), 6), c2.item(), p2.tolist()) == (1.2, 0.5, [[4], [1]])
    r3, c3, p3 = select_distinct_by_confidence(rmsd, cdis, conf, cl, top_n=3)           # only two clusters: -1 padding, same minima
    assert (round(r3.item(), 6), c3.item(), p3.tolist()) == (1.2, 0.5, [[4], [1], [-1]])
    assert select_by_confidence(rmsd, cdis, conf, 3)[0].item() == pytest.approx(1.2)    # (top-3 by confidence alone: poses 4, 1, 2)
    assert select_by_confidence(rmsd, cdis, conf, 2)[1].item() == 0.5
    m = distinct_sampling_metrics(rmsd, cdis, conf, cl, top_n=2)
    assert m["n_clusters_mean"] == 2.0 and m["top_cluster_share"] == pytest.approx(2 / 6) and m["rmsd_2A"] == 1.0
    assert distinct_sampling_metrics(rmsd, cdis, conf, cl, top_n=1)["rmsd_2A"] == 0.0
    with pytest.raises(ValueError):
        select_distinct_by_confidence(rmsd, cdis, conf, cl, top_n=7)
