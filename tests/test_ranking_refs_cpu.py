"""CPU: the float64 restatements of tests/ranking_refs.py against torch float64 autograd of the reference's own double loop
(FABind_plus/fabind/utils/training_confidence.py:48-73), the binding of the ranking entry points, and the torch-side selection and
sampling metrics of fabind_amd.plus.metrics against numpy."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ranking_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_loop(scores, rmsd, mode, with_ce):
    """training_confidence.py:48-73 as written, on float64 tensors (the stable argsort is the one liberty)."""
    s = torch.tensor(np.asarray(scores, dtype=np.float64), requires_grad=True)
    r = torch.tensor(np.asarray(rmsd, dtype=np.float64))
    order = torch.tensor(R.stable_order(r.tolist()))
    ss, sr = s[order], r[order]
    ranking_loss = 0.
    y = (r < 2).double()
    for i in range(len(ss)):
        for j in range(i):
            if mode == "dynamic_hinge":
                ranking_loss = ranking_loss + F.relu((sr[i] - sr[j]) - (ss[j] - ss[i]))
            else:
                ranking_loss = ranking_loss + -F.logsigmoid(ss[j] - ss[i])
    ranking_loss = ranking_loss / (len(ss) * (len(ss) - 1) / 2)
    loss = ranking_loss + F.binary_cross_entropy_with_logits(s, y) if with_ce else ranking_loss
    loss.backward()
    return float(loss.detach()), s.grad.numpy()


@pytest.mark.parametrize("with_ce", [False, True])
@pytest.mark.parametrize("mode", ["logsigmoid", "dynamic_hinge"])
@pytest.mark.parametrize("S", [2, 3, 63, 65])
def test_restatement_equals_torch_float64_autograd(S, mode, with_ce):
    scores, rmsd = R.make_rank_inputs([S], seed=100 + S)
    R.assert_rank_input_conditions(scores, rmsd, [S])
    ref = R.rank_group_ref(scores, rmsd, mode, with_ce)
    loss, grad = _torch_loop(scores, rmsd, mode, with_ce)
    assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ref["grad"] - grad).max() <= 1e-12
    assert ref["mean_abs_term"] >= 0 and ref["counts"][1] == S * (S - 1) // 2


def test_restatement_counts_on_a_hand_case():
    # rmsd order: sample 2 (0.5), 0 (1.0), 1 (3.0); scores 0.2, -1.0, 0.7
    ref = R.rank_group_ref([0.2, -1.0, 0.7], [1.0, 3.0, 0.5], "logsigmoid", True)
    # pairs (better, worse): (2, 0) 0.7 > 0.2, (2, 1) 0.7 > -1, (0, 1) 0.2 > -1 -> 3 right; best sample 2 has the top score -> hit;
    # first score 0.2 > 0 -> label 1 matches [rmsd < 2] of samples 0 and 2
    assert ref["counts"].tolist() == [3, 3, 1, 2]
    ref = R.rank_group_ref([0.5, 1.5, -0.25], [1.0, 1.0, 3.0], "dynamic_hinge")
    assert ref["counts"].tolist() == [2, 3, 0, 2]                # the tie 0 / 1 resolves by index: 0 is the better one


def test_grouped_restatement_is_the_mean_over_groups():
    sizes = [2, 5, 3]
    scores, rmsd = R.make_rank_inputs(sizes, seed=7)
    tot, per = R.rank_ref(scores, rmsd, sizes, "logsigmoid", True)
    assert abs(tot["loss"] - np.mean([p["loss"] for p in per])) < 1e-15
    assert tot["counts"].shape == (3, 4) and tot["grad"].shape == (10,)
    assert np.allclose(tot["grad"][2:7], per[1]["grad"] / 3, rtol=0, atol=1e-16)


def test_entry_points_are_declared_bound_and_built_from_source():
    from fabind_amd import _lib, build
    assert "ranking.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    for name in ("fabind_pose_stats", "fabind_rank_loss_fwd"):
        assert name in _lib.SIGNATURES
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name      # the binding mirrors the header
    assert _lib.ABI_VERSION == 19 and "#define FABIND_ABI_VERSION 19" in hdr        # additive: the version stays
    from fabind_amd.plus.models import compute_confidence_loss                      # noqa: F401
    from fabind_amd.plus.metrics import ConfidenceEvaluator, sampling_metrics, select_by_confidence  # noqa: F401


def test_group_sizes_are_refused_on_the_host_before_any_launch():
    from fabind_amd import ops
    # CPU tensors: a launch would raise RuntimeError (no CPU fallback), so a ValueError proves the check came first
    for B, gs in ((1, None), (1025, None), (8, 1), (10, 4), (4, 8)):
        with pytest.raises(ValueError):
            ops.rank_loss(torch.zeros(B), torch.ones(B), group_size=gs)
    with pytest.raises(ValueError):
        ops.rank_loss(torch.zeros(4), torch.ones(4), group_sizes=[3, 1])
    with pytest.raises(ValueError):
        ops.rank_loss(torch.zeros(4), torch.ones(5))
    with pytest.raises(ValueError):
        ops.rank_loss(torch.zeros(4), torch.ones(4), mode="hinge")
    with pytest.raises(ValueError):
        ops.pose_stats(torch.zeros(5, 3), torch.zeros(4, 3), torch.zeros(5, dtype=torch.int64), 2)


@pytest.mark.parametrize("top_n", [1, 3, 5])
def test_selection_and_sampling_metrics_match_numpy(top_n):
    from fabind_amd.plus.metrics import sampling_metrics, select_by_confidence
    rng = np.random.default_rng(3)
    S, B = 5, 17
    rmsd, cdis = rng.uniform(0.3, 9.0, (S, B)), rng.uniform(0.1, 7.0, (S, B))
    conf = rng.permutation(S * B).reshape(S, B) * 0.37 - 20.0     # distinct: numpy's reversed argsort has no tie rule
    r, c = select_by_confidence(torch.tensor(rmsd), torch.tensor(cdis), torch.tensor(conf), top_n)
    rr, cr = R.select_ref(rmsd, cdis, conf, top_n)
    assert np.array_equal(r.numpy(), rr) and np.array_equal(c.numpy(), cr)
    got = sampling_metrics(torch.tensor(rmsd), torch.tensor(cdis), torch.tensor(conf), top_n)
    ref = R.sampling_metrics_ref(rmsd, cdis, conf, top_n)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), k
    if top_n == S:                                                # every sample kept: the plain minimum
        assert np.array_equal(rr, rmsd.min(0))
    with pytest.raises(ValueError):
        select_by_confidence(torch.tensor(rmsd), torch.tensor(cdis), torch.tensor(conf), S + 1)
