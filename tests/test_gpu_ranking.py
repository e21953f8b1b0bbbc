"""GPU: FABind+ confidence training on the device (csrc/ranking.hip, ops.pose_stats / ops.rank_loss,
plus.models.compute_confidence_loss, plus.metrics.ConfidenceEvaluator) against the float64 restatements of tests/ranking_refs.py.

Bounds (eps = 2^-23), all against float64 and fixed before the kernels first ran:
  rmsd            relative error <= (n + 8) eps          n atoms summed in fp32, then a division and a square root
  centroid dist.  absolute error <= (n + 8) eps max_i |p_i - t_i|
  loss            |error| <= (S + 16) eps mean|term|     a row of at most S - 1 terms per thread, a butterfly, four waves, exp / log1p
                  (with the BCE: + (S + 16) eps mean|BCE term|, the same reasoning for its S-term mean), and 1e-5 relative
  gradient        every element within (S + 16) eps 2 / S (an element sums S - 1 derivatives of size <= 1, over P = S (S - 1) / 2)
  counts          exact
For G groups the loss is a mean of G group losses: the bounds are averaged, plus 4 eps |loss| for torch's mean."""
import random

import numpy as np
import pytest
import torch

import ranking_refs as R
from helpers import hetero_from_npz, load_npz, weights

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
MODES = ["logsigmoid", "dynamic_hinge"]
LAYOUTS = [[2], [3], [63], [64], [65], [130], [2, 65, 7]]


def _dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ pose statistics
def _pose_inputs(sizes, seed=0):
    rng = np.random.default_rng(seed)
    N = sum(sizes)
    t = rng.uniform(-31.0, 31.0, (N, 3)).astype(np.float32)
    p = np.clip(t + rng.normal(0.0, 0.6, (N, 3)).astype(np.float32), -32.0, 32.0).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cb = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    return p, t, off, cb


def _check_pose(rmsd, cdis, p, t, off):
    rr, cr, dmax = R.pose_stats_ref(p, t, off)
    n = np.diff(off)
    for b in range(len(n)):
        print("sample %d n=%d rmsd err %.3e (bound %.3e) cdis err %.3e (bound %.3e)"
              % (b, n[b], abs(rmsd[b] - rr[b]), (n[b] + 8) * EPS * rr[b], abs(cdis[b] - cr[b]), (n[b] + 8) * EPS * dmax[b]))
    for b in range(len(n)):
        assert abs(rmsd[b] - rr[b]) <= (n[b] + 8) * EPS * rr[b], b
        assert abs(cdis[b] - cr[b]) <= (n[b] + 8) * EPS * dmax[b], b
        assert abs(rmsd[b] - rr[b]) < 1e-4 and abs(cdis[b] - cr[b]) < 1e-4     # the project's 1e-4 A gate


def test_pose_stats_match_float64_and_keep_their_sentinels():
    from fabind_amd._lib import check, load, ptr, stream
    dev = _dev()
    sizes = [1, 2, 63, 64, 65, 200]
    p, t, off, _ = _pose_inputs(sizes)
    B = len(sizes)
    pd, td, od = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(off).to(dev)
    buf_r = torch.full((B + 2,), -777.0, device=dev)
    buf_c = torch.full((B + 2,), -555.0, device=dev)
    check(load().fabind_pose_stats(ptr(pd), ptr(td), ptr(od), B, buf_r.data_ptr() + 4, buf_c.data_ptr() + 4, stream()), "fabind_pose_stats")
    r, c = buf_r.cpu().numpy(), buf_c.cpu().numpy()
    assert r[0] == -777.0 and r[-1] == -777.0 and c[0] == -555.0 and c[-1] == -555.0
    _check_pose(r[1:-1].astype(np.float64), c[1:-1].astype(np.float64), p, t, off)


def test_pose_stats_from_the_batch_vector_with_an_empty_sample():
    from fabind_amd import ops
    dev = _dev()
    sizes = [3, 0, 70, 5]
    p, t, off, cb = _pose_inputs(sizes, seed=1)
    r, c = ops.pose_stats(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(cb).to(dev), len(sizes))
    assert ops.atom_offsets(torch.from_numpy(cb).to(dev), len(sizes)).cpu().tolist() == off.tolist()
    r, c = r.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64)
    assert r[1] == 0.0 and c[1] == 0.0                              # scatter_mean's empty row
    _check_pose(r, c, p, t, off)


# ------------------------------------------------------------------------------------------------ ranking loss
_REFS = {}


def _case(sizes, mode, with_ce):
    """Inputs and float64 reference of one layout, computed once and shared (never modified)."""
    key = (tuple(sizes), mode, with_ce)
    if key not in _REFS:
        scores, rmsd = R.make_rank_inputs(sizes, seed=1000 + 17 * sum(sizes) + len(sizes))
        R.assert_rank_input_conditions(scores, rmsd, sizes)
        _REFS[key] = (scores, rmsd) + R.rank_ref(scores, rmsd, sizes, mode, with_ce)
    return _REFS[key]


def _loss_bound(per):
    return [(len(p["grad"]) + 16) * EPS * (p["mean_abs_term"] + p["mean_abs_ce"]) for p in per]


def _run(scores, rmsd, sizes, mode, with_ce, upstream=None):
    from fabind_amd import ops
    dev = _dev()
    s = torch.from_numpy(np.asarray(scores, dtype=np.float32)).to(dev).requires_grad_(True)
    r = torch.from_numpy(np.asarray(rmsd, dtype=np.float32)).to(dev)
    kw = dict(group_size=None) if len(sizes) == 1 else dict(group_sizes=sizes)
    loss, ranking, ce, terms, counts = ops.rank_loss(s, r, mode=mode, with_ce=with_ce, **kw)
    (loss if upstream is None else loss * upstream).backward()
    return (float(loss.detach()), float(ranking), float(ce), terms.cpu().numpy().astype(np.float64), counts.cpu().numpy(),
            s.grad.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("with_ce", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)))
def test_rank_loss_matches_float64(sizes, mode, with_ce):
    scores, rmsd, tot, per = _case(sizes, mode, with_ce)
    loss, ranking, ce, terms, counts, grad = _run(scores, rmsd, sizes, mode, with_ce)
    G, bounds = len(sizes), _loss_bound(per)
    o = 0
    for g, (p, bd) in enumerate(zip(per, bounds)):
        S = sizes[g]
        gb = (S + 16) * EPS * 2 / S / G
        gerr = np.abs(grad[o:o + S] - p["grad"] / G).max()
        print("group %d S=%d %s ce=%d: loss err %.3e (bound %.3e), grad err %.3e (bound %.3e)"
              % (g, S, mode, with_ce, abs(terms[g, 2] - p["loss"]), bd, gerr, gb))
        assert abs(terms[g, 0] - p["ranking"]) <= bd and abs(terms[g, 1] - p["ce"]) <= bd and abs(terms[g, 2] - p["loss"]) <= bd
        assert abs(terms[g, 2] - p["loss"]) <= 1e-5 * abs(p["loss"])              # the project's relative loss gate
        assert gerr <= gb
        assert counts[g].tolist() == p["counts"].tolist()
        o += S
    slack = 0.0 if G == 1 else 4 * EPS * abs(tot["loss"])
    assert abs(loss - tot["loss"]) <= np.mean(bounds) + slack
    assert abs(ranking - tot["ranking"]) <= np.mean(bounds) + slack and abs(ce - tot["ce"]) <= np.mean(bounds) + slack
    assert abs(loss - tot["loss"]) <= 1e-5 * abs(tot["loss"])
    if not with_ce:
        assert ce == 0.0 and np.all(terms[:, 1] == 0.0)


def test_group_size_splits_consecutive_runs():
    from fabind_amd import ops
    sizes = [8] * 5
    scores, rmsd = R.make_rank_inputs(sizes, seed=5)
    tot, per = R.rank_ref(scores, rmsd, sizes, "logsigmoid", True)
    dev = _dev()
    loss, _, _, terms, counts = ops.rank_loss(torch.from_numpy(scores).to(dev), torch.from_numpy(rmsd).to(dev), group_size=8,
                                              mode="logsigmoid", with_ce=True)
    assert terms.shape == (5, 3) and counts.cpu().numpy().tolist() == tot["counts"].tolist()
    assert abs(float(loss) - tot["loss"]) <= np.mean(_loss_bound(per)) + 4 * EPS * abs(tot["loss"])


def test_exact_rmsd_tie_resolves_by_index():
    for mode in MODES:
        scores, rmsd = [0.5, 1.5, -0.25], [1.0, 1.0, 3.0]
        ref = R.rank_group_ref(scores, rmsd, mode)
        loss, _, _, _, counts, grad = _run(scores, rmsd, [3], mode, False)
        assert counts[0].tolist() == ref["counts"].tolist() == [2, 3, 0, 2]      # (the other tie order gives 3 ranked right)
        assert abs(loss - ref["loss"]) <= 19 * EPS * ref["mean_abs_term"]
        assert np.abs(grad - ref["grad"]).max() <= 19 * EPS * 2 / 3


def test_hinge_term_exactly_zero_has_zero_gradient():
    # margin 1.5 - 1.0 = 0.5 = score gap 0.75 - 0.25: relu(0) with gradient 0
    loss, _, _, _, counts, grad = _run([0.75, 0.25], [1.0, 1.5], [2], "dynamic_hinge", False)
    assert loss == 0.0 and np.all(grad == 0.0) and counts[0].tolist() == [1, 1, 1, 2]


def test_dyadic_hinge_inputs_agree_with_the_rounded_reference_to_one_ulp():
    rng = np.random.default_rng(11)
    S = 65
    scores = rng.integers(-40, 40, S) / 8.0
    rmsd = rng.permutation(S) / 16.0 + 0.25
    ref = R.rank_group_ref(scores, rmsd, "dynamic_hinge")           # every sum is exact in float64 AND in float32
    loss, _, _, _, counts, grad = _run(scores, rmsd, [S], "dynamic_hinge", False)
    want = np.float32(ref["loss"])
    assert abs(np.float32(loss) - want) <= np.spacing(want)
    gw = ref["grad"].astype(np.float32)
    assert np.all(np.abs(grad.astype(np.float32) - gw) <= np.spacing(np.abs(gw)))
    assert counts[0].tolist() == ref["counts"].tolist()


def test_large_scores_stay_finite_in_logsigmoid_mode():
    scores, rmsd = [80.0, -80.0, 40.0, -40.0, 0.5], [1.0, 2.5, 3.0, 1.5, 6.0]
    ref = R.rank_group_ref(scores, rmsd, "logsigmoid", True)
    loss, _, _, _, counts, grad = _run(scores, rmsd, [5], "logsigmoid", True)
    assert np.isfinite(loss) and np.all(np.isfinite(grad))
    assert abs(loss - ref["loss"]) <= 21 * EPS * (ref["mean_abs_term"] + ref["mean_abs_ce"])
    assert np.abs(grad - ref["grad"]).max() <= 21 * EPS * 2 / 5
    assert counts[0].tolist() == ref["counts"].tolist()


def test_group_sizes_outside_2_to_1024_raise_before_any_launch():
    from fabind_amd import ops
    dev = _dev()
    for B in (1, 1025):
        with pytest.raises(ValueError):
            ops.rank_loss(torch.zeros(B, device=dev), torch.ones(B, device=dev))
    with pytest.raises(ValueError):
        ops.rank_loss(torch.zeros(6, device=dev), torch.ones(6, device=dev), group_size=1)
    with pytest.raises(ValueError):
        ops.rank_loss(torch.zeros(6, device=dev), torch.ones(6, device=dev), group_sizes=[5, 1])


def test_the_largest_group_runs():
    scores, rmsd = R.make_rank_inputs([1024], seed=9)
    loss, _, _, _, counts, grad = _run(scores, rmsd, [1024], "dynamic_hinge", False)
    s64, r64 = scores.astype(np.float64), rmsd.astype(np.float64)
    better = r64[None, :] < r64[:, None]                           # [a, b]: b better than a (distinct rmsds)
    m = np.where(better, (r64[:, None] - r64[None, :]) - (s64[None, :] - s64[:, None]), 0.0)
    want = np.maximum(m, 0.0).sum() / (1024 * 1023 / 2)
    assert abs(loss - want) <= (1024 + 16) * EPS * want
    assert counts[0, 1] == 1024 * 1023 // 2 and counts[0, 0] == int((better & (s64[None, :] > s64[:, None])).sum())
    assert np.isfinite(grad).all() and abs(grad.sum()) <= 1024 * EPS


def test_autograd_with_upstream_gradient_and_bit_reproducibility():
    sizes, mode = [2, 65, 7], "logsigmoid"
    scores, rmsd, tot, per = _case(sizes, mode, True)
    a = _run(scores, rmsd, sizes, mode, True, upstream=3.0)
    b = _run(scores, rmsd, sizes, mode, True, upstream=3.0)
    o = 0
    for S in sizes:
        assert np.abs(a[5][o:o + S] - 3.0 * tot["grad"][o:o + S]).max() <= 3.0 * (S + 16) * EPS * 2 / S / len(sizes)
        o += S
    assert a[0] == b[0] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


# ------------------------------------------------------------------------------------------------ end to end
class _Logger:
    def log_message(self, s):
        pass


def _sampling_model(g, dev):
    """The model of tests/test_gpu_plus.py::_sampling_model, frozen like train_confidence.py:163-166."""
    from argparse import Namespace
    from fabind_amd.plus.models import get_model
    hidden, pocket_hidden, layers, n_iter, _ = [int(v) for v in g["cfg"]]
    a = Namespace(
        mode=5, n_iter=n_iter, mean_layers=layers, hidden_size=hidden, refine="refine_coord", coordinate_scale=5.0,
        geometry_reg_step_size=0.001, rm_layernorm=True, add_attn_pair_bias=True, explicit_pair_embed=True,
        add_cross_attn_layer=True, norm_type="per_sample", random_n_iter=False, inter_cutoff=10.0, intra_cutoff=8.0,
        ablation_no_attention=False, ablation_no_attention_with_cross_attn=False, keep_trig_attn=False, opm=False,
        rm_F_norm=False, fix_pocket=False, rm_LAS_constrained_optim=False, use_ln_mlp=True, mlp_hidden_scale=1, dropout=0.1,
        mha_heads=4, rel_dis_pair_bias="no", inter_additional_mlp=False, only_last_LAS=False, geom_reg_steps=1,
        pocket_pred_hidden_size=pocket_hidden, pocket_pred_layers=1, pocket_pred_n_iter=1, use_for_radius_pred="ligand",
        dis_map_thres=15.0, pocket_radius_buffer=5.0, min_pocket_radius=float(g["min_pocket_radius"]), force_fix_radius=False,
        gs_tau=1.0, gs_hard=False, pocket_radius=20.0, train_pred_pocket_noise=0.0, local_eval=False, confidence_training=True,
        stack_mlp=True, confidence_use_ln_mlp=True, confidence_dropout=0.2, confidence_mlp_hidden_scale=1, use_clustering=True,
        dbscan_eps=9.0, dbscan_min_samples=2, choose_cluster_prob=0.5)
    m = get_model(a, _Logger())
    m.load_state_dict(weights(g), strict=True)
    for name, p in m.named_parameters():
        p.requires_grad = "confidence" in name or "ranking" in name
    return m.to(dev).eval()


def _forward(m, g, dev, seed):
    random.seed(seed)
    data = hetero_from_npz(g).to(dev)
    return m(data, stage=1, train=True), data


def _outputs64(out, data):
    coords, cb, truth = (t.detach().cpu().numpy() for t in (out[0], out[1], data.coords))
    off = np.concatenate([[0], np.cumsum(np.bincount(cb, minlength=out[5].shape[0]))])
    rmsd, cdis, _ = R.pose_stats_ref(coords, truth, off)
    return out[5].detach().cpu().numpy().astype(np.float64).reshape(-1), rmsd, cdis, np.diff(off)


@pytest.mark.parametrize("mode", MODES)
def test_compute_confidence_loss_end_to_end(mode):
    from argparse import Namespace
    from fabind_amd import engine
    from fabind_amd.plus.models import compute_confidence_loss
    dev = _dev()
    engine.set_precision("fp32")
    g = load_npz("plus_model_sampling_tiny")
    m = _sampling_model(g, dev)
    out, data = _forward(m, g, dev, int(g["py_seed"]) + 2)
    assert len(out) == 7
    torch.cuda.set_sync_debug_mode("error")                         # the call makes no host round trip
    try:
        loss, info = compute_confidence_loss(out, data, Namespace(ranking_loss=mode, keep_cls_2A=True))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    scores, rmsd, cdis, n = _outputs64(out, data)
    ref = R.rank_group_ref(scores, rmsd, mode, True)
    S = len(scores)
    got_r = info["rmsd"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got_r - rmsd) <= (n + 8) * EPS * rmsd)
    assert np.all(np.abs(info["centroid_dis"].cpu().numpy() - cdis) < 1e-4)
    # the kernel ranks its own fp32 rmsds: in hinge mode a pair's margin carries their error on top of the loss bound
    bound = (S + 16) * EPS * (ref["mean_abs_term"] + ref["mean_abs_ce"]) + (2 * ((n + 8) * EPS * rmsd).max() if mode == "dynamic_hinge" else 0.0)
    print("end to end %s: loss %.8f ref %.8f bound %.3e" % (mode, float(loss.detach()), ref["loss"], bound))
    assert abs(float(loss) - ref["loss"]) <= bound
    assert abs(float(info["ranking"]) + float(info["ce"]) - float(loss)) <= 2 * EPS * abs(float(loss))
    assert info["counts"].cpu().numpy()[0].tolist() == ref["counts"].tolist()
    m.zero_grad()
    loss.backward()
    with_grad = [name for name, p in m.named_parameters() if p.grad is not None]
    assert with_grad and all(name.startswith(("ranking", "confidence")) for name in with_grad)
    assert any(name.startswith("ranking_score_mlp") for name in with_grad)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert any(float(p.grad.abs().max()) > 0 for p in m.parameters() if p.grad is not None)


def test_confidence_evaluator_over_two_updates_matches_the_restated_dictionary():
    from argparse import Namespace
    from fabind_amd import engine
    from fabind_amd.plus.metrics import ConfidenceEvaluator
    dev = _dev()
    engine.set_precision("fp32")
    g = load_npz("plus_model_sampling_tiny")
    m = _sampling_model(g, dev)
    ev = ConfidenceEvaluator(Namespace(ranking_loss="logsigmoid", keep_cls_2A=True))
    batches = []
    for k in (1, 2):
        with torch.no_grad():
            out, data = _forward(m, g, dev, int(g["py_seed"]) + k)
        if k == 2:                                                  # a second, different batch: the same poses, other scores
            out = out[:5] + (out[5] * -1.5 + 0.25,) + out[6:]
        torch.cuda.set_sync_debug_mode("error")                     # update never waits for the device
        try:
            ev.update(out, data.coords)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        scores, rmsd, cdis, _ = _outputs64(out, data)
        batches.append(dict(scores=scores, rmsd=rmsd, cdis=cdis, logits=out[2].cpu().numpy(), mask=out[3].cpu().numpy(),
                            less5=int(out[4]), mode="logsigmoid", with_ce=True))
    import warnings
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            got = ev.compute()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert sum("called a synchronizing" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]   # one read-back
    ref = R.metrics_ref(batches)
    assert list(got) == list(ref)                                   # the reference's keys, in its order
    for k in ref:
        print("%-22s %.8g %.8g" % (k, got[k], ref[k]))
        if isinstance(ref[k], (int, np.integer)) or k in ("confidence_accuracy", "ranking_accuracy", "hit_rate"):
            assert got[k] == ref[k], k
        else:
            assert abs(got[k] - ref[k]) <= 1e-5 * max(abs(ref[k]), 1e-3), k      # fp32 values against float64: the 1e-5 gate


def test_train_step_takes_the_confidence_loss():
    """parallel.train_step with compute_loss=compute_confidence_loss on the frozen model: the step moves the ranking head only."""
    from argparse import Namespace
    from fabind_amd import engine, parallel
    from fabind_amd.plus.models import compute_confidence_loss
    dev = _dev()
    engine.set_precision("fp32")
    g = load_npz("plus_model_sampling_tiny")
    m = _sampling_model(g, dev)
    args = Namespace(ranking_loss="logsigmoid", keep_cls_2A=True)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-2)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    random.seed(int(g["py_seed"]) + 2)
    res = parallel.train_step(m, hetero_from_npz(g).to(dev), opt, lambda out, data: compute_confidence_loss(out, data, args), stage=1)
    assert res is not None
    loss, terms = res
    assert torch.isfinite(loss) and sorted(terms) == ["ce", "centroid_dis", "counts", "ranking", "rmsd"]
    moved = [n for n, p in m.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert moved and all(n.startswith(("ranking", "confidence")) for n in moved)
