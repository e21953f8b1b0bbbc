"""GPU: the fused Adam / AdamW step (fabind_amd/optim.py + csrc/optim.hip: global-norm clip and non-finite skip folded in, two
launches) against torch.optim.Adam / AdamW + torch.nn.utils.clip_grad_norm_ in float64 on the CPU.

Bounds (five steps of one fp32 ulp with headroom for operation order; torch's own fp32 CPU Adam sits at 4.4e-7 / 5.5e-7 / 3.7e-7 /
1e-7 against float64 on these shapes): |dp| <= 2e-6 max(1, |p|); exp_avg, exp_avg_sq within 2e-6 of each tensor's largest magnitude;
grad_norm within 1e-6 relative; step counters equal."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GROUPS = (dict(lr=1e-3, weight_decay=0.01), dict(lr=3e-4, weight_decay=0.0))


def _shapes():
    from fabind_amd.optim import CHUNK as C
    return [(1,), (3,), (4,), (5,), (255,), (256,), (257,), (1023,), (C - 1,), (C,), (C + 1,), (2 * C + 3,), (7, 13), (64, 65)]


def _randn(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in shapes]


def _grouped(params):
    """Two groups: even tensors lr 1e-3 / wd 0.01, odd tensors lr 3e-4 / wd 0."""
    return [dict(params=params[0::2], **GROUPS[0]), dict(params=params[1::2], **GROUPS[1])]


def _pair(shapes, decoupled, seed=0, **kw):
    """(fused optimizer on device copies, float64 CPU torch optimizer) from the same initial values."""
    from fabind_amd.optim import FusedAdam
    init = _randn(shapes, seed)
    pf = [torch.nn.Parameter(t.to(DEV)) for t in init]
    pr = [torch.nn.Parameter(t.double()) for t in init]
    fused = FusedAdam(_grouped(pf), decoupled_weight_decay=decoupled, **kw)
    ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(_grouped(pr))
    return pf, fused, pr, ref


def _set_grads(pf, pr, grads, skip=()):
    for i, g in enumerate(grads):
        pf[i].grad = None if i in skip else g.to(DEV)
        pr[i].grad = None if i in skip else g.double()


def _ref_step(pr, ref, max_norm):
    """-> pre-clip norm (float64)."""
    have = [p for p in pr if p.grad is not None]
    if max_norm is not None:
        total = torch.nn.utils.clip_grad_norm_(have, max_norm)
    else:
        total = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in have]))
    ref.step()
    return float(total)


def _compare(pf, fused, pr, ref, tag):
    """Asserts the module docstring's bounds between a FusedAdam and a (float64 or fp32) torch reference; prints the maxima."""
    worst = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    fails = []
    for i, (a, b) in enumerate(zip(pf, pr)):
        bb = b.detach().double().cpu()
        gap = ((a.detach().double().cpu() - bb).abs() / bb.abs().clamp(min=1.0)).max().item()
        worst["p"] = max(worst["p"], gap)
        if not gap <= 2e-6:
            fails.append(("p", i, gap))
        sf, sr = fused.state[a], ref.state.get(b, {})
        assert float(sf["step"]) == (float(sr["step"]) if sr else 0.0), (tag, i, float(sf["step"]))
        for k in ("exp_avg", "exp_avg_sq"):
            want = sr[k].detach().double().cpu() if sr else torch.zeros_like(bb)
            diff, top = (sf[k].double().cpu() - want).abs().max().item(), want.abs().max().item()
            gap = diff / top if top > 0 else diff
            worst[k] = max(worst[k], gap)
            if not gap <= 2e-6:
                fails.append((k, i, gap))
    print("%s: max |dp| / max(1, |p|) %.2e, exp_avg %.2e, exp_avg_sq %.2e (of the tensor's max; bound 2e-6 each)"
          % (tag, worst["p"], worst["exp_avg"], worst["exp_avg_sq"]))
    assert not fails, (tag, fails[:6])


@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1.0])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_matches_torch_float64_over_five_steps(decoupled, scale):
    """The gradient of a tensor's FIRST step carries the sign of the parameter.  Adam's first step is p -= lr g' / (|g'| + eps): where
    |g'| is of the order of eps = 1e-8 its slope is lr / eps = 1e5, and with coupled decay g' = coef g + wd p is a sum that can cancel
    that far while its rounding stays at the size of its terms (6e-10 here).  With free signs one such element turned up (scale 1, Adam,
    the 4095-element tensor, element 3563): torch's own fp32 CPU Adam is 1.24e-5 off float64 there, as is this kernel (1.24e-5) -- the
    input is ill-conditioned, not the arithmetic.  With equal signs nothing cancels, so every first-step g' is relatively accurate."""
    shapes = _shapes()
    pf, fused, pr, ref = _pair(shapes, decoupled, max_grad_norm=1.0)
    late = 6                                        # this tensor's .grad is None for the first two steps
    sign = [torch.where(t >= 0, 1.0, -1.0) for t in _randn(shapes, 0)]           # (of the initial values `_pair` draws)
    for step in range(5):
        grads = _randn(shapes, 100 + step, scale)
        for i in (range(len(shapes)) if step == 0 else (late,) if step == 2 else ()):
            grads[i] = grads[i].abs() * sign[i]
        _set_grads(pf, pr, grads, skip=(late,) if step < 2 else ())
        fused.step()
        total = _ref_step(pr, ref, 1.0)
        got = float(fused.grad_norm)
        print("step %d scale %g: grad_norm %.9g vs %.9g (rel %.2e), clip %s" % (step, scale, got, total, abs(got - total) / total,
                                                                                 "active" if total > 1.0 else "inactive"))
        assert abs(got - total) <= 1e-6 * total
        assert (total > 1.0) == (scale == 1.0)
    _compare(pf, fused, pr, ref, "%s scale %g" % ("AdamW" if decoupled else "Adam", scale))
    assert float(fused.state[pf[late]]["step"]) == 3.0 and float(fused.state[pf[0]]["step"]) == 5.0
    assert int(fused.skipped) == 0
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(pf, _randn(shapes, 104, scale)))      # .grad is read, never rescaled


def _views(flat, sizes, offsets):
    """Views of `flat` whose first elements sit at element offsets = offsets[k] (mod 4) of the 16-byte grid."""
    out, pos = [], 0
    for n, o in zip(sizes, offsets):
        pos = (pos + 3) // 4 * 4 + o
        out.append(flat[pos:pos + n])
        pos += n
    return out


def test_misaligned_operands_equal_the_aligned_step_bit_for_bit():
    from fabind_amd.optim import CHUNK as C, FusedAdam
    sizes = [5, 257, C + 1, 2 * C + 3, 1, 1023, C - 1, 2 * C + 3, 64 * 65]
    g_off = [1, 2, 3, 1, 2, 3, 1, 0, 2]          # gradients: views at element offsets 1, 2, 3 of one flat buffer (and one aligned)
    p_off = [1, 1, 1, 1, 1, 1, 1, 1, 0]          # parameters: views at offset 1 of another (and one aligned under a misaligned gradient)
    init = _randn([(n,) for n in sizes], 3)
    pbuf = torch.zeros(sum(sizes) + 8 * len(sizes), device=DEV)
    gbuf = torch.zeros_like(pbuf)
    pv, gv = _views(pbuf, sizes, p_off), _views(gbuf, sizes, g_off)
    assert [v.data_ptr() % 16 // 4 for v in pv] == p_off and [v.data_ptr() % 16 // 4 for v in gv] == g_off
    pa = [torch.nn.Parameter(v) for v in pv]                       # (a Parameter of a view keeps the view's storage offset)
    assert [p.data_ptr() for p in pa] == [v.data_ptr() for v in pv]
    pb = [torch.nn.Parameter(torch.empty(n, device=DEV)) for n in sizes]
    with torch.no_grad():
        for a, b, t in zip(pa, pb, init):
            a.copy_(t.to(DEV))
            b.copy_(t.to(DEV))
    oa = FusedAdam(_grouped(pa), decoupled_weight_decay=True, max_grad_norm=1.0)
    ob = FusedAdam(_grouped(pb), decoupled_weight_decay=True, max_grad_norm=1.0)
    for step in range(2):
        for a, b, v, g in zip(pa, pb, gv, _randn([(n,) for n in sizes], 40 + step)):
            v.copy_(g.to(DEV))
            a.grad = v
            b.grad = g.to(DEV)
            assert b.grad.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        oa.step()
        ob.step()
    assert torch.equal(oa.grad_norm, ob.grad_norm) and float(oa.grad_norm) > 1.0
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k


def test_bit_reproducible():
    from fabind_amd.optim import FusedAdam
    shapes = _shapes()
    runs = []
    for _ in range(2):
        ps = [torch.nn.Parameter(t.to(DEV)) for t in _randn(shapes, 7)]
        opt = FusedAdam(_grouped(ps), max_grad_norm=1.0)
        for step in range(3):
            for p, g in zip(ps, _randn(shapes, 70 + step)):
                p.grad = g.to(DEV)
            opt.step()
        runs.append((ps, opt))
    (pa, oa), (pb, ob) = runs
    assert torch.equal(oa.grad_norm, ob.grad_norm)
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k


def _snapshot(ps, opt):
    return [t.clone() for p in ps for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"])]


def test_non_finite_gradient_skips_the_step():
    shapes = _shapes()
    pf, fused, pr, ref = _pair(shapes, True, max_grad_norm=1.0)
    before = _snapshot(pf, fused)
    for n_skipped, bad in ((1, float("inf")), (2, float("nan"))):
        grads = _randn(shapes, 200 + n_skipped)
        grads[11].view(-1)[4099] = bad                       # one element of the three-chunk tensor (plain data: nothing faults)
        _set_grads(pf, pr, grads)
        fused.step()
        assert int(fused.skipped) == n_skipped
        assert not bool(torch.isfinite(fused.grad_norm))
        assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(pf, fused)))          # p, m, v, step: bit-unchanged
    grads = _randn(shapes, 210)
    _set_grads(pf, pr, grads)
    fused.step()
    total = _ref_step(pr, ref, 1.0)                           # torch's FIRST step (t = 1): the skipped steps left no trace
    assert abs(float(fused.grad_norm) - total) <= 1e-6 * total and int(fused.skipped) == 2
    _compare(pf, fused, pr, ref, "first finite step after two skipped")
    assert float(fused.state[pf[0]]["step"]) == 1.0
    before = _snapshot(pf, fused)                             # and once more with non-zero moments
    grads[0][0] = float("nan")
    _set_grads(pf, pr, grads)
    fused.step()
    assert int(fused.skipped) == 3
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(pf, fused)))
    # skip_nonfinite=False: the update is applied, nothing is counted
    pf, fused, pr, ref = _pair(shapes, True, max_grad_norm=1.0, skip_nonfinite=False)
    _set_grads(pf, pr, grads)
    fused.step()
    assert int(fused.skipped) == 0 and float(fused.state[pf[0]]["step"]) == 1.0


def test_checkpoints_interchange_with_torch_adamw():
    from fabind_amd.optim import FusedAdam
    shapes = _shapes()
    init = _randn(shapes, 9)
    for direction in ("torch -> fused", "fused -> torch"):
        pt = [torch.nn.Parameter(t.to(DEV)) for t in init]
        pf = [torch.nn.Parameter(t.to(DEV)) for t in init]
        topt = torch.optim.AdamW(_grouped(pt))
        fopt = FusedAdam(_grouped(pf), decoupled_weight_decay=True)
        src_p, src, dst_p, dst = (pt, topt, pf, fopt) if direction.startswith("torch") else (pf, fopt, pt, topt)
        for step in range(2):
            for p, g in zip(src_p, _randn(shapes, 300 + step, 1e-2)):
                p.grad = g.to(DEV)
            src.step()
        with torch.no_grad():
            for a, b in zip(dst_p, src_p):
                a.copy_(b)
        dst.load_state_dict(copy.deepcopy(src.state_dict()))          # (what a checkpoint file does: independent tensors)
        assert set(fopt._params) == set(pf)
        for i, p in enumerate(fopt._params):                           # the fused state is (still) a set of views of the flat buffers (group order)
            st = fopt.state[p]
            assert st["exp_avg"].data_ptr() == fopt._exp_avg.data_ptr() + 4 * int(fopt._offs[i])
            assert st["exp_avg_sq"].data_ptr() == fopt._exp_avg_sq.data_ptr() + 4 * int(fopt._offs[i])
            assert st["step"].data_ptr() == fopt._steps.data_ptr() + 4 * i and float(st["step"]) == 2.0
        for a, b, g in zip(pt, pf, _randn(shapes, 302, 1e-2)):
            a.grad, b.grad = g.to(DEV), g.to(DEV)
        topt.step()
        fopt.step()
        _compare(pf, fopt, pt, topt, "step 3 after load, " + direction)
        assert float(fopt.state[pf[0]]["step"]) == 3.0


def test_updated_weights_reach_the_cached_parameter_pack():
    """engine.cached_pack keys the no-grad pack on (data_ptr, _version): the raw-pointer update must bump the versions."""
    from fabind_amd import engine, synthetic
    from fabind_amd.models.att_model import EfficientMCAttModel
    from fabind_amd.optim import FusedAdam
    from test_gpu_stack import _args, _run
    engine.set_precision("fp32")

    def model():
        return EfficientMCAttModel(_args(32, 1, 1), 32, 32, 1, n_layers=1, n_iter=1, normalize_coord=lambda x: x / 5.0,
                                   unnormalize_coord=lambda x: x * 5.0)
    torch.manual_seed(0)
    m = model().to(DEV).eval()
    inp = synthetic.make_stack_batch([(20, 5)], 32, seed=0)
    X0, H0 = _run(m, inp, DEV)
    params = list(m.parameters())
    opt = FusedAdam(params, lr=1e-2)
    versions = [p._version for p in params]
    for p, g in zip(params, _randn([tuple(p.shape) for p in params], 5)):
        p.grad = g.to(DEV)
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    X1, H1 = _run(m, inp, DEV)
    fresh = model()
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    X2, H2 = _run(fresh.to(DEV).eval(), inp, DEV)
    assert torch.equal(X1, X2) and torch.equal(H1, H2)
    assert not torch.equal(H1, H0)                                    # the step did move the output


def _stack_step(fused):
    """One training step of the tiny v1 stack (the setup of tests/test_gpu_training.py at hidden 64, two small complexes, fp32)."""
    from fabind_amd import engine, parallel, synthetic
    from fabind_amd.models.att_model import EfficientMCAttModel
    from fabind_amd.optim import FusedAdam
    from test_gpu_stack import _args
    H, L = 64, 2
    engine.set_precision("fp32")
    torch.manual_seed(0)
    m = EfficientMCAttModel(_args(H, L, 1), H, H, 1, n_layers=L, n_iter=1, dropout=0.0, normalize_coord=lambda x: x / 5.0,
                            unnormalize_coord=lambda x: x * 5.0)
    m = synthetic.condition_for_large_graphs(m).to(DEV).train()
    inp = synthetic.make_stack_batch([(50, 9), (64, 12)], H, seed=11)
    t = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    lig = t["mask"].bool()
    g = torch.Generator().manual_seed(5)
    target = (t["X"][lig] + 0.15 * torch.randn(t["X"][lig].shape, generator=g).to(DEV)).detach()
    params = list(m.parameters())
    opt = FusedAdam(params, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True) if fused else \
        torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01)
    X, Hh = m(t["X"].clone(), t["H"], t["batch_id"], t["segment_id"], t["mask"], t["is_global"], t["compound_edge_index"],
              t["LAS_edge_index"], t["coord_LAS"])
    loss = ((X[lig] - target) * 5.0).pow(2).sum(-1).mean() + 1e-4 * Hh.pow(2).mean()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    have = [p for p in params if p.grad is not None]
    if fused:                          # (max norm 0.1: the gradient norm of this step is 0.37, so the clip is active)
        opt.step(max_grad_norm=0.1)
        total = opt.grad_norm
    else:
        total = parallel.clip_grad_norm_(have, 0.1)
        opt.step()
    return [p.detach().clone() for p in params], float(total), len(have)


def test_stack_training_step_equals_todays_tail():
    want, n_want, have = _stack_step(False)
    got, n_got, _ = _stack_step(True)
    gap = max(((a - b).abs() / b.abs().clamp(min=1.0)).max().item() for a, b in zip(got, want))
    print("tiny stack, one step: %d of %d tensors have a gradient, norm %.6g (fused) vs %.6g; max |dp| / max(1, |p|) %.2e (bound 2e-6)"
          % (have, len(want), n_got, n_want, gap))
    assert abs(n_got - n_want) <= 1e-6 * n_want and n_want > 0.1            # the clip was active
    assert gap <= 2e-6


class _Tiny(torch.nn.Module):
    """Stand-in with IaBNet's call signature and nine outputs; `unused` never receives a gradient (train_step zero-fills it)."""
    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(8, 33), torch.nn.Linear(33, 9)
        self.unused = torch.nn.Parameter(torch.ones(5))

    def forward(self, data, stage=1, train=True):
        y = self.b(torch.tanh(self.a(data)))
        return tuple(y[:, i] for i in range(9))


def test_train_step_hands_the_clip_to_the_fused_step(monkeypatch):
    from fabind_amd import parallel
    from fabind_amd.optim import FusedAdam
    calls = {"clip": 0, "step": []}
    real_clip, real_step = parallel.clip_grad_norm_, FusedAdam.step

    def spy_clip(*a, **k):
        calls["clip"] += 1
        return real_clip(*a, **k)

    def spy_step(self, *a, **k):
        calls["step"].append(k)
        return real_step(self, *a, **k)
    monkeypatch.setattr(parallel, "clip_grad_norm_", spy_clip)
    monkeypatch.setattr(FusedAdam, "step", spy_step)
    data = torch.randn(16, 8, generator=torch.Generator().manual_seed(1)).to(DEV)

    def loss_fn(out, data):
        loss = 100.0 * sum(o.pow(2).mean() for o in out)
        return loss, {"sq": loss}
    res = []
    for fused in (False, True):
        torch.manual_seed(0)
        m = _Tiny().to(DEV)
        params = list(m.parameters())
        opt = FusedAdam(params, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True) if fused else \
            torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01)
        for _ in range(2):
            assert parallel.train_step(m, data, opt, loss_fn, world=1, clip=1.0) is not None
        res.append([p.detach().clone() for p in params])
        if fused:
            gnorm = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in params]))
            assert float(gnorm) > 1.0 and abs(float(gnorm) - float(opt.grad_norm)) <= 1e-6 * float(gnorm)     # .grad keeps the unclipped gradient
            assert calls["clip"] == 2 and calls["step"] == [{"max_grad_norm": 1.0}] * 2      # the two clip calls are the torch path's
            parallel.train_step(m, data, opt, loss_fn, world=1, clip=0)
            assert calls["step"][-1] == {"max_grad_norm": None}
        else:
            assert calls["clip"] == 2 and calls["step"] == []
    gap = max(((a - b).abs() / b.abs().clamp(min=1.0)).max().item() for a, b in zip(res[1], res[0]))
    print("train_step, two steps: FusedAdam vs clip_grad_norm_ + AdamW: max |dp| / max(1, |p|) %.2e (bound 2e-6)" % gap)
    assert gap <= 2e-6
    assert not torch.equal(res[0][-1], torch.ones(5, device=DEV))            # the never-used tensor was decayed in both


def test_linear_lr_scheduler_drives_the_step():
    from torch.optim.lr_scheduler import LinearLR
    shapes = _shapes()[:9]
    pf, fused, pr, ref = _pair(shapes, False)
    sf, sr = LinearLR(fused, start_factor=0.1, total_iters=4), LinearLR(ref, start_factor=0.1, total_iters=4)
    p0 = pf[8].detach().clone()
    moved = []
    for step in range(2):
        _set_grads(pf, pr, _randn(shapes, 400 + step))
        fused.step()
        _ref_step(pr, ref, None)
        sf.step()
        sr.step()
        moved.append((pf[8].detach() - p0).abs().max().item())
        p0 = pf[8].detach().clone()
        assert [g["lr"] for g in fused.param_groups] == [g["lr"] for g in ref.param_groups]
    _compare(pf, fused, pr, ref, "two steps under LinearLR")
    assert fused.param_groups[0]["lr"] == pytest.approx(1e-3 * 0.55)
    assert moved[0] == pytest.approx(1e-4, rel=1e-2)             # Adam's first step moves an element by lr = 0.1 * 1e-3 (to the fp32 spacing of p)


def test_unsupported_arguments_raise():
    from fabind_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(8, 4, device=DEV))
    with pytest.raises(NotImplementedError):
        FusedAdam([p], amsgrad=True)
    with pytest.raises(NotImplementedError):
        FusedAdam([p], maximize=True)
    opt = FusedAdam([p])
    p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError):
        opt.step(lambda: 0.0)
    with pytest.raises(TypeError, match="fp32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.bfloat16))])
    p.grad = torch.ones(4, 8, device=DEV).t()
    assert not p.grad.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    assert float(opt.state[p]["step"]) == 0.0 and not bool(p.detach().any())       # nothing ran
