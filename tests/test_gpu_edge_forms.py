"""GPU: every form of the fused intra-graph edge pipeline (csrc/fused_edge.hip, fused_edge_fwd2.hip, fused_edge_fwd3.hip,
fused_edge_bwd3.hip, fused_edge_bwd4.hip and the deterministic segment sum of csrc/fused_common.h) through kernels.gcl_edge_fused,
gcl_edge_fused_x3 and gcl_edge_fused_bwd against the float64 restatements of tests/edge_refs.py, on the topology table of that file:
every seam class of the 64-edge tiles, E = 1 to 27 tiles, tile counts on either side of the XCD-aware walk's threshold.

The metric is row-wise and relative to the companion sum over absolute terms (edge_refs: err_rows / err_elems): a node with three
edges is judged on the scale of its own three messages.  Bounds, nothing tuned to the kernels:
  bf16 pipeline outputs    err_hip <= max(8 err32, 2^-7); err32 = the float32 restatement against the float64 one, same rounding points
  split-bf16 forward       err_hip <= max(8 err_emul, 64 * 2^-23); err_emul = the three-product float64 emulation against exact float64
  saved tiles (bf16)       element-wise norm_refs.bf16_excess <= 0 against the unrounded float64 value with A = coord_refs.bound(err32) max|ref|
                           (err32: the float32 restatement of the unrounded value).  In the bf16 pipeline the value behind a saved element
                           depends on operands that were themselves rounded to bf16 (S1 for M and silu'(pre2), M for pre3), and a rounding
                           of those that falls the other way in the kernel's fast-exponential fp32 than in float64 moves the edge's whole
                           row by up to an operand ulp times a weight: such an edge may miss the element rule.  The kernel's fp32 value of an
                           operand is within 2^-20 of it, a bf16 rounding boundary is hit with probability <= 2^-20 / 2^-8 = 2^-12 per element,
                           so at most max(1, E H 2^-12) edges may do so, and those stay within A + 4 * 2^-8 max|operand| max|weight|.
                           The split-bf16 saving forward has no rounded operand in front of its saved tiles: no edge may miss the rule.
Every case runs twice and repeats bit for bit; rows without edges are exactly zero; every figure is printed before it is asserted
(`pytest -s`), the worst per form by the last test of the file.

The backward form is always selected explicitly (fabind_gcl_edge_fused_bwd_set_variant, restored to 5 in a finally block): the 'unset'
default of fabind_gcl_edge_fused_bwd_variant_for (variant 0 up to H = 128) exists only until the first set_variant call of the process --
the set flag is process-wide and sticky, and other tests of the suite set it -- so nothing here relies on it."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import coord_refs as CR
import edge_refs as ER
import norm_refs as NR

pytestmark = pytest.mark.gpu
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

CASES = [(n, H, p) for n in ER.NAMES for H in (64, 256) for p in (0.0, 0.25)] + \
        [(n, H, p) for n in ER.WIDE_H for H in (128, 512) for p in (0.0, 0.25)]
IDS = ["%s-H%d-p%g" % c for c in CASES]
WORST = {}


def _dev():
    return torch.device("cuda:0")


def _note(form, name, H, p, tensor, err, ref_err, bound):
    print("edge-forms | %-22s | %-12s | H=%3d p=%.2f | %-5s | err_hip %.2e | ref err %.2e | bound %.2e" % (form, name, H, p, tensor, err, ref_err, bound))
    w = WORST.setdefault(form, {})
    if tensor not in w or err / bound > w[tensor][0] / w[tensor][2]:
        w[tensor] = (err, ref_err, bound, "%s H=%d p=%g" % (name, H, p))
    return err <= bound


def _poison(*shape_dtype):
    """torch.empty of the wrappers takes its block from the caching allocator: leave NaN in blocks of the sizes they are about to ask
    for (the wrappers allocate their outputs themselves -- there is no out= to prefill)."""
    dev = _dev()
    for shape, dt in shape_dtype:
        t = torch.full(shape, float("nan"), dtype=dt, device=dev)
        del t


@functools.lru_cache(maxsize=2)
def _case(name, H, p):
    """Device operands of a case and its forward restatements."""
    from fabind_amd import kernels as K
    o = ER.operands(name, H, p)
    tp, dev = o.tp, _dev()
    d = SimpleNamespace(o=o, tp=tp, name=name, H=H, p=p)
    i32 = lambda t: t.to(torch.int32).to(dev)
    d.row, d.col, d.rowptr, d.colptr, d.perm = i32(tp.row), i32(tp.col), i32(tp.rowptr), i32(tp.colptr), i32(tp.perm)
    d.AB32, d.AB16 = o.AB.to(dev), o.AB.bfloat16().to(dev)
    d.rh, d.w_r, d.b2, d.bc, d.w3, d.ds, d.dagg = [t.to(dev) for t in (o.rh, o.w_r, o.b2, o.bc, o.w3, o.ds, o.dagg)]
    d.W2_32, d.Wc_32 = o.W2.to(dev), o.Wc.to(dev)
    d.W2_16, d.Wc_16 = o.W2.bfloat16().to(dev), o.Wc.bfloat16().to(dev)
    d.W2p, d.Wcp = K.pack_frag(d.W2_16), K.pack_frag(d.Wc_16)
    d.b64, d.b32 = ER.forward(o, F64, "bf16"), ER.forward(o, F32, "bf16")
    d.x64, d.x32, d.xem = ER.forward(o, F64, "exact"), ER.forward(o, F32, "exact"), ER.forward(o, F64, "split")
    d.empty = (tp.deg == 0).to(dev)
    return d


def _fwd16(d, **kw):
    from fabind_amd import kernels as K
    _poison(((d.tp.N, d.H), F32), ((d.tp.N, d.H), BF))
    return K.gcl_edge_fused(d.AB16, d.H, d.row, d.col, d.rh, d.w_r, d.W2p, d.b2, d.Wcp, d.bc, d.w3, d.tp.N, d.p, d.o.seed, rowptr=d.rowptr, **kw)


def _fwd32(d, **kw):
    from fabind_amd import kernels as K
    _poison(((d.tp.N, d.H), F32))
    return K.gcl_edge_fused_x3(d.AB32, d.H, d.row, d.col, d.rh, d.w_r, d.W2_32, d.b2, d.Wc_32, d.bc, d.w3, d.tp.N, p_drop=d.p, seed=d.o.seed,
                               rowptr=d.rowptr, **kw)


def _bwd(d, saved=None, x3=False, dab_bf16=False):
    """-> the result tuple of kernels.gcl_edge_fused_bwd.  x3: the operands of the split-bf16 step (a bf16 copy of the fp32 AB rows, fp32
    weights, as test_fused_edge_split_bf16_saving_forward_feeds_the_two_contraction_backward passes them)."""
    from fabind_amd import kernels as K
    _poison(((d.tp.N, 2 * d.H), BF if dab_bf16 else F32))
    W2, Wc = (d.W2_32, d.Wc_32) if x3 else (d.W2_16, d.Wc_16)
    return K.gcl_edge_fused_bwd(d.AB16, d.H, d.row, d.col, d.rh, d.w_r, W2, d.b2, Wc, d.bc, d.w3, d.ds, d.dagg, d.colptr, d.perm, d.p, d.o.seed,
                                dab_bf16=dab_bf16, w_dtype=F32, rowptr=d.rowptr, saved=saved)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check_saved(form, d, saved, f64, f32, flips):
    """saved = (M [E, H] bf16 row-major, d2f, z3f in fragment order) against the unrounded float64 values (module docstring)."""
    tp, H, o = d.tp, d.H, d.o
    E = tp.E
    assert saved[0].dtype == BF and tuple(saved[0].shape) == (E, H)
    nt = (E + ER.BM - 1) // ER.BM
    assert all(t.dtype == BF and tuple(t.shape) == (nt * ER.BM, H) for t in saved[1:])
    got = (saved[0].cpu(), ER.decode_frag(saved[1].cpu(), H)[:E], ER.decode_frag(saved[2].cpu(), H)[:E])
    wmax2, wmaxc = float(o.W2.abs().max()), float(o.Wc.abs().max())
    slack = (float(f64.S1.abs().max()) * wmax2, float(f64.S1.abs().max()) * wmax2, float(f64.M.abs().max()) * wmaxc)
    allowed = max(1, math.ceil(E * H * 2.0 ** -12)) if flips else 0
    fails = []
    for nm, g, r64, r32, sl in zip(("M", "d2f", "z3f"), got, (f64.Mf, f64.d2, f64.pre3), (f32.Mf, f32.d2, f32.pre3), slack):
        assert bool(torch.isfinite(g.float()).all()), (form, nm)
        A = CR.bound(CR.rel_err(r32, r64)) * max(float(r64.abs().max()), 1e-6)
        ex = (g.double() - r64).abs() - (NR.bf16_half_ulp(r64.abs() + A) + A)
        bad = int((ex.amax(1) > 0).sum())
        A2 = A + 4 * 2.0 ** -8 * sl
        ex2 = NR.bf16_excess(g, r64, A2) if flips else NR.bf16_excess(g, r64, A)
        print("edge-forms | %-22s | %-12s | H=%3d p=%.2f | %-5s | bf16 excess over half-ulp + A %.2e (A %.2e) | edges over it %d (allowed %d) | "
              "excess with the flipped-operand term %.2e" % (form, d.name, H, d.p, nm, float(ex.max()), A, bad, allowed, ex2))
        if bad > allowed or ex2 > 0.0:
            fails.append((nm, float(ex.max()), bad, allowed, ex2))
    assert not fails, (form, d.name, H, d.p, fails)


@pytest.mark.parametrize("name,H,p", CASES, ids=IDS)
def test_forward_forms(name, H, p):
    """The bf16 forward plain, with the bf16 copy of agg, and saving; the split-bf16 forward plain and saving."""
    d = _case(name, H, p)
    tp = d.tp
    rrow, _ = ER.has_rows(tp)
    fails = []
    # ---- bf16 pipeline
    plain, plain2 = _fwd16(d), _fwd16(d)
    w16, w16b = _fwd16(d, want16=True), _fwd16(d, want16=True)
    sv, sv2 = _fwd16(d, want16=True, save=True), _fwd16(d, want16=True, save=True)
    assert _same(plain, plain2) and _same(w16, w16b) and _same(sv[:3], sv2[:3]) and _same(sv[3], sv2[3])
    assert _same(plain, w16[:2]) and _same(w16, sv[:3])                    # neither the bf16 copy nor the saving stores change a result
    agg, s, agg16 = w16
    assert tuple(agg.shape) == (tp.N, H) and tuple(s.shape) == (tp.E, 1) and bool(torch.isfinite(agg).all()) and bool(torch.isfinite(s).all())
    assert torch.equal(agg16, agg.bfloat16())
    assert float(agg[d.empty].abs().sum()) == 0.0 and float(agg16[d.empty].float().abs().sum()) == 0.0
    e32a, e32s = ER.err_rows(d.b32.agg, d.b64.agg, d.b64.aggA, rrow), ER.err_elems(d.b32.s, d.b64.s, d.b64.sA)
    ea, es = ER.err_rows(agg.cpu(), d.b64.agg, d.b64.aggA, rrow), ER.err_elems(s[:, 0].cpu(), d.b64.s, d.b64.sA)
    if not _note("bf16 forward", name, H, p, "agg", ea, e32a, ER.bound_bf16(e32a)):
        fails.append(("bf16 agg", ea, e32a))
    if not _note("bf16 forward", name, H, p, "s", es, e32s, ER.bound_bf16(e32s)):
        fails.append(("bf16 s", es, e32s))
    _check_saved("bf16 saving forward", d, sv[3], d.b64, d.b32, flips=True)
    # ---- split-bf16 forward
    xp, xp2 = _fwd32(d), _fwd32(d)
    xs, xs2 = _fwd32(d, save=True), _fwd32(d, save=True)
    assert _same(xp, xp2) and _same(xs[:2], xs2[:2]) and _same(xs[2], xs2[2]) and _same(xp, xs[:2])
    agg, s = xp
    assert bool(torch.isfinite(agg).all()) and bool(torch.isfinite(s).all())
    assert float(agg[d.empty].abs().sum()) == 0.0
    eema, eems = ER.err_rows(d.xem.agg, d.x64.agg, d.x64.aggA, rrow), ER.err_elems(d.xem.s, d.x64.s, d.x64.sA)
    ea, es = ER.err_rows(agg.cpu(), d.x64.agg, d.x64.aggA, rrow), ER.err_elems(s[:, 0].cpu(), d.x64.s, d.x64.sA)
    if not _note("split-bf16 forward", name, H, p, "agg", ea, eema, ER.bound_x3(eema)):
        fails.append(("x3 agg", ea, eema))
    if not _note("split-bf16 forward", name, H, p, "s", es, eems, ER.bound_x3(eems)):
        fails.append(("x3 s", es, eems))
    _check_saved("split-bf16 saving fwd", d, xs[2], d.x64, d.x32, flips=False)
    assert not fails, fails


def _split(out, H):
    """The result tuple of gcl_edge_fused_bwd -> {name: cpu tensor} with the two halves of dAB apart."""
    dAB, drh, dw_r, dW2, db2, dWc, dbc, dw3 = [t.float().cpu() for t in out]
    return {"dABr": dAB[:, :H], "dABc": dAB[:, H:], "drh": drh, "dw_r": dw_r, "dW2": dW2, "db2": db2, "dWc": dWc, "dbc": dbc, "dw3": dw3}


def _judge(form, d, out, variant, x3):
    """Every gradient of one backward result against the restatement of its form; -> the failures."""
    o, tp = d.o, d.tp
    f64, f32 = (d.x64, d.x32) if x3 else (d.b64, d.b32)
    g64 = ER.backward(o, f64, F64, variant)
    e32 = ER.grad_errors(ER.backward(o, f32, F32, variant), g64, tp)
    assert all(bool(torch.isfinite(t.float()).all()) for t in out), form
    assert tuple(out[0].shape) == (tp.N, 2 * d.H) and tuple(out[1].shape) == (tp.E,)
    assert float(out[0][:, :d.H][d.empty].float().abs().sum()) == 0.0                      # receiving half: rows without edges
    assert float(out[0][tp.silent, d.H:].float().abs().sum()) == 0.0                       # sending half: the node nobody reads
    e = ER.grad_errors(_split(out, d.H), g64, tp)
    return [(form, k, e[k], e32[k]) for k in ER.GRADS if not _note(form, d.name, d.H, d.p, k, e[k], e32[k], ER.bound_bf16(e32[k]))]


def _recompute(d, variant, dab_bf16=False):
    """The recompute backward in form `variant`, selected explicitly (module docstring); the library is left at 5."""
    from fabind_amd import _lib
    lib = _lib.load()
    lib.fabind_gcl_edge_fused_bwd_set_variant(variant)
    try:
        assert lib.fabind_gcl_edge_fused_bwd_variant_for(d.H) == variant
        return _bwd(d, dab_bf16=dab_bf16)
    finally:
        lib.fabind_gcl_edge_fused_bwd_set_variant(5)


@pytest.mark.parametrize("name,H,p", CASES, ids=IDS)
def test_backward_forms(name, H, p):
    """Variants 0 and 5 (recompute), variant 6 over what the bf16 and the split-bf16 saving forwards left; the bf16 form of dAB."""
    d = _case(name, H, p)
    fails = []
    for variant in (0, 5):
        out, out2 = _recompute(d, variant), _recompute(d, variant)
        assert _same(out, out2), variant
        fails += _judge("backward variant %d" % variant, d, out, variant, False)
        if variant == 5:
            o16 = _recompute(d, variant, dab_bf16=True)
            assert o16[0].dtype == BF and torch.equal(o16[0], out[0].bfloat16()) and _same(o16[1:], out[1:])
    for x3 in (False, True):
        saved = (_fwd32(d, save=True) if x3 else _fwd16(d, save=True))[-1]
        out, out2 = _bwd(d, saved=saved, x3=x3), _bwd(d, saved=saved, x3=x3)
        assert _same(out, out2), x3
        fails += _judge("backward variant 6 (%s)" % ("split-bf16 fwd" if x3 else "bf16 fwd"), d, out, 6, x3)
        o16 = _bwd(d, saved=saved, x3=x3, dab_bf16=True)
        assert o16[0].dtype == BF and torch.equal(o16[0], out[0].bfloat16()) and _same(o16[1:], out[1:])
    assert not fails, fails


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("form", ["v0", "v5", "v6", "v6x3"])
def test_backward_group_counts(form, H, monkeypatch):
    """The persistent kernels walked: 27 tiles by 1, 3, 8 work-groups (27, 9, 3-4 tiles each; 8 takes the XCD-aware walk) and by the
    derived count -- the double-buffered tables, the sPart accumulation over a group's tiles, the reuse of the LDS tile.  Each run meets
    the bound; what does not depend on the grouping (d rhohat, the receiving half of dAB) is bit-identical across the counts."""
    from fabind_amd import kernels as K
    d = _case(ER.GROUPS_TOPOLOGY, H, 0.25)
    x3 = form == "v6x3"
    variant = {"v0": 0, "v5": 5}.get(form, 6)
    saved = None
    if variant == 6:
        saved = (_fwd32(d, save=True) if x3 else _fwd16(d, save=True))[-1]
    fails, first = [], None
    for g in (0, 1, 3, 8):
        monkeypatch.setattr(K, "EDGE_BWD_GROUPS", g)
        run = (lambda: _bwd(d, saved=saved, x3=x3)) if variant == 6 else (lambda: _recompute(d, variant))
        out, out2 = run(), run()
        assert _same(out, out2), g
        fails += _judge("%s groups=%s" % (form, g or "derived"), d, out, variant, x3)
        if first is None:
            first = out
        assert torch.equal(out[1], first[1]) and torch.equal(out[0][:, :H], first[0][:, :H]), g
        assert torch.equal(out[0][:, H:], first[0][:, H:]) and torch.equal(out[3], first[3]) and torch.equal(out[5], first[5]), g
    assert not fails, fails


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("name", ["one_edge", "ragged37", "heavy_to_end"])
def test_padding_of_the_ragged_last_tile_reaches_no_gradient(name, x3, H):
    """The rows past E of the fragment-ordered saved tiles overwritten with two different finite values: the variant-6 backward returns
    the same bits."""
    d = _case(name, H, 0.25)
    E = d.tp.E
    saved = (_fwd32(d, save=True) if x3 else _fwd16(d, save=True))[-1]
    nt = (E + ER.BM - 1) // ER.BM
    assert nt * ER.BM > E
    pad = ER.frag_index(nt, H)[E:].reshape(-1).to(_dev())
    ref = _bwd(d, saved=saved, x3=x3)
    outs = []
    for v in (7.0, -1000.0):
        d2f, z3f = saved[1].clone(), saved[2].clone()
        d2f.view(-1)[pad] = v
        z3f.view(-1)[pad] = v
        outs.append(_bwd(d, saved=(saved[0], d2f, z3f), x3=x3))
    assert _same(outs[0], outs[1]) and _same(outs[0], ref)


def test_zz_worst_errors_per_form():
    """Prints the worst figure of every (form, tensor) the tests above recorded (nothing to assert beyond their own assertions)."""
    for form in sorted(WORST):
        for tensor, (err, ref_err, bound, where) in sorted(WORST[form].items()):
            print("edge-forms worst | %-26s | %-5s | err_hip %.2e | ref err %.2e | bound %.2e | at %s" % (form, tensor, err, ref_err, bound, where))
