"""GPU: the kernels that produce the model's outputs and its loss (csrc/heads.hip: pair_dist, block_hadamard, the six-term loss, the pocket
centre) and the pair products round them (csrc/attn.hip: fabind_pair_hadamard, fabind_pair_bmat; csrc/bwd.hip: pair_hadamard_bwd,
pair_hadamard_bwd_rows, rows_hadamard_bwd, pair_hadamard_bwd_grid), each through its public Python entry where one exists, against the
float64 restatements of tests/head_refs.py on the same operands.  The case tables live in head_refs.py; tests/test_head_refs_cpu.py
asserts that they reach every tile / chunk / lane class.

Products and forward Hadamards are single multiplications: they must equal the float64 product rounded once to float32 (and once more to
bf16 where the kernel stores bf16) BIT FOR BIT.  Everything else is written as fp32 and held to the project's rule, nothing tuned:
  err_hip = coord_refs.rel_err(got, ref64) <= coord_refs.bound(err32) = max(8 err32, 64 * 2^-23),
  err32 = the float32 restatement on the same operands, which sums sequentially in pair order.
No kernel here writes a summed tensor as bf16 and none needed an `extra` depth term (DESIGN.md lists the summation trees).
Every deterministic entry runs twice and must repeat bit for bit; outputs and scratch are prefilled with NaN (where the entry allocates
them itself, the allocator's next block of that size is), so an element no kernel wrote fails the finiteness check; memory a kernel
must leave alone holds a sentinel and is compared bit for bit.  Every (case, tensor, err_hip, err32, bound) is printed before it is
asserted (`pytest -s`)."""
import itertools
import types

import pytest
import torch

import coord_refs as CR
import head_refs as HR
import reduce_refs as RR
from head_refs import BF, F32

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = 7.0
WORST = {}


def _dev():
    return torch.device("cuda:0")


def _d(t):
    return t.to(_dev())


@pytest.fixture(autouse=True)
def _fp32_mode():
    from fabind_amd import config, engine
    old = config.get_precision()
    engine.set_precision("fp32")
    yield
    engine.set_precision(old)


@pytest.fixture(scope="module", autouse=True)
def _worst_record():
    yield
    for (op, nm), (e_hip, e32, b, case) in sorted(WORST.items()):
        print("head-forms worst | %-18s | %-10s | err_hip %.2e | err32 %.2e | err_hip/err32 %s | bound %.2e | %s"
              % (op, nm, e_hip, e32, "%.2f" % (e_hip / e32) if e32 > 0 else "-", b, case))


def _L():
    from fabind_amd import _lib
    return _lib


def _poison(*specs):
    """The entry under test allocates its own outputs and scratch: fill the blocks the caching allocator hands out next for these
    (shape, dtype) with NaN."""
    ts = [torch.full(shape, NAN, dtype=dtype, device=_dev()) for shape, dtype in specs if all(s > 0 for s in shape)]
    del ts


def _view(host, pad):
    """host [R, C] float32 as a device view of a [R, C + pad] buffer whose first `pad` columns hold NaN."""
    if pad == 0:
        return _d(host)
    R, C = host.shape
    buf = torch.full((R, C + pad), NAN, device=_dev())
    v = buf[:, pad:]
    v.copy_(_d(host))
    return v


def _exact(op, case, nm, a, a2, r64):
    """A product: the float64 product is exact, one rounding to float32 (and one to bf16) is what the kernel must store."""
    want = r64.float().to(a.dtype)
    assert tuple(a.shape) == tuple(want.shape), (op, case, nm, a.shape, want.shape)
    assert torch.equal(a, a2), (op, case, nm, "second run differs")
    a = a.detach().cpu()
    bad = int((a.view(torch.int16 if a.dtype == BF else torch.int32) != want.view(torch.int16 if a.dtype == BF else torch.int32)).sum())
    print("head-forms | %-18s | %-44s | %-8s %s | %d elements, %d differ from the once-rounded product"
          % (op, case, nm, "bf16" if a.dtype == BF else "fp32", a.numel(), bad))
    assert bad == 0, (op, case, nm, bad)


def _compare(op, case, items, extra=0.0):
    """items: (name, got, got of the second run (None: no repeat check), ref64, ref32); all written as fp32."""
    fails = []
    for nm, a, a2, r64, r32 in items:
        assert tuple(a.shape) == tuple(r64.shape), (op, case, nm, a.shape, r64.shape)
        assert a.dtype == F32, (op, case, nm, a.dtype)
        assert bool(torch.isfinite(a).all()), (op, case, nm, "an element was not written")
        if a2 is not None:
            assert torch.equal(a, a2), (op, case, nm, "second run differs")
        a = a.detach().cpu()
        e_hip, e32 = CR.rel_err(a, r64), CR.rel_err(r32, r64)
        b = CR.bound(e32, extra)
        print("head-forms | %-18s | %-44s | %-8s fp32 | err_hip %.2e | err32 %.2e | bound %.2e" % (op, case, nm, e_hip, e32, b))
        w = WORST.setdefault((op, nm), [0.0, 0.0, 0.0, ""])
        if e_hip >= w[0]:
            w[:] = [e_hip, e32, b, case]
        if e_hip > b:
            fails.append((nm, e_hip, e32, b))
    assert not fails, (op, case, fails)


def test_tile_constants_are_the_librarys():
    lib = _L().load()
    assert lib.fabind_pair_block_tile() == HR.TP and lib.fabind_pair_block_chunk() == HR.CH
    for c in HR.LOSS_CASES:
        n = (c["n_pair"], c["n_atoms"] * 3, c["B"] * c["L"])
        assert lib.fabind_loss_blocks(*n) == HR.loss_blocks(*n), c["name"]


# ------------------------------------------------------------------------------------------------
# pair_dist
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HR.PAIR_DIST_CASES, ids=[c["name"] for c in HR.PAIR_DIST_CASES])
def test_pair_dist_forms(case):
    from fabind_amd import ops
    xp, xc, dy, pi, ci = HR.pair_dist_operands(case)
    sc, lo, hi = HR.PAIR_DIST_SCALE, case["lo"], HR.PAIR_DIST_HI
    bl = ops.PairBlocks(case["kcnt"], case["ncnt"], _dev())
    assert bl.n_pairs == pi.numel()
    xpd, dyd = _d(xp), _d(dy)

    def run():
        b = _d(xc).requires_grad_()
        _poison(((bl.n_pairs,), F32))
        y = ops.pair_dist(xpd, b, bl, scale=sc, lo=lo, hi=hi)
        _poison(((bl.B, 8, bl.max_C, 3), F32), (tuple(xc.shape), F32))
        y.backward(dyd)
        return y.detach(), b.grad
    a, b = run(), run()
    r64 = (HR.pair_dist(xp.double(), xc.double(), pi, ci, sc, lo, hi), HR.pair_dist_grad(xp.double(), xc.double(), pi, ci, dy.double(), sc, lo, hi))
    r32 = (HR.pair_dist(xp, xc, pi, ci, sc, lo, hi), HR.pair_dist_grad(xp, xc, pi, ci, dy, sc, lo, hi))
    _compare("pair_dist", case["name"], [("y", a[0], b[0], r64[0], r32[0]), ("dxc", a[1], b[1], r64[1], r32[1])])
    # the clamp's own values are exact: 0 at the zero distance (lo 0), lo and hi where it is active, hi at scale * r == hi
    y = a[0].cpu()
    assert torch.equal(y[r64[0] == hi], torch.full_like(y[r64[0] == hi], hi)) and torch.equal(y[r64[0] == lo], torch.full_like(y[r64[0] == lo], lo))


# ------------------------------------------------------------------------------------------------
# block Hadamard: ops.rows_hadamard on PairBlocks, forward values and adjoint
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HR.BLOCK_CASES, ids=[c["name"] for c in HR.BLOCK_CASES])
def test_block_hadamard_forms(case):
    from fabind_amd import engine, ops
    engine.set_precision("bf16")                                         # (the block kernels serve the bf16 activation path)
    W, kcnt, ncnt = case["W"], case["kcnt"], case["ncnt"]
    t, dout, ia, ib = HR.block_operands(case)
    npk, n = sum(kcnt), t.shape[0]
    bl = ops.PairBlocks(kcnt, ncnt, _dev())
    td = _view(t, 8 if case["slice"] else 0)
    assert (td.stride(0) > W) == case["slice"] and td.data_ptr() % 16 == 0
    iad, ibd, doutd = _d(ia), _d(ib), _d(dout).to(BF)
    assert (ops._block_hadamard_fwd(td, bl, npk) is not None) == case["fwd_block"]

    def run():
        t1 = td.detach().requires_grad_()
        _poison(((bl.n_pairs, W), BF))
        hd = ops.rows_hadamard(t1, iad, ibd, a_sorted=True, blocks=bl, n_a=npk)
        _poison(((n, W), F32), ((bl.n_tiles, bl.nchunk_max, bl.chunk, W), F32))
        hd.backward(doutd)
        return hd.detach(), t1.grad
    a, b = run(), run()
    assert a[0].dtype == BF
    _exact("block_hadamard_fwd" if case["fwd_block"] else "pair_hadamard(fallback)", case["name"], "out", a[0], b[0],
           HR.hadamard_blocks(t.double(), ia, ib))
    _compare("block_hadamard_bwd", case["name"], [("dt", a[1], b[1], HR.hadamard_blocks_grad(t.double(), ia, ib, dout.double()),
                                                  HR.hadamard_blocks_grad(t, ia, ib, dout))])
    # a complex without atoms / without residues: its rows of d t are zeros
    p0, c0 = 0, npk
    g = a[1].cpu()
    for P, C in zip(kcnt, ncnt):
        if C == 0:
            assert bool((g[p0:p0 + P] == 0).all()), (case["name"], "d tp of a complex without atoms")
        if P == 0:
            assert bool((g[c0:c0 + C] == 0).all()), (case["name"], "d tc of a complex without residues")
        p0, c0 = p0 + P, c0 + C


@pytest.mark.parametrize("kcnt,ncnt,W", [([129, 7], [0, 3], 128), ([3, 1], [21, 0], 512), ([0, 0], [5, 3], 64), ([4, 128], [0, 0], 256)])
def test_block_adjoint_writes_the_rows_of_empty_complexes(kcnt, ncnt, W):
    """fabind_block_hadamard_bwd called raw on a NaN-prefilled d t: the pocket rows of a complex with C = 0 (no chunk loop runs for it)
    and the ligand rows of a batch whose complexes all have P = 0 (no tile exists) must come back as zeros, not unwritten."""
    from fabind_amd import ops
    L = _L()
    lib = L.load()
    case = dict(W=W, kcnt=kcnt, ncnt=ncnt)
    t, dout, ia, ib = HR.block_operands(case)
    npk, n = sum(kcnt), t.shape[0]
    bl = ops.PairBlocks(kcnt, ncnt, _dev())
    td, doutd = _d(t), _d(dout).to(BF)
    dt_ = torch.full((n, W), NAN, device=_dev())
    part = torch.full((max(bl.n_tiles, 1), max(bl.nchunk_max, 1), bl.chunk, W), NAN, device=_dev())
    L.check(lib.fabind_block_hadamard_bwd(bl.desc_ptr, bl.B, bl.n_tiles, L.ptr(doutd), W, L.ptr(td), W, L.ptr(td[npk:]), W, W, bl.row_b_ptr,
                                          bl.n_crows, bl.nchunk_max, L.ptr(part), L.ptr(dt_), W, L.ptr(dt_[npk:]), W, L.stream()),
            "fabind_block_hadamard_bwd")
    g = dt_.cpu()
    unwritten = torch.isnan(g).any(1).nonzero().flatten().tolist()
    print("head-forms | block_hadamard_bwd | raw, P %s C %s W %d | rows of d t left unwritten: %s" % (kcnt, ncnt, W, unwritten[:8] + (["..."] if len(unwritten) > 8 else [])))
    assert not unwritten, (kcnt, ncnt, "rows of d t unwritten", len(unwritten))
    _compare("block_hadamard_bwd", "raw P %s C %s W %d" % (kcnt, ncnt, W),
             [("dt", dt_, None, HR.hadamard_blocks_grad(t.double(), ia, ib, dout.double()), HR.hadamard_blocks_grad(t, ia, ib, dout))])


# ------------------------------------------------------------------------------------------------
# the CSR-walk adjoint: ops.rows_hadamard without blocks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", HR.ROWS_WS)
def test_rows_hadamard_csr_walk_forms(W):
    from fabind_amd import engine, ops
    assert ops.ROWS_HADAMARD_WALK
    g = torch.Generator().manual_seed(W + 5)
    for sorted_a, prec in itertools.product((True, False), ("fp32", "bf16")):
        engine.set_precision(prec)
        adt = ops.act_dtype()
        ia, ib = HR.rows_pairs(sorted_a)
        t = HR.signed_feat(g, HR.ROWS_N, W)
        dout = RR.bf_exact(torch.randn(ia.numel(), W, generator=g) + 0.5)
        td, iad, ibd, doutd = _d(t), _d(ia), _d(ib), _d(dout).to(adt)
        case = "W%d %s dout %s" % (W, "sorted" if sorted_a else "unsorted", prec)

        def run():
            t1 = td.clone().requires_grad_()
            _poison(((ia.numel(), W), adt))
            hd = ops.rows_hadamard(t1, iad, ibd, a_sorted=sorted_a)
            _poison(((HR.ROWS_N, W), F32))
            hd.backward(doutd)
            return hd.detach(), t1.grad
        a, b = run(), run()
        assert a[0].dtype == adt
        _exact("pair_hadamard", case, "out", a[0], b[0], HR.hadamard_blocks(t.double(), ia, ib))
        _compare("rows_hadamard_bwd", case, [("dt", a[1], b[1], HR.hadamard_blocks_grad(t.double(), ia, ib, dout.double()),
                                              HR.hadamard_blocks_grad(t, ia, ib, dout))])
        assert bool((a[1][0] == 0).all())                                 # the row without pairs


# ------------------------------------------------------------------------------------------------
# the two-block product: kernels.pair_hadamard, kernels.pair_bmat
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,H2", HR.PAIR_HAD_HS)
def test_pair_hadamard_forward_forms(H, H2):
    from fabind_amd import kernels as K
    g = torch.Generator().manual_seed(H * 3 + H2)
    n = 11
    T0, T1 = HR.signed_feat(g, n, 2 * H + 4), HR.signed_feat(g, n, 2 * H2 + 4)          # (leading dimensions above the widths)
    T0d, T1d = _d(T0), _d(T1)
    for n_red, odt in itertools.product(HR.pair_had_nreds(H, H2), (F32, BF)):
        rp_, rc_ = torch.randint(0, n, (n_red,), generator=g, dtype=torch.int32), torch.randint(0, n, (n_red,), generator=g, dtype=torch.int32)
        a1, b1 = (T1d[:, :H2], T1d[:, H2:2 * H2]) if H2 else (T0d[:, :0], T0d[:, :0])

        def run():
            _poison(((n_red, H + H2), odt))
            return K.pair_hadamard(T0d[:, :H], T0d[:, H:2 * H], a1, b1, _d(rp_), _d(rc_), odt)
        lp, pb = HR.pair_hadamard_lp(H, H2)
        _exact("pair_hadamard", "H%d H2 %d lp%d n_red %d (%d a block)" % (H, H2, lp, n_red, pb), "hd", run(), run(),
               HR.pair_hadamard(T0.double(), H, T1.double(), H2, rp_, rc_))


@pytest.mark.parametrize("case", HR.BMAT_CASES, ids=lambda c: "H%d NO%d n_c%d" % (c["H"], c["NO"], c["n_c"]))
def test_pair_bmat_forms(case):
    from fabind_amd import kernels as K
    H, NO, n_c = case["H"], case["NO"], case["n_c"]
    g = torch.Generator().manual_seed(H + NO)
    a0b0, wc = HR.signed_feat(g, 9, 2 * H), HR.signed_feat(g, NO, H)
    cn = torch.randint(0, 9, (n_c,), generator=g, dtype=torch.int32)
    a0b0d, wcd, cnd = _d(a0b0), _d(wc), _d(cn)
    for odt in (F32, BF):
        def run():
            _poison(((n_c * NO, H), odt))
            return K.pair_bmat(a0b0d[:, H:], wcd, cnd, odt)
        _exact("pair_bmat", "H%d NO%d n_c%d" % (H, NO, n_c), "bmat", run(), run(), HR.pair_bmat(a0b0[:, H:].double(), wc.double(), cn))


# ------------------------------------------------------------------------------------------------
# the inter-graph adjoint: ops.pair_hadamard with the graph; raw with prefilled d0 / d1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,H2", HR.INTER_HS)
def test_pair_hadamard_inter_graph_adjoint_forms(H, H2):
    from fabind_amd import engine, ops
    assert ops.PAIRHAD_ROWS
    L = _L()
    G = HR.inter_graph()
    n, E = G["n"], G["red_p"].numel()
    g = torch.Generator().manual_seed(H + H2 + 1)
    T0, T1 = HR.signed_feat(g, n, 2 * H), HR.signed_feat(g, n, 2 * H2)
    dhd = RR.bf_exact(torch.randn(E, H + H2, generator=g) + 0.5)
    T0d, T1d = _d(T0), _d(T1)
    rpd, rcd = _d(G["red_p"]), _d(G["red_c"])
    graph = types.SimpleNamespace(rp_int=_d(G["rp"]), col_int=_d(G["col"]), red_idx=_d(G["red_idx"]))
    r64 = HR.pair_hadamard_grad(T0.double(), H, T1.double(), H2, G["red_p"], G["red_c"], dhd.double())
    r32 = HR.pair_hadamard_grad(T0, H, T1, H2, G["red_p"], G["red_c"], dhd)
    for prec in ("fp32", "bf16"):
        engine.set_precision(prec)
        adt = ops.act_dtype()
        case = "H%d H2 %d dhd %s" % (H, H2, prec)

        def run():
            a = T0d.clone().requires_grad_()
            b = T1d.clone().requires_grad_() if H2 else a.detach()[:, :0]
            _poison(((E, H + H2), adt))
            hd = ops.pair_hadamard(a, H, b, H2, rpd, rcd, graph=graph)
            hd.backward(_d(dhd).to(adt))
            return hd.detach(), a.grad, (b.grad if H2 else torch.zeros(n, 0, device=_dev()))
        a, b = run(), run()
        _exact("pair_hadamard", case, "hd", a[0], b[0], HR.pair_hadamard(T0.double(), H, T1.double(), H2, G["red_p"], G["red_c"]))
        _compare("pair_hadamard_bwd_rows", case, [("d0", a[1], b[1], r64[0], r32[0]), ("d1", a[2], b[2], r64[1], r32[1])])
    # raw: the kernel ADDS into d0 / d1 -- prefilled with known values; rows without edges and the halves a row does not own stay bit for bit
    d0i, d1i = RR.feat(g, n, 2 * H), RR.feat(g, n, 2 * H2)
    q64 = HR.pair_hadamard_grad(T0.double(), H, T1.double(), H2, G["red_p"], G["red_c"], dhd.double(), d0i.double(), d1i.double())
    q32 = HR.pair_hadamard_grad(T0, H, T1, H2, G["red_p"], G["red_c"], dhd, d0i, d1i)
    dhdd = _d(dhd)

    def raw():
        d0, d1 = _d(d0i.clone()), _d(d1i.clone())
        L.check(L.load().fabind_pair_hadamard_bwd_rows(L.ptr(dhdd), L.dt_code(F32), dhdd.stride(0), L.ptr(T0d), 2 * H, H, L.ptr(T1d) if H2 else None,
                                                       2 * H2, H2, L.ptr(graph.rp_int), L.ptr(graph.col_int), L.ptr(graph.red_idx), L.ptr(rcd), n,
                                                       L.ptr(d0), 2 * H, L.ptr(d1) if H2 else None, 2 * H2, L.stream()), "fabind_pair_hadamard_bwd_rows")
        return d0, d1
    a, b = raw(), raw()
    _compare("pair_hadamard_bwd_rows", "H%d H2 %d raw, d0 / d1 prefilled" % (H, H2), [("d0", a[0], b[0], q64[0], q32[0]), ("d1", a[1], b[1], q64[1], q32[1])])
    lig = torch.arange(n) < G["n_lig"]
    for got, init, h in ((a[0].cpu(), d0i, H), (a[1].cpu(), d1i, H2)):
        assert torch.equal(got[lig, :h], init[lig, :h]) and torch.equal(got[~lig, h:], init[~lig, h:]), "the half a row does not own was written"
        deg0 = torch.tensor(G["lens"]) == 0
        assert torch.equal(got[deg0], init[deg0])


# ------------------------------------------------------------------------------------------------
# the grid adjoint: plus.engine.pair_had with the layout; raw with a sentinel in d T
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", HR.GRID_WS)
def test_pair_hadamard_grid_adjoint_forms(W):
    from fabind_amd.plus import engine as PE
    L = _L()
    cnt = HR.grid_counts(W)
    lay_h = HR.grid_layout(cnt)
    N, E = lay_h["N"], lay_h["n_pairs"]
    g = torch.Generator().manual_seed(W + 9)
    T = HR.signed_feat(g, N, 2 * W)
    Td = _d(T)
    pn, cn = lay_h["p_node"], lay_h["c_node"]
    pnd, cnd = _d(pn), _d(cn)
    lay = types.SimpleNamespace(n_pairs=E, B=lay_h["B"], N=N, node_off=_d(lay_h["node_off"]), c_cnt=_d(lay_h["c_cnt"]), desc_p=_d(lay_h["desc_p"]))
    node_b = _d(lay_h["node_b"])
    is_lig = torch.zeros(N, dtype=torch.bool)
    for b, (P, C) in enumerate(cnt):
        o = int(lay_h["node_off"][b])
        is_lig[o:o + C] = True
    owned = torch.zeros(N, 2 * W, dtype=torch.bool)
    owned[is_lig, W:] = True
    owned[~is_lig, :W] = True
    owned_d = _d(owned)
    for odt in (F32, BF):
        dhd = RR.bf_exact(torch.randn(E, W, generator=g) + 0.5)
        dhdd = _d(dhd).to(odt)
        case = "W%d G%d (P, C) %s dhd %s" % (W, HR.grid_groups(W), cnt, "bf16" if odt == BF else "fp32")

        def raw():
            dT = torch.full((N, 2 * W), SENT, device=_dev())
            dT[owned_d] = NAN
            L.check(L.load().fabind_pair_hadamard_bwd_grid(L.ptr(dhdd), L.dt_code(odt), W, L.ptr(Td), 2 * W, W, L.ptr(lay.node_off), L.ptr(lay.c_cnt),
                                                           L.ptr(node_b), L.ptr(lay.desc_p), N, L.ptr(dT), 2 * W, L.stream()), "fabind_pair_hadamard_bwd_grid")
            assert bool((dT[~owned_d] == SENT).all()), (case, "the other half of dT was written")
            return torch.where(owned_d, dT, torch.zeros_like(dT))
        a, b = raw(), raw()
        r64 = HR.pair_hadamard_grad(T.double(), W, T.double()[:, :0], 0, pn, cn, dhd.double())[0]
        r32 = HR.pair_hadamard_grad(T, W, T[:, :0], 0, pn, cn, dhd)[0]
        _compare("pair_hadamard_bwd_grid", case, [("dT", a, b, r64, r32)])

        def public():
            Tg = Td.clone().requires_grad_()
            _poison(((E, W), odt))
            hd = PE.pair_had(Tg, W, pnd, cnd, odt, lay)
            hd.backward(dhdd)
            return hd.detach(), Tg.grad
        p, q = public(), public()
        _exact("pair_hadamard", case, "hd", p[0], q[0], HR.pair_hadamard(T.double(), W, T.double()[:, :0], 0, pn, cn))
        assert torch.equal(p[1], a) and torch.equal(q[1], a), (case, "pair_had's adjoint is not the grid kernel's")


# ------------------------------------------------------------------------------------------------
# the atomics adjoint, raw: held to the bound only (its summation order is the arrival order)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,H2", [(64, 0), (32, 64)])
def test_pair_hadamard_atomics_adjoint_raw(H, H2):
    L = _L()
    G = HR.inter_graph()
    n, E = G["n"], G["red_p"].numel()
    g = torch.Generator().manual_seed(H + H2 + 2)
    T0, T1 = HR.signed_feat(g, n, 2 * H), HR.signed_feat(g, n, 2 * H2)
    dhd = torch.randn(E, H + H2, generator=g) + 0.5
    T0d, T1d, dhdd, rpd, rcd = _d(T0), _d(T1), _d(dhd), _d(G["red_p"]), _d(G["red_c"])
    d0, d1 = torch.zeros(n, 2 * H, device=_dev()), torch.zeros(n, max(2 * H2, 4), device=_dev())
    p1 = (lambda t, o: t.data_ptr() + 4 * o)
    L.check(L.load().fabind_pair_hadamard_bwd(L.ptr(dhdd), L.dt_code(F32), H + H2, p1(T0d, 0), p1(T0d, H), 2 * H, H,
                                              p1(T1d, 0) if H2 else None, p1(T1d, H2) if H2 else None, 2 * H2, H2, L.ptr(rpd), L.ptr(rcd), E,
                                              p1(d0, 0), p1(d0, H), 2 * H, p1(d1, 0), p1(d1, H2), d1.stride(0), L.stream()), "fabind_pair_hadamard_bwd")
    r64 = HR.pair_hadamard_grad(T0.double(), H, T1.double(), H2, G["red_p"], G["red_c"], dhd.double())
    r32 = HR.pair_hadamard_grad(T0, H, T1, H2, G["red_p"], G["red_c"], dhd)
    _compare("pair_hadamard_bwd", "atomics H%d H2 %d" % (H, H2), [("d0", d0, None, r64[0], r32[0]), ("d1", d1[:, :2 * H2].contiguous(), None, r64[1], r32[1])])


# ------------------------------------------------------------------------------------------------
# six-term loss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HR.LOSS_CASES, ids=[c["name"] for c in HR.LOSS_CASES])
def test_six_term_loss_forms(case):
    from fabind_amd import ops
    t = HR.loss_operands(case)
    gl, gt = HR.loss_upstream(case)
    td = [_d(x) for x in t]
    nblk = HR.loss_blocks(case["n_pair"], case["n_atoms"] * 3, case["B"] * case["L"])
    gld, gtd = (None if gl is None else _d(gl)), (None if gt is None else _d(gt))

    def run():
        leaves = [x.clone().requires_grad_() for x in td[:5]]
        _poison(((nblk, 8), F32), ((8,), F32), ((1,), F32), ((6,), F32))
        loss, terms = ops.six_term_loss(*leaves, *td[5:], HR.LOSS_W)
        assert list(terms) == list(HR.LOSS_TERMS)
        tv = torch.stack([terms[k] for k in HR.LOSS_TERMS])
        up = (gld * loss if gld is not None else 0) + ((gtd * tv).sum() if gtd is not None else 0)
        _poison(*[(tuple(x.shape), F32) for x in leaves])
        up.backward()
        assert all(int(v.item()) == 0 for v in ops._LOSS_TICKET.values()), "the ticket was not re-armed"
        return [loss.detach().reshape(1)] + [tv.detach()[k].reshape(1) for k in range(6)] + [x.grad for x in leaves]
    a, b = run(), run()
    refs = []
    for dt in (torch.float64, F32):
        tt = [x.to(dt) if x.is_floating_point() else x for x in t]
        total, terms = HR.six_term_loss(*tt, HR.LOSS_W)
        refs.append([total.reshape(1)] + [terms[k].reshape(1) for k in range(6)] + list(HR.six_term_loss_grad(*tt, HR.LOSS_W, gl, gt)))
    names = ["loss"] + list(HR.LOSS_TERMS) + ["d_coords", "d_y_pred", "d_y_by", "d_logits", "d_center"]
    print("head-forms | six_term_loss      | %s: %d blocks, cls %s" % (case["name"], nblk, case["cls_dt"]))
    _compare("six_term_loss", case["name"], [(nm, a[k], b[k], refs[0][k], refs[1][k]) for k, nm in enumerate(names)])
    if case["n_pair"] == 0:
        assert all(float(a[k]) == 0.0 for k in (3, 4, 5))                 # the empty terms are exactly 0


# ------------------------------------------------------------------------------------------------
# pocket centre
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", HR.POCKET_LS)
def test_pocket_center_forms(L):
    from fabind_amd import ops
    tau, B = HR.pocket_tau(L), HR.POCKET_B
    dc = torch.randn(B, 3, generator=torch.Generator().manual_seed(5))
    for noisy, hard in itertools.product((False, True), (False, True)):
        logits, mask, xyz, noise = HR.pocket_operands(L, noisy)
        lgd, md, xd, nd, dcd = _d(logits), _d(mask), _d(xyz), (None if noise is None else _d(noise)), _d(dc)
        case = "L%d tau %.1f %s %s" % (L, tau, "hard" if hard else "soft", "noise" if noisy else "no noise")

        def run():
            lg = lgd.clone().requires_grad_()
            _poison(((B, 3), F32), ((B,), F32))
            c = ops.pocket_center(lg, md, xd, tau=tau, hard=hard, noise=nd)
            _poison(((B, L), F32))
            c.backward(dcd)
            return c.detach(), lg.grad
        a, b = run(), run()
        r64 = HR.pocket_center_grad(logits.double(), mask, xyz.double(), tau, hard, noise, dc.double())
        r32 = HR.pocket_center_grad(logits, mask, xyz, tau, hard, noise, dc)
        _compare("pocket_center", case, [("center", a[0], b[0], r64[0], r32[0]), ("d_logits", a[1], b[1], r64[1], r32[1])])
        assert bool((a[1].cpu()[~mask] == 0).all()), (case, "a padding position received a gradient")
