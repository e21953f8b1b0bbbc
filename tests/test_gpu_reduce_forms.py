"""GPU: fabind_segment_sum (one-wave kernel and cooperative heavy-row kernel, both heavy_min values, rpw 64 / 128 / 1024, both slab
counts, strided operands), its adjoint gather_dact, and the "partials, then a fixed-order sum of the chunks" reductions of csrc/bwd.hip
and csrc/gemm.hip (colsum, split_sum, mul_dact, mul_dact_colsum / mul_dropmask_colsum, rowdot_bwd, gcl_pre_bwd), zero_empty_rows and
exclusive_scan, each through its public Python entry where one exists, against the float64 restatements of tests/reduce_refs.py on the
same operands.  The case tables live in reduce_refs.py; tests/test_reduce_refs_cpu.py asserts that they reach every dispatch class.

Every case runs twice on the device and must repeat bit for bit (bwd.hip: "no float atomics").  Outputs are prefilled with NaN (or, where
the entry allocates its own output, the allocator's next block of that size is), so an element no kernel wrote fails the finiteness check;
memory a kernel must not touch holds a sentinel and is compared bit for bit.

Bounds (coord_refs.rel_err / coord_refs.bound, norm_refs.bf16_excess; nothing tuned):
  tensors written as fp32:  err_hip <= bound(err32) = max(8 err32, 64 * 2^-23), err32 = the float32 restatement on the same operands,
                            which sums sequentially in operand order;
  tensors written as bf16:  per element |got - ref64| <= half_ulp_bf16(|ref64| + A) + A, A = bound(err32) max|ref64|.
No kernel needed an `extra` depth term: depth = 0 for every one of them (DESIGN.md lists the summation trees all the same).
Every (case, tensor, err_hip, err32, bound) is printed before it is asserted (`pytest -s`)."""
import types

import pytest
import torch

import coord_refs as CR
import norm_refs as NR
import reduce_refs as RR
from reduce_refs import ACT_NONE, ACT_RELU, ACT_SILU, BF, F32

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


def _L():
    from fabind_amd import _lib
    return _lib


def _dt(dtype):
    return "bf16" if dtype == BF else "f32"


def _poison(*specs):
    """The entry under test allocates its own outputs and scratch: fill the blocks the caching allocator hands out next for these
    (shape, dtype) with NaN."""
    ts = [torch.full(shape, NAN, dtype=dtype, device=_dev()) for shape, dtype in specs]
    del ts


def _scratch(nchunk, C):
    """Scratch of a raw call: NaN in every chunk row (an empty chunk must write its zeros) and in one row past the last (a chunk loop
    that runs one too far reads it)."""
    return torch.full((nchunk + 1, C), NAN, device=_dev())


def _compare(op, case, items, extra=0.0):
    """items: (name, got, got of the second run, ref64, ref32 (not rounded)); the rule follows the dtype the kernel wrote."""
    fails = []
    for nm, a, a2, r64, r32 in items:
        assert tuple(a.shape) == tuple(r64.shape), (op, case, nm, a.shape, r64.shape)
        assert bool(torch.isfinite(a).all()), (op, case, nm, "an element was not written")
        assert torch.equal(a, a2), (op, case, nm, "second run differs")
        a = a.detach().cpu()
        e_hip, e32 = CR.rel_err(a, r64), CR.rel_err(r32, r64)
        b = CR.bound(e32, extra)
        if a.dtype == BF:
            A = b * max(float(r64.abs().max()), 1e-6) if r64.numel() else 0.0
            ex = NR.bf16_excess(a, r64, A)
            print("reduce-forms | %-14s | %-44s | %-5s bf16 | err_hip %.2e | err32 %.2e | bound %.2e | excess over half-ulp + A %.2e"
                  % (op, case, nm, e_hip, e32, b, ex))
            ok = ex <= 0.0
        else:
            assert a.dtype == F32, (op, case, nm, a.dtype)
            print("reduce-forms | %-14s | %-44s | %-5s fp32 | err_hip %.2e | err32 %.2e | bound %.2e" % (op, case, nm, e_hip, e32, b))
            ok = e_hip <= b
        w = WORST.setdefault((op, nm, _dt(a.dtype)), [0.0, 0.0, 0.0, ""])
        if e_hip >= w[0]:
            w[:] = [e_hip, e32, b, case]
        if not ok:
            fails.append((nm, e_hip, e32, b))
    assert not fails, (op, case, fails)


def _print_worst(op):
    for (o, nm, dt), (e_hip, e32, b, case) in sorted(WORST.items()):
        if o == op:
            print("reduce-forms worst | %-14s | %-5s %-4s | err_hip %.2e | err32 %.2e | bound %.2e | %s" % (o, nm, dt, e_hip, e32, b, case))


def _zfeat(g, shape, dtype, signed=True):
    """Features with mean 4 and spread 1.5 (sums do not cancel); `signed`: one element in ten negated and exact 0.0 / -0.0 elements, so
    that an activation takes both branches.  bf16 operands hold bf16-exact values."""
    t = RR.feat(g, *shape)
    if signed and t.numel():
        t = torch.where(torch.rand(*shape, generator=g) < 0.1, -t, t)
        f = t.view(-1)
        f[0], f[-1] = 0.0, -0.0
        if f.numel() >= 7:
            f[3], f[6] = -0.0, 0.0
    return RR.bf_exact(t) if dtype == BF else t


def _view(host, pad, dtype, off=None):
    """host [R, C] as a device view of a [R, C + pad] buffer whose other columns hold NaN, starting at column `off` (default pad)."""
    R, C = host.shape
    if pad == 0:
        return _d(host.to(dtype))
    buf = torch.full((R, C + pad), NAN, dtype=dtype, device=_dev())
    off = pad if off is None else off
    v = buf[:, off:off + C]
    v.copy_(_d(host.to(dtype)))
    return v


# ------------------------------------------------------------------------------------------------
# segment_sum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RR.SEG_CASES, ids=[c["name"] for c in RR.SEG_CASES])
def test_segment_sum_forms(case):
    from fabind_amd import kernels as K
    dev = _dev()
    n, H, act, form = case["n_rows"], case["H"], case["act"], case["out_form"]
    lens = RR.seg_case_lengths(case)
    rp = RR.rowptr_of(lens)
    E = int(rp[-1])
    p = RR.seg_launch(n, H)
    g = torch.Generator().manual_seed(n * 31 + H)
    Zh = _zfeat(g, (E, H), case["z_dt"], signed=act != ACT_NONE)
    perm = torch.randperm(E, generator=g).to(torch.int32) if case["perm"] else None
    Zd = _view(Zh, case["ldz_pad"], case["z_dt"])
    assert (Zd.stride(0) > H) == (case["ldz_pad"] > 0)
    rpd, pd = _d(rp), (_d(perm) if perm is not None else None)

    def run():
        if form == "fresh":
            out = torch.full((n, H), NAN, device=dev)
            K.segment_sum(Zd, rpd, n, act, pd, out=out)
            return [("out", out)]
        if form in ("dAB_lo", "dAB_hi"):                                  # _GclPre.backward: ldo = 2H, the second half H floats in
            dAB = torch.full((n, 2 * H), SENT, device=dev)
            mine, other = (dAB[:, :H], dAB[:, H:]) if form == "dAB_lo" else (dAB[:, H:], dAB[:, :H])
            mine.fill_(NAN)
            K.segment_sum(Zd, rpd, n, act, pd, out=mine)
            assert bool((other == SENT).all()), (case["name"], "the other half of dAB was written")
            return [("out", mine.contiguous())]
        if form == "out16":
            o16 = torch.full((n, H), NAN, dtype=BF, device=dev)
            K.segment_sum(Zd, rpd, n, act, pd, out16=o16)
            return [("out16", o16)]
        out = torch.full((n, H), NAN, device=dev)                         # "both": out next to a bf16 copy with ldo16 > H
        b16 = torch.full((n, H + 8), SENT, dtype=BF, device=dev)
        b16[:, :H].fill_(NAN)
        K.segment_sum(Zd, rpd, n, act, pd, out=out, out16=b16[:, :H])
        assert bool((b16[:, H:] == SENT).all()), (case["name"], "columns beyond H of out16 were written")
        return [("out", out), ("out16", b16[:, :H].contiguous())]

    a, b = run(), run()
    r64 = RR.segment_sum(Zh, rp, act, perm)
    r32 = RR.segment_sum(Zh, rp, act, perm, dtype=torch.float32)
    print("reduce-forms | segment_sum    | %s: E %d heavy_min %d rpw %d U %d depth 0" % (case["name"], E, p["heavy_min"], p["rpw"], p["U"]))
    _compare("segment_sum", case["name"], [(nm, x, y[1], r64, r32) for (nm, x), y in zip(a, b)])
    if case is RR.SEG_CASES[-1]:
        _print_worst("segment_sum")


# ------------------------------------------------------------------------------------------------
# gather_dact: the adjoint of segment_sum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", RR.GATHER_HS)
def test_gather_dact_forms(H):
    from fabind_amd import ops
    L, dev = _L(), _dev()
    lib = L.load()
    i = 0
    for E in RR.GATHER_ES:
        g = torch.Generator().manual_seed(H * 7 + E)
        lens = [0, 1, 0] if E == 1 else [0, 3, 0, 2, 0] if E == 5 else [0, 0] + [11] * 92 + [0, 9, 0]      # repeats, rows no edge points to
        rp = RR.rowptr_of(lens)
        row = CR.rows_of(rp).to(torch.int32)
        n = len(lens)
        assert row.numel() == E
        douth = RR.feat(g, n, H)
        doutd = _view(douth, 4, F32)                                      # ldo = H + 4, the base 16 bytes in
        for z_dt in (F32, BF):
            Zh = _zfeat(g, (E, H), z_dt)
            Zd = _d(Zh.to(z_dt))
            for act in RR.ACTS:
                case = "E%d H%d %s %s ldo+4" % (E, H, _dt(z_dt), RR.ACT_NAMES[act])

                def run():
                    dZ = torch.full((E, H), NAN, dtype=z_dt, device=dev)
                    L.check(lib.fabind_gather_dact(L.ptr(doutd), doutd.stride(0), L.ptr(_d(row)), L.ptr(Zd), L.dt_code(z_dt), act, L.ptr(dZ),
                                                   L.dt_code(z_dt), E, H, L.stream()), "fabind_gather_dact")
                    return dZ
                a, b = run(), run()
                _compare("gather_dact", case, [("dZ", a, b, RR.gather_dact(douth, row, Zh, act), RR.gather_dact(douth, row, Zh, act, torch.float32))])
                # through ops.segment_sum under autograd (the forward needs H % 8 == 0)
                if H % 8 == 0 and act in (ACT_NONE, ACT_SILU, ACT_RELU) and (i % 2 == 0 or E == 1021):
                    cot = _d(douth)

                    def run_ag():
                        Zg = Zd.clone().requires_grad_()
                        _poison(((E, H), z_dt))
                        ops.segment_sum(Zg, _d(rp), _d(row), n, act).backward(cot)
                        return Zg.grad
                    a, b = run_ag(), run_ag()
                    _compare("gather_dact", case + " autograd", [("dZ", a, b, RR.gather_dact(douth, row, Zh, act),
                                                                  RR.gather_dact(douth, row, Zh, act, torch.float32))])
                i += 1
    _print_worst("gather_dact")


# ------------------------------------------------------------------------------------------------
# colsum
# ------------------------------------------------------------------------------------------------
def _colsum_case(K, R, C, layout, dt, acc, g, nchunk=None):
    L = _L()
    xh = _zfeat(g, (R, C), dt, signed=False)
    if layout == "tight":
        xd = _d(xh.to(dt))
    elif layout == "ld+1":
        xd = _view(xh, 1, dt, off=0)
    elif layout == "ld+4":
        xd = _view(xh, 4, dt, off=0)
    elif layout == "ld%4":                                                # C % 4 != 0 under a leading dimension that is a multiple of 4:
        xd = _view(xh, 4 + (-C) % 4, dt, off=0)                           # 4-wide lanes and a scalar lane for the last columns
    else:                                                                 # "off1": buf[:, 1:] -- the base is 4 (fp32) / 2 (bf16) bytes off
        xd = _view(xh, 4 + (-C) % 4, dt, off=1)
        assert xd.data_ptr() % (8 if dt == BF else 16) != 0 or R == 0
    o0 = RR.feat(g, C)
    case = "R%d C%d %s %s %s%s" % (R, C, layout, _dt(dt), "acc" if acc else "store", "" if nchunk is None else " nchunk%d" % nchunk)

    def run():
        out = _d(o0.clone()) if acc else torch.full((C,), NAN, device=_dev())
        if nchunk is None:
            _poison(((RR.nchunk_colsum(R), C), F32))
            K.colsum(xd, out=out, accumulate=acc)
        else:
            scratch = _scratch(nchunk, C)
            L.check(L.load().fabind_colsum(L.ptr(xd), L.dt_code(dt), xd.stride(0), L.ptr(out), R, C, 1 if acc else 0, L.ptr(scratch), nchunk,
                                           L.stream()), "fabind_colsum")
        return out
    a, b = run(), run()
    r64, r32 = RR.colsum(xh), RR.colsum(xh, torch.float32)
    if acc:
        r64, r32 = o0.double() + r64, o0 + r32
    _compare("colsum", case, [("sum", a, b, r64, r32)])


@pytest.mark.parametrize("C", RR.COLSUM_CS)
def test_colsum_forms(C):
    from fabind_amd import kernels as K
    g = torch.Generator().manual_seed(C)
    layouts = ["tight", "ld+1", "ld+4", "off1"] + (["ld%4"] if C % 4 else [])
    i = 0
    for R in RR.COLSUM_RS:
        for layout in layouts:
            for dt in (F32, BF):
                # accumulate alternates against the dtype from one layout to the next; R <= 256 without it is the single-chunk direct path
                _colsum_case(K, R, C, layout, dt, bool((i + (dt == BF)) % 2), g)
            i += 1
    for nchunk in (3, 5, 7):                                              # colsum_final_kernel strides the chunks by 4
        _colsum_case(K, 1000, C, "tight", F32, nchunk == 5, g, nchunk=nchunk)
    if C == 4:                                                            # nchunk capped at 1024: chunks 1021 .. 1023 are empty and must hold zeros
        assert RR.chunk_rows(RR.COLSUM_BIG_R, RR.nchunk_colsum(RR.COLSUM_BIG_R))[-3:] == [0, 0, 0]
        _colsum_case(K, RR.COLSUM_BIG_R, 4, "tight", F32, False, g)
        _colsum_case(K, RR.COLSUM_BIG_R, 4, "tight", BF, True, g)
    if C == RR.COLSUM_CS[-1]:
        _print_worst("colsum")


# ------------------------------------------------------------------------------------------------
# split_sum
# ------------------------------------------------------------------------------------------------
def test_split_sum_forms():
    L, dev = _L(), _dev()
    lib = L.load()
    g = torch.Generator().manual_seed(11)
    for splits in RR.SPLIT_SPLITS:
        for n in RR.SPLIT_NS:
            for n_tail in (0, 4, n):
                for out_dt in (F32, BF):
                    ph = RR.feat(g, splits, n)
                    pd = _d(ph)
                    case = "splits%d n%d tail%d %s" % (splits, n, n_tail, _dt(out_dt))

                    def run():
                        out = torch.full((n,), SENT, dtype=out_dt, device=dev)        # the head is written, the rest stays
                        out[:n - n_tail].fill_(NAN)
                        tail = torch.full((n_tail,), NAN, device=dev) if n_tail else None
                        L.check(lib.fabind_split_sum(L.ptr(pd), splits, n, L.ptr(out), L.dt_code(out_dt), n_tail, L.ptr(tail), L.stream()),
                                "fabind_split_sum")
                        assert bool((out[n - n_tail:] == SENT).all()), (case, "out behind the head was written")
                        return out[:n - n_tail].contiguous(), (tail if tail is not None else torch.zeros(0, device=dev))
                    a, b = run(), run()
                    h64, t64 = RR.split_sum(ph, n_tail)
                    h32, t32 = RR.split_sum(ph, n_tail, torch.float32)
                    _compare("split_sum", case, [("head", a[0], b[0], h64, h32), ("tail", a[1], b[1], t64, t32)])
    _print_worst("split_sum")


# ------------------------------------------------------------------------------------------------
# mul_dact, mul_dact_colsum, mul_dropmask_colsum
# ------------------------------------------------------------------------------------------------
def test_mul_dact_forms():
    from fabind_amd import ops
    g = torch.Generator().manual_seed(21)
    scale = 0.75
    for n in RR.MUL_DACT_NS:
        for dy_dt, aux_dt, out_dt in RR.MUL_DACT_DTYPES:
            for act in (RR.ACTS if aux_dt is not None else (ACT_NONE,)):
                dyh = _zfeat(g, (n,), dy_dt, signed=False)
                yh = _zfeat(g, (n,), aux_dt, signed=True) if aux_dt is not None else dyh
                dyd = _d(dyh.to(dy_dt))
                yd = _d(yh.to(aux_dt)) if aux_dt is not None else None
                case = "n%d %s/%s->%s %s" % (n, _dt(dy_dt), _dt(aux_dt) if aux_dt is not None else "-", _dt(out_dt), RR.ACT_NAMES[act])

                def run():
                    _poison(((n,), out_dt))
                    return ops._mul_dact(dyd, yd, act, out_dt, scale)
                a, b = run(), run()
                _compare("mul_dact", case, [("out", a, b, RR.mul_dact(dyh, yh, act, scale)[0], RR.mul_dact(dyh, yh, act, scale, torch.float32)[0])])
    _print_worst("mul_dact")


def _mdc_case(ops, R, C, dts, act, g, p=None):
    dy_dt, aux_dt, out_dt = dts
    dyh = _zfeat(g, (R, C), dy_dt, signed=False)
    dyd = _d(dyh.to(dy_dt))
    nchunk = RR.nchunk_mul_dact_colsum(R)
    if p is None:
        yh = _zfeat(g, (R, C), aux_dt, signed=True) if aux_dt is not None else None
        yd = _d(yh.to(aux_dt)) if aux_dt is not None else None
        op, case = "mul_dact_colsum", "R%d C%d nchunk%d %s/%s->%s %s" % (R, C, nchunk, _dt(dy_dt), _dt(aux_dt) if aux_dt is not None else "-", _dt(out_dt),
                                                                       RR.ACT_NAMES[act])

        def run():
            _poison(((R, C), out_dt), ((nchunk, C), F32), ((C,), F32))
            return ops._mul_dact_colsum(dyd, yd, act, out_dt, 0.75)
        ref = [RR.mul_dact(dyh, yh if yh is not None else dyh, act, 0.75, dt) for dt in (torch.float64, torch.float32)]
    else:
        op, case = "mul_dropmask", "R%d C%d nchunk%d %s->%s p%.1f" % (R, C, nchunk, _dt(dy_dt), _dt(out_dt), p)

        def run():
            _poison(((R, C), out_dt), ((nchunk, C), F32), ((C,), F32))
            return ops._mul_dropmask_colsum(dyd, p, RR.DROP_SEED, out_dt)
        ref = [RR.mul_dropmask(dyh, RR.DROP_SEED, p, dt) for dt in (torch.float64, torch.float32)]
    a, b = run(), run()
    _compare(op, case, [("out", a[0], b[0], ref[0][0], ref[1][0]), ("db", a[1], b[1], ref[0][1], ref[1][1])])


@pytest.mark.parametrize("C", RR.MDC_CS)
def test_mul_dact_colsum_and_dropmask_forms(C):
    from fabind_amd import ops
    g = torch.Generator().manual_seed(C + 1)
    rs = RR.mdc_rows()
    for i, R in enumerate(rs):
        dts = RR.MUL_DACT_DTYPES[i % len(RR.MUL_DACT_DTYPES)]
        act = ACT_NONE if dts[1] is None else RR.ACTS[i % len(RR.ACTS)]
        _mdc_case(ops, R, C, dts, act, g)
        _mdc_case(ops, R, C, (dts[0], None, dts[2]), None, g, p=RR.DROP_PS[i % 2])
    if C == 4:                                                            # nchunk capped at 4096, rows_per 65: chunks 4034 .. 4095 are empty
        assert RR.chunk_rows(RR.MDC_BIG_R, 4096)[-1] == 0
        _mdc_case(ops, RR.MDC_BIG_R, 4, (F32, F32, BF), ACT_SILU, g)
        _mdc_case(ops, RR.MDC_BIG_R, 4, (BF, None, F32), None, g, p=0.1)
    if C == RR.MDC_CS[-1]:
        _print_worst("mul_dact_colsum")
        _print_worst("mul_dropmask")


# ------------------------------------------------------------------------------------------------
# rowdot_bwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", RR.ROWDOT_NS)
def test_rowdot_bwd_forms(N):
    from fabind_amd import ops
    L, dev = _L(), _dev()
    g = torch.Generator().manual_seed(N + 2)
    np_ = (N + 127) // 128
    for i, (M, nchunk) in enumerate(RR.rowdot_cases()):
        for z_dt in (F32, BF):
            act = (ACT_NONE, ACT_SILU, ACT_RELU)[(i + (z_dt == BF)) % 3]
            zh = _zfeat(g, (M, N), z_dt)
            dph = RR.feat(g, M, np_)
            uh = torch.rand(N, generator=g) + 0.5
            zd, dpd, ud = _d(zh.to(z_dt)), _d(dph), _d(uh)
            case = "M%d N%d %s %s nchunk %s" % (M, N, _dt(z_dt), RR.ACT_NAMES[act], nchunk if nchunk else "own(%d)" % RR.nchunk_colsum(M))

            def run():
                if nchunk is None:
                    _poison(((M, N), z_dt), ((RR.nchunk_colsum(M), N), F32), ((N,), F32))
                    return ops._rowdot_bwd(zd, dpd, ud, act)
                dz = torch.full((M, N), NAN, dtype=z_dt, device=dev)
                du = torch.full((N,), NAN, device=dev)
                scratch = _scratch(nchunk, N)
                L.check(L.load().fabind_rowdot_bwd(L.ptr(zd), L.dt_code(z_dt), L.ptr(dpd), np_, L.ptr(ud), act, M, N, L.ptr(dz), L.ptr(du),
                                                   L.ptr(scratch), nchunk, L.stream()), "fabind_rowdot_bwd")
                return dz, du
            a, b = run(), run()
            r64, r32 = RR.rowdot_bwd(zh, dph, uh, act), RR.rowdot_bwd(zh, dph, uh, act, torch.float32)
            _compare("rowdot_bwd", case, [("dz", a[0], b[0], r64[0], r32[0]), ("du", a[1], b[1], r64[1], r32[1])])
    if N == RR.ROWDOT_NS[-1]:
        _print_worst("rowdot_bwd")


# ------------------------------------------------------------------------------------------------
# gcl_pre_bwd
# ------------------------------------------------------------------------------------------------
def _gcl_raw(H, E, dt, g):
    L, dev = _L(), _dev()
    dph = _zfeat(g, (E, H), dt, signed=False)
    rhh, wh = torch.rand(E, generator=g), torch.rand(H, generator=g) + 0.5
    dpd, rhd, wd = _d(dph.to(dt)), _d(rhh), _d(wh)
    nchunk = RR.nchunk_gcl_pre(E)
    case = "E%d H%d %s nchunk%d" % (E, H, _dt(dt), nchunk)

    def run():
        drh, dw = torch.full((E,), NAN, device=dev), torch.full((H,), NAN, device=dev)
        scratch = _scratch(nchunk, H)
        L.check(L.load().fabind_gcl_pre_bwd(L.ptr(dpd), L.dt_code(dt), H, L.ptr(rhd), L.ptr(wd), E, L.ptr(drh), L.ptr(dw), L.ptr(scratch), nchunk,
                                            L.stream()), "fabind_gcl_pre_bwd")
        return drh, dw
    a, b = run(), run()
    r64, r32 = RR.gcl_pre_bwd(dph, rhh, wh), RR.gcl_pre_bwd(dph, rhh, wh, torch.float32)
    _compare("gcl_pre_bwd", case, [("drh", a[0], b[0], r64[0], r32[0]), ("dw", a[1], b[1], r64[1], r32[1])])


@pytest.mark.parametrize("H", RR.GCL_HS)
def test_gcl_pre_bwd_forms(H):
    from fabind_amd import ops
    g = torch.Generator().manual_seed(H + 3)
    for E in RR.GCL_ES:
        for dt in (F32, BF):
            _gcl_raw(H, E, dt, g)
    if H == 4:                                                            # nchunk capped at 2048, 257 edges each: chunks 2041 .. 2047 are empty
        assert RR.chunk_rows(RR.GCL_BIG_E, 2048)[-1] == 0
        _gcl_raw(4, RR.GCL_BIG_E, F32, g)
    if H % 8 == 0:
        # ops.gcl_pre under autograd: dAB through the two strided segment sums (by row, and by column through the permutation), drh and dw
        n = 23
        lens = torch.randint(0, 9, (n,), generator=g).tolist()
        lens[0], lens[5], lens[-1] = 0, 40, 0                             # a heavy row among them
        rp = RR.rowptr_of(lens)
        row = CR.rows_of(rp)
        E = row.numel()
        col = torch.randint(0, n - 2, (E,), generator=g)                  # nodes n - 2 and n - 1 send nothing
        perm = torch.argsort(col, stable=True)
        colptr = RR.rowptr_of(torch.bincount(col, minlength=n).tolist())
        graph = types.SimpleNamespace(row_ctx=_d(row.to(torch.int32)), col_ctx=_d(col.to(torch.int32)), rp_ctx=_d(rp),
                                      ctx_by_col=lambda: (_d(colptr), _d(perm.to(torch.int32))))
        ABh, rhh, wh = RR.feat(g, n, 2 * H), torch.rand(E, generator=g), torch.rand(H, generator=g) + 0.5
        coth = RR.feat(g, E, H)

        def run():
            AB, rh, w = _d(ABh).requires_grad_(), _d(rhh).requires_grad_(), _d(wh).requires_grad_()
            _poison(((n, 2 * H), F32), ((E,), F32), ((RR.nchunk_gcl_pre(E), H), F32), ((H,), F32))
            ops.gcl_pre(AB, H, graph, rh, w).backward(_d(coth))
            return AB.grad, rh.grad, w.grad
        a, b = run(), run()
        refs = []
        for dt in (torch.float64, torch.float32):
            drh, dw = RR.gcl_pre_bwd(coth, rhh, wh, dt)
            refs.append((torch.cat([RR.segment_sum(coth, rp, ACT_NONE, dtype=dt), RR.segment_sum(coth, colptr, ACT_NONE, perm, dtype=dt)], 1), drh, dw))
        _compare("gcl_pre_bwd", "autograd n%d E%d H%d" % (n, E, H), [(nm, a[k], b[k], refs[0][k], refs[1][k]) for k, nm in enumerate(("dAB", "drh", "dw"))])
    if H == RR.GCL_HS[-1]:
        _print_worst("gcl_pre_bwd")


# ------------------------------------------------------------------------------------------------
# zero_empty_rows, exclusive_scan
# ------------------------------------------------------------------------------------------------
def test_zero_empty_rows_forms():
    from fabind_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(31)
    i = 0
    for n in RR.ZER_ROWS:
        tables = [[0], [3]] if n == 1 else [[0, 2, 0, 1, 0]] if n == 5 else [torch.randint(0, 2, (n,), generator=g).tolist()]
        for lens in tables:
            rp = RR.rowptr_of(lens)
            for C in RR.ZER_CS:
                for dt in (F32, BF):
                    dt2, pad, pad2 = (BF, F32)[dt == BF], (1, 3, 8)[i % 3], (2, 5)[i % 2]
                    with2 = i % 2 == 0
                    i += 1
                    # a sentinel pattern with a different value per element: rows with edges and columns >= C must come back bit for bit
                    s1 = (torch.arange(n * (C + pad)).reshape(n, C + pad) % 97 + 1).to(dt)
                    s2 = (torch.arange(n * (C + pad2)).reshape(n, C + pad2) % 89 + 1).to(dt2)
                    for _ in range(2):
                        out, out2 = _d(s1.clone()), (_d(s2.clone()) if with2 else None)
                        K.zero_empty_rows(_d(rp), out, C, out2)
                        assert torch.equal(out.cpu(), RR.zero_empty_rows(rp, s1, C)), (lens[:5], C, dt)
                        if with2:
                            assert torch.equal(out2.cpu(), RR.zero_empty_rows(rp, s2, C)), (lens[:5], C, dt2)
    assert dev.type == "cuda"


def test_exclusive_scan_forms():
    from fabind_amd import kernels as K
    g = torch.Generator().manual_seed(41)
    for n in RR.SCAN_NS:
        deg = torch.randint(0, 50, (n,), generator=g, dtype=torch.int32)
        a, b = K.exclusive_scan(_d(deg)), K.exclusive_scan(_d(deg))
        ref = RR.exclusive_scan(deg)
        assert int(ref[-1]) < 2 ** 31 and a.dtype == torch.int32
        assert torch.equal(a.cpu().long(), ref) and torch.equal(a, b), n
