"""GPU: every kernel form of csrc/norm.hip (row LayerNorm and its adjoint, row_stats, edge_ln_concat / edge_concat, the LayerNorm-folded
first edge Linear and its adjoint, inter_coord_fold, the base model's layernorm) through its public entry against the float64
restatements of tests/norm_refs.py on the same operands.  A case table per operation: each row names the form it expects, the form
report (fabind_*_form, the host function the launcher itself dispatches through) must say so before the launch, and a closing test
per operation asserts that the table reaches every form id declared in include/fabind_hip.h.  Every case runs twice on the device
(bit-identical: no float atomics) and through the reference in float64 and float32.

Bounds (coord_refs.rel_err / coord_refs.bound; nothing tuned):
  tensors written as fp32:  err_hip <= bound(err32) = max(8 err32, 64 * 2^-23), err = max|T - T64| / max(max|T64|, 1e-6), err32 = the
                            float32 host restatement on the same operands;
  tensors written as bf16:  per element |got - ref64| <= half_ulp_bf16(|ref64| + A) + A, A = bound(err32) max|ref64|, err32 taken before the
                            output rounding; half_ulp_bf16(x) = 2^(floor(log2 x) - 8), the element's own half-ulp under round-to-nearest-even
                            (v_cvt_pk_bf16_f32).  It lies between 2^-9 x and 2^-8 x: bf16 keeps 8 significand bits, so a correctly
                            rounded output misses the envelope 2^-9 |ref64| + (1 + 2^-9) A by up to 2^-9 |ref64| (shown on exact inputs in
                            tests/test_norm_refs_cpu.py); the excess over that envelope is printed with every bf16 tensor, not asserted.
No element is masked out: ReLU is compared by value, dropout masks are restated exactly (norm_refs.drop_keep), the adjoint's mask is an
input.  Every (case, tensor, err_hip, err32, bound) is printed before it is asserted (`pytest -s`); DESIGN.md carries the table."""
import pytest
import torch

import coord_refs as CR
import norm_refs as NR

pytestmark = pytest.mark.gpu
EPS = 1e-5
BF, F32 = torch.bfloat16, torch.float32


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


def _compare(op, case, items):
    """items: (name, got, got of the second run, ref64, ref32 (not rounded)); the rule follows the dtype the kernel wrote."""
    fails = []
    for nm, a, a2, r64, r32 in items:
        assert tuple(a.shape) == tuple(r64.shape), (op, case, nm, a.shape, r64.shape)
        assert bool(torch.isfinite(a).all()), (op, case, nm)
        assert torch.equal(a, a2), (op, case, nm, "second run differs")
        a = a.detach().cpu()
        e_hip, e32 = CR.rel_err(a, r64), CR.rel_err(r32, r64)
        b = CR.bound(e32)
        if a.dtype == BF:
            A = b * max(float(r64.abs().max()), 1e-6) if r64.numel() else 0.0
            ex = NR.bf16_excess(a, r64, A)
            print("norm-forms | %-14s | %-30s | %-6s bf16 | err_hip %.2e | err32 %.2e | bound %.2e | excess over half-ulp + A %.2e | over 2^-9|ref| + A %.2e"
                  % (op, case, nm, e_hip, e32, b, ex, NR.bf16_excess_literal(a, r64, A)))
            ok = ex <= 0.0
        else:
            assert a.dtype == F32, (op, case, nm, a.dtype)
            print("norm-forms | %-14s | %-30s | %-6s fp32 | err_hip %.2e | err32 %.2e | bound %.2e" % (op, case, nm, e_hip, e32, b))
            ok = e_hip <= b
        if not ok:
            fails.append((nm, e_hip, e32, b))
    assert not fails, (op, case, fails)


def _feat(g, *shape):
    """Features with mean 4 and spread 1.5."""
    return torch.randn(*shape, generator=g) * 1.5 + 4.0


def _bf_exact(t):
    return t.bfloat16().float()


# ------------------------------------------------------------------------------------------------
# row LayerNorm and its adjoint (plus.engine.ln_rows / kernels.layernorm_rows)
# ------------------------------------------------------------------------------------------------
def _L():
    from fabind_amd import _lib
    return _lib


# (case, R, C, ld of x, pad_to, x dtype, y dtype, forward form, adjoint form, special rows)
# rows per work-group: 16 (8S16), 8 (8S32), 4 elsewhere; the adjoint's grid is capped at 2048 work-groups
LN_CASES = [
    ("8s16 C100/104 R1", 1, 100, 104, 104, BF, BF, "LNR_8S16", "LNB_8S16", False),
    ("8s16 C100/104 R15", 15, 100, 104, 104, BF, F32, "LNR_8S16", "LNB_8S16", False),
    ("8s16 C100/104 R17", 17, 100, 104, 104, F32, BF, "LNR_8S16", "LNB_8S16", False),
    ("8s16 C64/72 pad80 R33", 33, 64, 72, 80, F32, F32, "LNR_8S16", "LNB_8S16", False),
    ("8s16 C16 R32771 2nd trip", 4 * 2048 * 4 + 3, 16, 16, 16, F32, F32, "LNR_8S16", "LNB_8S16", False),
    ("8s16 C128 stats rows", 6, 128, 128, 128, F32, F32, "LNR_8S16", "LNB_8S16", True),
    ("8s32 C200/256 pad208 R7", 7, 200, 256, 208, BF, BF, "LNR_8S32", "LNB_8S32", False),
    ("8s32 C256 R9", 9, 256, 256, 256, F32, F32, "LNR_8S32", "LNB_8S32", False),
    ("v8<1> C512/520 R3", 3, 512, 520, 512, BF, BF, "LNR_V8_1", "LNB_V8_1", False),
    ("v8<1> C260 pad272 R5", 5, 260, 264, 272, F32, F32, "LNR_V8_1", "LNB_V8_1", False),
    ("v8<2> C1000/1008 R5", 5, 1000, 1008, 1000, BF, F32, "LNR_V8_2", "LNB_V8_2", False),
    ("v8<2> C520 R3", 3, 520, 520, 520, F32, BF, "LNR_V8_2", "LNB_V8_2", False),
    ("v8<3> C1025/1088 R5", 5, 1025, 1088, 1088, BF, BF, "LNR_V8_3", "LNB_V8_3", False),
    ("v8<3> C1536 R3", 3, 1536, 1536, 1536, F32, F32, "LNR_V8_3", "LNB_V8_3", False),
    ("v8<4> C2048 R5", 5, 2048, 2048, 2048, BF, BF, "LNR_V8_4", "LNB_S32", False),
    ("v8<4> C1540/1544 R3", 3, 1540, 1544, 1544, F32, F32, "LNR_V8_4", "LNB_S32", False),
    ("s<2> C36 pad44 R5", 5, 36, 36, 44, F32, F32, "LNR_S2", "LNB_S2", False),
    ("s<2> C36 R8195 2nd trip", 2048 * 4 + 3, 36, 36, 36, BF, BF, "LNR_S2", "LNB_S2", False),
    ("s<2> C128/129 stats rows", 6, 128, 129, 128, F32, F32, "LNR_S2", "LNB_S2", True),
    ("s<8> C300/301 pad304 R3", 3, 300, 301, 304, F32, BF, "LNR_S8", "LNB_S8", False),
    ("s<8> C512/513 R5", 5, 512, 513, 512, BF, F32, "LNR_S8", "LNB_S8", False),
    ("s<16> C1000/1001 R5", 5, 1000, 1001, 1000, F32, F32, "LNR_S16", "LNB_S16", False),
    ("s<16> C513 R1", 1, 513, 513, 513, BF, BF, "LNR_S16", "LNB_S16", False),
    ("s<32>/s<20> C1100/1101 R5", 5, 1100, 1101, 1100, F32, F32, "LNR_S32", "LNB_S20", False),
    ("s<32>/s<20> C1025 R3", 3, 1025, 1025, 1025, BF, BF, "LNR_S32", "LNB_S20", False),
    ("s<32> C2047 R5", 5, 2047, 2047, 2047, F32, F32, "LNR_S32", "LNB_S32", False),
    ("s<32> C1281 pad1288 R3", 3, 1281, 1281, 1288, BF, F32, "LNR_S32", "LNB_S32", False),
]


@pytest.mark.parametrize("case", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_layernorm_rows_forms(case, monkeypatch):
    from fabind_amd import kernels as K
    from fabind_amd.plus import engine as pe
    name, R, C, ld, pad, x_dt, y_dt, f_fwd, f_bwd, special = case
    L, dev = _L(), _dev()
    g = torch.Generator().manual_seed(R * 7 + C)
    buf = _feat(g, R, ld)
    if special:
        buf[0] = 2.5                                                   # variance 0
        buf[1] = 1e3 + torch.randn(ld, generator=g)                    # mean 1e3, unit spread
    buf = buf.to(x_dt)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    cot = _bf_exact(torch.randn(R, C, generator=g))                    # (a bf16 output hands its cotangent on as bf16: exact)

    # the report is asked with the arguments of the launches themselves: both launchers are wrapped for the duration of the test
    lib, seen = L.load(), {"fwd": [], "bwd": []}
    fwd0, bwd0 = lib.fabind_layernorm_rows, lib.fabind_layernorm_rows_bwd

    def fwd_spy(*a):       # (x, x_dt, ldx, w, b, eps, R, C, y, y_dt, ldy, pad_to, stream)
        seen["fwd"].append(lib.fabind_layernorm_rows_form(a[0], a[2], a[7], a[8], a[10], a[11]))
        return fwd0(*a)

    def bwd_spy(*a):       # (x, x_dt, ldx, w, dy, dy_dt, lddy, eps, R, C, dx, dx_dt, lddx, dw_part, db_part, nblk, stream)
        seen["bwd"].append(lib.fabind_layernorm_rows_bwd_form(a[0], a[2], a[4], a[6], a[10], a[12], a[9]))
        return bwd0(*a)

    monkeypatch.setattr(lib, "fabind_layernorm_rows", fwd_spy)
    monkeypatch.setattr(lib, "fabind_layernorm_rows_bwd", bwd_spy)

    def hip():
        xd = _d(buf)[:, :C].requires_grad_(True)
        wd, bd = _d(w).requires_grad_(True), _d(b).requires_grad_(True)
        y_like = torch.empty((R, pad), dtype=y_dt, device=dev)
        assert K.layernorm_rows_form(xd, y_like, C, pad) == getattr(L, f_fwd), (name, K.layernorm_rows_form(xd, y_like, C, pad))   # before any launch
        y0 = K.layernorm_rows(xd.detach(), wd.detach(), bd.detach(), y_dt, pad)
        y = pe.ln_rows(xd, wd, bd, y_dt, pad)
        assert torch.equal(y0, y.detach())
        (y[:, :C].float() * _d(cot)).sum().backward()
        assert xd.grad.dtype == x_dt
        return [y.detach(), xd.grad, wd.grad, bd.grad]

    def ref(dt):
        x = NR.cast(dt, buf)[:, :C].clone().requires_grad_(True)
        wr, br = w.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
        y = NR.layer_norm_rows(x, wr, br, EPS, pad)
        (y[:, :C] * cot.to(dt)).sum().backward()
        return [y.detach(), x.grad, wr.grad, br.grad]

    h1, h2, r64, r32 = hip(), hip(), ref(torch.float64), ref(torch.float32)
    assert seen["fwd"] == [getattr(L, f_fwd)] * 4 and seen["bwd"] == [getattr(L, f_bwd)] * 2, (name, seen)      # what was launched
    assert h1[0].shape == (R, pad) and (pad == C or float(h1[0][:, C:].float().abs().max()) == 0.0)       # exact zeros in [C, pad_to)
    _compare("layernorm_rows", name, list(zip(("y", "dx", "dw", "db"), h1, h2, r64, r32)))


def test_layernorm_rows_tables_reach_every_form():
    L = _L()
    assert {getattr(L, c[7]) for c in LN_CASES} == set(range(L.LNR_COUNT))
    assert {getattr(L, c[8]) for c in LN_CASES} == set(range(L.LNB_COUNT))


# ------------------------------------------------------------------------------------------------
# ops.layernorm (fabind_layernorm_fwd / _bwd)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [36, 64, 512, 2048])
@pytest.mark.parametrize("R", [1, 5, 77])
def test_base_layernorm_forward_and_adjoint(R, C):
    from fabind_amd import ops
    g = torch.Generator().manual_seed(R * 11 + C)
    x0, w, b, cot = _feat(g, R, C), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(R, C, generator=g)

    def run(fn, dt, dev):
        ls = [t.to(device=dev, dtype=dt).requires_grad_(True) for t in (x0, w, b)]
        y = fn(*ls)
        (y * cot.to(device=dev, dtype=dt)).sum().backward()
        return [y.detach()] + [l.grad for l in ls]

    hip = lambda x, w_, b_: ops.layernorm(x, w_, b_, EPS)
    ref = lambda x, w_, b_: NR.layer_norm_rows(x, w_, b_, EPS)
    h1, h2 = run(hip, F32, _dev()), run(hip, F32, _dev())
    r64, r32 = run(ref, torch.float64, "cpu"), run(ref, F32, "cpu")
    _compare("ops.layernorm", "R%d C%d" % (R, C), list(zip(("y", "dx", "dw", "db"), h1, h2, r64, r32)))


# ------------------------------------------------------------------------------------------------
# row_stats
# ------------------------------------------------------------------------------------------------
# (case, R, C, ld, dtype, form)
RST_CASES = [
    ("bf16<1> C8 R5", 5, 8, 8, BF, "RST_BF16_1"),
    ("bf16<1> C512/520 R6", 6, 512, 520, BF, "RST_BF16_1"),
    ("bf16<2> C520 R5", 5, 520, 520, BF, "RST_BF16_2"),
    ("bf16<2> C1024 R3", 3, 1024, 1024, BF, "RST_BF16_2"),
    ("bf16<4> C1032 R7", 7, 1032, 1032, BF, "RST_BF16_4"),
    ("bf16<4> C2048 R5", 5, 2048, 2048, BF, "RST_BF16_4"),
    ("generic fp32 C512 R5", 5, 512, 512, F32, "RST_GENERIC"),
    ("generic bf16 C100 R6", 6, 100, 100, BF, "RST_GENERIC"),
    ("generic bf16 C1025/1088 R1", 1, 1025, 1088, BF, "RST_GENERIC"),
]


@pytest.mark.parametrize("case", RST_CASES, ids=[c[0] for c in RST_CASES])
def test_row_stats_forms(case):
    from fabind_amd import kernels as K
    name, R, C, ld, dt, form = case
    g = torch.Generator().manual_seed(R + C)
    buf = _feat(g, R, ld).to(dt)
    buf[0] = 2.5                                                       # variance 0: rs = rsqrt(eps)
    xd = _d(buf)[:, :C]
    assert K.row_stats_form(xd) == getattr(_L(), form), (name, K.row_stats_form(xd))
    h1, h2 = K.row_stats(xd, EPS), K.row_stats(xd, EPS)
    r64, r32 = NR.row_stats(NR.cast(torch.float64, buf)[:, :C], EPS), NR.row_stats(NR.cast(F32, buf)[:, :C], EPS)
    _compare("row_stats", name, list(zip(("mu", "rs"), h1, h2, r64, r32)))


def test_row_stats_table_reaches_every_form():
    L = _L()
    assert {getattr(L, c[5]) for c in RST_CASES} == set(range(L.RST_COUNT))


# ------------------------------------------------------------------------------------------------
# edge_ln_concat / edge_concat and _EdgeConcat's adjoint
# ------------------------------------------------------------------------------------------------
def _edge_lists(g, N, E):
    """Receiving nodes sorted (CSR order), self-loops, the lists' extremes present."""
    row = torch.sort(torch.randint(0, N, (E,), generator=g))[0].to(torch.int32)
    col = torch.randint(0, N, (E,), generator=g).to(torch.int32)
    col[::3] = row[::3]                                                # self-loop edges
    col[-1] = N - 1
    return row, col


CAT_CASES = [(H, E, dt) for H, E in ((4, 1), (4, 5), (20, 1), (20, 5), (20, 4097), (64, 4097), (100, 5), (512, 5), (512, 4097)) for dt in (F32, BF)]


@pytest.mark.parametrize("H,E,dt", CAT_CASES, ids=["H%d E%d %s" % (H, E, "bf16" if dt == BF else "fp32") for H, E, dt in CAT_CASES])
def test_edge_concat_and_edge_ln_concat(H, E, dt):
    from fabind_amd import kernels as K
    from fabind_amd.plus import engine as pe
    g = torch.Generator().manual_seed(H * 5 + E)
    N, C = 41, 2 * H + 1
    pad = (C + 7) // 8 * 8 + 8                                         # pad_to beyond 2H + 1
    h = _feat(g, N, H)
    row, col = _edge_lists(g, N, E)
    rh = torch.rand(E, generator=g) * 3.0
    rh[E // 2] = 0.0                                                   # an edge with rhohat = 0
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    cot = _bf_exact(torch.randn(E, pad, generator=g))
    rp = torch.zeros(N + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(torch.bincount(row.long(), minlength=N), 0).to(torch.int32)
    cs, perm = torch.sort(col.long(), stable=True)
    cp = torch.zeros(N + 1, dtype=torch.int32)
    cp[1:] = torch.cumsum(torch.bincount(cs, minlength=N), 0).to(torch.int32)
    bycol = (_d(cp), _d(perm.to(torch.int32).contiguous()))
    name = "H%d E%d" % (H, E)

    def hip():
        hd, rd = _d(h).requires_grad_(True), _d(rh).requires_grad_(True)
        yl = K.edge_ln_concat(hd.detach(), _d(row), _d(col), rd.detach(), _d(w), _d(b), dt, pad)
        y = pe._EdgeConcat.apply(hd, rd, _d(row), _d(col), _d(rp), lambda: bycol, dt, pad)
        if H % 8:                                                      # the adjoint's segment sums take H % 8 == 0: refused, not mis-summed
            with pytest.raises(RuntimeError, match="multiples of 8"):
                (y.float() * _d(cot)).sum().backward()
            return [yl, y.detach()]
        (y.float() * _d(cot)).sum().backward()
        return [yl, y.detach(), hd.grad, rd.grad]

    def ref(t):
        hr, rr = h.to(t).requires_grad_(True), rh.to(t).requires_grad_(True)
        yl = NR.edge_ln_concat(hr.detach(), row, col, rr.detach(), w.to(t), b.to(t), EPS, pad)
        y = NR.edge_concat(hr, row, col, rr, pad)
        (y * cot.to(t)).sum().backward()
        return [yl, y.detach(), hr.grad, rr.grad][:4 if H % 8 == 0 else 2]

    h1, h2, r64, r32 = hip(), hip(), ref(torch.float64), ref(F32)
    assert float(h1[0][:, C:].float().abs().max()) == 0.0 and float(h1[1][:, C:].float().abs().max()) == 0.0
    assert torch.equal(h1[1].cpu(), r64[1].to(dt))                     # the concatenation is a copy: exactly the rounded input
    _compare("edge_concat", name, list(zip(("ln_y", "y", "dh", "drho"), h1, h2, r64, r32)))


# ------------------------------------------------------------------------------------------------
# edge_lnfold forward
# ------------------------------------------------------------------------------------------------
N_NODES = 37


def _fold_operands(H, Kp, ldab, E, seed):
    """Operand-level inputs of the folded edge Linear: projections of O(1), node means around 4 with their own spread (dr, dc, dq of
    O(1): a column vector read at the wrong chunk moves the result by O(1)), centred sums of squares of features of spread 1.5."""
    g = torch.Generator().manual_seed(seed)
    AB = torch.randn(N_NODES, ldab, generator=g).bfloat16()
    stat = torch.stack([4.0 + 0.5 * torch.randn(N_NODES, generator=g), H * 2.25 * (1.0 + 0.1 * torch.randn(N_NODES, generator=g)).abs()], 1).contiguous()
    row, col = _edge_lists(g, N_NODES, E)
    rho = torch.rand(E, generator=g) * 3.0
    rho[E // 2] = 0.0
    w_r, c_r, c_c = (torch.randn(Kp, generator=g) for _ in range(3))
    dvec = torch.randn(Kp, generator=g) * 0.3
    return g, AB, stat, row, col, rho, w_r, c_r, c_c, dvec


def _elf_cases():
    """(case, H, Kp, ldab, E or None (two full sweeps of the capped grid + 3, from the launcher's cap and U), p_drop, form)."""
    from fabind_amd import kernels as K
    out = []
    for form, (H, Kp), more in (("ELF_WAVE1", (8, 24), [(128, 264, 536, 0.25), (128, 512, 1024, 0.0)]),
                                ("ELF_WAVE1_TAIL", (256, 520), [(256, 576, 1160, 0.25), (256, 520, 1048, 0.25)]),
                                ("ELF_WAVE2_TAIL", (260, 528), [(512, 1032, 2064, 0.0), (512, 1088, 2184, 0.25), (512, 1032, 2072, 0.25)])):
        _, U, cap = K.edge_lnfold_form(Kp, H)
        for E in sorted({1, max(U - 1, 1), U + 1}):
            out.append(("%s H%d Kp%d E%d" % (form[4:], H, Kp, E), H, Kp, 2 * Kp, E, 0.25 if E > 1 else 0.0, form))
        out.append(("%s H%d Kp%d two sweeps + 3" % (form[4:], H, Kp), H, Kp, 2 * Kp, 2 * cap * 4 * U + 3, 0.25 if Kp == 24 else 0.0, form))
        for H2, Kp2, ld2, p in more:
            out.append(("%s H%d Kp%d ld%d p%.2f" % (form[4:], H2, Kp2, ld2, p), H2, Kp2, ld2, 37, p, form))
    out += [("CHUNK H30 Kp64 p0.25", 30, 64, 136, 37, 0.25, "ELF_CHUNK"), ("CHUNK H516 Kp1040", 516, 1040, 2080, 5, 0.0, "ELF_CHUNK"),
            ("CHUNK H30 Kp64 E1", 30, 64, 128, 1, 0.0, "ELF_CHUNK")]
    return out


# the table reads the launcher's U and cap: host functions of the library, answered without a device
ELF_CASES = _elf_cases()


@pytest.mark.parametrize("case", ELF_CASES, ids=[c[0] for c in ELF_CASES])
def test_edge_lnfold_forward_forms(case):
    from fabind_amd import kernels as K
    name, H, Kp, ldab, E, p, form = case
    assert K.edge_lnfold_form(Kp, H)[0] == getattr(_L(), form), (name, K.edge_lnfold_form(Kp, H))
    _, AB, stat, row, col, rho, w_r, c_r, c_c, dvec = _fold_operands(H, Kp, ldab, E, seed=H + Kp + E)
    seed = 99 + E
    args = [_d(t) for t in (row, col, rho, stat)]
    vecs = [_d(t) for t in (w_r, c_r, c_c, dvec)]
    hip = lambda: K.edge_lnfold(_d(AB), Kp, H, args[0], args[1], args[2], args[3], EPS, vecs[0], vecs[1], vecs[2], vecs[3], p, seed)
    keep = NR.drop_keep(seed, E, Kp, p) if p > 0 else None
    ref = lambda dt: NR.edge_lnfold(*NR.cast(dt, AB, Kp, H, row, col, rho, stat, EPS, w_r, c_r, c_c, dvec), keep, p)
    h1, h2, r64 = hip(), hip(), ref(torch.float64)
    assert h1.shape == (E, Kp) and h1.dtype == BF
    if keep is not None:                                               # every dropped position is an exact zero (the kept ones: by value below)
        assert not bool((h1.cpu() != 0)[~keep].any())
    _compare("edge_lnfold", name, [("out", h1, h2, r64, ref(F32))])


def test_edge_lnfold_table_reaches_every_form():
    L = _L()
    assert {getattr(L, c[6]) for c in ELF_CASES} == set(range(L.ELF_COUNT))
    assert all(any(c[6] == f and c[0].endswith("two sweeps + 3") for c in ELF_CASES) for f in ("ELF_WAVE1", "ELF_WAVE1_TAIL", "ELF_WAVE2_TAIL"))


# ------------------------------------------------------------------------------------------------
# edge_lnfold adjoint
# ------------------------------------------------------------------------------------------------
# (H, Kp) per form, smaller Kp first: the second runs through the same instantiation with a larger dynamic-LDS request
ELB_SHAPES = {"ELB_NPL1": [(8, 24), (250, 512)], "ELB_NPL2": [(256, 520), (500, 1024)], "ELB_NPL3": [(512, 1032), (512, 1088)]}


def _elb_check(name, H, Kp, ldab, E, p, form):
    from fabind_amd import kernels as K
    assert K.edge_lnfold_bwd_form(Kp)[0] == getattr(_L(), form), (name, K.edge_lnfold_bwd_form(Kp))
    g, AB, stat, row, col, rho, w_r, c_r, c_c, dvec = _fold_operands(H, Kp, ldab, E, seed=H + Kp + E + 1)
    keep = NR.drop_keep(1234 + E, E, Kp, p) if p > 0 else None
    ops64 = NR.cast(torch.float64, AB, Kp, H, row, col, rho, stat, EPS, w_r, c_r, c_c)
    out = NR.edge_lnfold(*ops64, dvec.double(), keep, p).bfloat16()    # the saved output: the float64 forward rounded to bf16
    dout = torch.randn(E, Kp, generator=g).bfloat16()
    frac = float((out != 0).float().mean())
    assert (0.15 < frac < 0.85) or E * Kp < 200, frac
    dev = [_d(t) for t in (AB, row, col, rho, stat, w_r, c_r, c_c, out, dout)]
    hip = lambda: list(K.edge_lnfold_bwd(dev[0], Kp, H, dev[1], dev[2], dev[3], dev[4], EPS, dev[5], dev[6], dev[7], dev[8], dev[9], p))
    ref = lambda dt: list(NR.edge_lnfold_bwd(*NR.cast(dt, AB, Kp, H, row, col, rho, stat, EPS, w_r, c_r, c_c, out, dout), p))
    h1, h2, r64, r32 = hip(), hip(), ref(torch.float64), ref(F32)
    assert h1[1].shape == (E, 8) and float(h1[1][:, 4:].abs().max()) == 0.0
    h1[1], h2[1] = h1[1][:, :4].contiguous(), h2[1][:, :4].contiguous()
    _compare("edge_lnfold_bwd", name, list(zip(("du", "es", "drho", "vecs"), h1, h2, r64, r32)))


def _elb_cases():
    from fabind_amd import kernels as K
    out = []
    for form, ((H, Kp), (H2, Kp2)) in ELB_SHAPES.items():
        _, U, cap = K.edge_lnfold_bwd_form(Kp)
        for E in sorted({1, max(U - 1, 1), U + 1}):
            out.append(("%s Kp%d E%d" % (form[4:], Kp, E), H, Kp, 2 * Kp + 8, E, 0.0 if E == 1 else 0.25, form))
        out.append(("%s Kp%d two sweeps + 3" % (form[4:], Kp), H, Kp, 2 * Kp, 2 * cap * 4 * U + 3, 0.25 if Kp == 24 else 0.0, form))
        out.append(("%s Kp%d E37 p0.25" % (form[4:], Kp2), H2, Kp2, 2 * Kp2, 37, 0.25, form))
    return out


ELB_CASES = _elb_cases()


@pytest.mark.parametrize("case", ELB_CASES, ids=[c[0] for c in ELB_CASES])
def test_edge_lnfold_bwd_forms(case):
    _elb_check(*case)


@pytest.mark.parametrize("form", list(ELB_SHAPES))
def test_edge_lnfold_bwd_larger_kp_second_through_the_same_instantiation(form):
    """The dynamic-LDS allowance of an instantiation is set once per process and device: a small Kp first, the instantiation's larger
    Kp after it, then the small one again, in one process."""
    (H, Kp), (H2, Kp2) = ELB_SHAPES[form]
    _elb_check("%s Kp%d first" % (form[4:], Kp), H, Kp, 2 * Kp, 9, 0.0, form)
    _elb_check("%s Kp%d second" % (form[4:], Kp2), H2, Kp2, 2 * Kp2 + 16, 9, 0.0, form)
    _elb_check("%s Kp%d third" % (form[4:], Kp), H, Kp, 2 * Kp, 9, 0.25, form)


def test_edge_lnfold_bwd_table_reaches_every_form():
    L = _L()
    assert {getattr(L, c[6]) for c in ELB_CASES} == set(range(L.ELB_COUNT))
    assert {c[2] for c in ELB_CASES} == {24, 512, 520, 1024, 1032, 1088}
    assert all(any(c[6] == f and c[0].endswith("two sweeps + 3") for c in ELB_CASES) for f in ELB_SHAPES)


# ------------------------------------------------------------------------------------------------
# inter_coord_fold
# ------------------------------------------------------------------------------------------------
ICF_CASES = [(8, 1, 0.0, 8), (8, 5, 0.25, 16), (8, None, 0.25, 8), (72, 5, 0.0, 80), (72, 37, 0.25, 72), (128, 1, 0.25, 128), (128, 37, 0.0, 136),
             (512, 5, 0.25, 520), (512, 37, 0.0, 512)]


@pytest.mark.parametrize("H,E,p,ldp", ICF_CASES, ids=["H%d E%s p%.2f ld%d" % (H, E or "two-sweeps", p, ld) for H, E, p, ld in ICF_CASES])
def test_inter_coord_fold(H, E, p, ldp):
    from fabind_amd import kernels as K
    if E is None:
        E = 2 * K.inter_coord_fold_blocks() * 4 + 3                    # two full sweeps of the capped grid (one edge per wave and trip) + 3
        assert K.inter_coord_fold_blocks(E) == K.inter_coord_fold_blocks()
    g = torch.Generator().manual_seed(H * 3 + E)
    N = N_NODES
    P = torch.randn(N, ldp, generator=g).bfloat16()
    wc = torch.randn(H, generator=g) * 0.5
    Vc = torch.randn(N, H, generator=g) * 1.5
    stat = torch.stack([(Vc * Vc).sum(1), Vc @ wc], 1).contiguous()     # (|Vc|^2, Vc . wc) of consistent vectors: the quadratic form is >= 0
    q_w = float(torch.tensor(float((wc * wc).sum()), dtype=F32))        # (a float argument crosses the C interface as fp32)
    col = torch.randint(0, N, (E,), generator=g).to(torch.int32)
    rho = torch.rand(E, generator=g) * 3.0
    rho[E // 2] = 0.0
    u, d, w3 = torch.randn(H, generator=g), torch.randn(H, generator=g) * 0.3, torch.randn(H, generator=g)
    seed = 4242 + E
    dv = [_d(t) for t in (P, col, rho, stat, u, d, w3)]
    hip = lambda: K.inter_coord_fold(dv[0], H, dv[1], dv[2], dv[3], q_w, EPS, dv[4], dv[5], dv[6], p, seed)
    keep = NR.drop_keep(seed, E, H, p) if p > 0 else None
    ref = lambda dt: NR.inter_coord_fold(*NR.cast(dt, P, H, col, rho, stat, q_w, EPS, u, d, w3), keep, p)
    _compare("inter_coord_fold", "H%d E%d p%.2f ld%d" % (H, E, p, ldp), [("s", hip(), hip(), ref(torch.float64), ref(F32))])
