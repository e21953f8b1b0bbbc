"""CPU: the restatements of tests/norm_refs.py pinned to what they restate -- the folded forms to the unfolded LayerNorm -> Linear
forms (the algebra, float64, operands not rounded), the adjoint of the folded edge Linear to torch autograd through its forward, and
the counter-based dropout mask to its literal; and the form report of csrc/norm.hip answered without a device."""
import ctypes

import pytest
import torch

import norm_refs as NR

EPS = 1e-5


def _edge_problem(H, Kp, N=23, E=157, seed=0):
    g = torch.Generator().manual_seed(1000 * H + seed)
    Cn = 2 * H + 1
    h = torch.randn(N, H, generator=g, dtype=torch.float64) * 1.5 + 4.0
    row = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    col = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    col[:3] = row[:3]                                                   # self-loops
    rho = torch.rand(E, generator=g, dtype=torch.float64) * 3.0
    rho[3] = 0.0
    ln_w = torch.rand(Cn, generator=g, dtype=torch.float64) + 0.5
    ln_b = torch.randn(Cn, generator=g, dtype=torch.float64) * 0.2
    W1 = torch.randn(Cn, Cn, generator=g, dtype=torch.float64) / Cn ** 0.5
    b1 = torch.randn(Cn, generator=g, dtype=torch.float64) * 0.3
    return g, h, row, col, rho, ln_w, ln_b, W1, b1


@pytest.mark.parametrize("H,Kp", [(4, 16), (30, 64), (64, 136), (130, 264)])
def test_folded_edge_linear_equals_layernorm_then_linear_in_float64(H, Kp):
    """relu(W1 LN([h_r | h_c | rho]) + b1) == edge_lnfold of the composed operands, to 1e-12 of the largest entry; padding columns zero."""
    _, h, row, col, rho, ln_w, ln_b, W1, b1 = _edge_problem(H, Kp)
    Cn = 2 * H + 1
    ref = NR.edge_mlp_unfolded(h, row, col, rho, ln_w, ln_b, W1, b1, EPS)
    f = NR.fold_edge(h, ln_w, ln_b, W1, b1, Kp)
    out = NR.edge_lnfold(f["AB"], Kp, H, row, col, rho, f["stat"], EPS, f["w_r"], f["c_r"], f["c_c"], f["dvec"])
    assert out.shape == (row.numel(), Kp) and float(out[:, Cn:].abs().max()) == 0.0
    assert float(ref.abs().max()) > 1.0
    assert float((out[:, :Cn] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("H", [8, 72, 130])
def test_folded_inter_coord_mlp_equals_layernorm_mlp_in_float64(H):
    g = torch.Generator().manual_seed(H)
    N, E = 19, 143
    V = torch.randn(N, H, generator=g, dtype=torch.float64) * 1.5 + 4.0
    w_rv = torch.randn(H, generator=g, dtype=torch.float64) * 0.5 + 0.3
    col = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    rho = torch.rand(E, generator=g, dtype=torch.float64) * 3.0
    rho[0] = 0.0
    ln_w, ln_b = torch.rand(H, generator=g, dtype=torch.float64) + 0.5, torch.randn(H, generator=g, dtype=torch.float64) * 0.2
    W1, b1 = torch.randn(H, H, generator=g, dtype=torch.float64) / H ** 0.5, torch.randn(H, generator=g, dtype=torch.float64) * 0.3
    w3 = torch.randn(H, generator=g, dtype=torch.float64)
    ref = NR.inter_coord_unfolded(V, col, rho, w_rv, ln_w, ln_b, W1, b1, w3, EPS)
    f = NR.fold_inter(V, w_rv, ln_w, ln_b, W1, b1)
    s = NR.inter_coord_fold(f["P"], H, col, rho, f["stat"], f["q_w"], EPS, f["u"], f["d"], w3)
    assert float((s - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_layer_norm_restatements_equal_torch_layer_norm_in_float64():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 37, generator=g, dtype=torch.float64) * 1.5 + 4.0
    w, b = torch.randn(37, generator=g, dtype=torch.float64), torch.randn(37, generator=g, dtype=torch.float64)
    y = NR.layer_norm_rows(x, w, b, EPS, 40)
    ref = torch.nn.functional.layer_norm(x, (37,), w, b, EPS)
    assert y.shape == (7, 40) and float(y[:, 37:].abs().max()) == 0.0
    assert float((y[:, :37] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    mu, rs = NR.row_stats(x, EPS)
    assert torch.allclose(mu, x.mean(1), rtol=0, atol=1e-13) and torch.allclose(rs, torch.rsqrt(x.var(1, unbiased=False) + EPS), rtol=1e-13)
    h = x[:, :9].contiguous()
    row, col = torch.tensor([0, 3, 6, 2], dtype=torch.int32), torch.tensor([1, 3, 0, 5], dtype=torch.int32)
    rh = torch.tensor([0.3, 0.0, 1.5, 2.0], dtype=torch.float64)
    cat = NR.edge_concat(h, row, col, rh, 24)
    assert cat.shape == (4, 24) and torch.equal(cat[:, :9], h[row.long()]) and torch.equal(cat[:, 9:18], h[col.long()])
    assert torch.equal(cat[:, 18], rh) and float(cat[:, 19:].abs().max()) == 0.0
    yl = NR.edge_ln_concat(h, row, col, rh, w[:19], b[:19], EPS, 24)
    ref = torch.nn.functional.layer_norm(cat[:, :19], (19,), w[:19], b[:19], EPS)
    assert float((yl[:, :19] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()) and float(yl[:, 19:].abs().max()) == 0.0


@pytest.mark.parametrize("H,Kp,p", [(4, 16, 0.0), (30, 64, 0.25), (64, 136, 0.25)])
def test_edge_lnfold_bwd_equals_autograd_through_edge_lnfold_in_float64(H, Kp, p):
    """The adjoint restated from the kernel's comment block against autograd through the forward restatement, with a fixed mask:
    the gradient of AB (du scattered to the receiving node for the A half and to the sending node for the B half), of stat (es
    scattered likewise), rho, dvec, c_r, c_c and w_r, each to 1e-10 of its largest entry."""
    g, h, row, col, rho, ln_w, ln_b, W1, b1 = _edge_problem(H, Kp, seed=1)
    f = NR.fold_edge(h, ln_w, ln_b, W1, b1, Kp)
    E, N = row.numel(), h.shape[0]
    keep = NR.drop_keep(77, E, Kp, p) if p > 0 else None
    leaves = [f[k].clone().requires_grad_(True) for k in ("AB", "stat", "w_r", "c_r", "c_c", "dvec")] + [rho.clone().requires_grad_(True)]
    AB, stat, w_r, c_r, c_c, dvec, rho_l = leaves
    out = NR.edge_lnfold(AB, Kp, H, row, col, rho_l, stat, EPS, w_r, c_r, c_c, dvec, keep, p)
    dout = torch.randn(E, Kp, generator=g, dtype=torch.float64)
    (out * dout).sum().backward()
    with torch.no_grad():
        du, es, drho, vecs = NR.edge_lnfold_bwd(AB, Kp, H, row, col, rho_l, stat, EPS, w_r, c_r, c_c, out, dout, p)
    r, c = row.long(), col.long()
    dAB = torch.zeros(N, 2 * Kp, dtype=torch.float64)
    dAB[:, :Kp].index_add_(0, r, du)
    dAB[:, Kp:].index_add_(0, c, du)
    dstat = torch.zeros(N, 2, dtype=torch.float64)
    dstat.index_add_(0, r, es[:, 0:2])
    dstat.index_add_(0, c, es[:, 2:4])
    assert 0.2 < float((out.detach() != 0).double().mean()) < 0.8           # the mask is neither empty nor full
    for name, got, want in (("AB", dAB, AB.grad), ("stat", dstat, stat.grad), ("rho", drho, rho_l.grad), ("dvec", vecs[0], dvec.grad),
                            ("c_r", vecs[1], c_r.grad), ("c_c", vecs[2], c_c.grad), ("w_r", vecs[3], w_r.grad)):
        assert float(want.abs().max()) > 0
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max()), name


def test_drop_keep_is_the_counter_hash_and_keeps_the_stated_share():
    seed, E, H, p = 4242, 37, 24, 0.2
    thr = int(p * 65536.0 + 0.5)
    e = torch.arange(E, dtype=torch.int64)[:, None]; c = torch.arange(H, dtype=torch.int64)[None, :]
    x = (seed + e * H + c) & 0xFFFFFFFF
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & 0xFFFFFFFF
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    assert torch.equal(NR.drop_keep(seed, E, H, p), (x & 0xFFFF) >= thr)
    # 32-bit wrap-around of the counter: a seed near 2^32 equals the wrapped counter hashed directly
    k = NR.drop_keep(0xFFFFFFF0, 3, 16, 0.5)
    assert torch.equal(k, (NR.hash32((0xFFFFFFF0 + torch.arange(48, dtype=torch.int64)) & 0xFFFFFFFF).view(3, 16) & 0xFFFF) >= 32768)
    assert bool(NR.drop_keep(1, 5, 8, 0.0).all())
    n = 2 ** 20
    q = 1.0 - round(0.25 * 65536) / 65536.0
    assert NR.drop_thr(0.25) == round(0.25 * 65536)
    rate = float(NR.drop_keep(99, n // 1024, 1024, 0.25).double().mean())
    assert abs(rate - q) <= 4.0 * (q * (1.0 - q) / n) ** 0.5, (rate, q)


def test_bf16_excess_accepts_round_to_nearest_and_refuses_the_next_bf16_value():
    """The bf16 rule of the GPU tests on the host: the round-to-nearest-even bf16 of the fp32 rounding of r passes with A = one fp32
    rounding of the largest entry; the neighbouring bf16 value on the far side does not.  bf16 keeps 8 significand bits, so its unit
    roundoff is 2^-8: the same correctly rounded values miss 2^-9 |r| + (1 + 2^-9) A (the half-ulp's lower envelope) by up to 2^-9 |r|."""
    g = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=g, dtype=torch.float64) * 3.0
    A = 2.0 ** -24 * float(r.abs().max())
    rne = r.float().bfloat16()
    assert NR.bf16_excess(rne, r, A) <= 0.0
    assert torch.equal(NR.bf16_half_ulp(torch.tensor([1.0, 1.99, 2.0, 6.9, 0.75])), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9], dtype=torch.float64))
    lit = NR.bf16_excess_literal(rne, r, A)
    assert 0.0 < lit <= 2.0 ** -9 * float(r.abs().max())
    away = rne.double() + torch.sign(rne.double() - r) * 2 * NR.bf16_half_ulp(rne.double())       # one bf16 step further from r
    sel = (rne.double() - r).abs() > 0.1 * NR.bf16_half_ulp(r)                                       # (where the step's direction is defined)
    for i in torch.nonzero(sel).flatten()[:64]:
        one = rne.double().clone()
        one[i] = away[i]
        assert NR.bf16_excess(one, r, A) > 0.0


def test_norm_form_report_runs_without_a_device():
    """The form functions are host code: they answer from sizes, dtypes and addresses (never dereferenced).  Every boundary of the five
    ladders, and every declared form id reached."""
    from fabind_amd import _lib as L
    lib = L.load()
    a16, odd = 0x10000, 0x10004
    rows = lambda C, ld=None, pad=None, x=a16, y=a16: lib.fabind_layernorm_rows_form(x, ld or C, C, y, pad or ld or C, pad or ld or C)
    got = {(C,): rows(C) for C in (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 1536, 1544, 2048)}
    assert list(got.values()) == [L.LNR_8S16, L.LNR_8S16, L.LNR_8S32, L.LNR_8S32, L.LNR_V8_1, L.LNR_V8_1, L.LNR_V8_2, L.LNR_V8_2, L.LNR_V8_3,
                                  L.LNR_V8_3, L.LNR_V8_4, L.LNR_V8_4]
    assert [rows(C, x=odd) for C in (128, 136, 512, 520, 1024, 1032, 2048)] == [L.LNR_S2, L.LNR_S8, L.LNR_S8, L.LNR_S16, L.LNR_S16, L.LNR_S32, L.LNR_S32]
    assert rows(100, 104) == L.LNR_8S16 and rows(100, 100) == L.LNR_S2 and rows(1025, 1088) == L.LNR_V8_3 and rows(64, y=odd) == L.LNR_S2
    assert lib.fabind_layernorm_rows_form(a16, 104, 100, a16, 100, 100) == L.LNR_S2          # pad_to < C rounded up to 8
    bwd = lambda C, ld=None, x=a16, dy=a16, dx=a16: lib.fabind_layernorm_rows_bwd_form(x, ld or C, dy, ld or C, dx, ld or C, C)
    assert [bwd(C) for C in (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 1536, 1544, 2048)] == \
        [L.LNB_8S16, L.LNB_8S16, L.LNB_8S32, L.LNB_8S32, L.LNB_V8_1, L.LNB_V8_1, L.LNB_V8_2, L.LNB_V8_2, L.LNB_V8_3, L.LNB_V8_3, L.LNB_S32, L.LNB_S32]
    assert [bwd(C, dy=odd) for C in (128, 136, 512, 520, 1024, 1032, 1280, 1288)] == \
        [L.LNB_S2, L.LNB_S8, L.LNB_S8, L.LNB_S16, L.LNB_S16, L.LNB_S20, L.LNB_S20, L.LNB_S32]
    assert bwd(36) == L.LNB_S2 and bwd(64, x=odd) == L.LNB_S2 and bwd(64, dx=odd) == L.LNB_S2
    st = lambda C, dt=L.DT_BF16, ld=None, x=a16: lib.fabind_row_stats_form(x, dt, ld or C, C)
    assert [st(C) for C in (8, 512, 520, 1024, 1032, 2048)] == [L.RST_BF16_1, L.RST_BF16_1, L.RST_BF16_2, L.RST_BF16_2, L.RST_BF16_4, L.RST_BF16_4]
    assert st(512, L.DT_F32) == st(100) == st(512, x=odd) == st(512, ld=516) == st(2056) == L.RST_GENERIC
    u = ctypes.c_int(-1)
    fwd = lambda Kp, H: (lib.fabind_edge_lnfold_form(Kp, H, ctypes.byref(u)), u.value)
    f1, u1 = fwd(24, 8)
    f1t, u1t = fwd(520, 256)
    f2t, u2t = fwd(528, 260)
    assert (f1, f1t, f2t) == (L.ELF_WAVE1, L.ELF_WAVE1_TAIL, L.ELF_WAVE2_TAIL) and u1 == u1t and u1 >= 1 and u2t >= 1
    assert fwd(264, 128)[0] == L.ELF_WAVE1 and fwd(512, 128)[0] == L.ELF_WAVE1 and fwd(576, 256)[0] == L.ELF_WAVE1_TAIL
    assert fwd(1032, 512)[0] == fwd(1088, 512)[0] == L.ELF_WAVE2_TAIL
    assert fwd(64, 30) == (L.ELF_CHUNK, 0) and fwd(1040, 516) == (L.ELF_CHUNK, 0) and fwd(1048, 128)[0] == L.ELF_CHUNK      # a tail beyond 64 chunks
    assert lib.fabind_edge_lnfold_form(24, 8, None) == L.ELF_WAVE1
    b = lambda Kp: (lib.fabind_edge_lnfold_bwd_form(Kp, ctypes.byref(u)), u.value)
    assert [b(Kp)[0] for Kp in (24, 512, 520, 1024, 1032, 1088, 1536)] == [L.ELB_NPL1, L.ELB_NPL1, L.ELB_NPL2, L.ELB_NPL2, L.ELB_NPL3, L.ELB_NPL3, L.ELB_NPL3]
    assert all(b(Kp)[1] >= 1 for Kp in (24, 520, 1032))
    for blocks in (lib.fabind_edge_lnfold_blocks, lib.fabind_edge_lnfold_bwd_blocks, lib.fabind_inter_coord_fold_blocks):
        cap = blocks(2 ** 31 - 1)
        assert blocks(1) == 1 and blocks(5) == 2 and blocks(4 * cap) == cap and blocks(4 * cap + 1) == cap and cap >= 256
