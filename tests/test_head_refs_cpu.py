"""CPU: the restatements of tests/head_refs.py against float64 torch autograd of the reference formulas quoted in
tests/test_gpu_heads.py (ref_center, ref_loss, cdist-clamp, the einsum product) and against the oracle's statement of the loss
and of the centre, the case tables of tests/test_gpu_head_forms.py against the classes they claim to reach (computed from the kernels' own
constants, restated in head_refs.py with the lines they come from), the exactness of the float64 product, and the host side of
ops.PairBlocks for complexes without atoms or without residues."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import head_refs as HR
import reduce_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def _src(name):
    with open(os.path.join(ROOT, "fabind_amd", "csrc", name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------
# the constants the tables are built on are the sources'
# ------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    heads, attn, bwd = _src("heads.hip"), _src("attn.hip"), _src("bwd.hip")
    assert int(re.search(r"constexpr int PB_TP = (\d+);", heads).group(1)) == HR.TP
    assert int(re.search(r"constexpr int PB_CH = (\d+);", heads).group(1)) == HR.CH
    assert "constexpr int LOSS_THREADS = 256;" in heads and "(n + LOSS_THREADS * 8 - 1) / (LOSS_THREADS * 8)" in heads
    assert "b > 1024 ? 1024 : b" in heads and "b += 64" in heads                      # the cap; the finaliser's 64-lane stride
    assert "constexpr int CT = W / 8, RP = 256 / CT;" in heads and "constexpr int CT = W / 2, NL = 256 / CT;" in heads
    assert "const int nl = 256 / cw" in heads and "i += 8 * nl" in heads              # pair_dist_bwd: protein lanes, eight strides
    assert "const int lp = widest <= 64 ? 16 : widest <= 128 ? 32 : 64;" in attn and "const int per_block = 4 * (64 / lp);" in attn
    assert "const int LPR = W / 4;" in bwd and "const int G = 64 / LPR" in bwd and "if (LPR >= 64)" in bwd
    assert "W == 64 || W == 128 || W == 256 || W == 512" in heads and HR.BLOCK_WS == (64, 128, 256, 512)


# ------------------------------------------------------------------------------------------------
# restatements against float64 autograd of the reference formulas
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HR.PAIR_DIST_CASES, ids=[c["name"] for c in HR.PAIR_DIST_CASES])
def test_pair_dist_is_cdist_clamp_and_its_autograd(case):
    xp, xc, dy, pi, ci = HR.pair_dist_operands(case)
    lo, hi, sc = case["lo"], HR.PAIR_DIST_HI, HR.PAIR_DIST_SCALE
    a = xc.double().requires_grad_()
    # cdist per complex, [z_mask] = the block in protein-major order
    ys, p0, c0 = [], 0, 0
    for P, C in zip(case["kcnt"], case["ncnt"]):
        # (a - b).norm, not torch.cdist: cdist's backward at a zero distance is its own convention
        ys.append((sc * (xp.double()[p0:p0 + P, None, :] - a[None, c0:c0 + C, :]).norm(dim=-1)).clamp(lo, hi).reshape(-1))
        p0, c0 = p0 + P, c0 + C
    ref = torch.cat(ys) if ys else a.new_zeros(0)
    got = HR.pair_dist(xp.double(), xc.double(), pi, ci, sc, lo, hi)
    assert (got - ref.detach()).abs().max() <= 1e-13 if got.numel() else True
    (ref * dy.double()).sum().backward()
    g = HR.pair_dist_grad(xp.double(), xc.double(), pi, ci, dy.double(), sc, lo, hi)
    assert bool(torch.isfinite(g).all())
    assert (a.grad.nan_to_num() - g).abs().max() <= 1e-12 if g.numel() else True
    # every pair that is not planted stays clear of both clamp corners, in float64 and float32 alike
    v = sc * (xp.double()[pi] - xc.double()[ci]).norm(dim=-1)
    planted = (v == hi) | (v == 0)
    assert float(((v - hi).abs()[~planted]).min()) > 1e-4 if (~planted).any() else True
    assert float(((v - lo).abs()[~planted]).min()) > 1e-4 if (~planted).any() else True


def test_pair_dist_table_reaches_every_class():
    cases = HR.PAIR_DIST_CASES
    Ps = {P for c in cases for P in c["kcnt"]}
    Cs = {C for c in cases for C in c["ncnt"]}
    assert set(HR.P_CLASSES) <= Ps and set(HR.C_CLASSES) <= Cs
    assert {len(c["kcnt"]) for c in cases} >= {1, 2, 3, 5}
    pos = set()
    for c in cases:
        k = c["kcnt"]
        if len(k) >= 3:
            pos |= {("first" if i == 0 else "last" if i == len(k) - 1 else "middle") for i, P in enumerate(k) if P == 0}
    assert pos == {"first", "middle", "last"}                                           # pb_find with a tile-less complex anywhere
    assert any(len(set(c["ncnt"])) > 1 and max(c["ncnt"]) > min(x for x in c["ncnt"]) for c in cases)       # max_C above a complex's own
    assert any(0 < P < 8 and C > 0 for c in cases for P, C in zip(c["kcnt"], c["ncnt"]))                    # strides without a protein
    # pair_dist_bwd lanes: nl = 256 / cw with idle threads (3, 129), cw == 256 (nl 1), a second chunk (C 257: cw 1, nl 256)
    live = {C for c in cases for P, C in zip(c["kcnt"], c["ncnt"]) if P > 0}
    assert {3, 129, 256, 257} <= live and 256 % 3 and 256 % 129
    assert any(P > 0 and C == 0 for c in cases for P, C in zip(c["kcnt"], c["ncnt"]))
    found = dict(zero=False, hi=False, lo=False, hi_clamped=False)
    for c in cases:
        xp, xc, dy, pi, ci = HR.pair_dist_operands(c)
        v = HR.PAIR_DIST_SCALE * (xp.double()[pi] - xc.double()[ci]).norm(dim=-1)
        v32 = HR.PAIR_DIST_SCALE * ((xp[pi] - xc[ci]) ** 2).sum(1).sqrt()
        found["zero"] |= bool((v == 0).any())
        found["hi"] |= bool((v == HR.PAIR_DIST_HI).any() and (v32 == HR.PAIR_DIST_HI).any())
        found["hi_clamped"] |= bool((v > HR.PAIR_DIST_HI).any())
        found["lo"] |= c["lo"] > 0 and bool(((v > 0) & (v < c["lo"])).any())
    assert all(found.values()), found


@pytest.mark.parametrize("W", [4, 64])
def test_hadamard_adjoint_is_autograd_of_the_einsum(W):
    g = torch.Generator().manual_seed(W)
    kcnt, ncnt = [3, 0, 2], [2, 4, 5]
    npk = sum(kcnt)
    pi, ci = HR.block_index(kcnt, ncnt)
    t = torch.randn(npk + sum(ncnt), W, generator=g, dtype=F64).requires_grad_()
    # einsum('bik,bjk->bijk') per complex, flattened protein-major = [z_mask] of the padded tensor
    outs, p0, c0 = [], 0, npk
    for P, C in zip(kcnt, ncnt):
        outs.append(torch.einsum("ik,jk->ijk", t[p0:p0 + P], t[c0:c0 + C]).reshape(-1, W))
        p0, c0 = p0 + P, c0 + C
    ref = torch.cat(outs)
    got = HR.hadamard_blocks(t.detach(), pi, npk + ci)
    assert torch.equal(got, ref.detach())
    dout = torch.randn(ref.shape, generator=g, dtype=F64)
    ref.backward(dout)
    assert (t.grad - HR.hadamard_blocks_grad(t.detach(), pi, npk + ci, dout)).abs().max() <= 1e-13
    # a self pair and an unsorted list
    ia, ib = HR.rows_pairs(False)
    t2 = torch.randn(HR.ROWS_N, W, generator=g, dtype=F64).requires_grad_()
    d2 = torch.randn(ia.numel(), W, generator=g, dtype=F64)
    (t2[ia] * t2[ib]).backward(d2)
    assert (t2.grad - HR.hadamard_blocks_grad(t2.detach(), ia, ib, d2)).abs().max() <= 1e-12


@pytest.mark.parametrize("H,H2", [(8, 0), (8, 4)])
def test_pair_hadamard_adjoint_and_bmat_are_autograd(H, H2):
    g = torch.Generator().manual_seed(H + H2)
    G = HR.inter_graph()
    n = G["n"]
    T0 = torch.randn(n, 2 * H, generator=g, dtype=F64).requires_grad_()
    T1 = torch.randn(n, 2 * H2, generator=g, dtype=F64).requires_grad_()
    hd = HR.pair_hadamard(T0, H, T1, H2, G["red_p"], G["red_c"])
    dhd = torch.randn(hd.shape, generator=g, dtype=F64)
    hd.backward(dhd)
    d0i, d1i = torch.randn(n, 2 * H, generator=g, dtype=F64), torch.randn(n, 2 * H2, generator=g, dtype=F64)
    d0, d1 = HR.pair_hadamard_grad(T0.detach(), H, T1.detach(), H2, G["red_p"], G["red_c"], dhd, d0i, d1i)
    assert (d0 - d0i - T0.grad).abs().max() <= 1e-12
    assert (d1 - d1i - (T1.grad if H2 else 0)).abs().max() <= 1e-12 if H2 else d1.numel() == 0
    # the row walk of the inter graph visits exactly the pairs, each from both of its ends, in pair order
    rows = RR.CR.rows_of(G["rp"])
    assert sorted(G["red_idx"].tolist()) == sorted(list(range(G["red_p"].numel())) * 2)
    for e in range(rows.numel()):
        pr = int(G["red_idx"][e])
        assert {int(rows[e]), int(G["col"][e])} == {int(G["red_p"][pr]), int(G["red_c"][pr])}
    b0, wc = torch.randn(5, H, generator=g, dtype=F64), torch.randn(3, H, generator=g, dtype=F64)
    cn = torch.tensor([4, 0, 4])
    bm = HR.pair_bmat(b0, wc, cn)
    assert bm.shape == (9, H) and torch.equal(bm[2 * 3 + 1], b0[4] * wc[1]) and torch.equal(bm[1 * 3 + 2], b0[0] * wc[2])


def _ref_loss(coords, y_pred, y_by, logits, center, coords_true, dis_map, cls, mask, center_true, w):
    terms = dict(
        pocket_cls=w['cls'] * F.binary_cross_entropy_with_logits(logits, cls.to(logits.dtype)) * (mask.numel() / mask.sum().to(logits.dtype)),      # (int / int64 tensor would round the quotient to float32)
        pocket_center=w['center'] * F.huber_loss(center, center_true, delta=w['delta']),
        contact=w['pair'] * F.mse_loss(y_pred, dis_map), contact_by_pred=w['pair'] * F.mse_loss(y_by, dis_map),
        distill=w['distill'] * F.mse_loss(y_by, y_pred), coord=w['coord'] * F.smooth_l1_loss(coords, coords_true))
    return sum(terms.values()), terms


@pytest.mark.parametrize("case", [c for c in HR.LOSS_CASES if c["n_pair"] <= 2049], ids=lambda c: c["name"])
def test_six_term_loss_and_seeds_are_the_reference_formulas(case):
    t = HR.loss_operands(case)
    gl, gt = HR.loss_upstream(case)
    dbl = [x.double() if x.is_floating_point() else x for x in t]
    total, terms = HR.six_term_loss(*dbl, HR.LOSS_W)
    seeds = HR.six_term_loss_grad(*dbl, HR.LOSS_W, gl, gt)
    if case["n_pair"] == 0:
        assert float(terms[2]) == 0.0 and float(terms[3]) == 0.0 and float(terms[4]) == 0.0          # the empty terms are 0, not NaN
        assert seeds[1].numel() == 0 and seeds[2].numel() == 0
        dbl[1] = dbl[2] = dbl[6] = torch.zeros(1, dtype=F64)                                         # (torch's own formula needs an element)
    leaves = [x.clone().requires_grad_() for x in dbl[:5]]
    l_ref, t_ref = _ref_loss(*leaves, *dbl[5:], HR.LOSS_W)
    tr = torch.stack([t_ref[k] for k in HR.LOSS_TERMS])
    assert (terms - tr.detach()).abs().max() <= 1e-12 * max(1.0, float(tr.detach().abs().max()))
    assert abs(float(total) - float(l_ref.detach())) <= 1e-12 * max(1.0, abs(float(l_ref.detach())))
    # the oracle's statement of the same loss (its total adds the terms in another order)
    import types
    import fabind_oracle as orc
    wo = dict(HR.LOSS_W, huber_delta=HR.LOSS_W["delta"])
    out = (dbl[0], None, dbl[1], dbl[2], dbl[3], dbl[7], dbl[8], None, dbl[4], dbl[6], None)
    l_orc, t_orc = orc.compute_loss(out, types.SimpleNamespace(coords_center=dbl[9], coords=dbl[5]), wo)
    # (the oracle forms numel / sum(mask) as a float32 tensor: the class term, and the total with it, agree to that rounding)
    assert abs(float(l_orc) - float(total)) <= 2.0 ** -23 * max(1.0, abs(float(total)))
    assert all(abs(float(t_orc[k]) - float(terms[i])) <= (2.0 ** -23 if i == 0 else 1e-12) * max(1.0, abs(float(terms[i])))
               for i, k in enumerate(HR.LOSS_TERMS))
    up = (gl.double() * l_ref if gl is not None else 0) + ((gt.double() * tr).sum() if gt is not None else 0)
    up.backward()
    for k, (a, b) in enumerate(zip(seeds, leaves)):
        if case["n_pair"] == 0 and k in (1, 2):
            continue
        assert (a - b.grad).abs().max() <= 1e-12 * max(1.0, float(b.grad.abs().max())), k


def test_loss_table_reaches_every_class():
    cases = HR.LOSS_CASES
    assert [c["n_pair"] for c in cases][:7] == [0, 1, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 2 ** 21 + 1]
    nblk = [HR.loss_blocks(c["n_pair"], c["n_atoms"] * 3, c["B"] * c["L"]) for c in cases]
    assert nblk[:7] == [1, 1, 1, 2, 64, 65, 1024]                                       # one wave pass, the second pass of one lane, the cap
    assert 2 ** 21 + 1 > 1024 * 2048
    assert {c["cls_dt"] for c in cases} == {torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool}
    assert {c["g"] for c in cases} == {"total", "terms", "both"}
    pick = lambda c: (c["n_pair"], c["n_atoms"] * 3, c["B"] * c["L"])
    assert any(p[1] > p[0] and p[1] > p[2] and HR.loss_blocks(*p) > HR.loss_blocks(p[0], 0, 0) for p in map(pick, cases))
    assert any(p[2] > p[0] and p[2] > p[1] and HR.loss_blocks(*p) > HR.loss_blocks(p[0], 0, 0) for p in map(pick, cases))
    for c in cases:
        if c["n_atoms"] >= 40:
            t = HR.loss_operands(c)
            d = (t[0] - t[5]).abs()
            assert bool((d < 1).any() and (d > 1).any())
            d = (t[4] - t[9]).abs()
            assert bool((d < 3).any() and (d > 3).any()) or c["B"] < 3
        t = HR.loss_operands(c)
        assert float(t[3].max()) == 30.0 and float(t[3].min()) == -30.0


def _ref_center(logits, mask, xyz, tau, hard, noise):
    pt = logits.sigmoid().unsqueeze(-1)
    logp = torch.log(torch.clamp(torch.cat([1. - pt, pt], dim=-1), min=1e-6, max=1 - 1e-6))
    g = logp if noise is None else logp + noise
    y_soft = (g / tau).softmax(-1)
    if hard:
        idx = y_soft.max(-1, keepdim=True)[1]
        y = torch.zeros_like(logp).scatter_(-1, idx, 1.0) - y_soft.detach() + y_soft
    else:
        y = y_soft
    w = (y[:, :, 1] * mask).unsqueeze(-1)
    return (w * xyz).sum(1) / w.sum(1)


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", HR.POCKET_LS)
def test_pocket_center_is_the_reference_formula(L, noisy, hard):
    logits, mask, xyz, noise = HR.pocket_operands(L, noisy)
    tau = HR.pocket_tau(L)
    dc = torch.randn(HR.POCKET_B, 3, generator=torch.Generator().manual_seed(5), dtype=F64)
    l1 = logits.double().requires_grad_()
    c_ref = _ref_center(l1, mask, xyz.double(), tau, hard, None if noise is None else noise.double())
    (c_ref * dc).sum().backward()
    c, dl = HR.pocket_center_grad(logits.double(), mask, xyz.double(), tau, hard, noise, dc)
    assert torch.equal(c, c_ref.detach()) and torch.equal(dl, l1.grad)
    assert bool(torch.isfinite(c).all()) and bool((dl[~mask] == 0).all())
    if not noisy:                                                                       # the oracle states the centre without noise
        import fabind_oracle as orc
        assert torch.equal(orc._soft_center(logits.double(), mask, xyz.double(), tau, hard), c)
    # the hard decision is the same in float32 and float64: no margin within 0.04 of zero but the planted tie
    m = HR.pocket_margin(logits, noise)
    tie = (logits == 0) & mask
    assert float(m.abs()[mask & ~tie].min()) > 0.04
    if L > 2 and not noisy:
        assert bool(tie[0, 2]) and int(tie.sum()) == 1 and float(m[0, 2]) == 0.0
        if hard:                                                                        # the tie goes to class 0: residue 2 carries no weight
            x2 = xyz.double().clone()
            x2[0, 2] += 1000.0
            assert (HR.pocket_center(logits.double(), mask, x2, tau, True, None) - c).abs().max() < 1e-6
    assert int(mask[1].sum()) == 1 and float(logits[0, 0]) == 20.0 and (L == 1 or float(logits[0, 1]) == -20.0)


def test_pocket_table_reaches_every_class():
    assert HR.POCKET_LS == (1, 37, 63, 64, 65, 256, 257)
    assert {HR.pocket_tau(L) for L in HR.POCKET_LS} == {1.0, 0.7}
    assert any(L < 64 for L in HR.POCKET_LS) and 64 in HR.POCKET_LS and any(L > 256 for L in HR.POCKET_LS)      # < a wave, a wave, a second pass of the 256 threads
    for L in HR.POCKET_LS:
        _, mask, _, _ = HR.pocket_operands(L, False)
        assert L == 1 or bool((~mask).any())                                            # padding positions exist


# ------------------------------------------------------------------------------------------------
# table coverage: the block Hadamard
# ------------------------------------------------------------------------------------------------
def test_block_table_reaches_every_class():
    cases = HR.BLOCK_CASES
    assert {c["W"] for c in cases} == set(HR.BLOCK_WS)
    assert [HR.fwd_rows_parallel(W) for W in HR.BLOCK_WS] == [32, 16, 8, 4] and [HR.bwd_lanes(W) for W in HR.BLOCK_WS] == [8, 4, 2, 1]
    live = lambda c: [(P, C) for P, C in zip(c["kcnt"], c["ncnt"]) if P > 0]
    for W in HR.BLOCK_WS:
        mine = [c for c in cases if c["W"] == W]
        rp = HR.fwd_rows_parallel(W)
        fwdC = {C for c in mine if c["fwd_block"] for _, C in live(c)}
        assert {rp - 1, rp, rp + 1} <= fwdC, W                                          # forward: atoms below, at, above the rows in flight
        pc = {pc_ for c in mine for pc_ in live(c)}
        Ps, Cs = {P for P, _ in pc}, {C for _, C in pc}
        assert {1, 129} <= Ps, W                                                        # one row; a second tile of ONE row (lanes il >= 1 empty)
        assert any(0 < C < HR.CH for C in Cs) and HR.CH in Cs and any(C > HR.CH and C % HR.CH for C in Cs), W    # chunk: partial, full, full + partial
        assert any(c["slice"] for c in mine), W
        # nchunk_max above a complex's own chunk count
        assert any(len({(C + HR.CH - 1) // HR.CH for C in c["ncnt"]}) > 1 for c in mine), W
    assert set(HR.C_CLASSES) <= {C for c in cases for _, C in live(c)}                   # every C, on a complex that has residues
    assert set(HR.P_CLASSES) <= {P for c in cases for P in c["kcnt"]}
    assert any(c["W"] == 256 for c in cases)                                            # the width test_gpu_heads.py never ran (NL = 2)
    assert any(not c["fwd_block"] for c in cases) and any(c["fwd_block"] and sum(c["kcnt"]) for c in cases)
    assert any(C == 0 and P > 0 for c in cases for P, C in zip(c["kcnt"], c["ncnt"]))   # the complex without atoms: its d tp rows are zeros
    assert any(sum(c["kcnt"]) == 0 for c in cases) and any(sum(c["ncnt"]) == 0 for c in cases)
    assert {len(c["kcnt"]) for c in cases} >= {1, 2, 3, 4, 5}
    for c in cases:
        t, dout, ia, ib = HR.block_operands(c)
        assert ia.numel() == sum(P * C for P, C in zip(c["kcnt"], c["ncnt"])) and torch.equal(dout, RR.bf_exact(dout))


def test_rows_inter_grid_pair_tables_reach_every_class():
    assert HR.ROWS_WS == (4, 64, 256, 260, 1024)
    for s in (True, False):
        ia, ib = HR.rows_pairs(s)
        deg = HR.rows_degrees(ia, ib, HR.ROWS_N)
        assert {0, 1, 64, 65} <= set(deg) and bool(((ia == ib)).any())
        assert bool((ia[1:] >= ia[:-1]).all()) == s
    G = HR.inter_graph()
    lens = G["lens"]
    assert {0, 1, 64, 65} <= set(lens[:G["n_lig"]]) and {0, 1, 64, 65} <= set(lens[G["n_lig"]:])
    assert {h for h, _ in HR.INTER_HS} == {64, 512, 1024} and {h2 for _, h2 in HR.INTER_HS} == {0, 64, 256}
    assert {HR.pair_hadamard_lp(H, H2)[0] for H, H2 in HR.PAIR_HAD_HS} == {16, 32, 64}
    for H, H2 in HR.PAIR_HAD_HS:
        pb = HR.pair_hadamard_lp(H, H2)[1]
        assert HR.pair_had_nreds(H, H2) == [1, pb - 1, pb + 1]
    assert HR.GRID_WS == (4, 32, 64, 128, 256, 260, 512)
    for W in HR.GRID_WS:
        G_ = HR.grid_groups(W)
        cnt = HR.grid_counts(W)
        walked = {P for P, _ in cnt} | {C for _, C in cnt}
        assert (1, 1) in cnt
        if G_ > 1:
            assert {G_ - 1, G_, G_ + 1} <= walked, W
        assert W >= 256 or 256 % W == 0
        lay = HR.grid_layout(cnt)
        assert lay["n_pairs"] == sum(P * C for P, C in cnt) == lay["p_node"].numel() and lay["N"] == sum(P + C for P, C in cnt)
    assert {HR.grid_groups(W) for W in HR.GRID_WS} == {64, 8, 4, 2, 1}


# ------------------------------------------------------------------------------------------------
# exactness of the product
# ------------------------------------------------------------------------------------------------
def test_float64_product_of_float32_operands_is_exact():
    """(a64 * b64).float() == a32 * b32 bit for bit, and its bf16 rounding is one rounding of the float32 product."""
    for case in HR.BLOCK_CASES[:6]:
        t, _, ia, ib = HR.block_operands(case)
        p64 = HR.hadamard_blocks(t.double(), ia, ib)
        p32 = HR.hadamard_blocks(t, ia, ib)
        if p64.numel() == 0:
            continue
        assert float(p64.abs().min()) > 2.0 ** -100 and float(p64.abs().max()) < 2.0 ** 100          # normal range, no subnormal product
        assert torch.equal(p64.float(), p32)
        # exact: the 24 x 24-bit product fits the 53-bit significand -- undoing it by an exact division returns the operand
        assert torch.equal((p64 / t.double()[ib]).float(), t[ia])
        assert torch.equal(p64.float().bfloat16(), p32.bfloat16())
    g = torch.Generator().manual_seed(1)
    b0, wc = HR.signed_feat(g, 7, 64), HR.signed_feat(g, 8, 64)
    cn = torch.tensor([1, 6, 6])
    assert torch.equal(HR.pair_bmat(b0.double(), wc.double(), cn).float(), HR.pair_bmat(b0, wc, cn))


# ------------------------------------------------------------------------------------------------
# host side of PairBlocks: complexes without atoms or residues are accepted and described; the kernels define them
# ------------------------------------------------------------------------------------------------
def test_pair_block_descriptors_of_empty_complexes():
    """The layout ops.PairBlocks uploads, restated: a P = 0 complex owns no tile (its tile0 equals the next complex's, pb_find takes the
    LAST descriptor with tile0 <= tile), a C = 0 complex owns tiles and no pairs."""
    import numpy as np
    kc, nc = np.array([0, 129, 0, 7, 0]), np.array([3, 0, 2, 5, 1])
    tiles = (kc + HR.TP - 1) // HR.TP
    tile0 = np.cumsum(tiles) - tiles
    assert tile0.tolist() == [0, 0, 2, 2, 3] and int(tiles.sum()) == 3

    def pb_find(tile):
        lo, hi = 0, len(kc) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if tile0[mid] <= tile:
                lo = mid
            else:
                hi = mid - 1
        return lo
    # a tile belongs to the last complex that starts at or before it; that complex must be the one with residues there
    owner = [pb_find(t) for t in range(3)]
    for t, b in enumerate(owner):
        i0 = (t - tile0[b]) * HR.TP
        assert b in (1, 3) and 0 <= i0 < kc[b], (t, b)
    assert owner == [1, 1, 3]
