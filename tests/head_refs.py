"""Plain-torch restatements of the output-head and pair-product kernels (csrc/heads.hip: pair_dist, block_hadamard, the six-term loss,
the pocket centre; csrc/attn.hip: fabind_pair_hadamard, fabind_pair_bmat; csrc/bwd.hip: the four adjoint forms of the pair Hadamard),
the tile constants of those kernels restated from their sources, and the case tables of tests/test_gpu_head_forms.py.  No GPU is
needed to import this.

Every restatement computes in the dtype of its floating-point arguments, on host tensors: float64 is the reference, float32 gives that
reference's own rounding on the same operands (`err32`).  Sums over pairs run SEQUENTIALLY in pair order (CPU index_add_,
reduce_refs.seq_sum0), never as a tree: a sequential sum carries the largest rounding any order can have, so a kernel's tree stays
inside `coord_refs.bound(err32)`.  The loss's sums over up to 2^21 elements run on the kernel's two levels (`_total`).  Products are single multiplications: the float64 product of two float32 values is exact, so
`ref64.float()` IS the float32 product and `ref64.float().bfloat16()` what a kernel that stores bf16 must hold, bit for bit.
tests/test_head_refs_cpu.py pins the restatements to float64 autograd of the reference formulas and the tables to their classes."""
import numpy as np
import torch

import reduce_refs as RR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

TP = 128          # `constexpr int PB_TP = 128;`  proteins per tile (csrc/heads.hip) = fabind_pair_block_tile()
CH = 20           # `constexpr int PB_CH = 20;`   ligand atoms per register chunk of the block adjoint = fabind_pair_block_chunk()
LOSS_PER_BLOCK = 256 * 8     # fabind_loss_blocks: `(n + LOSS_THREADS * 8 - 1) / (LOSS_THREADS * 8)`, at least 1, at most 1024
LOSS_BLOCK_CAP = 1024
P_CLASSES = (0, 1, 127, 128, 129, 257)
C_CLASSES = (0, 1, 3, 19, 20, 21, 40, 41, 128, 129, 256, 257)
BLOCK_WS = (64, 128, 256, 512)


# ------------------------------------------------------------------------------------------------
# pair blocks
# ------------------------------------------------------------------------------------------------
def block_index(kcnt, ncnt):
    """The pair list of PairBlocks(kcnt, ncnt): complex after complex, protein-major  ->  (pocket row, ligand row) per pair, int64."""
    pi, ci = [], []
    p0 = c0 = 0
    for P, C in zip(kcnt, ncnt):
        pi.append((p0 + torch.arange(P)).repeat_interleave(C))
        ci.append((c0 + torch.arange(C)).repeat(P))
        p0, c0 = p0 + P, c0 + C
    z = torch.zeros(0, dtype=torch.int64)
    return torch.cat(pi + [z]), torch.cat(ci + [z])


def pair_dist(xp, xc, pi, ci, scale, lo, hi):
    """y[pair] = clamp(scale * |xp[pi] - xc[ci]|, lo, hi)."""
    d = xp.to(xc.dtype)[pi] - xc[ci]
    return (scale * (d * d).sum(1).sqrt()).clamp(lo, hi)


def pair_dist_grad(xp, xc, pi, ci, dy, scale, lo, hi):
    """d xc[j] = sum over the pairs of j, in pair order, of dy * scale * (xc_j - xp_i) / |xc_j - xp_i| where lo <= v <= hi (torch's
    clamp rule: the bounds themselves pass) and the distance is not zero; 0 elsewhere."""
    dt = xc.dtype
    d = xc[ci] - xp.to(dt)[pi]
    r = (d * d).sum(1).sqrt()
    v = scale * r
    on = (r > 0) & (v >= lo) & (v <= hi)
    g = torch.where(on, dy.to(dt) * scale / torch.where(on, r, torch.ones_like(r)), torch.zeros_like(r))
    return torch.zeros_like(xc).index_add_(0, ci, g[:, None] * d)


def hadamard_blocks(t, ia, ib):
    """out[e, :] = t[ia[e], :] * t[ib[e], :]."""
    return t[ia.long()] * t[ib.long()]


def hadamard_blocks_grad(t, ia, ib, dout):
    """d t = sum_e dout[e] * t[ib[e]] into row ia[e]  +  sum_e dout[e] * t[ia[e]] into row ib[e], each in pair order (a self pair
    t[i] * t[i] receives both)."""
    ia, ib = ia.long(), ib.long()
    g = dout.to(t.dtype)
    return torch.zeros_like(t).index_add_(0, ia, g * t[ib]).index_add_(0, ib, g * t[ia])


def pair_hadamard(T0, H, T1, H2, red_p, red_c):
    """hd[e, :H] = T0[p, :H] * T0[c, H:2H];  hd[e, H:H + H2] = T1[p, :H2] * T1[c, H2:2 H2]."""
    p, c = red_p.long(), red_c.long()
    return torch.cat([T0[p, :H] * T0[c, H:2 * H], T1[p, :H2] * T1[c, H2:2 * H2]], 1)


def pair_hadamard_grad(T0, H, T1, H2, red_p, red_c, dhd, d0=None, d1=None):
    """(d T0, d T1): the a-halves of the p rows and the b-halves of the c rows, each summed in pair order and then ADDED to d0 / d1
    (zeros when None): the kernels sum a row's pairs first and add the row's sum to what the buffer holds."""
    p, c = red_p.long(), red_c.long()
    g = dhd.to(T0.dtype)
    a0 = torch.zeros_like(T0)
    a0[:, :H] = torch.zeros_like(T0[:, :H]).index_add_(0, p, g[:, :H] * T0[c, H:2 * H])
    a0[:, H:2 * H] = torch.zeros_like(T0[:, :H]).index_add_(0, c, g[:, :H] * T0[p, :H])
    a1 = torch.zeros_like(T1)
    if H2:
        a1[:, :H2] = torch.zeros_like(T1[:, :H2]).index_add_(0, p, g[:, H:H + H2] * T1[c, H2:2 * H2])
        a1[:, H2:2 * H2] = torch.zeros_like(T1[:, :H2]).index_add_(0, c, g[:, H:H + H2] * T1[p, :H2])
    return (a0 if d0 is None else d0.to(T0.dtype) + a0), (a1 if d1 is None else d1.to(T1.dtype) + a1)


def pair_bmat(b0, wcomp, c_node):
    """bmat[j * NO + o, :] = b0[c_node[j], :] * wcomp[o, :]."""
    NO, H = wcomp.shape
    return (b0[c_node.long()][:, None, :] * wcomp[None, :, :]).reshape(-1, H)


# ------------------------------------------------------------------------------------------------
# six-term loss
# ------------------------------------------------------------------------------------------------
LOSS_TERMS = ("pocket_cls", "pocket_center", "contact", "contact_by_pred", "distill", "coord")


def _total(x):
    """Sum of every element in the dtype of x on the loss kernel's two levels, each level SEQUENTIAL: chunks of LOSS_PER_BLOCK = 2048
    consecutive elements one element after the other, then the chunk sums one after the other.  (One sequential pass over 2^21 float32
    elements loses 1e-3 of the sum: a bound drawn from it would let a dropped work-group, 1 / 1024 of the sum, pass.)"""
    v = x.reshape(-1)
    n = v.numel()
    nchunk = max(1, (n + LOSS_PER_BLOCK - 1) // LOSS_PER_BLOCK)
    pad = torch.zeros(nchunk * LOSS_PER_BLOCK, dtype=v.dtype)
    pad[:n] = v
    part = RR.seq_sum0(pad.reshape(nchunk, LOSS_PER_BLOCK).T.contiguous())
    return RR.seq_sum0(part.reshape(-1, 1))[0]


def _mean(x):
    """_total / numel; the mean of nothing is defined as 0 (torch gives NaN)."""
    return _total(x) / x.numel() if x.numel() else torch.zeros((), dtype=x.dtype)


def six_term_loss(coords, y_pred, y_by, logits, center, coords_true, dis_map, cls, mask, center_true, w):
    """(total, terms [6]) of main_fabind.py:398-417 in the order of LOSS_TERMS: BCE-with-logits over ALL positions times
    numel / sum(mask), 0.05-weighted Huber of the centre, the three MSEs, SmoothL1(beta 1) of the coordinates; the total is
    ((((t0 + t1) + t2) + t3) + t4) + t5, python's sum(terms.values())."""
    dt = coords.dtype
    y = cls.to(dt)
    x = logits
    bce = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    t_cls = w["cls"] * _total(bce) / mask.sum().to(dt) if x.numel() else torch.zeros((), dtype=dt)
    d = (center - center_true).abs()
    t_cen = w["center"] * _mean(torch.where(d <= w["delta"], 0.5 * d * d, w["delta"] * (d - 0.5 * w["delta"])))
    t_con = w["pair"] * _mean((y_pred - dis_map) ** 2)
    t_cby = w["pair"] * _mean((y_by - dis_map) ** 2)
    t_dis = w["distill"] * _mean((y_by - y_pred) ** 2)
    d = (coords - coords_true).abs()
    t_crd = w["coord"] * _mean(torch.where(d < 1, 0.5 * d * d, d - 0.5))
    terms = torch.stack([t_cls, t_cen, t_con, t_cby, t_dis, t_crd]).to(dt)
    total = terms[0]
    for k in range(1, 6):
        total = total + terms[k]
    return total, terms


def six_term_loss_grad(coords, y_pred, y_by, logits, center, coords_true, dis_map, cls, mask, center_true, w, g_loss, g_terms):
    """The five gradient seeds (d coords, d y_pred, d y_by, d logits, d center) for the upstream gradients g_loss (scalar or None) on
    the total and g_terms ([6] or None) on the single terms: term k receives g_loss + g_terms[k]."""
    dt = coords.dtype
    g = torch.zeros(6, dtype=dt)
    if g_loss is not None:
        g = g + g_loss.to(dt)
    if g_terms is not None:
        g = g + g_terms.to(dt)
    n_pair, n_coord, n_cls, n_center = y_pred.numel(), coords.numel(), logits.numel(), center.numel()
    s_pair = 2.0 * w["pair"] / n_pair if n_pair else 0.0
    s_dis = 2.0 * w["distill"] / n_pair if n_pair else 0.0
    d_yp = g[2] * s_pair * (y_pred - dis_map) - g[4] * s_dis * (y_by - y_pred)
    d_yb = g[3] * s_pair * (y_by - dis_map) + g[4] * s_dis * (y_by - y_pred)
    d = coords - coords_true
    d_co = (g[5] * w["coord"] / n_coord if n_coord else 0.0) * torch.where(d.abs() < 1, d, torch.sign(d))
    d_lg = (g[0] * w["cls"] / mask.sum().to(dt) if n_cls else 0.0) * (torch.sigmoid(logits) - cls.to(dt))
    d = center - center_true
    d_ce = (g[1] * w["center"] / n_center if n_center else 0.0) * torch.where(d.abs() <= w["delta"], d, torch.sign(d) * w["delta"])
    return d_co, d_yp, d_yb, d_lg, d_ce


def loss_blocks(n_pair, n_coord, n_cls):
    """fabind_loss_blocks restated."""
    n = max(n_pair, n_coord, n_cls)
    return max(1, min(LOSS_BLOCK_CAP, (n + LOSS_PER_BLOCK - 1) // LOSS_PER_BLOCK))


# ------------------------------------------------------------------------------------------------
# pocket centre
# ------------------------------------------------------------------------------------------------
def pocket_center(logits, mask, xyz, tau, hard, noise):
    """models/model.py:146-158: p = clamp([1 - s, s], 1e-6, 1 - 1e-6), s = sigmoid(logit); y = softmax((log p + noise) / tau); hard: the
    straight-through one-hot of the argmax (a tie goes to class 0, torch.max's first index); centre = sum_l y1 mask xyz / sum_l y1 mask.
    Differentiable in `logits`."""
    pt = torch.sigmoid(logits).unsqueeze(-1)
    logp = torch.log(torch.clamp(torch.cat([1.0 - pt, pt], dim=-1), min=1e-6, max=1 - 1e-6))
    g = logp if noise is None else logp + noise.to(logits.dtype)
    y = (g / tau).softmax(-1)
    if hard:
        idx = y.max(-1, keepdim=True)[1]
        y = torch.zeros_like(logp).scatter_(-1, idx, 1.0) - y.detach() + y
    wt = (y[:, :, 1] * mask.to(logits.dtype)).unsqueeze(-1)
    return (wt * xyz.to(logits.dtype)).sum(1) / wt.sum(1)


def pocket_center_grad(logits, mask, xyz, tau, hard, noise, dcenter):
    """(centre, d logits) for the upstream gradient dcenter, by autograd of the restatement in the dtype of `logits`."""
    lg = logits.clone().requires_grad_(True)
    c = pocket_center(lg, mask, xyz, tau, hard, noise)
    (c * dcenter.to(lg.dtype)).sum().backward()
    return c.detach(), lg.grad


def pocket_margin(logits, noise):
    """(log p1 + n1) - (log p0 + n0) in float64: the sign decides the hard one-hot."""
    pt = torch.sigmoid(logits.double()).unsqueeze(-1)
    logp = torch.log(torch.clamp(torch.cat([1.0 - pt, pt], dim=-1), min=1e-6, max=1 - 1e-6))
    if noise is not None:
        logp = logp + noise.double()
    return logp[..., 1] - logp[..., 0]


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def signed_feat(g, *shape):
    """reduce_refs.feat (mean 4, spread 1.5: sums do not cancel, products stay normal) with one element in eight negated."""
    t = RR.feat(g, *shape)
    return torch.where(torch.rand(*shape, generator=g) < 0.125, -t, t)


def rowptr_of(lens):
    return RR.rowptr_of(lens)


# ------------------------------------------------------------------------------------------------
# case tables: pair_dist
# ------------------------------------------------------------------------------------------------
# lo 0: the zero distance passes the clamp and only `r > 0` keeps its gradient finite; lo 0.5: the lower clamp is active
PAIR_DIST_CASES = [
    dict(name="B1 P1 C1", kcnt=[1], ncnt=[1], lo=0.0),
    dict(name="B3 P0 first, C 3|19|256", kcnt=[0, 127, 5], ncnt=[3, 19, 256], lo=0.0),
    dict(name="B3 P0 middle, C 20|21|40", kcnt=[128, 0, 129], ncnt=[20, 21, 40], lo=0.5),
    dict(name="B3 P0 last, C 41|129|1", kcnt=[257, 3, 0], ncnt=[41, 129, 1], lo=0.0),
    dict(name="B5 C0 twice, C 128|0|257|0|3", kcnt=[129, 7, 1, 128, 2], ncnt=[128, 0, 257, 0, 3], lo=0.5),
    dict(name="B2 all P0", kcnt=[0, 0], ncnt=[4, 2], lo=0.0),
    dict(name="B2 all C0", kcnt=[4, 128], ncnt=[0, 0], lo=0.0),
]
PAIR_DIST_SCALE, PAIR_DIST_HI = 5.0, 10.0


def pair_dist_operands(case):
    """(xp, xc, dy, pi, ci) float32 on the host.  Planted in the first complex that has pairs: a zero distance (pair (0, 0)), a pair
    with scale * r == hi exactly (difference (2, 0, 0); the last protein and atom) and one below lo = 0.5 (difference (0.0625, 0, 0))
    where the block has room for them."""
    kcnt, ncnt = case["kcnt"], case["ncnt"]
    g = torch.Generator().manual_seed(sum(kcnt) * 7 + sum(ncnt))
    xp = torch.randn(sum(kcnt), 3, generator=g) * 1.2
    xc = torch.randn(sum(ncnt), 3, generator=g) * 0.6
    p0 = c0 = 0
    for P, C in zip(kcnt, ncnt):
        if P and C:
            xc[c0] = xp[p0]
            if P > 1 and C > 1:
                xp[p0 + P - 1] = torch.tensor([1.0, 0.5, -0.25])
                xc[c0 + C - 1] = torch.tensor([-1.0, 0.5, -0.25])
            if P > 2 and C > 2:
                xc[c0 + 1] = xp[p0 + 1] + torch.tensor([0.0625, 0.0, 0.0])
            break
        p0, c0 = p0 + P, c0 + C
    pi, ci = block_index(kcnt, ncnt)
    dy = torch.randn(pi.numel(), generator=g)
    return xp, xc, dy, pi, ci


# ------------------------------------------------------------------------------------------------
# case tables: the block Hadamard (ops.rows_hadamard with blocks), forward and adjoint
# ------------------------------------------------------------------------------------------------
def fwd_rows_parallel(W):
    """block_hadamard_fwd_kernel: `constexpr int CT = W / 8, RP = 256 / CT;` atoms side by side."""
    return 256 // (W // 8)


def bwd_lanes(W):
    """block_hadamard_bwd_kernel: `constexpr int CT = W / 2, NL = 256 / CT;` protein lanes."""
    return 256 // (W // 2)


def _fwd_edge(W):
    rp = fwd_rows_parallel(W)
    return [rp - 1, rp, rp + 1]


# sum(kcnt) % 4 == 0 unless the case is the fallback; `slice`: t is a column slice of a wider buffer; `fwd_block`: the forward takes
# block_hadamard_fwd_kernel (else the fabind_pair_hadamard fallback, which must give the same values)
BLOCK_CASES = []
for _W in BLOCK_WS:
    BLOCK_CASES.append(dict(name="W%d fwd edge C %s" % (_W, _fwd_edge(_W)), W=_W, kcnt=[129, 1, 2, 0], ncnt=_fwd_edge(_W) + [CH + 1], slice=False))
BLOCK_CASES += [
    dict(name="W64 C 0|1|3|19", W=64, kcnt=[129, 1, 129, 1], ncnt=[0, 1, 3, 19], slice=False),
    dict(name="W64 C 20|21|40|41", W=64, kcnt=[1, 129, 1, 129], ncnt=[20, 21, 40, 41], slice=True),
    dict(name="W64 C 128|129|256|257", W=64, kcnt=[1, 129, 129, 1], ncnt=[128, 129, 256, 257], slice=False),
    dict(name="W128 C 257|21|20|256 P0 first", W=128, kcnt=[0, 1, 129, 1, 1], ncnt=[5, 257, 21, 20, 256], slice=False),
    dict(name="W128 P 127|128|257", W=128, kcnt=[127, 128, 257], ncnt=[3, 1, 2], slice=True),
    dict(name="W256 C 21|129|19 P0 last", W=256, kcnt=[129, 1, 2, 0], ncnt=[21, 129, 19, 7], slice=True),
    dict(name="W256 C 20|40 P1", W=256, kcnt=[1, 3], ncnt=[20, 40], slice=False),
    dict(name="W512 C 128|20|41", W=512, kcnt=[1, 129, 2], ncnt=[128, 20, 41], slice=False),
    dict(name="W512 C 19|1 P1", W=512, kcnt=[1, 129, 2], ncnt=[19, 1, 3], slice=True),
    dict(name="W64 n_a%4 fallback", W=64, kcnt=[5], ncnt=[3], slice=False),
    dict(name="W256 n_a%4 fallback", W=256, kcnt=[129, 1], ncnt=[9, 21], slice=False),
    dict(name="W128 C0 first of two", W=128, kcnt=[129, 7], ncnt=[0, 3], slice=False),
    dict(name="W512 C0 last", W=512, kcnt=[3, 1], ncnt=[21, 0], slice=False),
    dict(name="W64 all P0", W=64, kcnt=[0, 0], ncnt=[5, 3], slice=False),
    dict(name="W256 all C0", W=256, kcnt=[4, 128], ncnt=[0, 0], slice=False),
]
for _c in BLOCK_CASES:
    _c["fwd_block"] = sum(_c["kcnt"]) % 4 == 0


def block_operands(case):
    """(t [sum P + sum C, W], dout [pairs, W] with bf16-exact values, ia, ib) on the host; ib indexes t (ligand rows follow the pocket's)."""
    W, kcnt, ncnt = case["W"], case["kcnt"], case["ncnt"]
    g = torch.Generator().manual_seed(W * 13 + sum(kcnt) + 3 * sum(ncnt))
    t = signed_feat(g, sum(kcnt) + sum(ncnt), W)
    pi, ci = block_index(kcnt, ncnt)
    dout = RR.bf_exact(torch.randn(pi.numel(), W, generator=g) + 0.5)
    return t, dout, pi, sum(kcnt) + ci


# ------------------------------------------------------------------------------------------------
# case tables: the CSR-walk adjoint (ops.rows_hadamard without blocks)
# ------------------------------------------------------------------------------------------------
ROWS_WS = (4, 64, 256, 260, 1024)
ROWS_N = 9


def rows_pairs(sorted_a):
    """Pairs over 9 rows whose CSR rows (pairs as first factor, then as second) have 0, 64, 65, 2 (a self pair), many, ..., 1 entries:
    row 0 none; row 1 first factor of 64 pairs, row 2 of 65, their partners rows 4 .. 7 in turn; row 3 the self pair t[3] * t[3];
    row 8 second factor of one pair of row 2.  `sorted_a`: ia non-decreasing (a_sorted=True), else a fixed shuffle."""
    ia = [1] * 64 + [2] * 65 + [3]
    ib = [4 + k % 4 for k in range(64)] + [4 + k % 4 for k in range(64)] + [8] + [3]
    ia, ib = torch.tensor(ia), torch.tensor(ib)
    if not sorted_a:
        p = torch.randperm(ia.numel(), generator=torch.Generator().manual_seed(3))
        ia, ib = ia[p], ib[p]
    return ia, ib


def rows_degrees(ia, ib, n):
    return (torch.bincount(ia, minlength=n) + torch.bincount(ib, minlength=n)).tolist()


# ------------------------------------------------------------------------------------------------
# case tables: the inter-graph adjoint (ops.pair_hadamard with graph) and the two-block forward
# ------------------------------------------------------------------------------------------------
INTER_HS = ((64, 0), (64, 64), (512, 64), (512, 256), (1024, 0), (1024, 256))


def inter_graph():
    """A symmetric bipartite inter graph whose ligand rows AND protein rows have 0, 1, 64 and 65 edges.
    Ligand nodes 0 .. 68, protein nodes 69 .. 136:  L0 - p0 .. p64 (65), L1 - p0 .. p63 (64), L2 - p0 (1), L3 none;
    L4 .. L68 - q0 (q0: 65), L4 .. L67 - q1 (q1: 64), q2 none; p64 has the one edge of L0.
    -> dict(n, red_p, red_c (one entry per reduced pair), rp, col, red_idx (CSR over all nodes, a row's edges in pair order))."""
    nl = 69
    p = lambda k: nl + k                    # p0 .. p64
    q = lambda k: nl + 65 + k               # q0 .. q2
    pairs = [(p(k), 0) for k in range(65)] + [(p(k), 1) for k in range(64)] + [(p(0), 2)]
    pairs += [(q(0), l) for l in range(4, 69)] + [(q(1), l) for l in range(4, 68)]
    n = nl + 68
    rows = [[] for _ in range(n)]
    for e, (pn, cn) in enumerate(pairs):
        rows[pn].append((cn, e))
        rows[cn].append((pn, e))
    lens = [len(r) for r in rows]
    col = torch.tensor([c for r in rows for c, _ in r], dtype=torch.int32)
    red_idx = torch.tensor([e for r in rows for _, e in r], dtype=torch.int32)
    return dict(n=n, n_lig=nl, red_p=torch.tensor([a for a, _ in pairs], dtype=torch.int32), red_c=torch.tensor([b for _, b in pairs], dtype=torch.int32),
                rp=rowptr_of(lens), col=col, red_idx=red_idx, lens=lens)


def pair_hadamard_lp(H, H2):
    """fabind_pair_hadamard: `const int lp = widest <= 64 ? 16 : widest <= 128 ? 32 : 64;` lanes per pair; 4 * (64 / lp) pairs a block."""
    widest = max(H, H2)
    lp = 16 if widest <= 64 else 32 if widest <= 128 else 64
    return lp, 4 * (64 // lp)


PAIR_HAD_HS = ((64, 0), (32, 64), (128, 64), (64, 128), (512, 64), (260, 0))


def pair_had_nreds(H, H2):
    pb = pair_hadamard_lp(H, H2)[1]
    return [1, pb - 1, pb + 1]


BMAT_CASES = [dict(H=64, NO=8, n_c=1), dict(H=260, NO=3, n_c=3), dict(H=512, NO=8, n_c=5), dict(H=4, NO=1, n_c=1)]


# ------------------------------------------------------------------------------------------------
# case tables: the grid adjoint (plus.engine.pair_had with the layout)
# ------------------------------------------------------------------------------------------------
GRID_WS = (4, 32, 64, 128, 256, 260, 512)


def grid_groups(W):
    """pair_hadamard_bwd_grid_kernel: `LPR = W / 4`; LPR >= 64 is the wide path (one row at a time), else G = 64 / LPR rows side by side."""
    lpr = W // 4
    return 1 if lpr >= 64 else 64 // lpr


def grid_counts(W):
    """(P, C) per complex: a ligand node walks P rows, a protein node C rows -- below, at and one above the G groups, and P = C = 1."""
    G = grid_groups(W)
    if G == 1:
        return [(3, 5), (1, 1), (2, 2)]
    return [(G - 1, G + 1), (G, G), (1, 1)] if G > 2 else [(1, 3), (2, 2), (1, 1), (3, 1)]


def grid_layout(counts):
    """The node layout of fabind_amd.engine.BatchLayout: per complex its C ligand nodes, then its P protein nodes; pair (b, i, j) at
    pair_off[b] + i * C_b + j.  -> dict(N, B, n_pairs, node_off, c_cnt, node_b, desc_p [B, 8], p_node, c_node)."""
    off, po, node_off, c_cnt, node_b, desc, pn, cn = 0, 0, [0], [], [], [], [], []
    pf = cf = 0
    for b, (P, C) in enumerate(counts):
        c_cnt.append(C)
        node_b += [b] * (P + C)
        desc.append([pf, P, cf, C, po & 0xFFFFFFFF, po >> 32, C, 1])
        for i in range(P):
            pn += [off + C + i] * C
            cn += list(range(off, off + C))
        off, po, pf, cf = off + P + C, po + P * C, pf + P, cf + C
        node_off.append(off)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return dict(N=off, B=len(counts), n_pairs=po, node_off=i32(node_off), c_cnt=i32(c_cnt), node_b=i32(node_b), desc_p=i32(desc).reshape(-1, 8),
                p_node=i32(pn), c_node=i32(cn))


# ------------------------------------------------------------------------------------------------
# case tables: six-term loss
# ------------------------------------------------------------------------------------------------
LOSS_W = dict(coord=1.5, pair=0.75, distill=1.25, cls=0.875, center=0.0625, delta=3.0)       # float32-exact weights
LOSS_CASES = [
    dict(name="n_pair 0 int64 total", n_pair=0, n_atoms=5, B=2, L=9, cls_dt=torch.int64, g="total"),
    dict(name="n_pair 1 bool both", n_pair=1, n_atoms=3, B=1, L=4, cls_dt=torch.bool, g="both"),
    dict(name="n_pair 2048 uint8 terms", n_pair=2048, n_atoms=40, B=2, L=37, cls_dt=torch.uint8, g="terms"),
    dict(name="n_pair 2049 int32 total", n_pair=2049, n_atoms=40, B=2, L=37, cls_dt=torch.int32, g="total"),
    dict(name="n_pair 64x2048 fp32 both", n_pair=64 * 2048, n_atoms=77, B=3, L=211, cls_dt=torch.float32, g="both"),
    dict(name="n_pair 64x2048+1 int64 terms", n_pair=64 * 2048 + 1, n_atoms=77, B=3, L=211, cls_dt=torch.int64, g="terms"),
    dict(name="n_pair 2^21+1 int64 total (cap)", n_pair=2 ** 21 + 1, n_atoms=77, B=3, L=211, cls_dt=torch.int64, g="total"),
    dict(name="n_coord picks the grid", n_pair=1000, n_atoms=1400, B=2, L=50, cls_dt=torch.int32, g="both"),
    dict(name="n_cls picks the grid", n_pair=100, n_atoms=8, B=3, L=1500, cls_dt=torch.bool, g="terms"),
]
LOSS_G_TERMS = (0.3, -1.2, 2.0, 0.0, 0.5, 1.1)
LOSS_G_TOTAL = 0.7


def loss_operands(case):
    """[coords, y_pred, y_by, logits, center, coords_true, dis_map, cls, mask, center_true] float32 / the case's class dtype on the host:
    |d| on both sides of the SmoothL1 knee (1) and of the Huber knee (delta = 3), logits of +-30."""
    g = torch.Generator().manual_seed(case["n_pair"] % 9973 + case["n_atoms"])
    r = lambda *s: torch.randn(*s, generator=g)
    n_atoms, n_pair, B, L = case["n_atoms"], case["n_pair"], case["B"], case["L"]
    coords, coords_true = r(n_atoms, 3) * 3, r(n_atoms, 3) * 3
    y_pred, y_by, dis_map = (torch.rand(n_pair, generator=g) * 10 for _ in range(3))
    lens = torch.randint(max(1, L // 2), L + 1, (B,), generator=g)
    mask = torch.arange(L)[None, :] < lens[:, None]
    logits = r(B, L) * 3 * mask
    logits[0, 0] = 30.0
    if L > 1:
        logits[0, 1] = -30.0
    cls = ((torch.rand(B, L, generator=g) < 0.3) & mask)
    cls[0, 0] = False                                              # a confident miss: the term's largest element
    center, center_true = r(B, 3) * 4, r(B, 3) * 4
    return [coords, y_pred, y_by, logits, center, coords_true, dis_map, cls.to(case["cls_dt"]), mask, center_true]


def loss_upstream(case):
    """(g_loss, g_terms) float32 host tensors or None."""
    gl = torch.tensor(LOSS_G_TOTAL) if case["g"] in ("total", "both") else None
    gt = torch.tensor(LOSS_G_TERMS) if case["g"] in ("terms", "both") else None
    return gl, gt


# ------------------------------------------------------------------------------------------------
# case tables: pocket centre
# ------------------------------------------------------------------------------------------------
POCKET_LS = (1, 37, 63, 64, 65, 256, 257)
POCKET_B = 3


def pocket_tau(L):
    return 0.7 if POCKET_LS.index(L) % 2 else 1.0


def pocket_operands(L, noisy):
    """(logits [3, L], mask, xyz, noise or None) float32 on the host.  Complex 1 has ONE unmasked residue; position 0 of every complex
    holds +20 (the upper clamp branch; the hard one-hot has a member in every complex), position 1 of complex 0 holds -20, position 2 of
    complex 0 an exact 0 (the hard tie without noise).  The other logits stay inside +-12 (the clamp's corner at 13.8 is a kink of the
    gradient) and at least 0.05 away from a change of the hard decision."""
    g = torch.Generator().manual_seed(L * 5 + int(noisy))
    lens = torch.randint(max(1, L // 3), L + 1, (POCKET_B,), generator=g)
    lens[0], lens[1] = L, 1
    mask = torch.arange(L)[None, :] < lens[:, None]
    logits = (torch.randn(POCKET_B, L, generator=g) * 4).clamp(-12, 12)
    xyz = torch.randn(POCKET_B, L, 3, generator=g) * 15
    noise = -torch.empty(POCKET_B, L, 2).exponential_(generator=g).log() if noisy else None
    near = pocket_margin(logits, noise).abs() < 0.05
    logits = torch.where(near, logits + 0.25, logits)
    logits[:, 0] = 20.0
    if L > 1:
        logits[0, 1] = -20.0
    if L > 2 and not noisy:
        logits[0, 2] = 0.0
    return logits, mask, xyz, noise
