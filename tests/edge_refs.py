"""Host restatements of the fused intra-graph edge pipeline (csrc/fused_edge.hip, fused_edge_fwd2.hip, fused_edge_fwd3.hip,
fused_edge_bwd3.hip, fused_edge_bwd4.hip; the deterministic segment sum of csrc/fused_common.h) in float64 and float32, the absolute-sum
companion of every output that is a sum, the row-wise metric built on them, and the table of CSR topologies that walks every seam class
of the 64-edge tiles.  tests/test_edge_refs_cpu.py checks this file on the CPU, tests/test_gpu_edge_forms.py runs the kernels against it.

    S1  = silu(A[row] + B[col] + rhohat w_r)          M = silu(S1 W2^T + b2) * keep          agg = segsum_row(M)
    s   = w3 . silu(M Wc^T + bc)                      loss = <agg, dagg> + <s, ds>

The metric.  An output that is a sum of terms is judged against the same sum over ABSOLUTE terms (its companion): the error of an
element is |got - ref64| / companion, and for a per-node output it is taken row-wise, max_c |err[r, c]| / max_c companion[r, c], then the
maximum over the rows that have edges.  A node with three edges is so judged on the scale of its own three messages, not on that of the
heaviest row of the graph.

Rounding points of the bf16 pipeline (where the kernels round to bf16, the restatement rounds too; `rb`):
  AB, W2, Wc            bf16 operands (kernels.gcl_edge_fused takes AB16 and pack_frag()-ed weights)
  S1                    fused_edge_fwd2.hip:116 (fw_pack into the LDS tile); fused_edge_bwd3.hip:252; fused_edge.hip:245-246; bwd4: :306
  M                     fused_edge_fwd2.hip:159 (after the keep factor, :156); fused_edge_bwd3.hip:290; fused_edge.hip:294
  silu'(pre2) * keep    fused_edge_fwd2.hip:160 (saved d2f); fused_edge_bwd3.hip:289; fused_edge.hip:296-297
  pre3                  fused_edge_fwd2.hip:198 (saved z3f), read back by fused_edge_bwd4.hip:174-175 BEFORE silu / silu' (variant 6 only;
                        variants 0 and 5 evaluate them on the fp32 accumulator: fused_edge.hip:323, fused_edge_bwd3.hip:319-320)
  dT                    fused_edge_bwd4.hip:179, fused_edge_bwd3.hip:324, fused_edge.hip:327 -- d bc sums the UNROUNDED values (:178 / :323 / :326)
  dP2                   fused_edge_bwd4.hip:236, fused_edge_bwd3.hip:378, fused_edge.hip:365 -- d b2 sums the unrounded values
  dS1                   fused_edge_bwd4.hip:259, fused_edge_bwd3.hip:403, fused_edge.hip:386
  silu'(pre1)           bf16 in variant 5 only (fused_edge_bwd3.hip:253, through the scratch slab); fp32 in variants 0 and 6
  dP1                   fused_edge_bwd4.hip:307, fused_edge_bwd3.hip:431, fused_edge.hip:412 -- d rhohat sums the unrounded products with w_r;
                        d w_r, both halves of dAB sum the ROUNDED rows (fe_scan_rows reads the LDS tile; segment_sum reads the stored rows)
  dW2 = dP2^T S1, dWc = dT^T M    contractions of the stored bf16 rows (kernels.gemm_tn)
Split-bf16 forward (fused_edge_fwd3.hip): fp32 operands; S1 and M live as hi = bf16(x), lo = bf16(x - hi) (fe_split2, fused_common.h:256-259;
:119 and :168-169), the weights likewise (kernels.pack_frag_split); a product term is W_hi X_lo + W_lo X_hi + W_hi X_hi
(fe_gemm_x3, fused_common.h:222-226: lo * lo dropped); the segment sum and the second contraction read hi + lo (fused_common.h:369-372)."""
import functools
import math
from types import SimpleNamespace

import torch

from helpers import fused_edge_keep_mask

BM = 64                                   # edges per tile of every kernel of the family (FE_BM)
F64, F32 = torch.float64, torch.float32
FLOOR_BF16 = 2.0 ** -7                    # two bf16 ulps of the row's own absolute sum
FLOOR_X3 = 64 * 2.0 ** -23                # = coord_refs.FLOOR
MARGIN = 8.0                              # the project's standing margin over the float32 restatement


def rb(t):
    """Round to nearest-even bf16, keep the dtype."""
    return t.float().bfloat16().to(t.dtype)


def split(t):
    """hi = bf16(x), lo = bf16(x - hi)."""
    hi = rb(t)
    return hi, rb(t - hi)


def _silu_d(z):
    """(silu(z), silu'(z))."""
    sg = torch.sigmoid(z)
    return z * sg, sg * (1.0 + z * (1.0 - sg))


def segsum(idx, X, n):
    return torch.zeros((n, X.shape[1]), dtype=X.dtype).index_add_(0, idx, X)


# ------------------------------------------------------------------------------------------------ topologies
def _fill(target, seed, hi=40):
    """Light rows (degree 0..hi, some empty) that add up to `target` edges exactly."""
    g = torch.Generator().manual_seed(seed)
    deg, tot = [], 0
    while tot < target:
        d = min(int(torch.randint(0, hi + 1, (1,), generator=g)), target - tot)
        deg.append(d)
        tot += d
    return deg


def _topologies():
    t = {}
    t["one_edge"] = [0, 1, 0]
    t["ragged37"] = [5, 0, 11, 1, 20]
    t["exact64"] = [10, 0, 20, 14, 20]
    t["seam128"] = [30, 34, 40, 24]                                        # a node boundary exactly at edge 64
    t["straddle"] = [25, 38, 2, 30, 15]                                    # the two-edge row holds edges 63 and 64
    t["row200"] = [12, 18, 200, 20, 13]                                    # edges 30 .. 229: partial, through, through, partial
    t["aligned128"] = [40, 24, 128, 33, 9]                                 # edges 64 .. 191: whole-tile runs that start and stop on seams
    t["heavy_to_end"] = [20, 15, 0, 190]                                   # runs to the last edge, ragged last tile (E = 225)
    t["single_row"] = [0, 150, 0, 0]
    t["empty_rows"] = [0, 0, 40, 24, 0, 0, 30, 34, 0, 17, 0]               # empty rows first, last, and at the seams 64 and 128
    t["two_heavy"] = [10, 118, 100, 90, 12]                                # 10..127 | 128..227 | 228..317: back to back at a seam and inside a tile
    t["tiles7"] = _fill(7 * BM - 20, 7)
    t["tiles8"] = _fill(8 * BM, 8)                                         # E a multiple of 64
    t["tiles9"] = _fill(8 * BM + 1, 9)                                     # the last tile holds one edge
    t["tiles17"] = _fill(17 * BM - 5, 17)
    a, b = _fill(11 * BM + 7, 25), _fill(27 * BM - 9 - (11 * BM + 7) - 333, 26)
    t["tiles27"] = a + [0, 333, 0] + b                                     # >= 25 tiles: the group-count cases; one heavy row among light ones
    return t


TOPOLOGIES = _topologies()
NAMES = tuple(TOPOLOGIES)
WIDE_H = ("straddle", "row200", "aligned128", "heavy_to_end")             # also run at H = 128 and 512
GROUPS_TOPOLOGY = "tiles27"
SMALL_TILES = ("straddle", "aligned128", "heavy_to_end")                  # <= 4 tiles: one tile of a weight gradient is visible


@functools.lru_cache(maxsize=None)
def topology(name):
    """-> namespace(name, N, E, deg, row, col, rowptr, colptr, perm, silent, hub).  Sending side: node `silent` is read by no edge; in
    the topologies with at least 100 edges node `hub` is read by 70 of them (more than one tile's worth)."""
    deg = torch.tensor(TOPOLOGIES[name], dtype=torch.long)
    N = deg.shape[0]
    row = torch.repeat_interleave(torch.arange(N), deg)
    E = row.shape[0]
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    silent, hub = N - 1, None
    col = torch.randint(0, N - 1, (E,), generator=g)                       # never N - 1
    if E >= 100:
        hub = 0
        col[torch.randperm(E, generator=g)[:70]] = hub
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(deg, 0)]).to(torch.int32)
    colsorted, perm = torch.sort(col, stable=True)
    colptr = torch.zeros(N + 1, dtype=torch.int32)
    colptr[1:] = torch.cumsum(torch.bincount(colsorted, minlength=N), 0)
    return SimpleNamespace(name=name, N=N, E=E, deg=deg, row=row, col=col, rowptr=rowptr, colptr=colptr, perm=perm, silent=silent, hub=hub)


def tile_classes(row):
    """Per 64-edge tile, from `row` alone, the conditions the kernels branch on (fe_scan_rows / fe_scan_runs64 / fe_boundary_fix_kernel)
    -> list of sets of class names."""
    row = [int(r) for r in row]
    E = len(row)
    out = []
    for t in range((E + BM - 1) // BM):
        e0 = t * BM
        ne = min(BM, E - e0)
        c = set()
        head = e0 > 0 and row[e0 - 1] == row[e0]
        tail = e0 + ne < E and row[e0 + ne] == row[e0 + ne - 1]
        one = row[e0] == row[e0 + ne - 1]
        if head:
            c.add("head_cont")
        if tail:
            c.add("tail_cont")
        if one and head and tail:
            c.add("through")                                               # the whole tile continues a run and hands it on
        if one and not head and tail and e0 > 0:
            c.add("whole_tile_run_starts_on_seam")
        if one and head and not tail:
            c.add("whole_tile_run_stops_on_seam" if ne == BM else "whole_tile_run_stops_at_E")
        if head and tail and not one:
            c.add("two_spanning_runs")                                     # both boundary slots of the tile are used
        if e0 > 0 and not head:
            c.add("run_starts_on_seam")
        if e0 + ne < E and not tail:
            c.add("run_ends_on_seam")
        if e0 + ne == E:
            c.add("run_ends_at_E")
            c.add("ragged_last" if ne < BM else "full_last")
            if head:
                c.add("spanning_run_ends_at_E")
        if e0 > 0 and row[e0] - row[e0 - 1] > 1:
            c.add("empty_rows_at_seam")
        if tail and not (one and head):                                    # fe_boundary_fix_kernel: the tile where a spanning run starts
            k, u = 1, t + 1
            while True:
                k += 1
                f0 = u * BM
                fn = min(BM, E - f0)
                if not (row[f0 + fn - 1] == row[e0 + ne - 1] and f0 + fn < E and row[f0 + fn] == row[e0 + ne - 1]):
                    break
                u += 1
            c.add("fix_2_pieces" if k == 2 else "fix_3_or_more_pieces")
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(name, H, p_drop):
    """fp32 operands of one case (the bf16 pipeline takes their bf16 roundings), the cotangents, the dropout mask."""
    tp = topology(name)
    g = torch.Generator().manual_seed(7919 * NAMES.index(name) + H)
    o = SimpleNamespace(tp=tp, H=H, p_drop=p_drop, seed=40503 + H)
    o.AB = torch.randn(tp.N, 2 * H, generator=g)
    o.rh = torch.rand(tp.E, generator=g)
    o.w_r, o.b2, o.bc, o.w3 = [torch.randn(H, generator=g) * 0.5 for _ in range(4)]
    o.W2 = torch.randn(H, H, generator=g) / H ** 0.5
    o.Wc = torch.randn(H, H, generator=g) / H ** 0.5
    o.ds = torch.randn(tp.E, generator=g)
    o.dagg = torch.randn(tp.N, H, generator=g)
    o.keep = fused_edge_keep_mask(o.seed, tp.E, H, p_drop)
    return o


# ------------------------------------------------------------------------------------------------ forward
def forward(o, dt, mode, swap_ab_edge=None, keep=None, row=None, col=None):
    """mode 'bf16': the bf16 pipeline (bf16 operands, S1 and M rounded); 'exact': no rounding at all (the split-bf16 kernel's target);
    'split': the three-product emulation of the split-bf16 kernel.  -> namespace of pre1, S1, pre2, M (the value the segment sum adds),
    Mf (before rounding), d2 = silu'(pre2) * keep, agg, pre3, s and the companions aggA, sA.
    swap_ab_edge / keep: the faults of tests/test_edge_refs_cpu.py."""
    H, tp = o.H, o.tp
    row = tp.row if row is None else row
    col = tp.col if col is None else col
    c = lambda t: t.to(dt)
    AB, W2, Wc = c(o.AB), c(o.W2), c(o.Wc)
    rh, w_r, b2, bc, w3 = c(o.rh), c(o.w_r), c(o.b2), c(o.bc), c(o.w3)
    keep = c(o.keep if keep is None else keep)
    if mode == "bf16":
        AB, W2, Wc = rb(AB), rb(W2), rb(Wc)
    a_, b_ = AB[row, :H], AB[col, H:]
    if swap_ab_edge is not None:
        e = swap_ab_edge
        a_, b_ = a_.clone(), b_.clone()
        a_[e], b_[e] = AB[row[e], H:], AB[col[e], :H]
    f = SimpleNamespace()
    f.pre1 = a_ + b_ + rh[:, None] * w_r
    S1 = torch.nn.functional.silu(f.pre1)

    def contract(X, W):
        if mode == "split":
            (xh, xl), (wh, wl) = split(X), split(W)
            return xl @ wh.T + xh @ wl.T + xh @ wh.T, xh + xl
        if mode == "bf16":
            X = rb(X)
        return X @ W.T, X

    f.pre2, f.S1 = contract(S1, W2)
    f.pre2 = f.pre2 + b2
    m2, d2 = _silu_d(f.pre2)
    f.Mf, f.d2 = m2 * keep, d2 * keep
    f.pre3, f.M = contract(f.Mf, Wc)
    f.pre3 = f.pre3 + bc
    f.agg, f.aggA = segsum(row, f.M, tp.N), segsum(row, f.M.abs(), tp.N)
    t3 = w3 * torch.nn.functional.silu(f.pre3)
    f.s, f.sA = t3.sum(1), t3.abs().sum(1)
    return f


# ------------------------------------------------------------------------------------------------ backward
GRADS = ("dABr", "dABc", "drh", "dw_r", "dW2", "db2", "dWc", "dbc", "dw3")


def backward(o, f, dt, variant):
    """Every gradient kernels.gcl_edge_fused_bwd returns, with the bf16 roundings of the given kernel form (0: fused_edge.hip, 5:
    fused_edge_bwd3.hip, 6: fused_edge_bwd4.hip over what a saving forward left), from the forward `f` of the same dtype ('bf16' mode for
    the bf16 pipeline; 'exact' for variant 6 fed by the split-bf16 saving forward: bf16(M), bf16(silu'(pre2) keep), bf16(pre3) of the
    fp32-grade values, and the bf16 copies of AB, W2, Wc the backward is given).  -> namespace of GRADS and their companions (<name>A),
    plus the stored rows S1, dT, dP2, dP1."""
    H, tp = o.H, o.tp
    row, col = tp.row, tp.col
    c = lambda t: t.to(dt)
    AB, W2, Wc = rb(c(o.AB)), rb(c(o.W2)), rb(c(o.Wc))
    rh, w_r, w3, ds, dagg = c(o.rh), c(o.w_r), c(o.w3), c(o.ds), c(o.dagg)
    M16, d2 = rb(f.M), rb(f.d2)
    z3 = rb(f.pre3) if variant == 6 else f.pre3
    b = SimpleNamespace()
    m3, d3 = _silu_d(z3)
    dTf = (w3[None, :] * ds[:, None]) * d3
    b.dbc, b.dbcA = dTf.sum(0), dTf.abs().sum(0)
    t = m3 * ds[:, None]
    b.dw3, b.dw3A = t.sum(0), t.abs().sum(0)
    b.dT = rb(dTf)
    dP2f = (b.dT @ Wc + dagg[row]) * d2
    b.db2, b.db2A = dP2f.sum(0), dP2f.abs().sum(0)
    b.dP2 = rb(dP2f)
    dS1 = rb(b.dP2 @ W2)
    pre1 = AB[row, :H] + AB[col, H:] + rh[:, None] * w_r
    m1, d1 = _silu_d(pre1)
    b.S1 = rb(m1)
    if variant == 5:
        d1 = rb(d1)
    dP1f = dS1 * d1
    t = dP1f * w_r
    b.drh, b.drhA = t.sum(1), t.abs().sum(1)
    b.dP1 = rb(dP1f)
    t = rh[:, None] * b.dP1
    b.dw_r, b.dw_rA = t.sum(0), t.abs().sum(0)
    b.dABr, b.dABrA = segsum(row, b.dP1, tp.N), segsum(row, b.dP1.abs(), tp.N)
    b.dABc, b.dABcA = segsum(col, b.dP1, tp.N), segsum(col, b.dP1.abs(), tp.N)
    b.dW2, b.dW2A = b.dP2.T @ b.S1, b.dP2.abs().T @ b.S1.abs()
    b.dWc, b.dWcA = b.dT.T @ M16, b.dT.abs().T @ M16.abs()
    return b


# ------------------------------------------------------------------------------------------------ the metric
def _ratio(err, comp):
    """err / comp element-wise; 0 / 0 = 0, x / 0 = inf."""
    err, comp = err.double(), comp.double()
    return torch.where(comp > 0, err / comp.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def err_elems(got, ref64, comp64):
    """max over elements of |got - ref64| / companion."""
    if ref64.numel() == 0:
        return 0.0
    return float(_ratio((got.double() - ref64).abs(), comp64).max())


def err_rows(got, ref64, comp64, rows):
    """Row-wise: max_c |err[r, c]| / max_c companion[r, c], maximum over `rows` (bool [N]: the rows with edges)."""
    if not bool(rows.any()):
        return 0.0
    e = (got.double() - ref64).abs().amax(1)
    return float(_ratio(e, comp64.amax(1))[rows].max())


def bound_bf16(err32):
    return max(MARGIN * err32, FLOOR_BF16)


def bound_x3(err_emul):
    return max(MARGIN * err_emul, FLOOR_X3)


def old_criterion_accepts(got, ref):
    """The forward assertion of tests/test_gpu_kernels.py: max|got - ref| <= 2e-2 max(1, max|ref|)."""
    return float((got - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))


def has_rows(tp):
    """(rows with outgoing edges on the receiving side, nodes read by some edge)."""
    return tp.deg > 0, torch.bincount(tp.col, minlength=tp.N) > 0


def grad_errors(got, ref64, tp):
    """{name: error in the metric} of a backward result (namespace or dict with GRADS) against the float64 restatement `ref64`."""
    rrow, rcol = has_rows(tp)
    g = (lambda n: got[n]) if isinstance(got, dict) else (lambda n: getattr(got, n))
    out = {}
    for n in GRADS:
        ref, comp = getattr(ref64, n), getattr(ref64, n + "A")
        if n in ("dABr", "dABc"):
            out[n] = err_rows(g(n), ref, comp, rrow if n == "dABr" else rcol)
        else:
            out[n] = err_elems(g(n), ref, comp)
    return out


# ------------------------------------------------------------------------------------------------ the saved tiles' fragment order
def frag_index(n_tiles, H):
    """idx [n_tiles * 64, H] (int64): the flat element position of (edge, feature) in the fragment-ordered d2f / z3f arrays of the saving
    forwards.  Header of fused_edge_fwd2.hip: tile t, wave w, quad (i, j), lane l -> 4 consecutive features at
    (((t * NW + w) * 16 + i * 4 + j) * 64 + l) * 4; its SAVE store loop (:127-128, :160, :198; FW_QOFF's comment): the quad holds edge
    t * 64 + i * 16 + (l & 15), features w * 64 + j * 16 + (l >> 4) * 4 .. + 3."""
    NW = H // 64
    e = torch.arange(n_tiles * BM)[:, None]
    ft = torch.arange(H)[None, :]
    t, el = e // BM, e % BM
    i, fr = el // 16, el % 16
    w, fw = ft // 64, ft % 64
    j, cq, k = fw // 16, (fw % 16) // 4, fw % 4
    lane = cq * 16 + fr
    return ((((t * NW + w) * 16 + i * 4 + j) * 64 + lane) * 4 + k).long()


def decode_frag(buf, H):
    """A fragment-ordered [n_tiles * 64, H] array -> row-major [n_tiles * 64, H]."""
    return buf.reshape(-1)[frag_index(buf.shape[0] // BM, H).to(buf.device)]
