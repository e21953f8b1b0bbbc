"""CPU: tests/edge_refs.py checked on its own -- the topology table reaches every seam class of the 64-edge tiles, the float32
restatement follows the float64 one, the fragment map of the saved tiles is a bijection, and the row-wise companion metric rejects the
faults a fused edge kernel can have (a dropped edge of a light row, a dropped boundary piece, exchanged A / B halves, a dropout mask
shifted by one edge, a tile missing from a weight gradient) by at least twice its bound -- while the earlier criterion of
tests/test_gpu_kernels.py, 2e-2 of the largest entry of the whole tensor, accepts the dropped edge."""
import pytest
import torch

import coord_refs as CR
import edge_refs as ER

F64, F32 = ER.F64, ER.F32


def test_topology_table_reaches_every_seam_class():
    seen, tiles = {}, {}
    for name in ER.NAMES:
        tp = ER.topology(name)
        assert tp.N <= 400 and 1 <= tp.E <= 2000, name
        assert bool((tp.row[1:] >= tp.row[:-1]).all()) and int(tp.rowptr[-1]) == tp.E
        heavy = tp.deg > ER.BM
        assert int(tp.deg[~heavy].max()) <= 40, name                       # a row is light (<= 40 edges) or spans tiles
        tiles[name] = (tp.E + ER.BM - 1) // ER.BM
        for c in ER.tile_classes(tp.row):
            for k in c:
                seen.setdefault(k, set()).add(name)
    want = ("head_cont", "tail_cont", "through", "whole_tile_run_starts_on_seam", "whole_tile_run_stops_on_seam", "whole_tile_run_stops_at_E",
            "two_spanning_runs", "run_starts_on_seam", "run_ends_on_seam", "run_ends_at_E", "ragged_last", "full_last",
            "spanning_run_ends_at_E", "empty_rows_at_seam", "fix_2_pieces", "fix_3_or_more_pieces")
    assert not [k for k in want if k not in seen], [k for k in want if k not in seen]
    # the named cases of the table are what their names say
    E = {n: ER.topology(n).E for n in ER.NAMES}
    assert E["one_edge"] == 1 and E["ragged37"] == 37 and E["exact64"] == 64 and E["seam128"] == 128 and E["single_row"] == 150
    assert E["tiles8"] % ER.BM == 0
    r = ER.topology("seam128").row
    assert r[63] != r[64]
    r = ER.topology("straddle").row
    assert r[62] != r[63] and r[63] == r[64] and r[64] != r[65]
    tp = ER.topology("row200")
    assert int(tp.rowptr[2]) == 30 and int(tp.deg[2]) == 200
    assert [sorted(c & {"head_cont", "tail_cont", "through"}) for c in ER.tile_classes(tp.row)] == \
        [["tail_cont"], ["head_cont", "tail_cont", "through"], ["head_cont", "tail_cont", "through"], ["head_cont", "tail_cont"], ["head_cont"]]
    tp = ER.topology("aligned128")
    assert int(tp.rowptr[2]) == 64 and int(tp.rowptr[3]) == 192
    tp = ER.topology("heavy_to_end")
    assert int(tp.row[-1]) == tp.N - 1 and int(tp.deg[-1]) > ER.BM and tp.E % ER.BM != 0
    tp = ER.topology("empty_rows")
    assert tp.deg[0] == 0 and tp.deg[-1] == 0 and int(tp.rowptr[4]) == 64 and tp.deg[4] == 0 and int(tp.rowptr[8]) == 128 and tp.deg[8] == 0
    assert "two_spanning_runs" in seen and "two_heavy" in seen["two_spanning_runs"]
    assert [tiles[n] for n in ("tiles7", "tiles8", "tiles9", "tiles17")] == [7, 8, 9, 17]
    assert tiles[ER.GROUPS_TOPOLOGY] >= 25
    assert all(tiles[n] <= 4 for n in ER.SMALL_TILES)
    # the sending side: a node nobody reads, a node read by more than one tile's worth of edges
    for name in ER.NAMES:
        tp = ER.topology(name)
        indeg = torch.bincount(tp.col, minlength=tp.N)
        assert int(indeg[tp.silent]) == 0, name
        if tp.hub is not None:
            assert int(indeg[tp.hub]) > ER.BM, name
    assert sum(ER.topology(n).hub is not None for n in ER.NAMES) >= 10


@pytest.mark.parametrize("H", [64, 128, 256, 512])
def test_fragment_map_is_a_bijection(H):
    for nt in (1, 3):
        idx = ER.frag_index(nt, H)
        assert idx.shape == (nt * ER.BM, H)
        assert torch.equal(torch.sort(idx.reshape(-1))[0], torch.arange(nt * ER.BM * H))
        # a lane's quad is four consecutive features of one edge at four consecutive positions; a store instruction (64 lanes) is contiguous
        assert bool((idx[:, 1::4] == idx[:, 0::4] + 1).all()) and bool((idx[:, 3::4] == idx[:, 0::4] + 3).all())
        assert bool((idx[:, 0::4] % 4 == 0).all())
        buf = torch.arange(nt * ER.BM * H, dtype=torch.float32).reshape(nt * ER.BM, H)
        assert torch.equal(ER.decode_frag(buf, H).reshape(-1)[torch.argsort(idx.reshape(-1))], buf.reshape(-1))
    # tile t, wave w, quad (i, j), lane l of the kernel's formula, spelled out for one element
    NW = H // 64
    t, w, i, j, l, k = 2, NW - 1, 3, 1, 37, 2
    pos = ((((t * NW + w) * 16 + i * 4 + j) * 64 + l) * 4) + k
    assert int(ER.frag_index(3, H)[t * 64 + i * 16 + (l & 15), w * 64 + j * 16 + (l >> 4) * 4 + k]) == pos


CASES32 = [(n, 64, p) for n in ER.NAMES for p in (0.0, 0.25)] + [(n, 256, 0.25) for n in ("straddle", "tiles9")]


@pytest.mark.parametrize("name,H,p", CASES32)
def test_float32_restatement_follows_float64(name, H, p):
    """Same rounding points, two arithmetics.  Outputs that are not rounded again (the exact pipeline) within coord_refs.bound of
    float64 as plain relative errors; the bf16 pipeline -- where a float32 rounding can flip a bf16 rounding downstream -- in the
    companion metric, within the two-ulp floor."""
    o = ER.operands(name, H, p)
    tp = o.tp
    rrow, _ = ER.has_rows(tp)
    f64, f32 = ER.forward(o, F64, "exact"), ER.forward(o, F32, "exact")
    for nm in ("agg", "s"):
        e = CR.rel_err(getattr(f32, nm), getattr(f64, nm))
        assert e <= CR.bound(0.0), (nm, e)
    em = ER.forward(o, F64, "split")
    e_agg, e_s = ER.err_rows(em.agg, f64.agg, f64.aggA, rrow), ER.err_elems(em.s, f64.s, f64.sA)
    assert e_agg <= 2.0 ** -15 and e_s <= 2.0 ** -15, (e_agg, e_s)         # three products of 16-bit operands: 2^-16-grade terms
    b64, b32 = ER.forward(o, F64, "bf16"), ER.forward(o, F32, "bf16")
    assert ER.err_rows(b32.agg, b64.agg, b64.aggA, rrow) <= ER.FLOOR_BF16
    assert ER.err_elems(b32.s, b64.s, b64.sA) <= ER.FLOOR_BF16
    for variant, (g64, g32) in ((0, (b64, b32)), (5, (b64, b32)), (6, (b64, b32)), (6, (f64, f32))):
        e = ER.grad_errors(ER.backward(o, g32, F32, variant), ER.backward(o, g64, F64, variant), tp)
        assert all(v <= ER.FLOOR_BF16 for v in e.values()), (variant, e)


def test_backward_restatement_is_the_autograd_gradient_without_roundings(monkeypatch):
    """The hand-written adjoint against torch autograd in float64 on an unrounded pipeline (rb replaced by the identity)."""
    o = ER.operands("straddle", 64, 0.25)
    tp, H = o.tp, o.H
    monkeypatch.setattr(ER, "rb", lambda t: t)
    f = ER.forward(o, F64, "exact")
    b = ER.backward(o, f, F64, 0)
    leaf = lambda t: t.double().clone().requires_grad_(True)
    AB, rh, w_r, W2, b2, Wc, bc, w3 = map(leaf, (o.AB, o.rh, o.w_r, o.W2, o.b2, o.Wc, o.bc, o.w3))
    silu = torch.nn.functional.silu
    S1 = silu(AB[tp.row, :H] + AB[tp.col, H:] + rh[:, None] * w_r)
    M = silu(S1 @ W2.T + b2) * o.keep.double()
    agg = torch.zeros(tp.N, H, dtype=F64).index_add(0, tp.row, M)
    s = (silu(M @ Wc.T + bc) * w3).sum(1)
    ((agg * o.dagg.double()).sum() + (s * o.ds.double()).sum()).backward()
    got = {"dABr": b.dABr, "dABc": b.dABc, "drh": b.drh, "dw_r": b.dw_r, "dW2": b.dW2, "db2": b.db2, "dWc": b.dWc, "dbc": b.dbc, "dw3": b.dw3}
    ref = {"dABr": AB.grad[:, :H], "dABc": AB.grad[:, H:], "drh": rh.grad, "dw_r": w_r.grad, "dW2": W2.grad, "db2": b2.grad, "dWc": Wc.grad,
           "dbc": bc.grad, "dw3": w3.grad}
    for k in ER.GRADS:
        assert CR.rel_err(got[k], ref[k]) <= 1e-12, k
    assert CR.rel_err(f.agg, agg.detach()) <= 1e-13 and CR.rel_err(f.s, s.detach()) <= 1e-13


# ------------------------------------------------------------------------------------------------ the faults
def _bound(o):
    """The bound the GPU test would apply to agg and s of this case: max(8 err32, 2^-7) in the metric."""
    rrow, _ = ER.has_rows(o.tp)
    f64, f32 = ER.forward(o, F64, "bf16"), ER.forward(o, F32, "bf16")
    return (f64, ER.bound_bf16(ER.err_rows(f32.agg, f64.agg, f64.aggA, rrow)), ER.bound_bf16(ER.err_elems(f32.s, f64.s, f64.sA)))


def _light_row(tp):
    """The highest-degree row that is not heavy."""
    d = tp.deg.clone()
    d[d > ER.BM] = 0
    return int(torch.argmax(d))


@pytest.mark.parametrize("H", [64, 128, 512])
@pytest.mark.parametrize("name", ["row200", "two_heavy", "tiles17", "tiles27"])
def test_dropped_edge_of_a_light_row(name, H):
    """One edge's message missing from the sum of the busiest light row: rejected at twice the bound by the row-wise metric."""
    o = ER.operands(name, H, 0.0)
    tp = o.tp
    f64, b_agg, _ = _bound(o)
    r = _light_row(tp)
    e = int(tp.rowptr[r]) + int(tp.deg[r]) // 2
    bad = f64.agg.clone()
    bad[r] -= f64.M[e]
    err = ER.err_rows(bad, f64.agg, f64.aggA, tp.deg > 0)
    print("dropped edge | %-10s H=%3d | degree %d | metric %.2e | bound %.2e" % (name, H, int(tp.deg[r]), err, b_agg))
    assert err >= 2.0 * b_agg, (err, b_agg)


@pytest.mark.parametrize("H", [64, 128, 512])
def test_earlier_criterion_accepts_the_dropped_edge(H):
    """Why this file exists: with one heavy row in the graph, 2e-2 of the largest |agg| is more than a whole message, so the earlier
    forward assertion passes with an edge missing from the busiest light row -- and with the lightest row missing whole; the row-wise
    metric rejects both. Shown on the table's own heavy-row topology and on the topology of test_fused_edge_pipeline_matches_unfused."""
    g = torch.Generator().manual_seed(H)
    deg = torch.randint(0, 40, (300,), generator=g)
    deg[7] = 333
    cases = [(ER.operands(ER.GROUPS_TOPOLOGY, H, 0.0), None)]
    # the existing test's draw, as a topology of its own (it is larger than the table allows)
    row = torch.repeat_interleave(torch.arange(300), deg)
    col = torch.randint(0, 300, (row.shape[0],), generator=g)
    o2 = ER.SimpleNamespace(**vars(ER.operands(ER.GROUPS_TOPOLOGY, H, 0.0)))
    o2.tp = ER.SimpleNamespace(N=300, E=row.shape[0], deg=deg, row=row, col=col,
                               rowptr=torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(deg, 0)]))
    o2.AB = torch.randn(300, 2 * H, generator=g)
    o2.rh = torch.rand(o2.tp.E, generator=g)
    o2.keep = torch.ones(o2.tp.E, H)
    cases.append((o2, None))
    for o, _ in cases:
        tp = o.tp
        f64 = ER.forward(o, F64, "bf16")
        f32 = ER.forward(o, F32, "bf16")
        bnd = ER.bound_bf16(ER.err_rows(f32.agg, f64.agg, f64.aggA, tp.deg > 0))
        r = _light_row(tp)
        e = int(tp.rowptr[r]) + int(tp.deg[r]) // 2
        bad = f64.agg.clone()
        bad[r] -= f64.M[e]
        d = tp.deg.clone()
        d[d == 0] = 10 ** 6
        r1 = int(torch.argmin(d))                                           # the lightest row that has edges, dropped whole
        gone = f64.agg.clone()
        gone[r1] = 0.0
        for what, t, rr in (("one edge", bad, r), ("whole row", gone, r1)):
            err = ER.err_rows(t, f64.agg, f64.aggA, tp.deg > 0)
            old = float((t - f64.agg).abs().max()) / max(1.0, float(f64.agg.abs().max()))
            print("earlier criterion | E=%4d H=%3d | %-9s of a degree-%d row | old metric %.2e (bound 2e-2) | row-wise %.2e (bound %.2e)"
                  % (tp.E, H, what, int(tp.deg[rr]), old, err, bnd))
            assert ER.old_criterion_accepts(t, f64.agg), what
            assert err >= 2.0 * bnd, (what, err, bnd)


@pytest.mark.parametrize("name", ["straddle", "row200", "aligned128", "heavy_to_end", "single_row", "two_heavy"])
def test_dropped_boundary_piece(name):
    """One tile's piece of a tile-spanning row missing from its sum (a boundary slot not added by the fix-up)."""
    o = ER.operands(name, 64, 0.25)
    tp = o.tp
    f64, b_agg, _ = _bound(o)
    r = int(tp.row[ER.BM])                                                  # the row that holds edge 64 spans a seam in each of these
    lo, hi = int(tp.rowptr[r]), int(tp.rowptr[r + 1])
    seam = (lo // ER.BM + 1) * ER.BM
    assert lo < seam < hi
    for piece in (slice(lo, seam), slice(seam, min(seam + ER.BM, hi))):
        bad = f64.agg.clone()
        bad[r] -= f64.M[piece].sum(0)
        err = ER.err_rows(bad, f64.agg, f64.aggA, tp.deg > 0)
        assert err >= 2.0 * b_agg, (piece, err, b_agg)


@pytest.mark.parametrize("name", ["ragged37", "seam128", "tiles9"])
def test_exchanged_halves_of_one_edge(name):
    """A[col] + B[row] instead of A[row] + B[col] for one edge: its scalar s and its row of agg leave the bound."""
    o = ER.operands(name, 64, 0.0)
    tp = o.tp
    f64, b_agg, b_s = _bound(o)
    e = tp.E // 2
    assert int(tp.row[e]) != int(tp.col[e])
    bad = ER.forward(o, F64, "bf16", swap_ab_edge=e)
    e_s = ER.err_elems(bad.s, f64.s, f64.sA)
    e_a = ER.err_rows(bad.agg, f64.agg, f64.aggA, tp.deg > 0)
    assert e_s >= 2.0 * b_s and e_a >= 2.0 * b_agg, (e_s, b_s, e_a, b_agg)     # (light rows, degree <= 40: one message is >= 1/40 of the sum)
    g64, gbad = ER.backward(o, f64, F64, 5), ER.backward(o, bad, F64, 5)
    eg = ER.grad_errors(gbad, g64, tp)
    assert eg["drh"] >= 2.0 * ER.FLOOR_BF16, eg


@pytest.mark.parametrize("name", ["one_edge", "exact64", "tiles8"])
def test_dropout_mask_shifted_by_one_edge(name):
    o = ER.operands(name, 64, 0.25)
    tp = o.tp
    f64, b_agg, b_s = _bound(o)
    # (E = 1: the mask of edge 1 for edge 0)
    import helpers
    keep = helpers.fused_edge_keep_mask(o.seed, tp.E + 1, o.H, o.p_drop)[1:]
    assert not torch.equal(keep, o.keep)
    bad = ER.forward(o, F64, "bf16", keep=keep)
    assert ER.err_rows(bad.agg, f64.agg, f64.aggA, tp.deg > 0) >= 2.0 * b_agg
    assert ER.err_elems(bad.s, f64.s, f64.sA) >= 2.0 * b_s


@pytest.mark.parametrize("variant", [0, 5, 6])
@pytest.mark.parametrize("name", ER.SMALL_TILES)
def test_tile_missing_from_a_weight_gradient(name, variant):
    o = ER.operands(name, 64, 0.25)
    tp = o.tp
    f64, f32 = ER.forward(o, F64, "bf16"), ER.forward(o, F32, "bf16")
    g64 = ER.backward(o, f64, F64, variant)
    e32 = ER.grad_errors(ER.backward(o, f32, F32, variant), g64, tp)
    M16 = ER.rb(f64.M)
    for t in range((tp.E + ER.BM - 1) // ER.BM):
        sl = slice(t * ER.BM, min(tp.E, (t + 1) * ER.BM))
        bad = {k: getattr(g64, k) for k in ER.GRADS}
        bad["dW2"] = g64.dW2 - g64.dP2[sl].T @ g64.S1[sl]
        bad["dWc"] = g64.dWc - g64.dT[sl].T @ M16[sl]
        bad["db2"] = g64.db2 - (g64.dP2[sl]).sum(0)
        e = ER.grad_errors(bad, g64, tp)
        for k in ("dW2", "dWc", "db2"):
            assert e[k] >= 2.0 * ER.bound_bf16(e32[k]), (t, k, e[k], e32[k])
