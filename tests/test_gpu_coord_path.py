"""GPU: the kernels that move coordinates (ops.edge_geom, ops.coord_update, ops.las_step, ops.inter_attn in both of its forms) and
the edge construction above the LDS limit, each through its public entry against the float64 restatements of tests/coord_refs.py on
the same inputs: forward values, every gradient the op returns, and bit-identical repeats.

Bounds.  For every compared tensor T:  err(T) = max|T - T64| / max(max|T64|, 1e-6), once for the HIP result (err_hip) and once for
the same restatement evaluated by plain torch ops in float32 on the host (err32, the reference's own rounding at that shape).
Asserted: err_hip <= max(8 err32, 64 * 2^-23) (coord_refs.bound; the wide-logit case adds its derived term).  Every figure is printed
before it is asserted (`pytest -s`), DESIGN.md section 2 carries the table.

Clamp-active cases are conditions on the float64 reference, asserted here: 20 % .. 80 % of the updated components clamped and every
pre-clamp component at least 1e-3 clampv away from +-clampv (inputs are regenerated on the host with the next seed until that
holds), so float32 and float64 take the same clamp decision and no component is masked out of a comparison."""
import types

import pytest
import torch

import coord_refs as R
import fabind_oracle as orc

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


def _dev():
    return torch.device("cuda:0")


def _f32(v):
    """A Python float as the kernels receive it (float arguments cross the C interface as fp32)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _run(fn, leaves, cots, dtype, dev):
    """fn(*leaves) -> outputs; the first len(cots) of them are contracted with the cotangents (None: no cotangent on that output).
    -> ([outputs], [gradient of every leaf that is not None])."""
    ls = [None if t is None else t.detach().to(device=dev, dtype=dtype).clone().requires_grad_(True) for t in leaves]
    outs = fn(*ls)
    loss = sum((o * c.to(device=dev, dtype=dtype)).sum() for o, c in zip(outs, cots) if c is not None)
    loss.backward()
    grads = [(l.grad if l.grad is not None else torch.zeros_like(l)) for l in ls if l is not None]
    return [o.detach() for o in outs], grads


def _compare(op, case, names, hip, hip2, ref64, ref32, extra=0.0):
    """Prints and asserts err_hip <= bound(err32) per tensor, finite values, and the bit-identical repeat."""
    assert len(names) == len(hip) == len(hip2) == len(ref64) == len(ref32), (len(names), len(hip), len(ref64))
    fails = []
    for nm, a, a2, r64, r32 in zip(names, hip, hip2, ref64, ref32):
        assert tuple(a.shape) == tuple(r64.shape), (op, case, nm, a.shape, r64.shape)
        assert bool(torch.isfinite(a).all()), (op, case, nm)
        assert torch.equal(a, a2), (op, case, nm, "second run differs")
        e_hip, e32 = R.rel_err(a.cpu(), r64), R.rel_err(r32, r64)
        b = R.bound(e32, extra)
        print("coord-path | %-12s | %-34s | %-9s | err_hip %.2e | err32 %.2e | bound %.2e" % (op, case, nm, e_hip, e32, b))
        if not e_hip <= b:
            fails.append((nm, e_hip, e32, b))
    assert not fails, (op, case, fails)


def _check(op, case, names, hip_fn, ref_fn, leaves, cots, n_out, extra=0.0):
    """hip_fn on the device in fp32 (twice), ref_fn on the host in float64 and float32; compares the first n_out outputs and all gradients."""
    o1, g1 = _run(hip_fn, leaves, cots, torch.float32, _dev())
    o2, g2 = _run(hip_fn, leaves, cots, torch.float32, _dev())
    o64, g64 = _run(ref_fn, leaves, cots, torch.float64, CPU)
    o32, g32 = _run(ref_fn, leaves, cots, torch.float32, CPU)
    assert len(names) == n_out + len(g1)
    _compare(op, case, names, o1[:n_out] + g1, o2[:n_out] + g2, o64[:n_out] + g64, o32[:n_out] + g32, extra)
    return o1, g1, o64


def _clamp_at_median(pre, updated):
    """A clamp value (as fp32) in the middle of the |pre-clamp| components of the updated rows."""
    s = torch.sort(pre[updated].abs().flatten())[0]
    mid = s.numel() // 2
    return _f32(0.5 * (float(s[mid - 1]) + float(s[mid])))


def _clamp_conditions(pre, updated, clampv):
    """(share of the updated components that the clamp cuts, do all components keep the margin to +-clampv)."""
    a = pre[updated].abs().flatten()
    share = float((a > clampv).double().mean())
    return share, bool(((a - clampv).abs() >= 1e-3 * clampv).all())


@pytest.fixture(autouse=True)
def _fp32_mode():
    from fabind_amd import config, engine
    old = config.get_precision()
    engine.set_precision("fp32")
    yield
    engine.set_precision(old)


# ------------------------------------------------------------------------------------------------
# edge_geom
# ------------------------------------------------------------------------------------------------
def _geom_batch(kind):
    """(layout, graph, x [N,3] on the device, batch_id on the host).  'ragged': four complexes -- a compact one (every ligand atom
    within the cut-off of every residue: > 2048 inter edges, rows of > 64), a large ordinary one, one whose ligand is far away (no
    inter edge: its norm is 0) and a small one; 'single': one complex alone."""
    from fabind_amd import engine, synthetic
    dev = _dev()
    if kind == "single":
        inp = synthetic.make_stack_batch([(60, 12)], 8, seed=4, snap=False)
    else:
        inp = synthetic.make_stack_batch([(170, 9), (330, 24), (60, 7), (45, 5)], 8, seed=21, snap=False)
        pr = (inp["segment_id"] > 0.5) & ~inp["is_global"]
        lig = (inp["segment_id"] < 0.5) & ~inp["is_global"]
        g0 = torch.Generator().manual_seed(5)
        sel_l, sel_p = lig & (inp["batch_id"] == 0), pr & (inp["batch_id"] == 0)
        centre = inp["X"][sel_l].mean(0, keepdim=True)
        inp["X"][sel_l] = centre + 0.3 * (torch.rand(int(sel_l.sum()), 1, 3, generator=g0) - 0.5)
        inp["X"][sel_p] = centre + 1.3 * (torch.rand(int(sel_p.sum()), 1, 3, generator=g0) - 0.5) * 2 * 0.75
        inp["X"][lig & (inp["batch_id"] == 2)] += 50.0
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    lay = engine.Layout(t["batch_id"], t["segment_id"])
    br, bc_ = t["compound_edge_index"][0].to(torch.int32), t["compound_edge_index"][1].to(torch.int32)
    x = t["X"][:, 0].contiguous()
    g = engine.Graph(lay, x, br, bc_, lay.ranges(br), 1.6, 2.0)
    return lay, g, x, inp["batch_id"]


@pytest.mark.parametrize("cot", ["d", "rhohat", "both"])
@pytest.mark.parametrize("graph", ["ctx", "inter"])
@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_edge_geom_matches_float64(kind, graph, cot):
    """d, rhohat and dx of ops.edge_geom on the ctx graph (directed star edges; the adjoint's by-column grouping from
    Graph.ctx_by_col and from the sort fallback agree bit for bit) and on the inter graph (grouping = the mirror list), with a
    cotangent on d only, on rhohat only (the None branches of _EdgeGeom.backward) and on both.  The ragged batch holds a complex of
    more than 2 * 1024 edges (several strides of the 1024-thread work-group) with rows of more than 64 edges, and one complex
    WITHOUT inter edges: its norm is 0, and the gradient of its nodes must be exactly 0."""
    from fabind_amd import ops
    lay, g, x, bid = _geom_batch(kind)
    if graph == "ctx":
        row_d, col_d, rp, bycol = g.row_ctx, g.col_ctx, g.rp_ctx, g.ctx_by_col
    else:
        row_d, col_d, rp, bycol = g.row_int, g.col_int, g.rp_int, g.int_by_col
    row, col = row_d.cpu().long(), col_d.cpu().long()
    E = row.numel()
    deg = (rp[1:] - rp[:-1]).cpu().long()
    per_complex = torch.bincount(bid[row], minlength=lay.B)
    if kind == "ragged":
        assert lay.B >= 4 and int(per_complex.max()) > 2048 and int(deg.max()) > 64
        if graph == "inter":
            assert int(per_complex[2]) == 0 and int(per_complex.min()) == 0
    gen = torch.Generator().manual_seed(11)
    co_d = torch.randn(E, 3, generator=gen) if cot in ("d", "both") else None
    co_r = torch.randn(E, generator=gen) if cot in ("rhohat", "both") else None
    ref = lambda x_: R.edge_geom(x_, row, col, bid, lay.B)
    hip = lambda x_: ops.edge_geom(x_, row_d, col_d, rp, lay, bycol)
    _, g1, _ = _check("edge_geom", "%s %s cot=%s" % (kind, graph, cot), ("d", "rhohat", "dx"), hip, ref, [x], (co_d, co_r), 2)
    if graph == "ctx":
        _, g_sort = _run(lambda x_: ops.edge_geom(x_, row_d, col_d, rp, lay, None), [x], (co_d, co_r), torch.float32, _dev())
        assert torch.equal(g1[0], g_sort[0])
    if kind == "ragged" and graph == "inter":
        dx2 = g1[0][bid.to(g1[0].device) == 2]
        assert bool(torch.isfinite(dx2).all()) and bool((dx2 == 0).all())


# ------------------------------------------------------------------------------------------------
# coord_update
# ------------------------------------------------------------------------------------------------
CU_DEGREES = [0, 1, 63, 64, 65, 1500, 0, 2, 9, 130, 1, 0]


def _coord_update_inputs(seed, n_part):
    gen = torch.Generator().manual_seed(seed)
    deg = torch.tensor(CU_DEGREES)
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    return rowptr, torch.randn(deg.numel(), 3, generator=gen), torch.randn(E, 3, generator=gen), 0.5 * torch.randn(E, n_part, generator=gen)


@pytest.mark.parametrize("clamp", ["off", "on"])
@pytest.mark.parametrize("n_part", [1, 4])
@pytest.mark.parametrize("mean", [0, 1])
def test_coord_update_matches_float64(mean, n_part, clamp):
    """x_out and the gradients to x, d and s_part of ops.coord_update on one hand-built CSR with rows of degree 0, 1, 63, 64, 65
    (either side of a wave) and 1500, with the sum and the mean aggregation, 1 and 4 partial columns of s, the clamp never active and
    active on 20 % .. 80 % of the updated components (a gradient that leaks through a clamped component is the kernel's: the margin
    makes fp32 and float64 agree on every clamp decision)."""
    from fabind_amd import ops
    assert all(k in CU_DEGREES for k in (0, 1, 63, 64, 65)) and max(CU_DEGREES) >= 1500
    found = None
    for seed in range(20):
        rowptr, x, d, s_part = _coord_update_inputs(seed, n_part)
        row = R.rows_of(rowptr)
        upd = torch.tensor(CU_DEGREES) > 0
        _, pre = R.coord_update(x.double(), d.double(), s_part.double(), row, mean, float("inf"))
        clampv = _clamp_at_median(pre, upd) if clamp == "on" else _f32(4.0 * float(pre.abs().max()))
        share, margin = _clamp_conditions(pre, upd, clampv)
        if margin and ((0.2 <= share <= 0.8) if clamp == "on" else share == 0.0):
            found = seed
            break
    assert found is not None, "no seed met the clamp conditions"
    print("coord-path | coord_update | seed %d clampv %.6g clamped share %.2f" % (found, clampv, share))
    co = torch.randn(x.shape, generator=torch.Generator().manual_seed(100 + found))
    rp_d = rowptr.to(_dev())
    ref = lambda x_, d_, s_: R.coord_update(x_, d_, s_, row, mean, clampv)
    hip = lambda x_, d_, s_: (ops.coord_update(x_, d_, s_, rp_d, mean, clampv),)
    _check("coord_update", "mean=%d np=%d clamp=%s" % (mean, n_part, clamp), ("x_out", "dx", "dd", "ds_part"), hip, ref,
           [x, d, s_part], (co,), 1)


# ------------------------------------------------------------------------------------------------
# las_step
# ------------------------------------------------------------------------------------------------
LAS_SIZES = [(30, 1), (25, 2), (40, 41), (20, 7), (35, 17)]        # (residues, ligand atoms): C = 2 (no LAS edge) .. 41 atoms


def _las_inputs(seed, both):
    from fabind_amd import synthetic
    inp = synthetic.make_stack_batch(LAS_SIZES, 8, seed=seed, snap=False)
    las = inp["LAS_edge_index"]
    if not both:
        las = las[:, las[0] < las[1]]                                   # each pair listed once: only the second atom is moved
    lig = (inp["segment_id"] < 0.5) & ~inp["is_global"]
    x = inp["X"][:, 0].clone()
    x[lig] += 0.1 * torch.randn(int(lig.sum()), 3, generator=torch.Generator().manual_seed(seed + 50))
    return inp, las, x, inp["coord_LAS"][:, 0].clone()


@pytest.mark.parametrize("clamp", ["production", "active"])
@pytest.mark.parametrize("both", [True, False])
def test_las_step_matches_float64(both, clamp):
    """x_out and dx of ops.las_step against oracle.las_step in float64 on a ragged batch whose ligands run from one atom (C = 2, no
    LAS edge) to 41 atoms (> 64 LAS edges in the complex: the lanes stride), with the LAS list in both directions (as
    synthetic._las_edges makes it) and with each pair listed once; at the production constants (step 1e-3, clamp 3.0: never active)
    and with the step raised until the clamp cuts 20 % .. 80 % of the moved components.  torch.clamp's autograd passes nothing through
    a clamped component; the backward kernel must decide that from the value the forward clamped."""
    from fabind_amd import engine, ops
    dev = _dev()
    clampv, found = 3.0, None
    for seed in range(20):
        inp, las, x, x_las = _las_inputs(seed, both)
        moved = torch.zeros(x.shape[0], dtype=torch.bool)
        moved[las[1]] = True
        _, force = R.las_step(x.double(), x_las.double(), las, 1.0, float("inf"))          # step 1: the summed force itself
        step = _f32(1e-3) if clamp == "production" else _f32(clampv / _clamp_at_median(force, moved))
        share, margin = _clamp_conditions(force * step, moved, clampv)
        if margin and ((0.2 <= share <= 0.8) if clamp == "active" else share == 0.0):
            found = seed
            break
    assert found is not None, "no seed met the clamp conditions"
    per_complex = torch.bincount(inp["batch_id"][las[0]], minlength=len(LAS_SIZES))
    assert int(per_complex[0]) == 0 and int(per_complex.max()) > 64
    print("coord-path | las_step     | seed %d step %.6g clampv %.3g clamped share %.2f, LAS edges per complex %s"
          % (found, step, clampv, share, per_complex.tolist()))
    lay = engine.Layout(inp["batch_id"].to(dev), inp["segment_id"].to(dev))
    li, lj = las[0].to(torch.int32).to(dev).contiguous(), las[1].to(torch.int32).to(dev).contiguous()
    las_d = (li, lj, lay.ranges(li))
    x_las_d = x_las.to(dev).contiguous()
    co = torch.randn(x.shape, generator=torch.Generator().manual_seed(7))
    ref = lambda x_: (R.las_step(x_, x_las.to(x_.dtype), las, step, clampv)[0],)
    hip = lambda x_: (ops.las_step(x_, x_las_d, las_d, lay, step, clampv),)
    _check("las_step", "%s clamp=%s" % ("both directions" if both else "pairs once", clamp), ("x_out", "dx"), hip, ref, [x], (co,), 1)


# ------------------------------------------------------------------------------------------------
# inter_attn
# ------------------------------------------------------------------------------------------------
IA_SPEC = [([0, 1, 8, 9, 63, 64, 65, 140], 150), ([0, 0, 0], 10), ([5, 5, 5, 5], 12)]      # per complex: (ligand-atom degrees, residues)
IA_DEGREES = (0, 1, 8, 9, 63, 64, 65)


def _hand_inter_graph():
    """A symmetric ligand-protein CSR built by hand (node order per complex: glb_c, ligand atoms, glb_p, residues; ligand atom a is
    joined to deg(a) consecutive residues starting at residue 3a, wrapped; columns ascending inside a row), its pair bookkeeping from
    kernels.inter_meta, the deal by degree as engine.Graph makes it -> (namespace with what ops.inter_attn reads, layout, host copies)."""
    from fabind_amd import engine, kernels as K
    dev = _dev()
    nbrs, bid, seg = [], [], []
    off = 0
    for b, (degs, n_res) in enumerate(IA_SPEC):
        nl = len(degs)
        n = nl + n_res + 2
        mine = [[] for _ in range(n)]
        for a, dg in enumerate(degs):
            assert dg <= n_res
            for j in range(dg):
                res = nl + 2 + (3 * a + j) % n_res
                mine[1 + a].append(off + res)
                mine[res].append(off + 1 + a)
        nbrs += [sorted(m) for m in mine]
        bid += [b] * n
        seg += [0.0] * (nl + 1) + [1.0] * (n_res + 1)
        off += n
    N = off
    deg = torch.tensor([len(m) for m in nbrs])
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.tensor([c for m in nbrs for c in m], dtype=torch.int32)
    row = R.rows_of(rowptr).to(torch.int32)
    for k in IA_DEGREES:
        assert int((deg == k).sum()) > 0, k
    assert int(deg.max()) > 128 and int((deg > K.INTER_ATTN_HEAVY).sum()) > 0 and 0 <= int(col.min()) and int(col.max()) < N
    bid_t, seg_t = torch.tensor(bid), torch.tensor(seg)
    lay = engine.Layout(bid_t.to(dev), seg_t.to(dev))
    g = types.SimpleNamespace(rp_int=rowptr.to(dev), col_int=col.to(dev), row_int=row.to(dev))
    _, g.red_idx, g.red_c, g.red_p, g.mirror = K.inter_meta(lay.node_off, lay.c_cnt, lay.B, g.rp_int, g.col_int, g.row_int)
    deg_d = deg.to(torch.int32).to(dev)
    g.int_deal = (torch.argsort(deg_d, descending=True, stable=True).to(torch.int32), int((deg > K.INTER_ATTN_HEAVY).sum()), int((deg > 0).sum()))
    g.int_by_col = lambda: (g.rp_int, g.mirror)
    mir, red = g.mirror.cpu().long(), g.red_idx.cpu().long()
    E = col.numel()
    assert E % 2 == 0 and int(mir.min()) >= 0 and int(mir.max()) < E and int(red.min()) >= 0 and int(red.max()) < E // 2
    assert torch.equal(col.long()[mir], row.long()) and torch.equal(row.long()[mir], col.long()) and torch.equal(red[mir], red)
    return g, lay, dict(row=row.long(), col=col.long(), red_idx=red, deg=deg, bid=bid_t, N=N, E=E)


def _inter_operands(H, n_part, seed, hc):
    """Host fp32 operands of ops.inter_attn on the hand-built graph; d and rhohat come from coordinates, so mirrored edges carry
    d and -d and the same rhohat, as in the model."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.randn(*sh, generator=gen)
    N, E = hc["N"], hc["E"]
    x = rnd(N, 3)
    d, rhohat = R.edge_geom(x, hc["row"], hc["col"], hc["bid"], len(IA_SPEC))
    return dict(qkv=rnd(N, 3 * H) * 0.3, h=rnd(N, H), x=x, d=d.contiguous(), rhohat=rhohat.contiguous(), bias=rnd(E // 2, n_part) * 0.5,
                w_rk=rnd(H) * 0.3, w_rv=rnd(H) * 0.3, wcr=rnd(H) * 0.3, w3=rnd(H) * 0.05, s_ext=rnd(E) * 0.5,
                Wc=rnd(H, H) / H ** 0.5, bc=rnd(H) * 0.1, co_h=rnd(N, H), co_x=rnd(N, 3))


IA_NAMES = ["dqkv", "dcv", "dh", "dx", "dd", "drhohat", "dbias", "dw_rk", "dw_rv", "dwcr", "dw3", "ds_ext", "dWc", "dbc"]


def _inter_case(H, rows, g, hc, o, clampv, with_ext, cv_linear, case, monkeypatch, extra=0.0):
    from fabind_amd import kernels as K, ops
    monkeypatch.setattr(K, "INTER_ATTN_ROWS", rows)
    cv = None if cv_linear else (o["qkv"][:, 2 * H:] @ o["Wc"].T + o["bc"]).contiguous()
    leaves = [o["qkv"], cv, o["h"], o["x"], o["d"], o["rhohat"], o["bias"], o["w_rk"], o["w_rv"], o["wcr"], o["w3"],
              o["s_ext"] if with_ext else None, o["Wc"] if cv_linear else None, o["bc"] if cv_linear else None]
    names = ["h_out", "x_out", "alpha"] + [n for n, l in zip(IA_NAMES, leaves) if l is not None]

    def ref(qkv, cv_, h, x, d, rhohat, bias, w_rk, w_rv, wcr, w3, s_ext=None, Wc=None, bc=None):
        return R.inter_attn(qkv, cv_, h, x, d, rhohat, hc["row"], hc["col"], hc["red_idx"], bias, w_rk, w_rv, wcr, w3, clampv, s_ext, Wc, bc)

    def hip(qkv, cv_, h, x, d, rhohat, bias, w_rk, w_rv, wcr, w3, s_ext=None, Wc=None, bc=None):
        return ops.inter_attn(qkv, cv_, H, h, x, d, rhohat, g, bias, w_rk, w_rv, wcr, w3, clampv, s_ext=s_ext, Wc=Wc, bc=bc)

    o1, _, _ = _check("inter_attn", case, names, hip, ref, leaves, (o["co_h"], o["co_x"], None), 3, extra)
    nodeg = (hc["deg"] == 0).to(o1[0].device)                          # rows without edges pass h and x through, bit for bit
    assert torch.equal(o1[0][nodeg], o["h"].to(o1[0].device)[nodeg]) and torch.equal(o1[1][nodeg], o["x"].to(o1[1].device)[nodeg])


@pytest.mark.parametrize("variant", ["plain", "ext_clamped"])
@pytest.mark.parametrize("rows", [True, False], ids=["dealt_rows", "one_wave_per_row"])
@pytest.mark.parametrize("H", [64, 128, 192, 256, 512, 640])
def test_inter_attn_matches_float64(H, rows, variant, monkeypatch):
    """Both HIP forms of the inter-edge attention (rows dealt by degree, csrc/inter_attn_rows.hip; one wave per row, csrc/attn.hip +
    csrc/bwd.hip), EACH against the float64 restatement: h_out, x_out, alpha and every gradient ops.inter_attn returns, at every
    template width (H <= 256, <= 512, and 640 for the widest; 192 leaves part of a wave idle), on a graph with rows of degree 0, 1, 8
    and 9 (either side of INTER_ATTN_HEAVY), 63, 64, 65 and 140.
    'plain': 4 bias columns, no s_ext, cv evaluated inside from (Wc, bc) at the model's widths (passed directly at 192 / 640, which no
    model uses and the GEMM family does not promise), clamp never active.  'ext_clamped': 1 bias column, s_ext, cv passed directly,
    the clamp active on 20 % .. 80 % of the components of the rows that have edges."""
    g, lay, hc = _hand_inter_graph()
    plain = variant == "plain"
    upd = hc["deg"] > 0
    found = None
    for seed in range(20):
        o = _inter_operands(H, 4 if plain else 1, 1000 * H + seed, hc)
        cv64 = o["qkv"][:, 2 * H:].double() @ o["Wc"].double().T + o["bc"].double()
        pre = R.inter_attn(o["qkv"].double(), cv64, o["h"].double(), o["x"].double(), o["d"].double(), o["rhohat"].double(), hc["row"], hc["col"],
                           hc["red_idx"], o["bias"].double(), o["w_rk"].double(), o["w_rv"].double(), o["wcr"].double(), o["w3"].double(),
                           float("inf"), None if plain else o["s_ext"].double())[4]
        clampv = _f32(4.0 * float(pre.abs().max())) if plain else _clamp_at_median(pre, upd)
        share, margin = _clamp_conditions(pre, upd, clampv)
        if margin and (share == 0.0 if plain else 0.2 <= share <= 0.8):
            found = seed
            break
    assert found is not None, "no seed met the clamp conditions"
    print("coord-path | inter_attn   | seed %d clampv %.6g clamped share %.2f" % (found, clampv, share))
    cv_linear = plain and H in (64, 128, 256, 512)
    _inter_case(H, rows, g, hc, o, clampv, not plain, cv_linear, "H=%d %s %s" % (H, "rows" if rows else "wave", variant), monkeypatch)


@pytest.mark.parametrize("rows", [True, False], ids=["dealt_rows", "one_wave_per_row"])
def test_inter_attn_wide_logit_spread(rows, monkeypatch):
    """Attention biases spread over +-62: the row-wise max - min of the float64 logits lies between 100 and 150 on heavy and on light
    rows (asserted; exp(100) is beyond float32), so a softmax without the running maximum, or a wrong rescale where the four waves of a
    heavy row are combined, gives inf / NaN or a visibly wrong row.  The fast exponential's error grows with its argument: the bound
    carries the derived term 4 * 2^-23 * max|logit - rowmax|."""
    from fabind_amd import kernels as K
    H = 128
    g, lay, hc = _hand_inter_graph()
    o = _inter_operands(H, 4, 77, hc)
    gen = torch.Generator().manual_seed(78)
    o["bias"][:, 0] = (torch.rand(hc["E"] // 2, generator=gen) * 2 - 1) * 62.0
    o["bias"][:, 1:] *= 0.2
    cv64 = o["qkv"][:, 2 * H:].double() @ o["Wc"].double().T + o["bc"].double()
    out = R.inter_attn(o["qkv"].double(), cv64, o["h"].double(), o["x"].double(), o["d"].double(), o["rhohat"].double(), hc["row"], hc["col"],
                       hc["red_idx"], o["bias"].double(), o["w_rk"].double(), o["w_rv"].double(), o["wcr"].double(), o["w3"].double(),
                       float("inf"), o["s_ext"].double())
    logit, pre = out[3], out[4]
    N, row = hc["N"], hc["row"]
    mx = torch.full((N,), float("-inf"), dtype=torch.float64).scatter_reduce(0, row, logit, reduce="amax")
    mn = torch.full((N,), float("inf"), dtype=torch.float64).scatter_reduce(0, row, logit, reduce="amin")
    spread = torch.where(hc["deg"] > 0, mx - mn, torch.zeros(N, dtype=torch.float64))
    wide = (spread >= 100.0) & (spread <= 150.0)
    assert bool((wide & (hc["deg"] > K.INTER_ATTN_HEAVY)).any()) and bool((wide & (hc["deg"] > 1) & (hc["deg"] <= K.INTER_ATTN_HEAVY)).any())
    assert float(spread.max()) <= 150.0
    clampv = _f32(4.0 * float(pre.abs().max()))
    extra = 4.0 * 2.0 ** -23 * float((logit - mx[row]).abs().max())
    print("coord-path | inter_attn   | wide logits: largest row spread %.1f, derived term %.2e" % (float(spread.max()), extra))
    _inter_case(H, rows, g, hc, o, clampv, True, True, "H=128 %s wide logits" % ("rows" if rows else "wave"), monkeypatch, extra)


# ------------------------------------------------------------------------------------------------
# edge construction above the LDS limit
# ------------------------------------------------------------------------------------------------
def test_edges_of_a_complex_beyond_the_lds_limit_match_the_oracle():
    """engine.Graph on a batch of one complex of more than 4096 nodes (EB_LDS_NODES of csrc/graph.hip: its threads walk the
    coordinates in global memory) next to a small one (LDS walk) in the same launch, against oracle.construct_edges in float64: inter
    edges identical including their order, ctx edges identical as sets and row-sorted, every inter edge mirrored.  No pair distance
    lies within 2e-4 of a cut-off (asserted), so the float64 and the fp32 predicate agree."""
    from fabind_amd import engine, synthetic
    dev = _dev()
    inp = synthetic.make_stack_batch([(4200, 20), (50, 8)], 8, seed=2, snap=True)
    n0 = int((inp["batch_id"] == 0).sum())
    assert n0 > 4096
    x64 = inp["X"][:, 0].double()
    for b in range(2):
        xb = x64[inp["batch_id"] == b]
        dist = torch.cdist(xb, xb)
        assert not bool((((dist - 1.6).abs() < 2e-4) | ((dist - 2.0).abs() < 2e-4)).any())
    lay = engine.Layout(inp["batch_id"].to(dev), inp["segment_id"].to(dev))
    br = inp["compound_edge_index"][0].to(torch.int32).to(dev)
    bc_ = inp["compound_edge_index"][1].to(torch.int32).to(dev)
    gr = engine.Graph(lay, inp["X"][:, 0].contiguous().to(dev), br, bc_, lay.ranges(br), 8.0 / 5.0, 10.0 / 5.0)
    gr2 = engine.Graph(lay, inp["X"][:, 0].contiguous().to(dev), br, bc_, lay.ranges(br), 8.0 / 5.0, 10.0 / 5.0)
    ctx, inter = orc.construct_edges(inp["X"].double(), inp["batch_id"], inp["segment_id"], inp["is_global"], 2.0, 1.6)
    ref_ctx = torch.cat([inp["compound_edge_index"], ctx], 1)
    mine_int = torch.stack([gr.row_int.cpu().long(), gr.col_int.cpu().long()])
    assert inter.shape[1] > 0 and torch.equal(mine_int, inter)
    N = lay.N
    mine_ctx = torch.stack([gr.row_ctx.cpu().long(), gr.col_ctx.cpu().long()])
    assert mine_ctx.shape == ref_ctx.shape
    assert torch.equal(torch.sort(mine_ctx[0] * N + mine_ctx[1])[0], torch.sort(ref_ctx[0] * N + ref_ctx[1])[0])
    assert bool((mine_ctx[0][1:] >= mine_ctx[0][:-1]).all())
    mir = gr.mirror.cpu().long()
    assert torch.equal(mine_int[1][mir], mine_int[0]) and torch.equal(mine_int[0][mir], mine_int[1])
    per_complex = torch.bincount(inp["batch_id"][mine_int[0]], minlength=2)
    assert int(per_complex.min()) > 0                                    # both walks produced inter edges
    for a, b in ((gr.row_int, gr2.row_int), (gr.col_int, gr2.col_int), (gr.row_ctx, gr2.row_ctx), (gr.col_ctx, gr2.col_ctx)):
        assert torch.equal(a, b)
