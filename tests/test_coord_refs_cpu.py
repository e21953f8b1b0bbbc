"""CPU: pins the inter-edge attention restatement of tests/coord_refs.py (the float64 reference of tests/test_gpu_coord_path.py) to
per-layer captures of the reference itself, and covers engine.att_edge_params' slicing of the q | k | v projection on the way."""
import types

import numpy as np
import pytest
import torch

import coord_refs as R
import fabind_oracle as orc
from helpers import load_npz, stack_inputs, weights


def _last_iteration_edges(g, sd, inp, monkeypatch):
    """The captures of a golden come from its LAST refinement iteration: the inter edges of that iteration, as the oracle (itself
    pinned to the reference, tests/test_oracle_golden.py) builds them."""
    seen = []
    real = orc.construct_edges

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out
    monkeypatch.setattr(orc, "construct_edges", spy)
    hidden, layers, n_iter, _ = [int(v) for v in g["cfg"]]
    orc.stack_forward(sd, "", inp["X"], inp["H"], inp["batch_id"], inp["segment_id"], inp["mask"], inp["is_global"],
                      inp["compound_edge_index"], inp["LAS_edge_index"], inp["coord_LAS"], layers, n_iter)
    monkeypatch.setattr(orc, "construct_edges", real)
    assert len(seen) == n_iter
    return seen[-1][1]


@pytest.mark.parametrize("name", ["stack_tiny_it3", "stack_tiny_it1"])
@pytest.mark.parametrize("cv_as_linear", [False, True])
def test_inter_attn_restatement_matches_reference_captures(name, cv_as_linear, monkeypatch):
    """From cap_gcl_0.h/x: oracle.cross_attention as oracle.att_forward runs it gives the node features and the pair embedding that
    enter the edge attention; the operands are sliced from the state dict by engine.att_edge_params (de-interleaved k / v columns of
    linear_kv, its radial column, coord_mlp) and the attention bias is attn_bias_proj per undirected pair; the restatement's h_out,
    x_out, alpha against cap_att_0.h/x/alpha at the bounds of tests/test_oracle_golden.py::test_per_layer_intermediates."""
    from fabind_amd import config, engine
    g = load_npz(name)
    sd, inp = weights(g), stack_inputs(g)
    inter = _last_iteration_edges(g, sd, inp, monkeypatch)
    row, col = inter[0], inter[1]
    assert row.numel() == g["cap_att_0.alpha"].shape[0]
    bid = inp["batch_id"]
    lay = orc.Layout(bid, inp["segment_id"])
    p, pm, c, cm = lay.dense(inp["H"])
    z0, zm = orc.interaction(sd, "inter_layer.", p, c, pm, cm)
    z0 = z0 * zm.to(z0.dtype)[..., None]
    h = torch.from_numpy(g["cap_gcl_0.h"])
    x = torch.from_numpy(g["cap_gcl_0.x"])
    pre = "gnn.att_0."
    p, pm, c, cm = lay.dense(h)
    p, c, z = orc.cross_attention(sd, pre + "cross_attn_module.", p, pm, c, cm, z0, zm)
    h = lay.undense(p, c)
    N, H = h.shape

    # operands: the engine's own parameter slicing, on the CPU
    lin = lambda n, bias=True: types.SimpleNamespace(weight=sd[pre + n + ".weight"], bias=sd[pre + n + ".bias"] if bias else None)
    m = types.SimpleNamespace(linear_q=lin("linear_q"), linear_kv=lin("linear_kv"), coord_mlp=[lin("coord_mlp.0"), None, lin("coord_mlp.2", False)])
    old = config.get_precision()
    config.set_precision("fp32")
    try:
        P = engine.att_edge_params(m)
    finally:
        config.set_precision(old)
    assert P["Wqkv"].dtype == torch.float32 and tuple(P["Wqkv"].shape) == (3 * H, H)
    qkv = h @ P["Wqkv"].T + P["bqkv"]

    # one attention-bias value per undirected ligand-protein pair, red_idx: edge -> its pair
    lig_row = lay.is_c[row]
    cn, pn = torch.where(lig_row, row, col), torch.where(lig_row, col, row)
    key, red_idx = torch.unique(cn * N + pn, return_inverse=True)
    assert 2 * key.numel() == row.numel()                              # every pair listed in both directions
    rc, rp = key // N, key % N
    pair = z[bid[rc], lay.p_local[rp], lay.c_local[rc]]                # [n_red, H]
    bias_part = orc._lin(sd, pre + "attn_bias_proj", pair)             # [n_red, 1]

    d, rhohat = R.edge_geom(x, row, col, bid, lay.B)
    clampv = 10.0 / 5.0
    kw = dict(Wc=P["Wc"], bc=P["bc"]) if cv_as_linear else {}
    cv = None if cv_as_linear else qkv[:, 2 * H:] @ P["Wc"].T + P["bc"]
    h_out, x_out, alpha, _, _ = R.inter_attn(qkv, cv, h, x, d, rhohat, row, col, red_idx, bias_part, P["w_rk"], P["w_rv"], P["wcr"],
                                             P["w3"], clampv, **kw)
    for k, got in (("att_0.h", h_out), ("att_0.x", x_out), ("att_0.alpha", alpha)):
        ref = g["cap_" + k]
        assert np.abs(got.numpy().reshape(ref.shape) - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), k
    # the captures would not notice a restatement that ignored its inputs' structure: the attention must have moved something
    assert np.abs(g["cap_att_0.x"] - g["cap_gcl_0.x"]).max() > 1e-4 and np.abs(g["cap_att_0.h"] - h.numpy()).max() > 1e-3


def test_restatements_agree_with_the_oracle_layers_in_float64():
    """coord_update with `mean` against the coordinate half of oracle.gcl_forward's formula and las_step against oracle.las_step, on a
    small hand-made graph in float64 (exact up to rounding): the helper's own argument handling, including a row without edges."""
    g = torch.Generator().manual_seed(0)
    n = 7
    row = torch.tensor([0, 0, 0, 2, 3, 3, 6])
    col = torch.tensor([1, 2, 3, 0, 0, 6, 3])
    x = torch.randn(n, 3, generator=g, dtype=torch.float64)
    s_part = torch.randn(row.numel(), 4, generator=g, dtype=torch.float64)
    d = x[row] - x[col]
    trans = d * s_part.sum(1, keepdim=True)
    cnt = orc.seg_sum(torch.ones_like(trans), row, n).clamp(min=1)
    want = x + (orc.seg_sum(trans, row, n) / cnt).clamp(-0.3, 0.3)
    got, pre_ = R.coord_update(x, d, s_part, row, True, 0.3)
    assert torch.allclose(got, want, rtol=0, atol=1e-14) and bool((pre_.abs() > 0.3).any()) and torch.equal(got[1], x[1])
    want_sum = x + orc.seg_sum(trans, row, n).clamp(-0.3, 0.3)
    assert torch.allclose(R.coord_update(x, d, s_part, row, False, 0.3)[0], want_sum, rtol=0, atol=1e-14)
    x_las = torch.randn(n, 3, generator=g, dtype=torch.float64)
    las = torch.stack([row, col])
    out, pre_ = R.las_step(x, x_las, las, 1e-2, 0.05)
    assert torch.equal(out, orc.las_step(x, x_las, las, 1e-2, 0.05))
    assert torch.allclose(out, x + pre_.clamp(-0.05, 0.05), rtol=0, atol=1e-15)
    assert torch.equal(R.rows_of(torch.tensor([0, 3, 3, 4, 6, 6, 6, 7], dtype=torch.int32)), row)
