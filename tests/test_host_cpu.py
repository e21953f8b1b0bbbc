"""CPU: host-side logic -- state_dict compatibility with the reference's key set, the C-ABI library
loads and exports every symbol include/fabind_hip.h declares, and the product path refuses to run on CPU."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load_npz, weights
from test_gpu_stack import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Logger:
    def log_message(self, s):
        self.msg = s


def test_state_dict_keys_match_reference_capture():
    from fabind_amd.models import get_model
    g = load_npz("model_tiny")
    hidden, pocket_hidden, layers, n_iter, _ = [int(v) for v in g["cfg"]]
    a = _args(hidden, layers, n_iter)
    a.pocket_pred_hidden_size = pocket_hidden
    lg = _Logger()
    m = get_model(a, lg, None)
    assert lg.msg == "FABind"
    ref = weights(g)
    mine = m.state_dict()
    assert set(ref) == set(mine)
    assert all(tuple(ref[k].shape) == tuple(mine[k].shape) for k in ref)
    m.load_state_dict(ref, strict=True)


def test_production_model_has_394_keys_and_36M_parameters():
    from fabind_amd.models import get_model
    m = get_model(_args(512, 4, 8), _Logger(), None)
    m.pocket_pred_model  # noqa: B018
    a = _args(512, 4, 8)
    a.pocket_pred_hidden_size = 128
    m = get_model(a, _Logger(), None)
    assert len(m.state_dict()) == 394
    assert sum(p.numel() for p in m.parameters()) == 36270615


def test_library_exports_every_declared_symbol():
    from fabind_amd import _lib
    lib = _lib.load()                                        # loads without a GPU (HIP initialises lazily)
    from fabind_amd import _lib as L
    import ctypes
    assert lib.fabind_abi_version() == L.ABI_VERSION == 19
    # the ctypes mirrors have the library's struct sizes (load() refuses a mismatch; checked again here explicitly)
    for which, mirror in enumerate((L.GemmArgs, L.EdgeBwdArgs, L.PairUpdateArgs, L.TnJob, L.AttnFusedBwdArgs)):
        assert lib.fabind_sizeof_args(which) == ctypes.sizeof(mirror)
    assert lib.fabind_sizeof_args(99) == -1
    from fabind_amd import kernels as K
    assert K._TNJOB.itemsize == ctypes.sizeof(L.TnJob)        # the numpy form of the job table the queue uploads
    assert [n for n, _ in L.TnJob._fields_] == list(K._TNJOB.names)
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    names = set(re.findall(r"\b(fabind_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 30
    for n in sorted(names):
        assert hasattr(lib, n), "missing export: " + n
    for n in _lib.SIGNATURES:
        assert n in names, "binding without declaration: " + n


def test_product_path_refuses_cpu_tensors():
    """No silent CPU/eager fallback: the stack raises when handed host tensors."""
    from fabind_amd import synthetic
    from fabind_amd.models.att_model import EfficientMCAttModel
    m = EfficientMCAttModel(_args(32, 1, 1), 32, 32, 1, n_layers=1, n_iter=1, normalize_coord=lambda x: x / 5.0,
                            unnormalize_coord=lambda x: x * 5.0).eval()
    inp = synthetic.make_stack_batch([(20, 5)], 32, seed=0)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(inp["X"], inp["H"], inp["batch_id"], inp["segment_id"], inp["mask"], inp["is_global"],
          inp["compound_edge_index"], inp["LAS_edge_index"], inp["coord_LAS"])


def test_synthetic_generator_matches_survey_counts():
    """Seed-0 synthetic 1500/40 complex: edge counts of SURVEY.md 8(d) (E_c 24,048 incl. bonds/stars, E_i 2,648) are
    reproduced to within generator differences by the oracle's edge builder."""
    import fabind_oracle as orc
    from fabind_amd import synthetic
    inp = synthetic.make_stack_batch([(300, 30)], 8, seed=0)
    ctx, inter = orc.construct_edges(inp["X"], inp["batch_id"], inp["segment_id"], inp["is_global"], 2.0, 1.6)
    n_star = 2 * (300 + 30) + 2
    assert ctx.shape[1] > n_star and inter.shape[1] % 2 == 0 and inter.shape[1] > 0
    assert torch.all(inter[0][1:] >= inter[0][:-1])          # row-sorted


def _plus_args(hidden, pocket_hidden, layers, n_iter, min_radius=20.0):
    a = _args(hidden, layers, n_iter)
    for k, v in dict(pocket_pred_hidden_size=pocket_hidden, use_ln_mlp=True, mlp_hidden_scale=1, dropout=0.1, mha_heads=4,
                     rel_dis_pair_bias="no", inter_additional_mlp=False, only_last_LAS=False, geom_reg_steps=1,
                     use_for_radius_pred="ligand", dis_map_thres=15.0, pocket_radius_buffer=5.0, min_pocket_radius=min_radius,
                     force_fix_radius=False, use_clustering=False).items():
        setattr(a, k, v)
    return a


def test_plus_state_dict_keys_match_reference_capture():
    """FABind+: the host mirror loads the reference FABindPlus state_dict strictly."""
    from fabind_amd.plus.models import get_model
    g = load_npz("plus_model_tiny")
    hidden, pocket_hidden, layers, n_iter, _ = [int(v) for v in g["cfg"]]
    lg = _Logger()
    m = get_model(_plus_args(hidden, pocket_hidden, layers, n_iter), lg)
    assert lg.msg == "FABind plus"
    ref, mine = weights(g), m.state_dict()
    assert set(ref) == set(mine)
    assert all(tuple(ref[k].shape) == tuple(mine[k].shape) for k in ref)
    m.load_state_dict(ref, strict=True)


def test_plus_production_stack_parameter_count():
    """the FABind+ production stack (L=5, use_ln_mlp, mlp_hidden_scale=1, H=512) has 42,507,437 parameters."""
    from fabind_amd.plus.models.att_model import EfficientMCAttModel
    m = EfficientMCAttModel(_plus_args(512, 128, 5, 8), 512, 512, 1, n_layers=5, n_iter=8, normalize_coord=lambda x: x / 5.0,
                            unnormalize_coord=lambda x: x * 5.0)
    assert sum(p.numel() for p in m.parameters()) == 42507437


def test_plus_stack_refuses_cpu_tensors():
    from fabind_amd.plus.models.att_model import EfficientMCAttModel
    m = EfficientMCAttModel(_plus_args(32, 32, 1, 1), 32, 32, 1, n_layers=1, n_iter=1, normalize_coord=lambda x: x / 5.0,
                            unnormalize_coord=lambda x: x * 5.0).eval()
    X, H = torch.zeros(6, 1, 3), torch.zeros(6, 32)
    z = torch.zeros(6, dtype=torch.long)
    with pytest.raises(RuntimeError):
        m(X, H, z, z.bool(), z.bool(), z.bool(), torch.zeros(2, 0, dtype=torch.long), torch.zeros(2, 0, dtype=torch.long), X)


def _eval_fixture(device):
    import numpy as np
    import torch
    from helpers import load_npz
    g = load_npz("eval_metrics")
    names = ["coords", "compound_batch", "y_pred", "y_pred_by_coords", "pocket_cls_pred", "pocket_cls",
             "protein_out_mask_whole", "protein_coords_batched_whole", "pred_pocket_center", "dis_map"]
    batches = []
    for bi in range(int(g["n_batches"])):
        out = tuple(torch.from_numpy(np.asarray(g["b%d_%s" % (bi, n)])).to(device) for n in names) + (int(g["b%d_keepNode_less_5" % bi]),)
        batches.append((out, torch.from_numpy(g["b%d_data_coords" % bi]).to(device),
                        torch.from_numpy(g["b%d_coords_center" % bi]).to(device)))
    ref = {k.split("::", 1)[1]: float(v) for k, v in g.items() if k.startswith("metric::")}
    return batches, ref, float(g["gs_tau"])


def check_eval_metrics(device):
    """fabind_amd.utils.metrics against the metrics dict the reference's own evaluation loop (utils/utils.py:445-604)
    returned for the same per-batch model outputs (tests/golden/eval_metrics.npz, oracle/make_golden.py `eval`)."""
    from argparse import Namespace
    import torch
    from fabind_amd.utils.metrics import Evaluator, evaluate_mean_pocket_cls_coord_multi_task
    batches, ref, tau = _eval_fixture(device)
    args = Namespace(pair_distance_loss_weight=1.0, pair_distance_distill_loss_weight=1.0, pocket_cls_loss_weight=1.0,
                     pocket_distance_loss_weight=0.05, coord_loss_weight=1.0, gs_tau=tau)
    nn = torch.nn
    crit = (nn.SmoothL1Loss(), nn.MSELoss(), nn.BCEWithLogitsLoss(reduction="mean"), nn.HuberLoss(delta=3.0))
    ev = Evaluator(args, *crit, pred_dis=True)
    for out, coords, center in batches:
        ev.update(out, coords, center)
    got = ev.compute()
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert abs(got[k] - v) <= 2e-5 * max(1.0, abs(v)), (k, got[k], v)
    assert got["skip_samples"] == 3 and got["samples"] == 11          # the fixture exercises the all-negative branch

    class _D:                                                          # the reference's call signature, loader of batches
        def __init__(self, c, z):
            self.coords, self.coords_center = c, z

        def to(self, device):
            return self
    it = iter([b[0] for b in batches])
    got2 = evaluate_mean_pocket_cls_coord_multi_task(None, args, [_D(c, z) for _, c, z in batches], lambda data, stage: next(it),
                                                     *crit, 0.01, device, pred_dis=True, stage=1)
    assert got2 == got


def test_eval_metrics_match_reference_loop():
    import torch
    check_eval_metrics(torch.device("cpu"))


def test_ctypes_signatures_match_the_header_prototypes():
    """Every `int fabind_*(...)` prototype of include/fabind_hip.h against fabind_amd._lib.SIGNATURES: same entry points,
    same parameter count, and pointer / int / float kinds in the same positions (ctypes itself cannot detect a binding
    that passes fewer or differently typed arguments than the C side reads)."""
    import ctypes
    import os
    import re
    from fabind_amd import _lib as L
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fabind_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fabind_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    special = {"fabind_abi_version", "fabind_sizeof_args", "fabind_loss_blocks", "fabind_pair_block_tile", "fabind_pair_block_chunk", "fabind_gemm_set_config", "fabind_gemm_set_persistent", "fabind_gemm_tn_tile_n",
               "fabind_gemm_x3_occupancy", "fabind_cross_attn_fused_occupancy"}
    protos.update(dict(re.findall(r"\blong\s+(fabind_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)))
    special.update({"fabind_cross_attn_bwd_scratch", "fabind_pair_bias_cat_parts", "fabind_pair_bias_finish_parts", "fabind_cross_attn_fused_bwd_scratch",
                    "fabind_cross_attn_fused_bwd_parts"})
    assert set(protos) - special == set(L.SIGNATURES), (sorted(set(protos) - special - set(L.SIGNATURES)),
                                                         sorted(set(L.SIGNATURES) - set(protos)))

    def kind_c(param):
        p = param.strip()
        if p == "void" or p == "":
            return None
        if "*" in p or "hipStream_t" in p:
            return "ptr"
        if re.match(r"(const\s+)?float\b", p):
            return "float"
        if re.match(r"(const\s+)?(unsigned|int|long)\b", p):
            return "int"
        raise AssertionError("unparsed parameter: %r" % p)

    def kind_py(t):
        if t in (ctypes.c_void_p,) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
            return "ptr"
        if t is ctypes.c_float:
            return "float"
        if t in (ctypes.c_int, ctypes.c_long, ctypes.c_uint):
            return "int"
        raise AssertionError("unexpected ctypes type %r" % (t,))
    for name, argt in L.SIGNATURES.items():
        want = [k for k in (kind_c(p) for p in protos[name].split(",")) if k is not None]
        got = [kind_py(t) for t in argt]
        assert got == want, (name, got, want)


def test_product_package_never_touches_the_oracle():
    """The oracle is test infrastructure: no module of the shipped package may import, name or locate anything under
    oracle/ (a product path routed through the CPU restatement would void every parity claim)."""
    import ast
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fabind_amd")
    checked = 0
    for dirpath, _, files in os.walk(root):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            src = open(path).read()
            assert "oracle" not in src.lower(), path
            for node in ast.walk(ast.parse(src)):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                assert not any(n.split(".")[0] in ("oracle", "refshim", "make_golden") for n in names), (path, names)
            checked += 1
    assert checked >= 20


def test_missing_library_fails_loudly():
    """No fallback: without libfabind_hip.so the binding raises and says how to build it."""
    from fabind_amd import _lib as L
    saved = (L.LIB_PATH, L._lib)
    try:
        L.LIB_PATH, L._lib = os.path.join(os.path.dirname(saved[0]), "no_such_library.so"), None
        with pytest.raises(RuntimeError, match="fabind_amd.build"):
            L.load()
    finally:
        L.LIB_PATH, L._lib = saved
    assert L.load() is not None


def test_graft_entry_build_runs():
    """The driver's "does it build" entry point: compiles (incrementally here) every HIP source, loads the library and
    imports the package -- exercised in the CPU suite so that a stale hard-coded check in it cannot go unnoticed again."""
    import __graft_entry__ as g
    g.build()


def test_layout_cache_is_keyed_on_tensor_identity_and_version():
    """engine.Layout.of reuses the layout of the SAME index tensors only: another tensor object (a new batch, even with equal
    content) and an in-place change of either tensor rebuild it."""
    import torch
    from fabind_amd import engine
    b = torch.tensor([0] * 5 + [1] * 7)
    s = torch.tensor([0, 0, 1, 1, 1] + [0, 0, 0, 1, 1, 1, 1], dtype=torch.float32)
    l1 = engine.Layout.of(b, s)
    assert engine.Layout.of(b, s) is l1
    assert l1.N == 12 and l1.P.tolist() == [3, 4] and l1.C.tolist() == [2, 3]
    assert engine.Layout.of(b.clone(), s) is not l1                  # equal content, different object
    s[2] = 0                                                         # in-place edit bumps the version counter
    l2 = engine.Layout.of(b, s)
    assert l2 is not l1 and l2.P.tolist() == [2, 4]


def test_tn_split_count_keeps_the_xcds_evenly_loaded():
    """kernels._tn_splits (256x256 layout): work-group ids go round-robin over the 8 XCDs with all tiles of an e-range on one XCD, so
    the split count of a long operand is a multiple of 8, every split keeps at least 256 rows, and the edge-level contraction of the
    bench (4 tiles) runs in one round of 256 work-groups; the 256x128 layout keeps round 1's rule."""
    from fabind_amd import kernels as K
    for M, N, E in ((512, 512, 1539196), (512, 512, 98688), (1024, 512, 98688), (1536, 512, 98688), (1024, 576, 78837),
                    (256, 512, 98688), (512, 128, 98688), (512, 512, 9088)):
        s = K._tn_splits(M, N, E, 256)
        assert s % 8 == 0 and E // s >= 256, (M, N, E, s)
        assert K._tn_splits(M, N, E, 256) == s                      # memoised
    assert K._tn_splits(512, 512, 1539196, 256) == 64               # 4 tiles x 64 splits = 256 work-groups: one per CU
    assert K._tn_splits(1536, 512, 98688, 256) == 16                # 12 tiles: 24 work-groups per XCD, one round
    assert 1 <= K._tn_splits(512, 512, 2624, 256) <= 16             # short operands: a few splits of >= 256 rows
    assert K._tn_splits(512, 512, 1539196, 128) == 128              # round-1 layout: 8 tiles x 128 splits


def _emulate_multi_copy(table):
    """fabind_multi_copy restated on the host for CPU tensors: dst[r * dst_sr + c * dst_sc] = convert(src[r * src_sr + c * src_sc])
    for every segment of a launch table (include/fabind_hip.h FabindCopySeg); src == NULL writes zeros; dtype codes 0 = fp32, 1 = bf16."""
    import ctypes

    def arr(ptr, dt, n):
        ct = ctypes.c_float if dt == 0 else ctypes.c_uint16
        return np.ctypeslib.as_array((ct * n).from_address(int(ptr)))
    for s in table:
        R, C = int(s["rows"]), int(s["cols"])
        if R == 0 or C == 0:
            continue
        r, c = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
        di = (r * int(s["dst_sr"]) + c * int(s["dst_sc"])).reshape(-1)
        if int(s["src"]) == 0:
            vals = np.zeros(R * C, dtype=np.float32)
        else:
            si = (r * int(s["src_sr"]) + c * int(s["src_sc"])).reshape(-1)
            src = arr(s["src"], int(s["src_dt"]), int(si.max()) + 1)[si]
            vals = src.astype(np.float32) if int(s["src_dt"]) == 0 else (src.astype(np.uint32) << 16).view(np.float32)
        dst = arr(s["dst"], int(s["dst_dt"]), int(di.max()) + 1)
        if int(s["dst_dt"]) == 0:
            dst[di] = vals
        else:
            dst[di] = torch.from_numpy(vals.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_param_pack_plans_on_the_host(monkeypatch):
    """param_pack.ParamPack without a GPU: the launch tables of its planned forward and backward are interpreted on the host
    (`_emulate_multi_copy`) for CPU tensors -- concatenations with zero blocks, strided views, casts, the W^T copies, zero-padded
    weights (`pad2d`), 1-D pieces -- and must reproduce the same requests executed with torch ops (EagerPack) and torch autograd's
    parameter gradients; a second run of the kept plan after an in-place update follows the new values."""
    from fabind_amd import param_pack as pp
    monkeypatch.setattr(pp, "_launch", lambda table, dev: _emulate_multi_copy(table))
    torch.manual_seed(0)
    A = torch.nn.Parameter(torch.randn(6, 10))
    B = torch.nn.Parameter(torch.randn(4, 10))
    v = torch.nn.Parameter(torch.randn(6))
    K2 = torch.nn.Parameter(torch.randn(8, 7))
    D = torch.nn.Parameter(torch.randn(4, 10))
    E = torch.nn.Parameter(torch.randn(6, 10))
    leaves = (A, B, v, K2, D, E)
    bf = torch.bfloat16

    def build(pk):          # (every parameter element sits in ONE request: the pack writes gradient slices, it does not accumulate)
        return dict(cat0=pk.cat([A, pk.zeros(2, 10), B], 0, bf, with_T=True),
                    cat1=pk.cat([K2[0::2, 1:], K2[1::2, 1:]], 0),
                    col=pk.copy(K2[0::2, 0]),
                    vec=pk.cat([v, pk.zeros(2)]),
                    pad=pk.pad2d(D, 8, 16, bf, with_T=True),
                    pad_exact=pk.pad2d(E, 6, 10))
    pk = pp.ParamPack(torch.device("cpu"))
    tree = build(pk)
    got = pk.resolve(tree)
    want = build(pp.EagerPack(torch.device("cpu")))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].detach(), want[k].detach()), k
    assert torch.equal(got["cat0"]._fab_T, got["cat0"].detach().t().contiguous())
    assert torch.equal(got["pad"]._fab_T, got["pad"].detach().t().contiguous())
    g = torch.Generator().manual_seed(1)
    cots = {k: torch.randn(want[k].shape, generator=g) for k in want}
    for p_ in leaves:
        p_.grad = None
    sum((got[k].float() * cots[k]).sum() for k in got).backward()
    mine = [p_.grad.clone() for p_ in leaves]
    for p_ in leaves:
        p_.grad = None
    sum((want[k].float() * cots[k]).sum() for k in want).backward()
    for a_, p_ in zip(mine, leaves):
        assert torch.allclose(a_, p_.grad, rtol=0, atol=1e-6)
    # the kept plan, re-run after an in-place update
    with torch.no_grad():
        B.mul_(2.0)
        D.add_(1.0)
    again = pk.resolve(tree)
    assert torch.equal(again["pad"].detach()[:4, :10], D.detach().to(bf)) and float(again["pad"].detach()[4:].abs().max()) == 0.0
    assert float(again["pad"].detach()[:, 10:].abs().max()) == 0.0
    assert torch.equal(again["cat0"].detach()[8:], B.detach().to(bf))


def test_rows_hadamard_csr_lists_every_pair_under_both_rows():
    """ops._rows_hadamard_csr (index glue of the atomics-free adjoint of out[e] = t[ia[e]] * t[ib[e]], model.py:355): interpreting the
    CSR row by row on the host reproduces torch's index_add form bit for bit -- incl. a row that occurs on both sides and empty rows."""
    from fabind_amd import ops
    g = torch.Generator().manual_seed(0)
    n, P, W = 37, 400, 8
    ia = torch.randint(0, 20, (P,), generator=g).to(torch.int32)
    ib = (20 + torch.randint(0, 15, (P,), generator=g)).to(torch.int32)
    ib[5] = 3
    t, dout = torch.randn(n, W, generator=g), torch.randn(P, W, generator=g)
    rp, pi, pn = ops._rows_hadamard_csr(ia, ib, n)
    assert rp.dtype == torch.int32 and int(rp[-1]) == 2 * P and rp.shape[0] == n + 1
    got = torch.zeros(n, W)
    for r in range(n):
        for e in range(int(rp[r]), int(rp[r + 1])):
            got[r] += dout[int(pi[e])] * t[int(pn[e])]
    ref = torch.zeros(n, W).index_add_(0, ia.long(), dout * t[ib.long()]).index_add_(0, ib.long(), dout * t[ia.long()])
    assert torch.allclose(got, ref, rtol=0, atol=1e-5)
    assert int(rp[36]) == int(rp[37])                      # rows 35, 36 have no pair


def test_linear_adjoint_decisions_are_one_table(monkeypatch):
    """The two decisions every Linear's adjoint makes (ops._dpre_plan: which pass over dy, and does it carry the bias gradient;
    ops._wgrad_plan: which contraction computes dW, and does the bias gradient ride with it) as pure functions of dtype, shape, strides,
    alignment, the precision mode and the switches -- pinned on both sides of every condition against a restatement of the rules:
    rows around DB_IN_TN_ROWS and around the split mode's 256-row floor, widths 8 and 6, dy fp32 / bf16 in all three modes, the four
    (want_dW, want_db) combinations, drop mask, activation, FUSE_DB_TN, TN_DEFER, x3_backward.  The adjoint-side counterpart of the
    fabind_gemm_plan assertions."""
    import itertools
    from fabind_amd import config, ops
    from fabind_amd import kernels as K
    f32, bf = torch.float32, torch.bfloat16
    assert ops.DB_IN_TN_ROWS == 32768
    ROWS, KX = (255, 256, 32768, 32769), 16
    buf = {(R, C, dt): torch.empty((R, C), dtype=dt) for R in ROWS for C in (8, 6, KX) for dt in (f32, bf)}

    def want(mode, x3b, fuse, defer, dy, act, drop, want_dW, want_db):
        R, C = dy.shape
        md = bf if mode == "bf16" else f32
        kind = "dropmask" if drop else "act" if act else "cast" if dy.dtype != md else "none"
        in_tn = defer and R <= 32768 and md == bf
        in_pass = want_db and (kind == "dropmask" or (kind != "none" and C % 4 == 0 and not (want_dW and in_tn)))
        if mode == "bf16x3" and x3b == "bf16" and C % 8 == 0 and R >= 256:
            path, rides = "x3_tn", fuse and C % 4 == 0
        elif md == bf and C % 8 == 0:
            path, rides = "tn", fuse
        else:
            path, rides = "nt", False
        db_from = None if not want_db else "pass" if in_pass else "tn" if (want_dW and rides) else "colsum"
        return kind, db_from, (path if want_dW else None)

    def got(dy, act, drop, want_dW, want_db):
        kind, in_pass = ops._dpre_plan(dy, K.ACT_RELU if act else K.ACT_NONE, (0.1, 7) if drop else None, want_db, want_dW)
        md = ops.mm_dtype()
        dpre = dy if kind == "none" else buf[(dy.shape[0], dy.shape[1], md)]          # what the pass writes: mm dtype, contiguous
        assert not (in_pass and not want_db) and dpre.dtype == md
        path, rides = ops._wgrad_plan(dpre, buf[(dy.shape[0], KX, md)], None, want_db and not in_pass) if want_dW else (None, False)
        return kind, (None if not want_db else "pass" if in_pass else "tn" if rides else "colsum"), path

    mode0, x3b0 = config.get_precision(), ("bf16" if config.x3_backward_bf16() else "exact")
    try:
        n = 0
        for mode, x3b, fuse, defer in itertools.product(config.MODES, ("bf16", "exact"), (True, False), (True, False)):
            config.set_precision(mode)
            config.set_x3_backward(x3b)
            monkeypatch.setattr(ops, "FUSE_DB_TN", fuse)
            monkeypatch.setattr(K, "TN_DEFER", defer)
            for R, C, dt, act, drop, want_dW, want_db in itertools.product(ROWS, (8, 6), (f32, bf), (False, True), (False, True),
                                                                           (False, True), (False, True)):
                case = (mode, x3b, fuse, defer, R, C, dt, act, drop, want_dW, want_db)
                assert got(buf[(R, C, dt)], act, drop, want_dW, want_db) == want(mode, x3b, fuse, defer, buf[(R, C, dt)], act, drop, want_dW, want_db), case
                n += 1
        assert n == 3 * 2 * 2 * 2 * 4 * 2 * 2 * 2 * 2 * 2 * 2
        # a few rows of the table spelled out (bf16 mode, everything on): the cast of an fp32 dy
        config.set_precision("bf16")
        config.set_x3_backward("bf16")
        monkeypatch.setattr(ops, "FUSE_DB_TN", True)
        monkeypatch.setattr(K, "TN_DEFER", True)
        assert got(buf[(32768, 8, f32)], False, False, True, True) == ("cast", "tn", "tn")          # small batch: db rides with the queued TN
        assert got(buf[(32769, 8, f32)], False, False, True, True) == ("cast", "pass", "tn")        # large batch: db from the fused pass
        assert got(buf[(32768, 8, f32)], False, False, False, True) == ("cast", "pass", None)       # no dW: nothing to ride with
        assert got(buf[(32769, 6, f32)], False, False, True, True) == ("cast", "colsum", "nt")      # C % 4: the fused pass does not apply
        assert got(buf[(32768, 8, bf)], False, False, True, True) == ("none", "tn", "tn")
        assert got(buf[(32768, 8, bf)], False, False, False, True) == ("none", "colsum", None)
        assert got(buf[(32768, 8, f32)], False, True, True, False) == ("dropmask", None, "tn")
        monkeypatch.setattr(ops, "DB_IN_TN_ROWS", 0)                                                # (what the GPU tests' db_from="pass" sets)
        assert got(buf[(255, 8, f32)], True, False, True, True) == ("act", "pass", "tn")
        monkeypatch.setattr(ops, "DB_IN_TN_ROWS", 32768)
        # strides and alignment: the TN kernel wants 16-byte aligned rows
        d = buf[(256, 8, bf)]
        wide = torch.empty((256, 24), dtype=bf)
        assert ops._wgrad_plan(d, wide[:, :16], None, True) == ("tn", True)
        assert ops._wgrad_plan(d, wide[:, 1:17], None, True) == ("nt", False)                       # data pointer 2 bytes off
        assert ops._wgrad_plan(d, torch.empty((256, 20), dtype=bf)[:, :16], None, True) == ("nt", False)   # row stride 40 bytes
        assert ops._wgrad_plan(d, buf[(256, KX, bf)], buf[(256, 6, bf)], True) == ("nt", False)     # second operand of odd width
        assert ops._wgrad_plan(d, buf[(256, KX, bf)], buf[(256, 8, bf)], True) == ("tn", True)
        config.set_precision("bf16x3")
        assert ops._wgrad_plan(buf[(256, 8, f32)], buf[(256, KX, f32)], None, True) == ("x3_tn", True)
        assert ops._wgrad_plan(buf[(255, 8, f32)], buf[(255, KX, f32)], None, True) == ("nt", False)
        config.set_x3_backward("exact")
        assert ops._wgrad_plan(buf[(256, 8, f32)], buf[(256, KX, f32)], None, True) == ("nt", False)
    finally:
        config.set_precision(mode0)
        config.set_x3_backward(x3b0)


def test_bench_reports_rooflines_by_the_survey_classification():
    """bench.py (round 6): WHICH roofline a kernel family is reported against follows SURVEY 8(d)'s classification of the
    operation (bound_of), not whichever fraction is larger; the fraction is reproducible from flops (or 8(d) compulsory bytes), launch
    time and the peak; this design's own tile traffic rides along as `design_traffic`."""
    import bench
    assert bench.bound_of("gcl_edge_fused_bwd4_kernel<512> E=1539196") == "mfma" and bench.bound_of("fabind_gemm M=98688") == "mfma"
    assert bench.bound_of("cross_attn_fused_fwd mode=0") == "mfma" and bench.bound_of("fabind_gemm_tn M=512") == "mfma"
    assert bench.bound_of("segment_sum rows=98688") == "hbm" and bench.bound_of("inter_attn_fwd_rows") == "hbm"
    # the edge backward of the round-5 headline: 4 E H^2 = 1.614 TFLOP per launch in 3,267.5 us; 8(d)-style compulsory bytes 0.64 GB,
    # design tiles 9.98 GB.  Reported against the matrix cores: 0.494 PFLOP/s = 0.198 of 2.5 PFLOP/s -- NOT "hbm 0.38" as rounds 4-5 printed
    E, H, N = 1539196, 512, 98688
    r = bench.price_against_rooflines(4.0 * E * H * H, N * 6.0 * H * 2 + E * 20.0, 3.2675, "bf16", "mfma", design_bytes=9.98e9)
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["achieved"] - 494.0) < 1.0 and abs(r["frac"] - 0.1976) < 5e-4
    assert r["other_roofline"]["bound"] == "hbm" and r["other_roofline"]["frac"] < 0.03          # the compulsory bytes: 2 % of HBM
    assert abs(r["design_traffic"]["achieved"] - 3054.0) < 5.0 and abs(r["design_traffic"]["frac_of_hbm_peak"] - 0.382) < 2e-3
    # a stand-alone segment sum: 8(d): E H s + E 4 + N H s bytes against HBM
    nb = E * H * 2 + E * 4 + N * H * 2
    r = bench.price_against_rooflines(0.0, nb, 0.6, "bf16", "hbm")
    assert r["bound"] == "hbm" and abs(r["achieved"] - nb / 0.6e-3 / 1e9) < 1e-6 and abs(r["frac"] - r["achieved"] / 8000.0) < 1e-12
    assert "design_traffic" not in r
    # no time measured: zeros, not a division error; the split-bf16 mode is priced at a third of the bf16 peak
    r = bench.price_against_rooflines(1e12, 1e9, 0.0, "bf16x3", "mfma")
    assert r["achieved"] == 0.0 and r["other_roofline"]["achieved"] == 0.0 and r["peak"] == 2500.0 / 3.0


def test_bench_dump_outputs_budget_and_sampling(tmp_path):
    """bench.py --dump-outputs: every tensor / number of the step's outputs becomes one <name>.npy, float32 (float64 for float64 and integer
    arrays); together they stay under 64 MB, the small arrays whole and the large ones as the same seeded sample on every call."""
    import bench
    g = torch.Generator().manual_seed(0)
    big = torch.randn(4096, 4096, generator=g)                          # 64 MB alone: must be sampled
    out = (big, torch.arange(7), {"w": torch.randn(3, 5, generator=g, dtype=torch.float64)}, 0)
    arrays = list(bench.arrays_of("out", out, ("big", "idx"))) + [("grad.lin.weight", torch.ones(2, 2, dtype=torch.bfloat16))]
    assert [n for n, _ in arrays] == ["out.big", "out.idx", "out.2.w", "out.3", "grad.lin.weight"]
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        assert bench.dump_outputs(str(d), arrays) == 5
    files = sorted(os.listdir(dirs[0]))
    assert files == sorted(os.listdir(dirs[1])) == sorted(n + ".npy" for n, _ in arrays)
    assert sum(os.path.getsize(dirs[0] / f) for f in files) <= 64 * 2 ** 20
    ld = {f[:-4]: np.load(dirs[0] / f) for f in files}
    assert ld["out.idx"].dtype == np.float64 and (ld["out.idx"] == np.arange(7)).all()
    assert ld["out.2.w"].dtype == np.float64 and ld["out.3"].shape == () and float(ld["out.3"]) == 0.0
    assert ld["grad.lin.weight"].dtype == np.float32 and (ld["grad.lin.weight"] == 1).all()
    s = ld["out.big"]
    assert s.dtype == np.float32 and s.ndim == 1 and 2 ** 20 < s.size < big.numel()
    assert np.isin(s[::1009], big.numpy().reshape(-1)).all()               # a sample of the tensor's own elements
    for f in files:
        assert (np.load(dirs[1] / f) == ld[f[:-4]]).all()                   # the same sample on every call


# ------------------------------------------------------------------------------------------------
# the table of FABIND_* environment variables (fabind_amd/config.py)
# ------------------------------------------------------------------------------------------------
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _package_sources():
    for dirpath, _, files in os.walk(os.path.join(_ROOT, "fabind_amd")):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(dirpath, f)
                yield os.path.relpath(path, os.path.join(_ROOT, "fabind_amd")), open(path).read()


def test_environment_is_read_in_config_and_build_only():
    """No module of the package but config.py (the table) and build.py (HIPCC) looks at the process environment."""
    seen = 0
    for rel, src in _package_sources():
        seen += 1
        if rel not in ("config.py", "build.py"):
            assert not re.search(r"os\.environ|getenv", src), rel
    assert seen >= 20


def test_every_fabind_literal_is_in_the_table_and_every_table_name_is_read():
    """Every "FABIND_..." string literal of the package is a name of config.KNOBS (a typo would read nothing, silently), and every name
    of the table is consumed: by a config.knob("NAME") / config.read("NAME", ...) call, or -- 'native-dev' -- by the loop of _lib.load(),
    which needs a void setter that _lib declares."""
    import ast
    from fabind_amd import config
    read, lib_src = set(), None
    for rel, src in _package_sources():
        if rel == "_lib.py":
            lib_src = src
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"FABIND_[A-Z0-9_]+", node.value):
                assert node.value in config.KNOBS, (rel, node.value)
            if isinstance(node, ast.Call) and getattr(node.func, "attr", getattr(node.func, "id", None)) in ("knob", "read") and node.args \
                    and isinstance(node.args[0], ast.Constant):
                read.add(node.args[0].value)
    with pytest.raises(KeyError):
        config.knob("FABIND_NO_SUCH_KNOB")
    assert "native-dev" in lib_src and "k.setter" in lib_src
    for k in config.KNOBS.values():
        assert k.category in ("mode-seed", "ab", "native-dev", "debug") and k.type in (bool, int, str) and k.doc, k.name
        if k.category == "native-dev":
            assert k.default is None and k.type is int and '"%s"' % k.setter in lib_src, k.name
        else:
            assert k.name in read, k.name


def test_knob_attributes_exist_where_the_table_says():
    """The module attributes tests and probes assign are initialised from the table, under the names the table records."""
    import importlib
    from fabind_amd import config
    for k in config.KNOBS.values():
        if k.category == "mode-seed":
            continue
        mod, name = k.attr.rsplit(".", 1)
        assert hasattr(importlib.import_module("fabind_amd." + mod), name), k
        if k.type is bool and mod != "_lib":
            assert getattr(importlib.import_module("fabind_amd." + mod), name) is config.knob(k.name), k.name


def test_knobs_document_agrees_with_the_table():
    """docs/KNOBS.md: the A/B section is the table config.knobs_markdown() prints (names, defaults, notes); the mode seeds are named in
    the numerics section."""
    from fabind_amd import config
    doc = open(os.path.join(_ROOT, "docs", "KNOBS.md")).read()
    modes, ab = doc.split("## A/B knobs")
    rows = [ln for ln in ab.splitlines() if ln.startswith("|")]
    assert rows == config.knobs_markdown().splitlines()
    got = {m.group(1): m.group(2) for m in (re.match(r"\| `(FABIND_\w+)` \| `?([^`|]*?)`? \|", ln) for ln in rows) if m}
    want = {k.name: ("unset" if k.default in (None, "") else str(int(k.default) if k.type is bool else k.default))
            for k in config.KNOBS.values() if k.category != "mode-seed"}
    assert got == want
    assert set(re.findall(r"FABIND_\w+", modes)) == {k.name for k in config.KNOBS.values() if k.category == "mode-seed"}


def test_every_ab_knob_is_exercised_by_a_test_or_a_tool():
    """An 'ab' / 'native-dev' knob stays in the product path only while a test or a tool drives its non-default side: `exercised_by` is
    an existing file under tests/ or tools/ -- no retired probe, no script of a single past round -- that names the variable, the module
    attribute it initialises, or the native setter."""
    from fabind_amd import config
    n = 0
    for k in config.KNOBS.values():
        if k.category not in ("ab", "native-dev"):
            assert k.exercised_by is None, k.name
            continue
        n += 1
        ex = k.exercised_by
        assert ex and (ex.startswith("tests/") or ex.startswith("tools/")) and not ex.startswith("tools/probes/retired/"), k
        assert not re.match(r"r\d+_", os.path.basename(ex)), k
        text = open(os.path.join(_ROOT, ex)).read()
        assert k.name in text or re.search(r"\b%s\b" % re.escape(k.attr.rsplit(".", 1)[1]), text) or (k.setter and k.setter in text), k
    assert n >= 10


def test_knob_reader_keeps_the_spellings_of_the_scattered_reads():
    """config.read against the expressions the modules used before the table existed, for an unset variable, "0", "1" (and "check",
    "2", a word): a process started with the same environment takes the same sides."""
    from fabind_amd import config
    eq1 = lambda n, d: (lambda e: e.get(n, d) == "1")
    unless0 = lambda n: (lambda e: e.get(n, "1") != "0")
    int_if_set = lambda n: (lambda e: int(e[n]) if e.get(n) else None)
    old = {
        "FABIND_X3_WGRAD": lambda e: e.get("FABIND_X3_WGRAD", "bf16"),
        "FABIND_X3_PAIRBIAS_BWD": lambda e: e.get("FABIND_X3_PAIRBIAS_BWD", "bf16"),
        "FABIND_X3_EDGE": lambda e: e.get("FABIND_X3_EDGE", "split"),
        "FABIND_SPLIT_SITES": lambda e: int(e.get("FABIND_SPLIT_SITES", "3")),
        "FABIND_ATTN_FUSED_TRAIN": eq1("FABIND_ATTN_FUSED_TRAIN", "1"),
        "FABIND_EDGE_SAVE_FWD": unless0("FABIND_EDGE_SAVE_FWD"),
        "FABIND_FUSE_DB_TN": eq1("FABIND_FUSE_DB_TN", "1"),
        "FABIND_INTER_ATTN_ROWS": eq1("FABIND_INTER_ATTN_ROWS", "1"),
        "FABIND_LAYOUT_CACHE": lambda e: not e.get("FABIND_LAYOUT_CACHE", "1") == "0",
        "FABIND_PAIRHAD_ROWS": eq1("FABIND_PAIRHAD_ROWS", "1"),
        "FABIND_PARAM_PACK": lambda e: e.get("FABIND_PARAM_PACK", "1"),
        "FABIND_PLUS_FOLD_EDGE_LN": eq1("FABIND_PLUS_FOLD_EDGE_LN", "1"),
        "FABIND_PLUS_FOLD_EDGE_LN_TRAIN": eq1("FABIND_PLUS_FOLD_EDGE_LN_TRAIN", "1"),
        "FABIND_PLUS_FUSE_PAIR": eq1("FABIND_PLUS_FUSE_PAIR", "1"),
        "FABIND_ROWS_HADAMARD_WALK": eq1("FABIND_ROWS_HADAMARD_WALK", "1"),
        "FABIND_TN_DEFER": eq1("FABIND_TN_DEFER", "1"),
        "FABIND_EDGE_BWD3_EXP": int_if_set("FABIND_EDGE_BWD3_EXP"),
        "FABIND_EDGE_BWD_VARIANT": lambda e: int(e["FABIND_EDGE_BWD_VARIANT"]) if "FABIND_EDGE_BWD_VARIANT" in e else None,
        "FABIND_GEMM_SMALL_M": int_if_set("FABIND_GEMM_SMALL_M"),
        "FABIND_TN_WAVES": int_if_set("FABIND_TN_WAVES"),
        "FABIND_DEBUG_GRAPH": eq1("FABIND_DEBUG_GRAPH", "0"),
        "FABIND_DEBUG_SYNC": eq1("FABIND_DEBUG_SYNC", "0"),
        "FABIND_LIB": lambda e: e.get("FABIND_LIB") or "",
    }
    assert set(old) == set(config.KNOBS)
    for name, expr in old.items():
        k = config.KNOBS[name]
        spellings = [None, "0", "1", "2"] + ([] if k.type is int else ["check", "bf16", "x3"]) + ([""] if k.type is not int else [])
        for v in spellings:
            env = {"FABIND_UNRELATED": "1"} if v is None else {name: v}
            assert config.read(name, env) == expr(env) and type(config.read(name, env)) is type(expr(env)), (name, v)
    # the four call sites of FABIND_PARAM_PACK compared to "0" (torch ops), != "0" (the pack) and "check": one string serves them all
    for v, eager, check in ((None, False, False), ("0", True, False), ("1", False, False), ("check", False, True)):
        got = config.read("FABIND_PARAM_PACK", {} if v is None else {"FABIND_PARAM_PACK": v})
        assert ((got == "0"), (got == "check")) == (eager, check)
    with pytest.raises(KeyError):
        config.read("FABIND_NO_SUCH_KNOB", {})


def test_param_pack_switch_is_read_at_call_time(monkeypatch):
    from fabind_amd import config
    monkeypatch.delenv("FABIND_PARAM_PACK", raising=False)
    assert config.param_pack() == "1"
    monkeypatch.setenv("FABIND_PARAM_PACK", "check")
    assert config.param_pack() == "check"
    monkeypatch.setenv("FABIND_PARAM_PACK", "0")
    assert config.param_pack() == "0"


# ------------------------------------------------------------------------------------------------
# the C ABI is called from kernels.py (and the leaf modules that own a feature); the autograd nodes keep the calculus
# ------------------------------------------------------------------------------------------------
_LEAF_MODULES = ("optim.py", "symmetry.py", "conformer.py", "param_pack.py", os.path.join("utils", "generation_utils.py"),
                 os.path.join("utils", "post_optim_utils.py"))
# entry points no module of the package calls: development setters / queries and launchers that only tests and tools drive
_UNCALLED = {"fabind_gemm_plan", "fabind_gcl_edge_fused_bwd_set_tile", "fabind_gcl_edge_fused_bwd_tile", "fabind_gcl_edge_fused_bwd_set_variant",
             "fabind_gcl_edge_fused_set_variant", "fabind_gcl_edge_fused_variant", "fabind_gcl_edge_fused_bwd_variant", "fabind_pair_bot_pack",
             "fabind_add"}


def test_native_calls_live_in_one_module():
    """ops.py, engine.py, plus/engine.py and the model modules marshal nothing: no `.fabind_*(` call, no ctypes, none of _lib's marshalling
    names (imported, or borrowed through `K.`); and every entry point of _lib.SIGNATURES is named by exactly one module of the package."""
    from fabind_amd import _lib as L
    users = {n: set() for n in L.SIGNATURES}
    nodes = 0
    for rel, src in _package_sources():
        for n in re.findall(r"\.(fabind_\w+)\b", src):
            if n in users:
                users[n].add(rel)
        if rel in ("ops.py", "engine.py", os.path.join("plus", "engine.py")) or os.path.dirname(rel) in ("models", os.path.join("plus", "models")):
            nodes += 1
            assert not re.search(r"\.fabind_\w+\s*\(", src), rel
            assert not re.search(r"^\s*(import ctypes|from ctypes\b)", src, flags=re.M), rel
            for m in re.finditer(r"^\s*from\s+\.+_lib\s+import\s+(\([^)]*\)|[^\n]*)", src, flags=re.M):
                assert not set(re.findall(r"\w+", m.group(1))) & {"GemmArgs", "check", "load", "ptr", "stream", "dt_code"}, (rel, m.group(0))
            assert not re.search(r"\bK\.(_lib|ptr|check|stream|dt_code|GemmArgs)\b", src), rel
    assert nodes >= 6
    for n, files in sorted(users.items()):
        assert len(files) == (0 if n in _UNCALLED else 1), (n, sorted(files))
        assert files <= {"kernels.py"} | set(_LEAF_MODULES), (n, sorted(files))


class _FakeNative:
    """Stand-in for the loaded library: every SIGNATURES entry checks its positional arguments against its argtypes -- pointer slots take
    None or an address handed out by `ptr` / `stream` below, integer slots a Python int that is no such address and fits the type, float
    slots a number, struct slots a byref whose fields follow the same rule -- and records them; the size queries return small counts."""
    BASE = 2 ** 40
    QUERIES = dict(fabind_cross_attn_bwd_scratch=16, fabind_pair_bias_cat_parts=3, fabind_cross_attn_fused_bwd_parts=3,
                   fabind_pair_bias_finish_parts=2, fabind_loss_blocks=2, fabind_pair_block_tile=64, fabind_pair_block_chunk=4,
                   fabind_gemm_tn_tile_n=256)

    def __init__(self):
        self.handed, self.calls = {}, []

    def ptr(self, t):
        if t is None:
            return None
        assert torch.is_tensor(t)
        key = (t.data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)
        for a, (k, _) in self.handed.items():
            if k == key:
                return a
        a = self.BASE + 4096 * (len(self.handed) + 1)
        self.handed[a] = (key, t)
        return a

    def stream(self):
        a = self.BASE + 1
        self.handed.setdefault(a, (("stream",), None))
        return a

    def tensor(self, addr):
        return self.handed[addr][1]

    def last(self, name):
        return [a for n, a in self.calls if n == name][-1]

    def _scalar(self, t, v, where):
        import ctypes
        if t is ctypes.c_void_p:
            if isinstance(v, ctypes.Array):                      # the table of block pointers of fabind_pair_bias_cat
                assert all(e is None or e in self.handed for e in v), where
            else:
                assert v is None or (type(v) is int and v in self.handed), (where, v)
        elif t in (ctypes.c_int, ctypes.c_long, ctypes.c_uint, ctypes.c_longlong):
            lo, hi = (0, 2 ** 32) if t is ctypes.c_uint else (-2 ** 31, 2 ** 31) if t is ctypes.c_int else (-2 ** 63, 2 ** 63)
            assert type(v) is int and v not in self.handed and lo <= v < hi, (where, v)
        elif t is ctypes.c_float:
            assert type(v) in (int, float), (where, v)
        else:
            raise AssertionError("unexpected slot type %r at %s" % (t, where))

    def __getattr__(self, name):
        import ctypes
        from fabind_amd import _lib as L
        if name in self.QUERIES:
            return lambda *a: self.QUERIES[name]
        argt = L.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argt), (name, len(args), len(argt))
            rec = []
            for i, (t, v) in enumerate(zip(argt, args)):
                if isinstance(t, type) and issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure):
                    assert type(v) is type(ctypes.byref(ctypes.c_int())) and isinstance(v._obj, t._type_), (name, i)
                    for f, ft in t._type_._fields_:
                        self._scalar(ft, getattr(v._obj, f), (name, i, f))
                    rec.append({f: getattr(v._obj, f) for f, _ in t._type_._fields_})
                else:
                    self._scalar(t, v, (name, i))
                    rec.append(list(v) if isinstance(v, ctypes.Array) else v)
            self.calls.append((name, rec))
            return 0
        return call


def test_wrappers_hand_pointers_to_pointer_slots(monkeypatch):
    """Every wrapper this table of call sites moved into kernels.py, driven once on CPU tensors through _FakeNative: a size or a stride in a
    pointer slot, a pointer in an integer slot or a wrong argument count fails in the fake; the strides and sizes that arrive are asserted
    here against operands whose row counts, widths and leading dimensions all differ (5 x 8 views of 5 x 12 buffers and the like), so
    that a size passed where a stride belongs shows in the recorded value."""
    from types import SimpleNamespace as NS
    from fabind_amd import _lib as L, config, ops
    from fabind_amd import kernels as K
    fk = _FakeNative()
    monkeypatch.setattr(L, "load", lambda: fk)
    monkeypatch.setattr(K, "ptr", fk.ptr)
    monkeypatch.setattr(K, "stream", fk.stream)
    monkeypatch.setattr(K, "LOSS_TICKET", {})
    profiled = []
    monkeypatch.setattr(K, "_profiled", lambda label, flops, fn, nbytes=0.0, algo=None: (profiled.append((label, flops, nbytes, algo)), fn())[1])
    f32, bf, i32 = torch.float32, torch.bfloat16, torch.int32
    A, ST = fk.ptr, fk.stream()

    def v(r, c, ld, dt=f32):
        return torch.empty((r, ld), dtype=dt)[:, :c]

    def vec(n, dt=f32):
        return torch.empty(n, dtype=dt)

    def ld_of(addr):
        return fk.tensor(addr).stride(0)

    # ---- element-wise / reduction adjoints ----
    x = v(5, 8, 12)
    out = K.transpose_act(x, 64, bf)
    a = fk.last("fabind_transpose_act")
    assert a == [A(x), 0, 12, A(out), 1, 64, 5, 8, K.ACT_NONE, ST] and out.shape == (8, 64)
    out = K.colsum(x)
    assert fk.last("fabind_colsum")[:7] == [A(x), 0, 12, A(out), 5, 8, 0] and fk.last("fabind_colsum")[8:] == [1, ST]
    dy, aux = torch.empty((5, 8)), torch.empty((5, 8), dtype=bf)
    out = K.mul_dact(dy, aux, K.ACT_RELU, bf, 2.0)
    assert fk.last("fabind_mul_dact") == [A(dy), 0, A(aux), 1, K.ACT_RELU, A(out), 1, 40, 2.0, ST]
    out = K.mul_dact(dy, None, K.ACT_NONE, bf)
    assert fk.last("fabind_mul_dact") == [A(dy), 0, A(dy), 0, K.ACT_NONE, A(out), 1, 40, 1.0, ST]
    out, db = K.mul_dact_colsum(dy, aux, K.ACT_STORED_DERIV, bf, 0.5)
    a = fk.last("fabind_mul_dact_colsum")
    assert a[:10] == [A(dy), 0, A(aux), 1, K.ACT_STORED_DERIV, A(out), 1, 5, 8, A(db)] and a[11:] == [1, 0.5, ST]
    assert fk.tensor(a[10]).shape == (1, 8) and K._nchunk_fused(5) == 1 and K._nchunk_fused(64 * 4096 + 1) == 4096 and K._nchunk_fused(129) == 3
    out, db = K.mul_dropmask_colsum(dy, 0.125, 2 ** 32 + 7, bf)
    a = fk.last("fabind_mul_dropmask_colsum")
    assert a[:9] == [A(dy), 0, A(out), 1, 5, 8, 0.125, 7, A(db)] and a[10:] == [1, ST]
    z, dpart, u = torch.empty((5, 8), dtype=bf), torch.empty((5, 3)), vec(8)
    dz, du = K.rowdot_bwd(z, dpart, u, K.ACT_SILU)
    a = fk.last("fabind_rowdot_bwd")
    assert a[:10] == [A(z), 1, A(dpart), 3, A(u), K.ACT_SILU, 5, 8, A(dz), A(du)] and a[11:] == [1, ST] and K._nchunk(257) == 2
    E, n, B = 7, 5, 2
    d, rho, norm, row, rowptr, colptr, perm, node_off = torch.empty((E, 3)), vec(E), vec(B), vec(E, i32), vec(n + 1, i32), vec(n + 1, i32), \
        vec(E, i32), vec(B + 1, i32)
    dd, drh = torch.empty((E, 3)), vec(E)
    dx = K.edge_geom_bwd(d, rho, norm, dd, drh, row, rowptr, colptr, perm, node_off, B, n)
    a = fk.last("fabind_edge_geom_bwd")
    assert a[:14] == [A(d), A(rho), A(norm), A(dd), A(drh), A(row), A(rowptr), A(colptr), A(perm), A(node_off), B, E, n, A(dx)]
    assert fk.tensor(a[14]).shape == (E, 3) and fk.tensor(a[15]).shape == (B,) and dx.shape == (n, 3)
    dpre, w_r = torch.empty((E, 8), dtype=bf), vec(8)
    drh2, dw = K.gcl_pre_bwd(dpre, 8, rho, w_r)
    a = fk.last("fabind_gcl_pre_bwd")
    assert a[:8] == [A(dpre), 1, 8, A(rho), A(w_r), E, A(drh2), A(dw)] and a[9:] == [1, ST] and drh2.shape == (E,) and dw.shape == (8,)
    dout, Z = v(n, 8, 12), torch.empty((E, 8), dtype=bf)
    dZ = K.gather_dact(dout, row, Z, K.ACT_SILU)
    assert fk.last("fabind_gather_dact") == [A(dout), 12, A(row), A(Z), 1, K.ACT_SILU, A(dZ), 1, E, 8, ST]
    s, dxo = vec(E), torch.empty((n, 3))
    dd2, ds = K.coord_update_bwd(d, s, rowptr, dxo, True, 0.5)
    assert fk.last("fabind_coord_update_bwd") == [A(d), A(s), A(rowptr), n, 1, 0.5, A(dxo), A(dd2), A(ds), ST] and dd2.shape == (E, 3)
    h, hn = torch.empty((5, 8)), torch.empty((5, 8))
    out = K.drop_mix(h, hn, 0.25, 11)
    assert fk.last("fabind_drop_mix") == [A(h), A(hn), A(out), 40, 0.25, 11, ST]
    dhn, dh = K.drop_mix_bwd(h, 0.25, 2 ** 32 + 11)
    assert fk.last("fabind_drop_mix_bwd") == [A(h), A(dhn), A(dh), 40, 0.25, 11, ST]
    x0, mask, li, lj, lo, c_cnt = torch.empty((n, 3)), vec(n, torch.uint8), vec(4, i32), vec(4, i32), vec(B + 1, i32), vec(B, i32)
    dx = K.las_step_bwd(dxo, x0, mask, li, lj, lo, node_off, c_cnt, B, 3, 0.1, 0.5, dxo)
    assert fk.last("fabind_las_step_bwd") == [A(dxo), A(x0), A(mask), A(li), A(lj), A(lo), A(node_off), A(c_cnt), B, 3, 0.1, 0.5, A(dxo), A(dx), ST]
    assert K.lower_bound(row, node_off, B + 1).shape == (B + 1,)
    a = fk.last("fabind_lower_bound")
    assert a[:4] == [A(row), E, A(node_off), B + 1] and fk.tensor(a[4]).dtype == i32

    # ---- the GEMM's row-dot form: every field of the launch as ops._gemm_rowdot filled it before the wrapper owned it ----
    xg, Wg, bg, ug = v(5, 8, 12, bf), v(6, 8, 16, bf), vec(6), vec(6)
    fold = (vec(5), vec(5), vec(6))
    monkeypatch.setattr(K, "PROFILE", {})
    prec0 = config.get_precision()
    try:
        for mode, dt in (("bf16", bf), ("bf16x3", f32), ("fp32", f32)):
            config.set_precision(mode)
            xg, Wg = v(5, 8, 12, dt), v(6, 8, 16, dt)
            for store, post, fo, p in ((True, False, None, 0.0), (True, True, None, 0.25), (False, False, None, 0.0), (False, False, fold, 0.0)):
                z, part = ops._gemm_rowdot(xg, Wg, bg, ug, K.ACT_NONE, K.ACT_RELU, store, p_drop=p, seed=2 ** 32 + 3, fold=fo, post=post)
                g = fk.last("fabind_gemm")[0]
                x3 = mode == "bf16x3"
                want = dict.fromkeys(g, 0)
                want.update({k: None for k, t in L.GemmArgs._fields_ if t is L._vp})
                want.update(A=A(xg), W=A(Wg), C=A(z), bias=A(bg), dotvec=A(ug), dot_out=A(part), M=5, N=6, K=8, K1=8, lda=12, ldw=16, ldc=6, dot_ld=1,
                            a_dtype=L.dt_code(dt), w_dtype=L.dt_code(dt), c_dtype=(L.dt_code(z.dtype) if store else 0), act_epi=K.ACT_RELU,
                            store_preact=(0 if (post or fo is not None) else 1), alpha=1.0, p_drop=p, drop_seed=3, split3=int(x3))
                if fo is not None:
                    want.update(row_mu=A(fold[0]), row_rs=A(fold[1]), col_c=A(fold[2]))
                assert g == want, (mode, store, post, {k: (g[k], want[k]) for k in g if g[k] != want[k]})
                assert (z is None) == (not store) and part.shape == (5, 1) and (z is None or (z.shape == (5, 6) and z.dtype == ops.act_dtype()))
                name = str(dt).replace("torch.", "")
                assert profiled[-1] == ("%s <%s,%s%s> M=5 N=6 K=8" % ("fabind_gemm_x3" if x3 else "fabind_gemm", name, name, ",x3" if x3 else ""),
                                        2.0 * 5 * 6 * 8, 0.0, None)
        config.set_precision("bf16")
        # (the plain form keeps its own figures: k_splits 1, no stored pre-activation, every operand priced once)
        xg, Wg = v(5, 8, 12, bf), v(6, 8, 16, bf)
        c, _ = K.gemm(xg, Wg, bias=bg)
        g = fk.last("fabind_gemm")[0]
        assert (g["k_splits"], g["store_preact"], g["ldc"], g["lda"], g["ldw"], g["row_mu"], g["dot_out"]) == (1, 0, 6, 12, 16, None, None)
        assert profiled[-1][2] == 5.0 * 8 * 2 + 6.0 * 8 * 2 + 5.0 * 6 * 4
    finally:
        config.set_precision(prec0)
    monkeypatch.setattr(K, "PROFILE", None)

    # ---- attention and Hadamard adjoints ----
    qg, kv, bias, desc = v(5, 256, 260), v(6, 256, 264), v(30, 8, 12), torch.empty((B, 8), dtype=i32)
    o, lse, do_ = torch.empty((5, 128)), torch.empty((5, 4)), torch.empty((5, 128))
    dqg, dkv, dbias = torch.empty_like(qg), torch.empty_like(kv), torch.empty_like(bias)
    for mfma, name in ((True, "fabind_cross_attn_mfma_bwd"), (False, "fabind_cross_attn_bwd")):
        K.cross_attn_bwd(qg, kv, bias, 0, 4, desc, B, 3, 4, 0.125, o, lse, do_, dqg, dkv, dbias, mfma)
        a = fk.last(name)
        assert a[:19] == [A(qg), 260, A(kv), 264, A(bias), 12, 0, 4, A(desc), B, 3, 4, 0.125, A(o), A(lse), A(do_), A(dqg), A(dkv), A(dbias)]
        assert fk.tensor(a[19]).shape == (5, 128) and fk.tensor(a[20]).shape == (5, 4) and fk.tensor(a[21]).shape == (16,) and a[22] == ST
    T0, T1, rp, rc = torch.empty((5, 20)), torch.empty((5, 12)), vec(E, i32), vec(E, i32)
    a0, b0, a1, b1 = T0[:, :8], T0[:, 8:16], T1[:, :4], T1[:, 4:8]
    hd = K.pair_hadamard(a0, b0, a1, b1, rp, rc, bf)
    assert fk.last("fabind_pair_hadamard") == [A(a0), A(b0), 20, 8, A(a1), A(b1), 12, 4, A(rp), A(rc), E, A(hd), 1, 12, ST] and hd.shape == (E, 12)
    hd = K.pair_hadamard(a0, b0, None, None, rp, rc, f32)                              # no second pair: the first again, width 0
    assert fk.last("fabind_pair_hadamard") == [A(a0), A(b0), 20, 8, A(a0), A(b0), 20, 0, A(rp), A(rc), E, A(hd), 0, 8, ST] and hd.shape == (E, 8)
    dhd, d0, d1 = v(E, 12, 16, bf), torch.empty((5, 24)), torch.empty((5, 28))
    K.pair_hadamard_bwd(dhd, a0, b0, 8, a1, b1, 4, rp, rc, d0[:, :8], d0[:, 8:16], d1[:, :4], d1[:, 4:8])
    assert fk.last("fabind_pair_hadamard_bwd") == [A(dhd), 1, 16, A(a0), A(b0), 20, 8, A(a1), A(b1), 12, 4, A(rp), A(rc), E, A(d0[:, :8]),
                                                   A(d0[:, 8:16]), 24, A(d1[:, :4]), A(d1[:, 4:8]), 28, ST]
    K.pair_hadamard_bwd(dhd, T0, T0, 20, None, None, 0, rp, rc, d0, d0, None, None)     # ops._RowsHadamard: no second pair at all
    assert fk.last("fabind_pair_hadamard_bwd") == [A(dhd), 1, 16, A(T0), A(T0), 20, 20, None, None, 0, 0, A(rp), A(rc), E, A(d0), A(d0), 24,
                                                   None, None, 0, ST]
    K.pair_hadamard_bwd(dhd, a0, b0, 8, a0, b0, 0, rp, rc, d0[:, :8], d0[:, 8:16], d0[:, :8], d0[:, 8:16])     # plus/engine._PairHad1
    assert fk.last("fabind_pair_hadamard_bwd")[7:11] == [A(a0), A(b0), 20, 0] and fk.last("fabind_pair_hadamard_bwd")[17:20] == [A(d0[:, :8]), A(d0[:, 8:16]), 24]
    col, ridx = vec(E, i32), vec(E, i32)
    K.pair_hadamard_bwd_rows(dhd, T0, 8, T1, 4, rowptr, col, ridx, rc, d0, d1)
    assert fk.last("fabind_pair_hadamard_bwd_rows") == [A(dhd), 1, 16, A(T0), 20, 8, A(T1), 12, 4, A(rowptr), A(col), A(ridx), A(rc), 5, A(d0), 24,
                                                        A(d1), 28, ST]
    nb_, desc_p = vec(5, i32), torch.empty((B, 8), dtype=i32)
    K.pair_hadamard_bwd_grid(dhd, T0, 8, node_off, c_cnt, nb_, desc_p, 5, d0)
    assert fk.last("fabind_pair_hadamard_bwd_grid") == [A(dhd), 1, 16, A(T0), 20, 8, A(node_off), A(c_cnt), A(nb_), A(desc_p), 5, A(d0), 24, ST]
    t, pidx, partner = v(5, 8, 12), vec(2 * E, i32), vec(2 * E, i32)
    dt_ = K.rows_hadamard_bwd(dhd[:, :8], t, rowptr, pidx, partner)
    a = fk.last("fabind_rows_hadamard_bwd")
    assert a == [A(dhd[:, :8]), 1, 16, A(t), 12, 8, A(rowptr), A(pidx), A(partner), 5, A(dt_), dt_.stride(0), ST] and dt_.shape == (5, 8)
    raw = vec(64, torch.uint8)
    bl = NS(desc_ptr=A(raw), row_b_ptr=A(raw[32:]), B=B, n_tiles=3, n_pairs=6, n_crows=3, nchunk_max=1, chunk=4)
    assert K.pair_block_tile_chunk() == (64, 4)
    o = K.block_hadamard_fwd(bl, t, 2)
    assert fk.last("fabind_block_hadamard_fwd") == [A(raw), B, 3, A(t), 12, A(t[2:]), 12, 8, A(o), 8, ST] and o.shape == (6, 8) and o.dtype == bf
    do6 = v(6, 8, 16, bf)
    dt_ = K.block_hadamard_bwd(bl, do6, t, 2)
    a = fk.last("fabind_block_hadamard_bwd")
    assert a[:13] == [A(raw), B, 3, A(do6), 16, A(t), 12, A(t[2:]), 12, 8, A(raw[32:]), 3, 1] and fk.tensor(a[13]).shape == (3, 1, 4, 8)
    assert a[14:] == [A(dt_), dt_.stride(0), A(dt_[2:]), dt_.stride(0), ST]
    qkv, cv = v(5, 24, 28), v(5, 8, 12)
    ev = [vec(E) for _ in range(4)]
    wv = [vec(8) for _ in range(4)]
    mirror, dh_o, dx_o, order = vec(E, i32), torch.empty((5, 8)), torch.empty((5, 3)), vec(5, i32)
    for deal, name in ((None, "fabind_inter_attn_bwd"), ((order, 1, 3), "fabind_inter_attn_bwd_rows")):
        r = K.inter_attn_bwd(qkv, cv, 8, d, ev[0], rowptr, col, mirror, ridx, wv[0], wv[1], wv[2], wv[3], ev[1], ev[2], 0.5, dh_o, dx_o, 2, deal)
        a = fk.last(name)
        assert a[:21] == [A(qkv), 28, A(cv), 12, 8, A(d), A(ev[0]), A(rowptr), A(col), A(mirror), A(ridx), A(wv[0]), A(wv[1]), A(wv[2]), A(wv[3]),
                          A(ev[1]), A(ev[2]), 0.5, 5, A(dh_o), A(dx_o)]
        assert [tuple(fk.tensor(p).shape) for p in a[21:29]] == [(5, 24), (5, 8), (E, 3), (E,), (E // 2,), (E,), (E,), (2, 32)] and a[29] == 2
        assert a[30:] == ([ST] if deal is None else [A(order), 1, 3, ST])
        assert [tuple(x_.shape) for x_ in r] == [(5, 24), (5, 8), (E, 3), (E,), (E // 2,), (E,), (32,)]
        assert fk.calls[-1][0] == "fabind_colsum" and fk.calls[-1][1][0] == a[28]                 # the four vector gradients: one column sum

    # ---- pair bias adjoint ----
    lay = NS(B=B, sumP=4, sumC=3, max_P=3, max_C=2, desc_p=desc_p, desc_pf=torch.empty((B, 8), dtype=i32), c_index=vec(3, i32), p_index=vec(4, i32))
    a0b0, douts, wc = torch.empty((5, 16)), [torch.empty((6, 8)), None], torch.empty((2, 8, 8))
    Acat, BTcat, colpart = K.pair_bias_cat(douts, lay, 8, 32, a0b0[:, 8:], wc)
    a = fk.last("fabind_pair_bias_cat")
    assert a == [[A(douts[0]), None], 2, A(desc_p), B, 3, 32, A(Acat), 64, A(a0b0[:, 8:]), 16, A(lay.c_index), A(wc), 8, A(BTcat), 64, A(colpart), ST]
    assert Acat.shape == (4, 64) and BTcat.shape == (B * 8, 64) and colpart.shape == (3, 16) and Acat.dtype == BTcat.dtype == bf
    BT2 = K.pair_bias_btcat(a0b0[:, 8:], lay, wc, 8, 32)
    assert fk.last("fabind_pair_bias_btcat") == [A(a0b0[:, 8:]), 16, A(lay.c_index), A(desc_p), A(wc), 2, 8, 32, A(BT2), 64, B, ST] and BT2.shape == (B * 8, 64)
    Dt = K.batched_transpose_pad(Acat, desc_p, B, 2, 32, 64)
    assert fk.last("fabind_batched_transpose_pad") == [A(Acat), 64, A(desc_p), B, 2, 32, 64, A(Dt), ST] and Dt.shape == (2, B * 32, 64)
    a16 = v(5, 8, 16, bf)
    At = K.batched_transpose_pad(a16, lay.desc_pf, B, 1, 8, 64)
    assert fk.last("fabind_batched_transpose_pad") == [A(a16), 16, A(lay.desc_pf), B, 1, 8, 64, A(At), ST] and At[0].shape == (B * 8, 64)
    assert K.pair_bias_finish_parts(3) == 2 and K.cross_attn_fused_bwd_parts(B, 3) == 3
    Tm, da, fin = torch.empty((24, 8)), torch.empty((5, 16)), torch.empty((2, 128))
    K.pair_bias_finish(Tm, a0b0, 8, wc[1], lay.c_index, 3, da, fin[:, 64:])
    assert fk.last("fabind_pair_bias_finish") == [A(Tm), A(a0b0), 16, 8, A(wc[1]), A(lay.c_index), 3, A(da), A(fin[:, 64:]), 128, ST]
    dwk = K.pair_bias_bwd(douts[0], 8, a0b0, 8, wc[0], lay, da)
    assert fk.last("fabind_pair_bias_bwd") == [A(douts[0]), 8, A(a0b0), 16, 8, A(wc[0]), A(desc_p), B, 3, 2, A(lay.p_index), A(lay.c_index), A(da),
                                               A(dwk), ST] and dwk.shape == (B, 64)
    # the shared tail of ops: launch order and the operands of every launch, for a block list with a gap
    n0 = len(fk.calls)
    monkeypatch.setattr(ops, "_pair_bias_groups", lambda *a_: (vec(8, i32), vec(8, i32)))
    lay.n_pairs = 6
    dw = ops._pair_bias_adjoint_tail(lay, 8, a0b0, a16, da, Acat, BTcat, wc, [1], 32)
    assert [n_ for n_, _ in fk.calls[n0:]] == ["fabind_gemm", "fabind_batched_transpose_pad", "fabind_batched_transpose_pad", "fabind_gemm",
                                               "fabind_pair_bias_finish", "fabind_colsum"] and dw.shape == (2, 8, 8)
    g0, g1 = fk.calls[n0][1][0], fk.calls[n0 + 3][1][0]
    assert (g0["A"], g0["W"], g0["C"], g0["accumulate"], g0["ldc"], g0["M"], g0["N"], g0["n_groups"], g0["max_m"], g0["max_n"]) == \
        (A(Acat), A(BTcat), A(da), 1, 16, 4, B * 8, B, 3, 8)
    assert (g1["lda"], g1["ldw"], g1["ldc"], g1["M"], g1["N"], g1["K"], g1["max_m"], g1["accumulate"]) == (64, 64, 8, B * 32, B * 8, 64, 16, 0)
    fi = fk.calls[n0 + 4][1]
    assert fi[1:4] == [A(a0b0), 16, 8] and fi[4] == A(wc[1]) and fi[7] == A(da) and fi[9] == 128 and fk.tensor(fi[8]).shape == (2, 64)

    # ---- norms and heads ----
    xc, w8, b8 = torch.empty((5, 8)), vec(8), vec(8)
    y, mean, rstd = K.layernorm_fwd(xc, w8, b8, 1e-5)
    assert fk.last("fabind_layernorm_fwd") == [A(xc), A(w8), A(b8), 1e-5, 5, 8, A(y), A(mean), A(rstd), ST]
    dxl, dwl, dbl = K.layernorm_bwd(xc, w8, y, mean, rstd)
    a = fk.last("fabind_layernorm_bwd")
    assert a[:8] == [A(xc), A(w8), A(y), A(mean), A(rstd), 5, 8, A(dxl)] and fk.tensor(a[8]).shape == fk.tensor(a[9]).shape == (2, 8) and dwl.shape == (8,)
    x6, w6, dy6 = v(5, 6, 12, bf), vec(6), v(5, 6, 16)
    dx6, dw6, db6 = K.layernorm_rows_bwd(x6, w6, dy6)
    a = fk.last("fabind_layernorm_rows_bwd")
    assert a[:13] == [A(x6), 1, 12, A(w6), A(dy6), 0, 16, 1e-5, 5, 6, A(dx6), 1, 8] and a[15:] == [2, ST] and dx6.shape == (5, 6) and dw6.shape == (6,)
    y = K.edge_concat(x, row, col, rho, bf, 24)
    assert fk.last("fabind_edge_concat") == [A(x), 12, 8, A(row), A(col), A(rho), E, A(y), 1, 24, 24, ST] and y.shape == (E, 24)
    lg, m8, xyz, noise = torch.empty((B, 5)), torch.empty((B, 5), dtype=torch.uint8), torch.empty((B, 5, 3)), torch.empty((B, 5, 2))
    center, wsum = K.pocket_center_fwd(lg, m8, xyz, noise, 0.5, True)
    assert fk.last("fabind_pocket_center_fwd") == [A(lg), A(m8), A(xyz), A(noise), B, 5, 0.5, 1, A(center), A(wsum), ST]
    dc = torch.empty((B, 3))
    dlg = K.pocket_center_bwd(lg, m8, xyz, None, 0.5, center, wsum, dc)
    assert fk.last("fabind_pocket_center_bwd") == [A(lg), A(m8), A(xyz), None, B, 5, 0.5, A(center), A(wsum), A(dc), A(dlg), ST]
    co, ct, yp, yb, dm, cls, cen, cent = torch.empty((4, 3)), torch.empty((4, 3)), vec(6), vec(6), vec(6), torch.empty((B, 5)), torch.empty((B, 3)), torch.empty((B, 3))
    w = dict(coord=1.0, pair=2.0, distill=3.0, cls=4.0, center=5.0, delta=6.0)
    loss, terms, lo8 = K.loss_fwd(co, ct, yp, yb, dm, lg, cls, 0, m8, cen, cent, w)
    a = fk.last("fabind_loss_fwd")
    assert a[:21] == [A(co), A(ct), 12, A(yp), A(yb), A(dm), 6, A(lg), A(cls), 0, A(m8), 10, A(cen), A(cent), 6, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert fk.tensor(a[21]).shape == (2, 8) and fk.tensor(a[22]) is list(K.LOSS_TICKET.values())[0] and a[23:] == [A(lo8), A(loss), A(terms), ST]
    gl, gt, dl = torch.empty(()), vec(6), [torch.empty_like(co), None, torch.empty_like(yb), None, torch.empty_like(cen)]
    K.loss_bwd(co, ct, yp, yb, dm, lg, cls, 0, cen, cent, w, lo8, gl, gt, dl)
    assert fk.last("fabind_loss_bwd") == [A(co), A(ct), 12, A(yp), A(yb), A(dm), 6, A(lg), A(cls), 0, 10, A(cen), A(cent), 6, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0,
                                          A(lo8), A(gl), A(gt), A(dl[0]), None, A(dl[2]), None, A(dl[4]), ST]
    bl2 = NS(desc_ptr=A(raw), B=B, n_tiles=3, n_pairs=6, max_C=2)
    xp, xl = torch.empty((4, 3)), torch.empty((3, 3))
    yd = K.pair_dist_fwd(bl2, xp, xl, 5.0, 0.0, 10.0)
    assert fk.last("fabind_pair_dist_fwd") == [A(raw), B, 3, A(xp), A(xl), 5.0, 0.0, 10.0, A(yd), ST] and yd.shape == (6,)
    dxl = K.pair_dist_bwd(bl2, xp, xl, yd, 5.0, 0.0, 10.0)
    a = fk.last("fabind_pair_dist_bwd")
    assert a[:9] == [A(raw), B, 2, A(xp), A(xl), A(yd), 5.0, 0.0, 10.0] and fk.tensor(a[9]).shape == (B, 8, 2, 3) and a[10:] == [A(dxl), ST]
    rmsd, cdis = K.pose_stats(co, ct, lo, B)
    assert fk.last("fabind_pose_stats") == [A(co), A(ct), A(lo), B, A(rmsd), A(cdis), ST] and rmsd.shape == cdis.shape == (B,)
    sc, rm, goff = vec(6), vec(6), vec(3, i32)
    terms, dsc, counts = K.rank_loss_fwd(sc, rm, goff, 2, 1, True)
    assert fk.last("fabind_rank_loss_fwd") == [A(sc), A(rm), A(goff), 2, 1, 1, A(terms), A(dsc), A(counts), ST] and terms.shape == (2, 3) and counts.dtype == i32
    # every entry point that ops.py, engine.py and plus/engine.py reach through the wrappers above was driven
    moved = {"fabind_transpose_act", "fabind_mul_dact", "fabind_mul_dact_colsum", "fabind_mul_dropmask_colsum", "fabind_gemm", "fabind_rowdot_bwd",
             "fabind_edge_geom_bwd", "fabind_gcl_pre_bwd", "fabind_gather_dact", "fabind_coord_update_bwd", "fabind_drop_mix", "fabind_drop_mix_bwd",
             "fabind_cross_attn_bwd", "fabind_cross_attn_mfma_bwd", "fabind_pair_hadamard", "fabind_pair_hadamard_bwd", "fabind_pair_hadamard_bwd_rows",
             "fabind_pair_hadamard_bwd_grid", "fabind_rows_hadamard_bwd", "fabind_block_hadamard_fwd", "fabind_block_hadamard_bwd",
             "fabind_inter_attn_bwd", "fabind_inter_attn_bwd_rows", "fabind_las_step_bwd", "fabind_pair_bias_cat", "fabind_pair_bias_btcat",
             "fabind_batched_transpose_pad", "fabind_pair_bias_finish", "fabind_pair_bias_bwd", "fabind_layernorm_fwd", "fabind_layernorm_bwd",
             "fabind_layernorm_rows_bwd", "fabind_edge_concat", "fabind_pocket_center_fwd", "fabind_pocket_center_bwd", "fabind_loss_fwd",
             "fabind_loss_bwd", "fabind_pair_dist_fwd", "fabind_pair_dist_bwd", "fabind_lower_bound", "fabind_pose_stats", "fabind_rank_loss_fwd",
             "fabind_colsum"}
    assert moved <= {n_ for n_, _ in fk.calls}
