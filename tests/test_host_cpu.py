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
