"""CPU: the float64 reference, the dyadic input generator and the case table of tests/gemm_refs.py (which tests/test_gpu_gemm_forms.py
runs on the GPU) are themselves pinned here: the exactness bound holds for every case of the table from its input ranges, the
restated activations match autograd, the restated dropout mask matches an independent integer evaluation of the hash and keeps
half of the positions, and the table names every family and every epilogue code."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_refs as G
from fabind_amd._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_STORED_DERIV


def test_exactness_bound_holds_for_every_case_of_the_table():
    """Worst-case quanta of any intermediate, from the ranges and K alone, below 2^24 (fp32 holds 24 significand bits)."""
    assert len(G.CASES) > 500
    worst = max(G.CASES, key=G.exactness_bound)
    for c in G.CASES:
        assert G.exactness_bound(c) < 2 ** 24, (c, G.exactness_bound(c))
    assert G.exactness_bound(worst) > 2 ** 20, "the bound is not vacuous: the row-dot cases come within 2^4 of it"


@pytest.mark.parametrize("name", ["f32_res_drop", "bf16_relu_dot_post_drop", "dot_fold_relu", "bf16_auxderiv_alpha", "f32_relu_c2bf16_alpha",
                                  "f32_silu_c2", "a2_bf16_bias", "pro_bf16_relu_dot_pre", "splitk3", "ragged_bf16"])
def test_sampled_inputs_respect_the_ranges_and_fp32_reproduces_the_reference(name):
    """The generator's operands are bf16-representable dyadics, and -- what the bound promises -- a plain fp32 evaluation in torch's
    own summation order gives the float64 reference bit for bit on every exact-tier output."""
    case = max((c for c in G.CASES if c.form["name"] == name), key=lambda c: (c.K, c.M * c.N))
    f, d = case.form, G.make_inputs(case)
    for k, v in d.items():
        if k in ("seed", "r_index"):
            continue
        assert torch.equal(v.bfloat16().double(), v), k
        assert torch.equal(v * 64, (v * 64).round()), k             # multiples of 2^-6 at the finest (W under the SiLU scale)
    assert float(d["A"].abs().max()) <= G.AMAX and torch.equal(d["A"], d["A"].round())
    ref = G.reference(case, d)
    if f["tier"] != "exact" or f["groups"] or f["splits"] > 1:
        return
    d32 = {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.float64 else v) for k, v in d.items()}
    keep = G.drop_keep(d["seed"], case.M, case.N, G.P_DROP) if f["drop"] else None
    got = G._epilogue(f, G.act(d32["A"], f["act_pro"]) @ d32["W"].T, d32, case.M, case.N, d32.get("bias"), keep)
    for k in ("C", "C2", "C16", "dot"):
        if k in ref:
            assert got[k].dtype == torch.float32 and torch.equal(got[k].double(), ref[k]), k


def test_reference_activations_match_autograd_in_float64():
    x = (torch.arange(-96, 97, dtype=torch.float64) / 8).requires_grad_()
    F = torch.nn.functional
    for code, fn in ((ACT_SILU, F.silu), (ACT_RELU, F.relu), (ACT_SIGMOID, torch.sigmoid), (ACT_NONE, lambda t: t * 1.0)):
        y = fn(x)
        (g,) = torch.autograd.grad(y.sum(), x)
        assert (G.act(x.detach(), code) - y.detach()).abs().max() <= 1e-15 * max(1.0, float(y.detach().abs().max())), code
        assert (G.dact(x.detach(), code) - g).abs().max() <= 1e-14, code
    assert torch.equal(G.dact(x.detach(), ACT_STORED_DERIV), x.detach())
    assert float(G.dact(torch.zeros(1, dtype=torch.float64), ACT_RELU)) == 0.0       # relu'(0) = 0: `x > 0` in csrc/common.h


def _hash_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_restated_dropout_mask():
    """The vectorised hash equals a plain-integer evaluation (wrap-around of the counter included); p = 0.5 gives threshold 32768
    and a scale of exactly 2; the keep-rate lies inside five binomial standard deviations."""
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789, 0xDEADBEEF]
    assert G.fb_hash32(np.array(xs, dtype=np.uint64)).tolist() == [_hash_int(x) for x in xs]
    assert _hash_int(0) == 0 and len({_hash_int(x) for x in range(1000)}) == 1000      # a bijection of uint32 fixes 0 and never collides
    assert G.drop_threshold(0.5) == 32768 and G.drop_threshold(0.25) == 16384 and G.drop_threshold(0.1) == 6554
    M, N, seed = 257, 264, 0xFFFFFF00                               # the counter wraps inside the first row
    keep, scale = G.drop_keep(seed, M, N, 0.5)
    assert scale == 2.0 and keep.shape == (M, N)
    for r, c in ((0, 0), (0, 263), (1, 0), (256, 263), (100, 131)):
        assert bool(keep[r, c]) == ((_hash_int(seed + r * N + c) & 0xFFFF) >= 32768)
    n = M * N
    assert abs(int(keep.sum()) - n / 2) <= 5 * (n * 0.25) ** 0.5
    assert abs(int(keep[:, ::2].sum()) - n / 4) <= 5 * (n * 0.125) ** 0.5           # ... and in a column-parity subsample
    assert not np.array_equal(keep, G.drop_keep(seed + 1, M, N, 0.5)[0])


def test_rounding_helpers():
    x = torch.tensor([0.0, 1.0, 1.00390625, 1.01171875, -3.0, 255.0, 256.0, 257.0, 0.3], dtype=torch.float64)
    assert G.rne_bf16(x).tolist()[:8] == [0.0, 1.0, 1.0, 1.015625, -3.0, 255.0, 256.0, 256.0]     # ties to even, both ways
    assert G.bf16_ulp(x).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0, 2.0, 2.0 ** -9]


def test_split_k_ranges_follow_the_kernels():
    assert G.split_ranges(192, 2, 64) == [(0, 128), (128, 192)]     # uneven at BK 64
    assert G.split_ranges(192, 2, 32) == [(0, 96), (96, 192)]
    assert G.split_ranges(192, 3, 64) == [(0, 64), (64, 128), (128, 192)]
    assert G.split_ranges(64, 4, 32) == [(0, 32), (32, 64), (64, 64), (64, 64)]       # two empty ranges: zeros
    assert G.split_ranges(64, 4, 64) == [(0, 64), (64, 64), (64, 64), (64, 64)]


def test_table_names_every_family_code_and_edge():
    from fabind_amd import _lib as L
    fams = {c.family for c in G.CASES}
    assert fams == set(G.FAMILY_NAMES)
    assert {f["epi"] for f in G.FORMS} == set(G.EMITTED_CODES)
    for fam, skip in ((L.GEMM_FAM_PIPE, ()), (L.GEMM_FAM_X3, (12, 13))):
        assert {c.epi_run for c in G.CASES if c.family == fam} == set(G.EMITTED_CODES) - set(skip)
    assert {c.cfg for c in G.CASES if c.family == L.GEMM_FAM_PIPE} == set(G.PIPE_CONFIGS)
    for cfg in (13, 6):                                             # the whole form list, at every M, N, K and layout of the issue
        cs = [c for c in G.CASES if c.family == L.GEMM_FAM_PIPE and c.cfg == cfg]
        assert {c.form["name"] for c in cs} == {f["name"] for f in G.FORMS if f["act_pro"] == ACT_NONE}
        assert {c.M for c in cs} >= set(G.MS) and {c.N for c in cs} >= set(G.NS) and {c.K for c in cs} == set(G.KS)
        assert {c.layout for c in cs} == {"tight", "wide", "odd4", "odd6", "offC", "offR", "offaux"}
        assert {c.K1 for c in cs if c.form["a2"]} == {64, 128}
    assert {c.K for c in G.CASES if c.family == L.GEMM_FAM_NT_F32 and not c.via} == set(G.NT_KS)
    assert {c.via for c in G.CASES if c.family == L.GEMM_FAM_NT_BF16} == {"k", "pro", "offA"}       # the three ways into nt<bf16, bf16>
    for fam in (L.GEMM_FAM_NT_F32, L.GEMM_FAM_PIPE, L.GEMM_FAM_X3):
        assert {c.form["splits"] for c in G.CASES if c.family == fam} >= {1, 2, 3, 4}
    for fam in (L.GEMM_FAM_NT_BF16, L.GEMM_FAM_NT_F32, L.GEMM_FAM_GLDS, L.GEMM_FAM_PIPE, L.GEMM_FAM_X3):
        assert any(c.form["groups"] for c in G.CASES if c.family == fam), G.FAMILY_NAMES[fam]
    drop_codes = {f["epi"] for f in G.FORMS if f["drop"]}
    assert drop_codes == {9, 10, 1, 2, 4, 5, 6, 15, 0}


def test_gemm_plan_runs_without_a_device():
    """fabind_gemm_plan is host code: it answers from sizes, dtypes and addresses (never dereferenced) without touching the GPU."""
    from fabind_amd import _lib as L
    lib = L.load()
    a = L.GemmArgs()
    a.A, a.W, a.C = 0x10000, 0x20000, 0x30000
    a.M, a.N, a.K, a.K1, a.lda, a.ldw, a.ldc, a.alpha = 300, 264, 128, 128, 128, 128, 264, 1.0
    fam, epi, cfg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ask = lambda: (lib.fabind_gemm_plan(ctypes.byref(a), ctypes.byref(fam), ctypes.byref(epi), ctypes.byref(cfg)), fam.value, epi.value, cfg.value)
    assert ask() == (0, L.GEMM_FAM_NT_F32, 9, 0)
    a.split3 = 1
    assert ask() == (0, L.GEMM_FAM_X3, 9, 2)
    a.act_pro = ACT_RELU
    assert ask() == (0, L.GEMM_FAM_X3_PRO, 9, 2)
    a.act_pro, a.split3, a.a_dtype, a.w_dtype, a.c_dtype, a.bias = ACT_NONE, 0, L.DT_BF16, L.DT_BF16, L.DT_BF16, 0x40000
    assert ask() == (0, L.GEMM_FAM_PIPE, 1, 6)                      # six tiles: the small-M form of the default configuration
    a.K = a.K1 = a.lda = a.ldw = 96
    assert ask() == (0, L.GEMM_FAM_NT_BF16, 1, 0)
    a.a_dtype = L.DT_F32
    assert ask() == (0, L.GEMM_FAM_NT_F32_BF16, 1, 0)
    a.K = 4
    assert ask()[0] != 0 and fam.value == -1 and b"multiple of 8" in lib.fabind_last_error()
    a.K, a.M = 96, 0
    assert ask() == (0, -1, 1, 0)                                   # an empty problem: nothing would be launched
    assert lib.fabind_gemm_plan(ctypes.byref(a), None, None, None) == 0
