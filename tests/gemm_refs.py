"""Exact inputs, a float64 reference and the case table for fabind_gemm (csrc/gemm.hip); no GPU is needed to import this.

Inputs are small dyadic rationals: A holds integers in [-amax, amax], every other operand k / 4 with small |k| (W additionally
scaled by 2^-shift where a transcendental follows, so that pre-activations are O(1)).  Every operand is then exactly representable
in bf16 (the split-bf16 kernel's lo half is 0), and `exactness_bound` proves FROM THE RANGES AND K -- it samples nothing -- that
every product and every partial sum of the contraction and of the epilogue, in any order, is a multiple of its quantum below
2^24 quanta, i.e. exact in fp32.  For every form without a transcendental the float64 reference is therefore THE answer: an fp32
output must equal it, a bf16 output must equal its single round-to-nearest-even rounding, and every kernel family must agree
with every other one on these cases.  tests/test_gemm_refs_cpu.py checks the bound for every case of the table and pins the
restated activations and the restated dropout mask; tests/test_gpu_gemm_forms.py runs the table on the GPU.

Two fast epilogues legitimately round twice (documented in csrc/gemm.hip, gemm_epilogue_fast): form 14 (AUXMUL) and form 16
(RESADD) stage bf16(acc [+ bias]) in LDS and multiply / add during the flush.  `reference` states that arithmetic as `C_staged`
next to the single-rounded `C`."""
from fractions import Fraction

import numpy as np
import torch

from fabind_amd._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_STORED_DERIV, GEMM_FAM_GLDS, GEMM_FAM_NT_BF16,
                             GEMM_FAM_NT_F32, GEMM_FAM_NT_F32_BF16, GEMM_FAM_PIPE, GEMM_FAM_X3, GEMM_FAM_X3_PRO)

BN = 128                      # column tile of every kernel family: the row-dot is written per 128-column block
F32_TOL = 2e-5                # the project's fp32 bound of test_gemm_epilogues: 2e-5 * max(1, |ref|max)
P_DROP = 0.5                  # threshold 32768, scale exactly 2: dropout cases stay exact
FAST_FAMILIES = (GEMM_FAM_PIPE, GEMM_FAM_X3, GEMM_FAM_X3_PRO)       # the families that honour epi_fast; the others run the generic epilogue
FAMILY_NAMES = {GEMM_FAM_NT_F32: "nt<f32,f32>", GEMM_FAM_NT_F32_BF16: "nt<f32,bf16>", GEMM_FAM_NT_BF16: "nt<bf16,bf16>",
                GEMM_FAM_GLDS: "glds", GEMM_FAM_PIPE: "pipe", GEMM_FAM_X3: "x3", GEMM_FAM_X3_PRO: "x3-pro"}
PIPE_BK = {1: 32, 2: 64, 3: 32, 4: 64, 5: 32, 6: 32, 7: 32, 8: 32, 9: 64, 13: 32}     # k-tile of launch_pipe's configurations
PIPE_CONFIGS = tuple(sorted(PIPE_BK))


# ------------------------------------------------------------------------------------------------
# restatements: dropout mask (csrc/common.h fb_hash32 + the keep rule of the GEMM epilogues), activations
# ------------------------------------------------------------------------------------------------
def fb_hash32(x):
    """csrc/common.h fb_hash32 on uint32 values (computed in uint64, reduced mod 2^32 after every multiply)."""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def drop_threshold(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def drop_keep(seed, M, N, p):
    """keep[r, c] = (fb_hash32(seed + r * N + c) & 0xffff) >= round(p * 65536), the counter wrapping mod 2^32  ->  (bool [M, N], scale)."""
    thr = drop_threshold(p)
    r = np.arange(M, dtype=np.uint64)[:, None]
    c = np.arange(N, dtype=np.uint64)[None, :]
    key = (np.uint64(seed & 0xFFFFFFFF) + r * np.uint64(N) + c) & 0xFFFFFFFF
    keep = (fb_hash32(key) & 0xFFFF) >= thr
    return keep, 1.0 / (1.0 - thr / 65536.0)


def act(x, code):
    if code == ACT_SILU:
        return x * torch.sigmoid(x)
    if code == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if code == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def dact(x, code):
    """Derivative of act w.r.t. its pre-activation x (csrc/common.h apply_dact; STORED_DERIV: x already is the derivative)."""
    if code == ACT_SILU:
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    if code == ACT_RELU:
        return (x > 0).to(x.dtype)
    if code == ACT_SIGMOID:
        s = torch.sigmoid(x)
        return s * (1 - s)
    if code == ACT_STORED_DERIV:
        return x
    return torch.ones_like(x)


def rne_bf16(x):
    """float64 -> bf16 (round to nearest even) -> float64.  Exact-tier values are fp32-representable, so the fp32 step is exact."""
    return x.float().bfloat16().double()


def bf16_ulp(x):
    """One bf16 unit in the last place of the binade of |x| (8 significand bits); 0 at x = 0."""
    _, e = torch.frexp(x.abs().double())                     # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x, dtype=torch.float64), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8))


# ------------------------------------------------------------------------------------------------
# forms: one epilogue / prologue combination each, with the epi_fast code the dispatcher emits for it
# ------------------------------------------------------------------------------------------------
_DEFAULTS = dict(c="f32", bias=False, act=ACT_NONE, act_pro=ACT_NONE, c2=None, c16=False, r=None, gather=False, aux=None,
                 dact=ACT_NONE, alpha=1.0, accumulate=False, dot=False, pre=False, drop=False, fold=False, splits=1, a2=False,
                 groups=False, shift=0)


def _form(name, epi, **kw):
    d = dict(_DEFAULTS, name=name, epi=epi)
    assert set(kw) <= set(_DEFAULTS), kw
    d.update(kw)
    if d["act"] == ACT_SILU or d["act_pro"] == ACT_SILU or d["dact"] == ACT_SIGMOID:
        d["shift"] = 4                                            # pre-activation std ~ 1.4 at K = 192
    # tolerance tier: a transcendental, or the LayerNorm fold (forms 12 / 13: rs * (acc - mu * c) + b may contract into FMAs in any grouping;
    # its inputs are dyadic all the same, and exactness_bound follows them to the end)
    d["tier"] = "tol" if (d["shift"] or d["fold"]) else "exact"
    return d


# c: dtype of C (None: row-dot only); c2: None | "same" | "bf16" (stored derivative); r / aux: dtype of the operand; pre: store_preact
FORMS = [
    # ---- fp32 C
    _form("f32_plain", 9),
    _form("f32_bias", 9, bias=True),
    _form("f32_bias_c16", 9, bias=True, c16=True),
    _form("f32_res", 10, bias=True, r="f32"),
    _form("f32_res_c16", 10, r="f32", c16=True),
    _form("f32_accumulate", 10, accumulate=True),                 # rewritten to the residual epilogue with R = C
    _form("f32_auxrelu", 20, bias=True, aux="f32", dact=ACT_RELU),
    _form("f32_auxderiv", 21, bias=True, aux="f32", dact=ACT_STORED_DERIV),
    _form("f32_silu_c2", 22, bias=True, act=ACT_SILU, c2="same"),
    _form("f32_silu_c2bf16", 22, bias=True, act=ACT_SILU, c2="bf16", c16=True),
    _form("f32_silu", 23, bias=True, act=ACT_SILU),
    _form("f32_relu", 24, bias=True, act=ACT_RELU),
    _form("f32_relu_c16", 24, bias=True, act=ACT_RELU, c16=True),
    _form("f32_relu_c2", 25, bias=True, act=ACT_RELU, c2="same"),
    _form("f32_relu_c2bf16", 25, bias=True, act=ACT_RELU, c2="bf16", c16=True),
    # ---- bf16 C / row-dot
    _form("bf16_plain", 1, c="bf16"),
    _form("bf16_bias", 1, c="bf16", bias=True),
    _form("bf16_silu", 2, c="bf16", bias=True, act=ACT_SILU),
    _form("bf16_silu_c2", 3, c="bf16", bias=True, act=ACT_SILU, c2="same"),
    _form("dot_silu", 4, c=None, bias=True, act=ACT_SILU, dot=True),
    _form("bf16_relu", 5, c="bf16", bias=True, act=ACT_RELU),
    _form("dot_relu", 6, c=None, bias=True, act=ACT_RELU, dot=True),
    _form("bf16_silu_dot_pre", 7, c="bf16", bias=True, act=ACT_SILU, dot=True, pre=True),
    _form("bf16_relu_dot_pre", 8, c="bf16", bias=True, act=ACT_RELU, dot=True, pre=True),
    _form("bf16_relu_dot_post", 15, c="bf16", bias=True, act=ACT_RELU, dot=True),
    _form("bf16_gather_res", 11, c="bf16", bias=True, r="f32", gather=True),
    _form("bf16_res_bf16", 16, c="bf16", bias=True, r="bf16"),
    _form("bf16_auxrelu_alpha", 14, c="bf16", aux="bf16", dact=ACT_RELU, alpha=2.0),
    _form("bf16_auxderiv_alpha", 14, c="bf16", aux="bf16", dact=ACT_STORED_DERIV, alpha=0.5),
    _form("bf16_fold_relu", 12, c="bf16", bias=True, act=ACT_RELU, fold=True),
    _form("dot_fold_relu", 13, c=None, bias=True, act=ACT_RELU, dot=True, fold=True),
    # ---- generic epilogue
    _form("f32_alpha", 0, bias=True, alpha=0.5),
    _form("f32_alpha_c16", 0, bias=True, alpha=0.5, c16=True),
    _form("bf16_accumulate", 0, c="bf16", bias=True, accumulate=True),
    _form("f32_gather_res", 0, bias=True, r="f32", gather=True),
    _form("f32_auxsigmoid", 0, bias=True, aux="f32", dact=ACT_SIGMOID),
    _form("f32_relu_c2bf16_alpha", 0, bias=True, act=ACT_RELU, c2="bf16", alpha=0.5),
    _form("bf16_silu_dot_post", 0, c="bf16", bias=True, act=ACT_SILU, dot=True),
    # ---- epilogue dropout, p = 0.5, on every code the dispatcher lets it through
    _form("f32_plain_drop", 9, bias=True, drop=True),
    _form("f32_res_drop", 10, bias=True, r="f32", drop=True),
    _form("bf16_bias_drop", 1, c="bf16", bias=True, drop=True),
    _form("bf16_silu_drop", 2, c="bf16", bias=True, act=ACT_SILU, drop=True),
    _form("dot_silu_drop", 4, c=None, bias=True, act=ACT_SILU, dot=True, drop=True),
    _form("bf16_relu_drop", 5, c="bf16", bias=True, act=ACT_RELU, drop=True),
    _form("dot_relu_drop", 6, c=None, bias=True, act=ACT_RELU, dot=True, drop=True),
    _form("bf16_relu_dot_post_drop", 15, c="bf16", bias=True, act=ACT_RELU, dot=True, drop=True),
    _form("f32_alpha_drop", 0, bias=True, alpha=0.5, drop=True),
    _form("f32_relu_drop", 0, bias=True, act=ACT_RELU, drop=True),
    # ---- K-concatenated operand [A | A2]
    _form("a2_f32_plain", 9, a2=True),
    _form("a2_bf16_bias", 1, c="bf16", bias=True, a2=True),
    # ---- split-K partials and ragged groups (generic epilogue)
    _form("splitk2", 0, splits=2),
    _form("splitk3", 0, splits=3),
    _form("splitk4", 0, splits=4),
    _form("ragged_f32", 0, bias=True, groups=True),
    _form("ragged_bf16", 0, c="bf16", bias=True, groups=True),
    # ---- prologue activation (ReLU keeps the operand dyadic)
    _form("pro_f32_plain", 9, act_pro=ACT_RELU),
    _form("pro_bf16_bias", 1, c="bf16", bias=True, act_pro=ACT_RELU),
    _form("pro_bf16_relu_dot_pre", 8, c="bf16", bias=True, act=ACT_RELU, dot=True, pre=True, act_pro=ACT_RELU),
]
FORM = {f["name"]: f for f in FORMS}
assert len(FORM) == len(FORMS)
REDUCED = ("f32_plain", "bf16_bias", "bf16_relu_dot_pre")          # the list every other pipe configuration (and glds) runs
PRO_FORMS = ("pro_f32_plain", "pro_bf16_bias", "pro_bf16_relu_dot_pre")
EMITTED_CODES = tuple(range(0, 17)) + tuple(range(20, 26))         # every epi_fast the dispatcher can emit

# ragged groups: three straddling the 128- and 256-row / 128-column tile edges and an empty one (M = 0) whose output range stays untouched
GROUP_MS = (129, 0, 257, 130)
GROUP_NS = (130, 16, 120, 264)

# operand ranges (|k| of k / 4; A: integers)
AMAX, WK, BIASK, RK, AUXK = 4, 4, 4, 8, 4
MUK, COLCK = 2, 4                                                # LayerNorm fold: row_mu = k / 2, col_c integers, row_rs in {1/2, 1, 2}
UK = 2                                                             # row-dot vector: shrunk, its sum runs over 128 products


class Case:
    """One launch of the table: a form at a shape and layout, with the family / configuration it is meant to reach."""

    def __init__(self, form, ops, family, cfg, knobs, M, N, K, K1=None, layout="tight", via=""):
        self.form, self.ops, self.family, self.cfg, self.knobs = FORM[form], ops, family, cfg, dict(knobs)
        self.M, self.N, self.K, self.K1, self.layout, self.via = M, N, K, (K if K1 is None else K1), layout, via
        f = self.form
        self.bk = PIPE_BK[cfg] if family == GEMM_FAM_PIPE else (64 if family == GEMM_FAM_GLDS else 32)
        self.epi = f["epi"]                                                         # what fabind_gemm_plan must report
        self.epi_run = f["epi"] if family in FAST_FAMILIES else 0                   # what the kernel can honour
        self.group = "%s%s" % (FAMILY_NAMES[family], ("-cfg%d" % cfg) if cfg else "") + (("-" + via) if via else "")
        self.id = "%s:%s:%dx%dx%d%s:%s" % (self.group, f["name"], M, N, K, ("/%d" % self.K1) if f["a2"] else "", layout)

    @property
    def seed(self):
        return sum((i + 1) * ord(ch) for i, ch in enumerate(self.id)) & 0x7FFFFFFF

    def __repr__(self):
        return self.id


class _Dy:
    """Worst-case magnitude and quantum of a dyadic quantity; every value is a multiple of q with |value| <= mag."""

    def __init__(self, mag, q):
        self.mag, self.q = Fraction(mag), Fraction(q)

    def quanta(self):
        return self.mag / self.q

    def __mul__(self, o):
        return _Dy(self.mag * o.mag, self.q * o.q)

    def __add__(self, o):
        return _Dy(self.mag + o.mag, min(self.q, o.q))

    def times(self, n):                                            # sum of n such terms, any order: every partial sum obeys the same bound
        return _Dy(self.mag * n, self.q)


def exactness_bound(case):
    """Largest count of quanta any intermediate of the case can reach, from the operand ranges and K alone.  Below 2^24 every
    intermediate is exact in fp32 (24 significand bits), in every summation order."""
    f = case.form
    q4 = Fraction(1, 4)
    steps = []

    def see(x):
        steps.append(x.quanta())
        return x
    w = _Dy(Fraction(WK, 4) / 2 ** f["shift"], q4 / 2 ** f["shift"])
    v = see((_Dy(AMAX, 1) * w).times(case.K))                      # the contraction (relu(A) has A's range)
    if f["fold"]:                                                  # rs * (acc - mu * col_c)
        v = see(v + see(_Dy(Fraction(MUK, 2), Fraction(1, 2)) * _Dy(COLCK, 1)))
        v = see(v * _Dy(2, Fraction(1, 2)))
    v = see(v * _Dy(f["alpha"], f["alpha"]))                       # a power of two scales magnitude and quantum alike
    if f["bias"]:
        v = see(v + _Dy(Fraction(BIASK, 4), q4))
    if f["tier"] == "tol" and not f["fold"]:
        return max(steps)                                          # a transcendental follows: exactness is claimed for the pre-activation
    if f["aux"] is not None and f["dact"] == ACT_STORED_DERIV:
        v = see(v * _Dy(Fraction(AUXK, 4), q4))
    if f["drop"]:
        v = see(v * _Dy(2, 2))
    if f["r"] is not None:
        v = see(v + _Dy(Fraction(RK, 4), q4))
    if f["accumulate"]:
        v = see(v + _Dy(Fraction(RK, 4), q4))
    if f["dot"]:
        see((v * _Dy(Fraction(UK, 4), q4)).times(BN))
    return max(steps)


def _dy(rng, shape, k, scale=0.25):
    return rng.integers(-k, k + 1, shape).astype(np.float64) * scale


def make_inputs(case):
    """Dyadic operands of a case as float64 torch tensors (asserts the exactness bound first: a condition on the ranges)."""
    assert exactness_bound(case) < 2 ** 24, (case, exactness_bound(case))
    f, M, N, K = case.form, case.M, case.N, case.K
    rng = np.random.default_rng(case.seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    Mr, Nw = M, N
    d = {}
    if f["groups"]:
        Mr, Nw = sum(GROUP_MS), sum(GROUP_NS)
    d["A"] = t(_dy(rng, (Mr, K), AMAX, 1.0))
    d["W"] = t(_dy(rng, (Nw, K), WK, 0.25 / 2 ** f["shift"]))
    if f["bias"]:
        d["bias"] = t(_dy(rng, (Nw,), BIASK))
    if f["r"] is not None:
        rows = M + 5 if f["gather"] else M
        d["R"] = t(_dy(rng, (rows, N), RK))
        if f["gather"]:
            d["r_index"] = t(rng.integers(0, rows, (M,)).astype(np.int32))
    if f["accumulate"]:
        d["C_old"] = t(_dy(rng, (M, N), RK))
    if f["aux"] is not None:
        d["aux"] = t(_dy(rng, (M, N), AUXK))
    if f["dot"]:
        d["u"] = t(_dy(rng, (N,), UK))
    if f["fold"]:
        d["row_mu"] = t(_dy(rng, (M,), MUK, 0.5))
        d["row_rs"] = t(2.0 ** rng.integers(-1, 2, (M,)).astype(np.float64))
        d["col_c"] = t(_dy(rng, (N,), COLCK, 1.0))
    if f["drop"]:
        d["seed"] = int(rng.integers(0, 2 ** 32))
    return d


def split_ranges(K, splits, bk):
    """K range of every split-K work-group: `per` columns rounded up to the kernel's k-tile (csrc/gemm.hip); late ranges may be empty."""
    per = ((K // splits + bk - 1) // bk) * bk
    return [(min(K, s * per), min(K, s * per + per)) for s in range(splits)]


def _epilogue(f, acc, d, M, N, bias, keep_scale):
    out = {}
    if f["fold"]:
        acc = d["row_rs"][:, None] * (acc - d["row_mu"][:, None] * d["col_c"][None, :])
    v = acc * f["alpha"]
    if bias is not None:
        v = v + bias[None, :]
    vpre = v
    v = act(v, f["act"])
    if f["aux"] is not None:
        v = v * dact(d["aux"], f["dact"])
    if keep_scale is not None:
        keep, scale = keep_scale
        v = v * torch.where(torch.from_numpy(keep), scale, 0.0).to(v.dtype)
    if f["r"] is not None:
        v = v + (d["R"][d["r_index"].long()] if f["gather"] else d["R"])
    if f["c2"] is not None:
        out["C2"] = dact(vpre, f["act"])
    if f["dot"]:
        nt = (N + BN - 1) // BN
        out["dot"] = torch.stack([(v[:, t * BN:(t + 1) * BN] * d["u"][None, t * BN:(t + 1) * BN]).sum(1) for t in range(nt)], 1)
    if f["accumulate"]:
        v = v + d["C_old"]
    if f["c"] is not None:
        out["C"] = vpre if f["pre"] else v
    if f["c16"]:
        out["C16"] = v
    # forms 14 / 16 as the fast epilogue evaluates them: the staged tile is rounded to bf16 BEFORE the multiply / add of the flush
    if f["epi"] == 14:
        fac = dact(d["aux"], f["dact"]) * f["alpha"]
        out["C_staged"] = rne_bf16(rne_bf16(acc) * fac)
    if f["epi"] == 16:
        out["C_staged"] = rne_bf16(rne_bf16(vpre) + d["R"])
    return out


def reference(case, d):
    """float64 outputs of a case: C, C2, C16, dot [M, ceil(N / 128)] as the header's epilogue formula states them (unrounded);
    split-K: C is [splits * M, N]; ragged groups: `groups` = list of per-group C."""
    f, M, N = case.form, case.M, case.N
    A = act(d["A"], f["act_pro"])
    if f["groups"]:
        outs, a0, w0 = [], 0, 0
        for m, n in zip(GROUP_MS, GROUP_NS):
            acc = A[a0:a0 + m] @ d["W"][w0:w0 + n].T
            outs.append(_epilogue(f, acc, d, m, n, d["bias"][w0:w0 + n] if f["bias"] else None, None)["C"])
            a0, w0 = a0 + m, w0 + n
        return {"groups": outs}
    if f["splits"] > 1:
        parts = [A[:, lo:hi] @ d["W"][:, lo:hi].T for lo, hi in split_ranges(case.K, f["splits"], case.bk)]
        return {"C": torch.cat(parts, 0)}
    ks = drop_keep(d["seed"], M, N, P_DROP) if f["drop"] else None
    return _epilogue(f, A @ d["W"].T, d, M, N, d.get("bias"), ks)


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
MS, NS, KS = (1, 129, 257), (8, 120, 130, 132, 264), (64, 128, 192)
NT_KS = (8, 40, 96)
# one layout per N of a form's shape list: 8 contiguous; 120 with ld % 4 == 2 (no 16-byte rows at all); 130 and 132 with 16-byte rows, so
# that the vector flush meets its column tail (col + 8 > N) and the fp32 epilogues N % 4 != 0; 264 with ld % 8 == 4 (bf16: scalar flush
# over three column tiles, fp32: still vector)
LAYOUTS = ("tight", "odd6", "wide", "wide", "odd4")
DEFAULT_KNOBS = dict(config=13, small_m=100, x3_tile=2)


def _shapes(i, f, ks):
    """The launches of form number i: every N, with M, K and the layout rotating against it."""
    if f["groups"]:
        return [(max(GROUP_MS), max(GROUP_NS), ks[i % len(ks)], None, "tight")]
    if f["splits"] > 1:
        K = 64 if f["splits"] == 4 else 192
        return [(MS[(i + j) % 3], N, K, None, LAYOUTS[j]) for j, N in enumerate((8, 130, 264))]
    out = []
    for j, N in enumerate(NS):
        M, K = MS[(i + j) % 3], ks[(i + 2 * j) % len(ks)]
        K1 = None
        if f["a2"]:
            K1 = (64, 128)[(i + j) % 2]
            K = K1 + 64
        out.append((M, N, K, K1, LAYOUTS[j]))
    return out


def _full(ops, family, cfg, knobs, ks=KS, via="", names=None, misaligned=True):
    cases = []
    for i, f in enumerate(FORMS):
        if names is not None and f["name"] not in names:
            continue
        if names is None and f["act_pro"] != ACT_NONE:
            continue                                              # prologue forms are listed where a kernel has a prologue path
        if (f["fold"] and ops != "bf16") or (ks is NT_KS and (f["splits"] > 1 or f["a2"])):
            continue                                              # (the fold takes bf16 operands; split-K needs K % 64 == 0, K1 is 64 or 128)
        kn = knobs
        if f["groups"] and family == GEMM_FAM_PIPE:               # a ragged launch never takes the small-M switch: name the configuration
            kn = dict(knobs, config=cfg)
        for (M, N, K, K1, lay) in _shapes(i, f, ks):
            cases.append(Case(f["name"], ops, family, cfg, kn, M, N, K, K1, lay, via))
        if misaligned and not f["groups"] and f["splits"] == 1:    # C, R and aux each 8 bytes off a 16-byte boundary, one run each
            for what in ("C", "R", "aux"):
                if (what == "C" and f["c"] is None) or (what == "R" and f["r"] is None) or (what == "aux" and f["aux"] is None):
                    continue
                K = 128 if not f["a2"] else 192
                cases.append(Case(f["name"], ops, family, cfg, knobs, 129, 132, K, 128 if f["a2"] else None, "off" + what, via))
    return cases


def _build():
    P, X = GEMM_FAM_PIPE, GEMM_FAM_X3
    k13 = dict(DEFAULT_KNOBS, small_m=0)                           # the production default at a handful of tiles
    cases = _full("bf16", P, 13, k13) + _full("bf16", P, 6, DEFAULT_KNOBS)          # (6: what the default becomes below 100 tiles)
    for c in PIPE_CONFIGS:
        if c in (6, 13):
            continue
        for name in REDUCED:
            cases += [Case(name, "bf16", P, c, dict(DEFAULT_KNOBS, config=c), 257, 264, K) for K in KS]
    for name in REDUCED + ("ragged_f32", "ragged_bf16", "bf16_silu_dot_post", "bf16_accumulate"):
        ks = KS if name in REDUCED else (128,)
        cases += [Case(name, "bf16", GEMM_FAM_GLDS, 0, dict(DEFAULT_KNOBS, config=0), max(GROUP_MS) if FORM[name]["groups"] else 257,
                       264, K) for K in ks]
    # split-K with config 0 runs pipe configuration 3
    cases += [Case("splitk2", "bf16", P, 3, dict(DEFAULT_KNOBS, config=0), 129, 130, 192, via="from-cfg0")]
    for wm in (2, 4):
        cases += _full("x3", X, wm, dict(DEFAULT_KNOBS, x3_tile=wm), misaligned=(wm == 2))
    for name in PRO_FORMS:
        cases += [Case(name, "x3", GEMM_FAM_X3_PRO, 2, DEFAULT_KNOBS, MS[(j + 1) % 3], N, KS[j % 3], None, LAYOUTS[j])
                  for j, N in enumerate(NS)]
    # the MFMA-from-registers kernels: K < BK and K % 32 != 0
    cases += _full("f32", GEMM_FAM_NT_F32, 0, DEFAULT_KNOBS, ks=NT_KS, misaligned=False)
    cases += _full("f32", GEMM_FAM_NT_F32, 0, DEFAULT_KNOBS, ks=KS, names=("splitk2", "splitk3", "splitk4", "a2_f32_plain", "a2_bf16_bias"),
                   misaligned=False, via="k64")
    mixed = ("f32_plain", "bf16_bias", "bf16_relu_dot_pre", "f32_res_drop", "bf16_silu_c2", "bf16_res_bf16", "bf16_auxderiv_alpha", "ragged_bf16")
    cases += _full("mix", GEMM_FAM_NT_F32_BF16, 0, DEFAULT_KNOBS, ks=NT_KS, names=mixed, misaligned=False)
    cases += _full("bf16", GEMM_FAM_NT_BF16, 0, DEFAULT_KNOBS, ks=NT_KS, names=mixed + ("bf16_relu_drop", "f32_accumulate"), misaligned=False,
                   via="k")
    cases += _full("bf16", GEMM_FAM_NT_BF16, 0, DEFAULT_KNOBS, ks=KS, names=PRO_FORMS, misaligned=False, via="pro")
    # bf16 operands from a view whose base is only 8-byte aligned: the LDS-DMA kernels cannot take them
    for name in REDUCED:
        cases += [Case(name, "bf16", GEMM_FAM_NT_BF16, 0, DEFAULT_KNOBS, 257, 264, K, None, "offA", "offA") for K in KS]
    return cases


CASES = _build()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
