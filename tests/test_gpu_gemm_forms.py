"""GPU: every fabind_gemm kernel family and every epilogue form at tile edges, against the float64 reference of tests/gemm_refs.py.

The inputs are dyadic, so every form without a transcendental has ONE right answer: an fp32 output equals the float64 reference, a
bf16 output its single round-to-nearest-even rounding (values compared, so +0 == -0), in every family alike.  SiLU / stored SiLU
derivative / sigmoid-derivative / LayerNorm-fold forms are held to the project's fp32 bound 2e-5 * max(1, |ref|max) (bf16 outputs:
plus one bf16 ulp of the reference value).  Operands and outputs are views into sentinel-filled buffers with padded strides; after
every launch everything outside the output view must be untouched.  Which kernel and which epilogue ran is asserted through
fabind_gemm_plan, the host function fabind_gemm itself dispatches through."""
import contextlib
import ctypes

import pytest
import torch

import gemm_refs as G

pytestmark = pytest.mark.gpu

SENT = -1234.5                 # sentinel (bf16: rounds to -1232; buffers are compared with their own earlier contents)
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
_DEVICE_ERROR = None           # set by the first launch that raised; every later test fails without launching


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def _knobs(k):
    """The process-global development setters, restored to their defaults afterwards."""
    from fabind_amd import _lib, config
    from fabind_amd import kernels as K
    lib = _lib.load()
    small_m = config.knob("FABIND_GEMM_SMALL_M")
    try:
        lib.fabind_gemm_set_config(k["config"])
        lib.fabind_gemm_set_small_m(k["small_m"])
        lib.fabind_gemm_set_x3_tile(k["x3_tile"])
        yield lib
    finally:
        lib.fabind_gemm_set_config(K.GEMM_DEFAULT_CONFIG)
        lib.fabind_gemm_set_small_m(100 if small_m is None else small_m)
        lib.fabind_gemm_set_x3_tile(2)


class _Buf:
    """A [rows, cols] view with row stride ld, `off` elements into a sentinel-filled flat device buffer (two spare rows behind it)."""

    def __init__(self, dev, dtype, rows, cols, ld, off=0, data=None, fill=True):
        assert ld >= cols
        self.dtype, self.geom = dtype, ((rows, cols), (ld, 1), off)
        n = off + (rows + 2) * ld + 16
        if not fill:                                               # plan-only: addresses and strides matter, contents do not
            self.before, self.dev = None, torch.empty(n, dtype=dtype, device=dev)
        else:
            self.before = torch.full((n,), SENT, dtype=dtype)
            if data is not None:
                q = data.to(dtype)
                assert torch.equal(q.double(), data.double()), "operand is not representable in %s" % dtype
                self.view(self.before).copy_(q)
            self.dev = self.before.to(dev)
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + off * self.dev.element_size()

    def view(self, flat):
        return flat.as_strided(*self.geom)


def _vec(dev, x, dtype=torch.float32, fill=True):
    if x is None:
        return None
    return x.to(dtype).to(dev) if fill else torch.empty(x.shape, dtype=dtype, device=dev)


def _strides(case, n_cols):
    N, K, lay = n_cols, case.K, case.layout
    n8 = (N + 7) // 8 * 8
    if lay == "tight":
        return dict(pad_a=0, pad_w=0, ldc=N, ldr=N, ldaux=N, ldc16=n8)
    if lay == "odd4":                                               # bf16: ld % 8 != 0 (scalar flush); fp32: still 16-byte rows
        return dict(pad_a=8, pad_w=8, ldc=n8 + 4, ldr=n8 + 4, ldaux=n8 + 4, ldc16=n8 + 4)
    if lay == "odd6":                                               # fp32: ld % 4 != 0 (direct stores of 9 / 10, generic fallback of 20-25)
        return dict(pad_a=8, pad_w=8, ldc=n8 + 6, ldr=n8 + 6, ldaux=n8 + 6, ldc16=n8 + 12)
    return dict(pad_a=8, pad_w=16, ldc=n8 + 8, ldr=n8 + 16, ldaux=n8 + 24, ldc16=n8 + 32)       # wide, off*


class _Launch:
    """Device operands, sentinel-filled outputs and the FabindGemmArgs of one case (built like kernels.gemm builds its own)."""

    def __init__(self, case, dev, fill=True):
        from fabind_amd._lib import DT_BF16, DT_F32, GemmArgs
        f, M, N, K, K1 = case.form, case.M, case.N, case.K, case.K1
        self.case, self.keep = case, []
        d = self.inputs = G.make_inputs(case)
        code = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}
        a_dt = torch.bfloat16 if case.ops == "bf16" else torch.float32
        w_dt = torch.float32 if case.ops in ("f32", "x3") else torch.bfloat16
        c_dt = {"f32": torch.float32, "bf16": torch.bfloat16, None: None}[f["c"]]
        opt = {"f32": torch.float32, "bf16": torch.bfloat16, None: None}
        off8 = lambda what, dt: (8 // torch.empty(0, dtype=dt).element_size()) if case.layout == "off" + what else 0
        s = _strides(case, N if not f["groups"] else max(G.GROUP_NS))
        a = self.args = GemmArgs()
        mk = lambda *p, **kw: self._own(_Buf(dev, *p, fill=fill, **kw))
        rows_a = d["A"].shape[0]
        A = mk(a_dt, rows_a, K1, K1 + s["pad_a"], off8("A", a_dt), data=d["A"][:, :K1])
        W = mk(w_dt, d["W"].shape[0], K, K + s["pad_w"], off8("A", w_dt) if case.layout == "offA" else 0, data=d["W"])
        a.A, a.W, a.lda, a.ldw = A.ptr, W.ptr, A.geom[1][0], W.geom[1][0]
        if f["a2"]:
            A2 = mk(a_dt, rows_a, K - K1, K - K1 + s["pad_a"], data=d["A"][:, K1:])
            a.A2, a.lda2 = A2.ptr, A2.geom[1][0]
        a.M, a.N, a.K, a.K1 = rows_a if f["groups"] else M, d["W"].shape[0] if f["groups"] else N, K, K1
        a.a_dtype, a.w_dtype = code[a_dt], code[w_dt]
        a.split3 = 1 if case.ops == "x3" else 0
        a.act_pro, a.act_epi, a.dact_epi = f["act_pro"], f["act"], f["dact"]
        a.alpha, a.accumulate, a.store_preact, a.k_splits = f["alpha"], int(f["accumulate"]), int(f["pre"]), f["splits"]
        self.out = {}
        if f["groups"]:
            self._groups(dev, c_dt, code, fill)
        elif c_dt is not None:
            rows = M * f["splits"]
            self.out["C"] = mk(c_dt, rows, N, s["ldc"], off8("C", c_dt), data=d.get("C_old"))
            a.C, a.ldc, a.c_dtype = self.out["C"].ptr, s["ldc"], code[c_dt]
        if f["c2"] is not None:
            c2_dt = torch.bfloat16 if f["c2"] == "bf16" else c_dt
            self.out["C2"] = mk(c2_dt, M, N, s["ldc"])               # C2 shares C's row stride
            a.C2, a.c2_bf16 = self.out["C2"].ptr, int(c2_dt == torch.bfloat16 and c_dt == torch.float32)
        if f["c16"]:
            self.out["C16"] = mk(torch.bfloat16, M, N, s["ldc16"])
            a.C16, a.ldc16 = self.out["C16"].ptr, s["ldc16"]
        if f["dot"]:
            nt = (N + G.BN - 1) // G.BN
            self.out["dot"] = mk(torch.float32, M, nt, nt + 3)
            a.dot_out, a.dot_ld = self.out["dot"].ptr, nt + 3
            a.dotvec = self._own(_vec(dev, d["u"], fill=fill)).data_ptr()
        if f["bias"]:
            a.bias = self._own(_vec(dev, d["bias"], fill=fill)).data_ptr()
        if f["r"] is not None:
            R = mk(opt[f["r"]], d["R"].shape[0], N, s["ldr"], off8("R", opt[f["r"]]), data=d["R"])
            a.R, a.ldr, a.r_dtype = R.ptr, s["ldr"], code[opt[f["r"]]]
            if f["gather"]:
                a.r_index = self._own(d["r_index"].to(dev)).data_ptr()
        if f["aux"] is not None:
            X = mk(opt[f["aux"]], M, N, s["ldaux"], off8("aux", opt[f["aux"]]), data=d["aux"])
            a.aux, a.ldaux, a.aux_dtype = X.ptr, s["ldaux"], code[opt[f["aux"]]]
        if f["fold"]:
            a.row_mu, a.row_rs, a.col_c = (self._own(_vec(dev, d[k], fill=fill)).data_ptr() for k in ("row_mu", "row_rs", "col_c"))
        if f["drop"]:
            a.p_drop, a.drop_seed = G.P_DROP, d["seed"]

    def _own(self, t):
        self.keep.append(t)
        return t

    def _groups(self, dev, c_dt, code, fill):
        """int32[8] descriptors {a_row0, M, w_row0, N, c_off lo, c_off hi, ldc, 0}; every group has its own ldc and a gap behind it."""
        a, desc, a0, w0, c0 = self.args, [], 0, 0, 4
        self.group_geom = []
        for i, (m, n) in enumerate(zip(G.GROUP_MS, G.GROUP_NS)):
            ld = n + (0, 8, 4, 6)[i]
            desc.append([a0, m, w0, n, c0, 0, ld, 0])
            self.group_geom.append(((m, n), (ld, 1), c0))
            a0, w0, c0 = a0 + m, w0 + n, c0 + max(m, 3) * ld + 8
        n = c0 + 16
        flat = torch.full((n,), SENT, dtype=c_dt)
        self.out["groups"] = (flat, flat.to(dev) if fill else torch.empty(n, dtype=c_dt, device=dev))
        a.groups = self._own(torch.tensor(desc, dtype=torch.int32).to(dev)).data_ptr()
        a.n_groups, a.max_m, a.max_n = len(desc), max(G.GROUP_MS), max(G.GROUP_NS)
        a.C, a.ldc, a.c_dtype = self.out["groups"][1].data_ptr(), 1, code[c_dt]

    def plan(self, lib):
        fam, epi, cfg = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_int(-9)
        rc = lib.fabind_gemm_plan(ctypes.byref(self.args), ctypes.byref(fam), ctypes.byref(epi), ctypes.byref(cfg))
        return rc, fam.value, epi.value, cfg.value

    def run(self, lib):
        from fabind_amd._lib import check, stream
        global _DEVICE_ERROR
        try:
            check(lib.fabind_gemm(ctypes.byref(self.args), stream()), "fabind_gemm " + self.case.id)
            torch.cuda.synchronize()
        except RuntimeError as e:                                 # a refused launch or a device error: nothing more is launched from this file
            _DEVICE_ERROR = "%s: %s" % (self.case.id, e)
            raise


def _mismatch(case, name, got, want, bad):
    idx = bad.nonzero()
    rows, cols = sorted(set(idx[:, 0].tolist())), sorted(set(idx[:, 1].tolist()))
    first = ["(%d, %d): got %r want %r" % (r, c, float(got[r, c]), float(want[r, c])) for r, c in idx[:6].tolist()]
    return ("%s %s: %d of %d elements differ; rows %s..%s (%d), columns %s..%s (%d); k-tiles %d at BK %d; first: %s"
            % (case.id, name, len(idx), bad.numel(), rows[0], rows[-1], len(rows), cols[0], cols[-1], len(cols), case.K // case.bk, case.bk,
               "; ".join(first)))


def _check_view(case, name, got, ref, dtype, exact, staged=None):
    """got / ref: float64 [rows, cols]; dtype: the output's storage type."""
    is16 = dtype == torch.bfloat16
    if exact:
        want = G.rne_bf16(ref) if is16 else ref
        if staged is not None:                                    # forms 14 / 16: the documented second rounding, stated in the reference
            assert bool(((got - want).abs() <= G.bf16_ulp(want)).all()), _mismatch(case, name + " (one bf16 ulp of the single rounding)", got, want,
                                                                                (got - want).abs() > G.bf16_ulp(want))
            want = staged
        bad = got != want
        assert not bool(bad.any()), _mismatch(case, name, got, want, bad)
        return
    bound = G.F32_TOL * max(1.0, float(ref.abs().max())) + (G.bf16_ulp(ref) if is16 else 0.0)
    err = (got - ref).abs()
    print("%s %s: max err %.3e, %.3f of its bound" % (case.id, name, float(err.max()), float((err / bound).max())))
    bad = ~(err <= bound)
    assert not bool(bad.any()), _mismatch(case, name, got, ref, bad)


def _verify(L):
    case, f = L.case, L.case.form
    ref = G.reference(case, L.inputs)
    if f["groups"]:
        before, devbuf = L.out["groups"]
        after, expect = devbuf.cpu(), before.clone()
        for geom, r in zip(L.group_geom, ref["groups"]):
            if geom[0][0] == 0:
                continue                                          # the empty group: its range keeps the sentinel
            got = after.as_strided(*geom).double()
            _check_view(case, "C (group at %d)" % geom[2], got, r, before.dtype, True)
            expect.as_strided(*geom).copy_(after.as_strided(*geom))
        assert torch.equal(after.view(_BITS[before.dtype]), expect.view(_BITS[before.dtype])), case.id + ": ragged output touched outside its groups"
        return
    for name, buf in L.out.items():
        after = buf.dev.cpu()
        got = buf.view(after).double()
        # without a transcendental between the accumulator and the store, the value is exact whatever the form's tier
        exact = f["tier"] == "exact" or (name == "C" and f["pre"] and not f["fold"])
        staged = ref.get("C_staged") if (name == "C" and case.epi_run in (14, 16)) else None
        _check_view(case, name, got, ref[name], buf.dtype, exact, staged)
        if f["drop"] and name == "C":                              # the mask itself, also where the value carries a tolerance
            assert torch.equal(got == 0, ref["C"] == 0), case.id + ": dropout mask differs from the restatement"
        expect = buf.before.clone()
        buf.view(expect).copy_(buf.view(after))
        assert torch.equal(after.view(_BITS[buf.dtype]), expect.view(_BITS[buf.dtype])), \
            "%s %s: sentinel overwritten outside the [%d, %d] view (ld %d)" % (case.id, name, *buf.geom[0], buf.geom[1][0])


def _by_group_and_form():
    keys = {}
    for c in G.CASES:
        keys.setdefault((c.group, c.form["name"]), []).append(c)
    return keys


_KEYED = _by_group_and_form()


@pytest.mark.parametrize("group,form", sorted(_KEYED), ids=["%s:%s" % k for k in sorted(_KEYED)])
def test_gemm_form_matches_float64_reference(group, form):
    """Every case of the table: reaches the family / epi_fast / configuration its row names (fabind_gemm_plan), is bit-equal to
    the float64 reference (exact tier) or within the fp32 bound (tolerance tier), and leaves every sentinel intact."""
    dev = _dev()
    assert _DEVICE_ERROR is None, "not run: an earlier launch failed (%s)" % _DEVICE_ERROR
    for case in _KEYED[(group, form)]:
        with _knobs(case.knobs) as lib:
            L = _Launch(case, dev)
            rc, fam, epi, cfg = L.plan(lib)
            assert (rc, fam, epi, cfg) == (0, case.family, case.epi, case.cfg), \
                "%s: plan says family %s epi_fast %d cfg %d (rc %d), the table %s / %d / %d" % (
                    case.id, G.FAMILY_NAMES.get(fam, fam), epi, cfg, rc, G.FAMILY_NAMES[case.family], case.epi, case.cfg)
            L.run(lib)
        _verify(L)


def test_table_reaches_every_family_and_epilogue():
    """The union of (family, epi_fast) pairs the table reaches -- asked of fabind_gemm_plan for every case, nothing launched --
    covers every family, every code the dispatcher can emit, and every fast code in each family that honours it (pipe: all;
    x3: all but the LayerNorm fold 12 / 13, which exists for bf16 operands only; the prologue form of x3: the reduced list)."""
    from fabind_amd import _lib as L_
    dev = _dev()
    reached, pipe_cfgs, x3_tiles = set(), set(), set()
    for case in G.CASES:
        with _knobs(case.knobs) as lib:
            rc, fam, epi, cfg = _Launch(case, dev, fill=False).plan(lib)
        assert rc == 0, case.id
        reached.add((fam, epi if fam in G.FAST_FAMILIES else 0))
        if fam == L_.GEMM_FAM_PIPE:
            pipe_cfgs.add(cfg)
        if fam == L_.GEMM_FAM_X3:
            x3_tiles.add(cfg)
    want = {(fam, 0) for fam in G.FAMILY_NAMES}
    want |= {(L_.GEMM_FAM_PIPE, e) for e in G.EMITTED_CODES}
    want |= {(L_.GEMM_FAM_X3, e) for e in G.EMITTED_CODES if e not in (12, 13)}
    want |= {(L_.GEMM_FAM_X3_PRO, G.FORM[n]["epi"]) for n in G.PRO_FORMS}
    want.discard((L_.GEMM_FAM_X3_PRO, 0))                          # (its reduced list holds fast codes only)
    missing = sorted(want - reached)
    assert not missing, "unreached (family, epi_fast): %s" % [(G.FAMILY_NAMES[f], e) for f, e in missing]
    assert pipe_cfgs == set(G.PIPE_CONFIGS) and x3_tiles == {2, 4}, (pipe_cfgs, x3_tiles)
    # every configuration runs its whole list at every ring fill: nk = 1, 2, 3 at BK 64 / 2, 4, 6 at BK 32
    for c in G.PIPE_CONFIGS:
        ks = {case.K for case in G.CASES if case.family == L_.GEMM_FAM_PIPE and case.cfg == c and case.form["name"] in G.REDUCED}
        assert ks >= set(G.KS), (c, ks)


def test_plan_follows_the_small_m_switch_and_refuses_an_unreachable_fold():
    """fabind_gemm_plan alone (nothing is launched): the default configuration is 13 from 100 tiles of 256 x 128 on and 6 below;
    the LayerNorm fold is refused where the generic epilogue would run (it ignores row_mu / row_rs / col_c): under
    fabind_gemm_set_config(0) and for an A whose base is only 8-byte aligned."""
    from fabind_amd import _lib as L_
    dev = _dev()
    case = next(c for c in G.CASES if c.form["name"] == "bf16_fold_relu" and c.layout == "wide" and c.cfg == 13)
    with _knobs(G.DEFAULT_KNOBS) as lib:
        L = _Launch(case, dev, fill=False)
        for M, cfg in ((256 * 100, 13), (256 * 100 - 1, 13), (256 * 99, 6), (1, 6)):
            L.args.M, L.args.N = M, 128                            # (never launched: the buffers are those of the small case)
            assert L.plan(lib) == (0, L_.GEMM_FAM_PIPE, 12, cfg), (M, L.plan(lib))
        L.args.M, L.args.N = case.M, case.N
        L.args.A += 8
        rc, fam, _, _ = L.plan(lib)
        assert rc != 0 and fam == -1 and b"fold" in lib.fabind_last_error()
        L.args.A -= 8
        assert L.plan(lib)[0] == 0
    with _knobs(dict(G.DEFAULT_KNOBS, config=0)) as lib:
        rc, fam, _, _ = L.plan(lib)
        assert rc != 0 and fam == -1
