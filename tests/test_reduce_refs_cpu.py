"""CPU: the restatements of tests/reduce_refs.py against float64 torch autograd and against explicit sequential loops, the case tables
of tests/test_gpu_reduce_forms.py against the classes they claim to reach (computed from the launchers' own constants, restated in
reduce_refs.py with the lines they come from), the binding of the entry points under test, and the host-side guards of
fabind_gather_dact."""
import os
import re

import numpy as np
import pytest
import torch

import gemm_refs as GR
import reduce_refs as RR
from reduce_refs import ACT_NONE, ACT_RELU, ACT_SILU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _csr(g, n_rows, max_len):
    lens = torch.randint(0, max_len, (n_rows,), generator=g)
    lens[1] = 0
    rp = RR.rowptr_of(lens.tolist())
    return rp, RR.CR.rows_of(rp)


# ------------------------------------------------------------------------------------------------
# adjoints against float64 autograd of the forward restatements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_NONE, ACT_SILU, ACT_RELU, RR.ACT_SIGMOID])
@pytest.mark.parametrize("perm", [False, True])
def test_gather_dact_is_the_adjoint_of_segment_sum(act, perm):
    g = torch.Generator().manual_seed(5)
    rp, row = _csr(g, 9, 6)
    E = row.numel()
    Z = (torch.randn(E, 5, generator=g, dtype=F64) + 0.3).requires_grad_()
    eidx = torch.randperm(E, generator=g) if perm else None
    cot = torch.randn(9, 5, generator=g, dtype=F64)
    out = RR.segment_sum(Z, rp, act, eidx)
    out.backward(cot)
    # the permuted walk reads Z[eidx[e]] for the edge at position e: its adjoint scatters back through the same permutation
    src_row = row if eidx is None else torch.empty_like(row).scatter_(0, eidx, row)
    ref = RR.gather_dact(cot, src_row, Z.detach(), act)
    assert (Z.grad - ref).abs().max() <= 1e-13


@pytest.mark.parametrize("act", [ACT_NONE, ACT_SILU, ACT_RELU])
@pytest.mark.parametrize("N", [4, 132, 260])
def test_rowdot_bwd_is_the_adjoint_of_the_row_dot(N, act):
    g = torch.Generator().manual_seed(N)
    M, nt = 7, (N + 127) // 128
    z = (torch.randn(M, N, generator=g, dtype=F64) + 0.2).requires_grad_()
    u = torch.randn(N, generator=g, dtype=F64).requires_grad_()
    dpart = torch.randn(M, nt, generator=g, dtype=F64)
    prod = GR.act(z, act) * u
    part = torch.stack([prod[:, t * 128:(t + 1) * 128].sum(1) for t in range(nt)], 1)
    part.backward(dpart)
    dz, du = RR.rowdot_bwd(z.detach(), dpart, u.detach(), act)
    assert (z.grad - dz).abs().max() <= 1e-13 and (u.grad - du).abs().max() <= 1e-12


def test_gcl_pre_bwd_is_the_adjoint_of_gcl_pre():
    g = torch.Generator().manual_seed(2)
    n, H = 11, 6
    rp, row = _csr(g, n, 5)
    E = row.numel()
    col = torch.randint(0, n, (E,), generator=g)
    AB = torch.randn(n, 2 * H, generator=g, dtype=F64).requires_grad_()
    rh = torch.randn(E, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(H, generator=g, dtype=F64).requires_grad_()
    dpre = torch.randn(E, H, generator=g, dtype=F64)
    RR.gcl_pre_fwd(AB, row, col, rh, w, H).backward(dpre)
    drh, dw = RR.gcl_pre_bwd(dpre, rh.detach(), w.detach())
    assert (rh.grad - drh).abs().max() <= 1e-13 and (w.grad - dw).abs().max() <= 1e-13
    # dAB: the receiving half is the segment sum over the CSR rows, the sending half the one over the edges grouped by column
    perm = torch.argsort(col, stable=True)
    colptr = RR.rowptr_of(torch.bincount(col, minlength=n).tolist())
    assert (AB.grad[:, :H] - RR.segment_sum(dpre, rp, ACT_NONE)).abs().max() <= 1e-13
    assert (AB.grad[:, H:] - RR.segment_sum(dpre, colptr, ACT_NONE, perm)).abs().max() <= 1e-13


# ------------------------------------------------------------------------------------------------
# the float32 runs are sequential, bit for bit
# ------------------------------------------------------------------------------------------------
def test_float32_sums_run_in_operand_order():
    g = torch.Generator().manual_seed(0)
    x = RR.feat(g, 777, 5)

    def loop(rows):
        s = np.zeros(rows.shape[1], dtype=np.float32)
        for r in rows.numpy():
            s = s + r
        return torch.from_numpy(s)

    assert torch.equal(RR.colsum(x, torch.float32), loop(x))
    assert not torch.equal(RR.colsum(x, torch.float32).double(), RR.colsum(x))          # (float64 differs: the check above is not vacuous)
    lens = [0, 3, 0, 700, 1, 73]
    rp = RR.rowptr_of(lens)
    eidx = torch.randperm(777, generator=g)
    for e in (None, eidx):
        out = RR.segment_sum(x, rp, ACT_NONE, e, dtype=torch.float32)
        src = x if e is None else x[e]
        for r in range(len(lens)):
            assert torch.equal(out[r], loop(src[int(rp[r]):int(rp[r + 1])])), r
    head, tail = RR.split_sum(x[:7, :4].reshape(7, 4).contiguous().repeat(1, 2), 4, torch.float32)
    assert head.shape == (4,) and tail.shape == (4,) and torch.equal(head, loop(x[:7, :4]))


def test_small_restatements_on_hand_cases():
    assert RR.exclusive_scan(torch.tensor([3, 0, 2], dtype=torch.int32)).tolist() == [0, 3, 3, 5]
    assert RR.exclusive_scan(torch.zeros(0, dtype=torch.int32)).tolist() == [0]
    out = torch.full((4, 3), 7.0)
    z = RR.zero_empty_rows(RR.rowptr_of([0, 2, 0, 1]), out, 2)
    assert z.tolist() == [[0, 0, 7], [7, 7, 7], [0, 0, 7], [7, 7, 7]]
    dy = torch.tensor([[1.0, -2.0], [3.0, 4.0]])
    y = torch.tensor([[0.0, -0.0], [2.0, -1.0]])
    o, cs = RR.mul_dact(dy, y, ACT_RELU, 2.0)
    assert o.tolist() == [[0, 0], [6, 0]] and cs.tolist() == [6, 0]
    o, _ = RR.mul_dact(dy, y, ACT_SILU, 1.0)
    assert float(o[0, 0]) == 0.5 and float(o[0, 1]) == -1.0                              # silu'(+-0) = 1/2
    o, cs = RR.mul_dropmask(torch.ones(64, 8), RR.DROP_SEED, 0.5)
    keep, scale = GR.drop_keep(RR.DROP_SEED, 64, 8, 0.5)
    assert scale == 2.0 and torch.equal(o, torch.from_numpy(keep).double() * 2) and 0.3 < float(o.mean()) / 2 < 0.7
    assert RR.DROP_SEED + 63 * 8 + 7 > 2 ** 32                                           # the key wraps inside this small case already


# ------------------------------------------------------------------------------------------------
# the tables reach every class
# ------------------------------------------------------------------------------------------------
def test_launch_constants_match_the_sources():
    """The restated constants are the launchers' (a change there must come here too)."""
    gcl = open(os.path.join(ROOT, "fabind_amd", "csrc", "gcl.hip")).read()
    bwd = open(os.path.join(ROOT, "fabind_amd", "csrc", "bwd.hip")).read()
    gemm = open(os.path.join(ROOT, "fabind_amd", "csrc", "gemm.hip")).read()
    kern = open(os.path.join(ROOT, "fabind_amd", "kernels.py")).read()
    for text, src in (("const int heavy_min = n_rows < 16384 ? 32 : 128;", gcl),
                      ("while (rpw > 64 && (n_rows + rpw - 1) / rpw < 256) rpw >>= 1;", gcl),
                      ("ss_accum<NSLAB, 8 / NSLAB>(Z, z_dt, ldz, H, eidx, act, lane, e0, e1, 1, acc);", gcl),
                      ("ss_accum<NSLAB, 8 / NSLAB>(Z, z_dt, ldz, H, eidx, act, lane, rowptr[r] + w, rowptr[r + 1], 16, acc);", gcl),
                      ("if (e1 - e0 > heavy_min) return;", gcl), ("rowptr[rr + 1] - rowptr[rr] > heavy_min", gcl),
                      ("for (; r + 12 < r1; r += 16)", bwd), ("for (; k + 48 < nchunk; k += 64)", bwd), ("const int t = c / 128;", bwd),
                      ("for (; r + 12 < r1; r += 16)", gemm), ("for (int k = q; k < nchunk; k += 4)", gemm),
                      ("return max(1, min(4096, (rows + 63) // 64))", kern), ("nchunk = max(1, min(2048, (E + 255) // 256))", kern),
                      ("return max(1, min(1024, (rows + 255) // 256))", kern)):
        assert text in src, text


def test_segment_sum_table_reaches_every_class():
    names = [c["name"] for c in RR.SEG_CASES]
    assert len(set(names)) == len(names)
    seen = dict(heavy_min=set(), rpw=set(), light=set(), heavy=set(), H=set(), nrows=set(), form=set(), dt=set(), ldz=set(), act=set(), perm=set())
    heavy_perm_forms, groups_1024 = set(), None
    for c in RR.SEG_CASES:
        lens, p = RR.seg_case_lengths(c), RR.seg_launch(c["n_rows"], c["H"])
        U, hm = p["U"], p["heavy_min"]
        assert len(lens) == c["n_rows"] and lens[-1] > hm, c["name"]                     # a heavy row at n_rows - 1
        if c["n_rows"] >= 5:
            assert lens[0] == 0 and lens[-2] == 0, c["name"]                              # empty first rows, empty rows at the end
        for k in ("heavy_min", "rpw"):
            seen[k].add(p[k])
        for L in lens:
            if L <= hm:
                seen["light"].add((p["nslab"], RR.accum_class(L, U), L % U != 0))
            else:
                for n in RR.heavy_wave_edges(L):
                    seen["heavy"].add((p["nslab"], RR.accum_class(n, U), n % U != 0))
        if c["n_rows"] == 70:                                                             # the lengths the issue lists, relative to this launch
            want = {0, 1, U - 1, U, U + 1, 2 * U + 3, hm, hm + 1, hm + 15, 16 * U, 16 * U + 1, 32 * U + 7}
            assert want <= set(lens), (c["name"], want - set(lens))
            assert c["H"] > 136 or 1500 in lens
        seen["H"].add(c["H"]); seen["nrows"].add(c["n_rows"]); seen["form"].add((p["nslab"], c["out_form"])); seen["dt"].add(c["z_dt"])
        seen["ldz"].add(c["ldz_pad"] > 0); seen["act"].add(c["act"]); seen["perm"].add(c["perm"])
        if c["perm"]:
            heavy_perm_forms.add(p["nslab"])
        if p["rpw"] == 1024:
            heavy = [r for r, L in enumerate(lens) if L > hm]
            groups_1024 = [[r for r in heavy if r // 1024 == gidx] for gidx in range(c["n_rows"] // 1024)]
            assert c["H"] == 8 and c["z_dt"] == RR.BF and sum(lens) * 8 * 2 <= 6 * 2 ** 20
            assert sum(1 for L in lens if L <= 2) >= 0.99 * len(lens)
    assert seen["heavy_min"] == {32, 128} and seen["rpw"] == {64, 128, 1024}
    assert seen["H"] == set(RR.SEG_HS) and seen["nrows"] >= {1, 5, 70, 16383, 16384, 40000, 262144}
    assert seen["form"] == {(s, f) for s in (1, 2) for f in RR.SEG_OUT_FORMS}
    assert seen["dt"] == {RR.F32, RR.BF} and seen["ldz"] == {False, True} and seen["perm"] == {False, True} and heavy_perm_forms == {1, 2}
    assert seen["act"] == {ACT_NONE, ACT_SILU, ACT_RELU}
    for s in (1, 2):
        # one-wave rows: empty, only the ragged group, exactly one full group, full groups with and without a ragged group behind them
        assert {(s, "0", False), (s, "<U", True), (s, "=U", False), (s, ">U", True), (s, ">U", False)} <= seen["light"], (s, seen["light"])
        # a wave of the cooperative kernel: fewer than U, exactly U, more than U edges
        assert {(s, "<U", True), (s, "=U", False), (s, ">U", True)} <= seen["heavy"], (s, seen["heavy"])
    # a wave of the cooperative kernel with NO edge cannot occur behind this launcher: a heavy row has more than heavy_min >= 32 edges and
    # the 16 waves take them round-robin, so every wave owns at least two
    assert min(RR.heavy_wave_edges(33)) == 2 and not any(k[1] == "0" for k in seen["heavy"])
    # rpw = 1024: a work-group with >= 3 heavy rows among them its first and its last scanned row, and work-groups with none
    assert any(len(gr) >= 3 and gr[0] % 1024 == 0 and gr[-1] % 1024 == 1023 for gr in groups_1024)
    assert sum(1 for gr in groups_1024 if not gr) >= 200
    # the threshold pair: one table on both sides of n_rows = 16384 with rows of 33 .. 128 edges
    a = RR.seg_case_lengths(dict(n_rows=16383, H=8))
    b = RR.seg_case_lengths(dict(n_rows=16384, H=8))
    assert b == [0] + a and {33, 64, 100, 128, 129} <= set(a)
    # (heavy_min mutation: these rows are one-wave rows at 128 and cooperative rows at 32 -- a kernel pair that disagrees skips them)
    assert sum(1 for L in b if 32 < L <= 128) >= 8


def test_chunked_tables_reach_every_class():
    # mul_dact_colsum / mul_dropmask_colsum
    rs = RR.mdc_rows() + [RR.MDC_BIG_R]
    nch = {RR.nchunk_mul_dact_colsum(R) for R in rs}
    assert set(RR.MDC_NCHUNKS) <= nch and 4096 in nch
    assert set(RR.MDC_LAST_ROWS) <= {[n for n in RR.chunk_rows(R, RR.nchunk_mul_dact_colsum(R)) if n][-1] for R in rs}
    r4 = set().union(*[RR.rows4_class(n) for R in rs for n in RR.chunk_rows(R, RR.nchunk_mul_dact_colsum(R))])
    assert {(False, False), (False, True), (True, False), (True, True)} <= r4                    # both loops, alone and together, and neither
    # 13 rows: lane 0 runs the 4-in-flight loop only, lanes 1-3 the tail only (r + 12 < r1 against r + 16 < r1 differ here)
    assert RR.rows4_class(13) == {(True, False), (False, True)} and RR.rows4_class(16) == {(True, False)} and RR.rows4_class(17) == {(True, True), (True, False)}
    sc = {n: RR.sum_chunks_class(n) for n in nch}
    assert sc[48] == {(0, 3)} and (1, 0) in sc[49] and sc[64] == {(1, 0)} and (1, 1) in sc[65] and (2, 0) in sc[113]    # both sides of k + 48 < nchunk
    assert 0 in RR.chunk_rows(RR.MDC_BIG_R, 4096) and RR.chunk_rows(RR.MDC_BIG_R, 4096)[-1] == 0      # empty trailing chunks
    # rowdot_bwd: the same sum_chunks classes through explicit nchunk, a one-row last chunk
    rd = RR.rowdot_cases()
    assert {n for _, n in rd if n} == set(RR.MDC_NCHUNKS) - {1} and all(RR.chunk_rows(M, n)[-1] == 1 for M, n in rd if n)
    assert {RR.nchunk_colsum(M) for M, n in rd if n is None} >= {1, 2, 4}
    # gcl_pre_bwd and colsum: capped nchunk with empty trailing chunks
    assert RR.nchunk_gcl_pre(RR.GCL_BIG_E) == 2048 and RR.chunk_rows(RR.GCL_BIG_E, 2048)[-1] == 0
    assert RR.nchunk_colsum(RR.COLSUM_BIG_R) == 1024 and RR.chunk_rows(RR.COLSUM_BIG_R, 1024)[-1] == 0
    assert {RR.nchunk_colsum(R) for R in RR.COLSUM_RS} == {1, 2, 4}                                # the direct single-chunk path and the two-pass one
    r4 = set().union(*[RR.rows4_class(n) for R in RR.COLSUM_RS for n in RR.chunk_rows(R, RR.nchunk_colsum(R))])
    assert {(False, False), (False, True), (True, False), (True, True)} <= r4
    # colsum_part_kernel's paths: 4-wide (ldi % 4 == 0 and c + 3 < C), scalar by ldi, scalar by the last columns
    assert any(C % 4 == 0 for C in RR.COLSUM_CS) and any(C % 4 for C in RR.COLSUM_CS) and {1, 3, 5, 65} <= set(RR.COLSUM_CS)


def test_entry_points_are_declared_and_bound():
    from fabind_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fabind_hip.h")).read(), flags=re.S)    # (comments inside prototypes)
    for name in ("fabind_segment_sum", "fabind_zero_empty_rows", "fabind_exclusive_scan", "fabind_colsum", "fabind_split_sum",
                 "fabind_mul_dact", "fabind_mul_dact_colsum", "fabind_mul_dropmask_colsum", "fabind_rowdot_bwd", "fabind_gcl_pre_bwd",
                 "fabind_gather_dact"):
        assert name in _lib.SIGNATURES
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_gather_dact_refuses_on_the_host_before_any_launch():
    """H % 4, ldo % 4 and the alignment of dout are refused by the launcher itself (rc -1 and its own message): nothing is launched, so
    this runs without a device -- the pointers are never followed."""
    from fabind_amd import _lib
    lib = _lib.load()
    a = 1 << 20                                                    # any 16-byte aligned address
    for H, ldo, dout in ((6, 8, a), (8, 6, a), (8, 8, a + 4)):
        rc = lib.fabind_gather_dact(dout, ldo, a, a, _lib.DT_F32, ACT_NONE, a, _lib.DT_F32, 3, H, None)
        assert rc == -1 and lib.fabind_last_error().decode().startswith("fabind_gather_dact:"), (H, ldo, rc)
    assert lib.fabind_gather_dact(a, 8, a, a, _lib.DT_F32, ACT_NONE, a, _lib.DT_F32, 0, 6, None) == 0     # no edges: nothing to refuse
