"""Plain-torch restatements of the segment sums and of the fixed-order reduction adjoints (csrc/gcl.hip: fabind_segment_sum,
fabind_zero_empty_rows; csrc/bwd.hip: mul_dact, mul_dact_colsum / mul_dropmask_colsum, rowdot_bwd, gcl_pre_bwd, gather_dact;
csrc/gemm.hip: colsum, split_sum; csrc/graph.hip: exclusive_scan), the launch constants of those kernels restated from their host
launchers, and the case tables of tests/test_gpu_reduce_forms.py.  No GPU is needed to import this.

Every restatement computes in the `dtype` it is given, on host tensors: float64 is the reference, float32 gives that reference's own
rounding on the same operands (`err32`); bf16 operands enter with their exact values.  Sums in float32 run SEQUENTIALLY in operand
order (`seq_sum0`: numpy's add.accumulate; `segment_sum`: CPU index_add_), never as a tree: a sequential sum of n terms carries the
largest rounding any order can have, so a kernel's tree stays inside `coord_refs.bound(err32)`.  tests/test_reduce_refs_cpu.py pins
the sequential order bit for bit, the adjoints to float64 autograd and the tables to the classes they claim."""
import numpy as np
import torch

import coord_refs as CR
import gemm_refs as GR
from fabind_amd._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_STORED_DERIV

BF, F32 = torch.bfloat16, torch.float32
ACTS = (ACT_NONE, ACT_SILU, ACT_RELU, ACT_SIGMOID, ACT_STORED_DERIV)
ACT_NAMES = {ACT_NONE: "none", ACT_SILU: "silu", ACT_RELU: "relu", ACT_SIGMOID: "sigmoid", ACT_STORED_DERIV: "stored"}


# ------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------
def seq_sum0(x):
    """Sum over dim 0, one row after the other in the dtype of x  ->  [x.shape[1:]]."""
    if x.shape[0] == 0:
        return x.new_zeros(x.shape[1:])
    return torch.from_numpy(np.add.accumulate(x.contiguous().numpy(), axis=0)[-1].copy())


def segment_sum(Z, rowptr, act, eidx=None, dtype=torch.float64):
    """out[r] = sum over e in [rowptr[r], rowptr[r + 1]) of act(Z[eidx[e] if eidx is given else e]), edge after edge."""
    Z = Z.to(dtype)
    n_rows = rowptr.numel() - 1
    n_e = int(rowptr[-1])
    src = Z[eidx.long()[:n_e]] if eidx is not None else Z[:n_e]
    return torch.zeros(n_rows, Z.shape[1], dtype=dtype).index_add_(0, CR.rows_of(rowptr), GR.act(src, act))


def gather_dact(dout, row, Z, act, dtype=torch.float64):
    """dZ[e] = dout[row[e]] * act'(Z[e]): the adjoint of segment_sum."""
    return dout.to(dtype)[row.long()] * GR.dact(Z.to(dtype), act)


def colsum(x, dtype=torch.float64):
    return seq_sum0(x.to(dtype))


def split_sum(part, n_tail, dtype=torch.float64):
    """part [splits, n]  ->  (head [n - n_tail], tail [n_tail]) of the sum over the splits in split order."""
    s = seq_sum0(part.to(dtype))
    n = s.numel()
    return s[:n - n_tail], s[n - n_tail:]


def mul_dact(dy, y, act, scale, dtype=torch.float64):
    """(scale * dy * act'(y), its column sums when dy is a matrix)."""
    out = torch.tensor(scale, dtype=torch.float32).to(dtype) * dy.to(dtype) * GR.dact(y.to(dtype), act)
    return out, (seq_sum0(out) if out.dim() == 2 else None)


def mul_dropmask(dy, seed, p, dtype=torch.float64):
    """(dy * keep / (1 - thr / 65536), its column sums): keep[r, c] = fb_hash32(seed + r * C + c) & 0xffff >= thr, thr = round(p * 65536),
    the key wrapping mod 2^32."""
    R, C = dy.shape
    keep, _ = GR.drop_keep(seed, R, C, p)
    thr = GR.drop_threshold(p)
    scale = torch.tensor(1.0, dtype=dtype) / (torch.tensor(1.0, dtype=dtype) - torch.tensor(thr / 65536.0, dtype=dtype))
    out = torch.where(torch.from_numpy(keep), scale * dy.to(dtype), torch.zeros((), dtype=dtype))
    return out, seq_sum0(out)


def rowdot_bwd(z, dpart, u, act, dtype=torch.float64):
    """Adjoint of part[m, t] = sum over the 128-column tile t of act(z[m, n]) u[n]:
    dz[m, n] = dpart[m, n // 128] u[n] act'(z[m, n]);  du[n] = sum_m dpart[m, n // 128] act(z[m, n])."""
    z, dpart, u = z.to(dtype), dpart.to(dtype), u.to(dtype)
    g = dpart[:, torch.arange(z.shape[1]) // 128]
    return g * u * GR.dact(z, act), seq_sum0(g * GR.act(z, act))


def gcl_pre_fwd(AB, row, col, rhohat, w_r, H):
    """pre[e] = AB[row[e], :H] + AB[col[e], H:] + rhohat[e] w_r (differentiable: the forward whose adjoint gcl_pre_bwd states)."""
    return AB[row.long(), :H] + AB[col.long(), H:] + rhohat[:, None] * w_r


def gcl_pre_bwd(dpre, rhohat, w_r, dtype=torch.float64):
    """drh[e] = dpre[e] . w_r;  dw[c] = sum_e rhohat[e] dpre[e, c]."""
    dpre, rhohat, w_r = dpre.to(dtype), rhohat.to(dtype), w_r.to(dtype)
    return seq_sum0((dpre * w_r).t()), seq_sum0(rhohat[:, None] * dpre)


def zero_empty_rows(rowptr, out, C):
    """out with [0, C) of every row without edges set to zero; everything else as it was."""
    o = out.clone()
    rp = rowptr.long()
    o[(rp[1:] == rp[:-1]).nonzero().flatten(), :C] = 0
    return o


def exclusive_scan(deg):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg.long(), 0)])


def rowptr_of(lens):
    return exclusive_scan(torch.as_tensor(lens, dtype=torch.int64)).to(torch.int32)


# ------------------------------------------------------------------------------------------------
# launch constants, restated from the host launchers (the comments name the lines they come from)
# ------------------------------------------------------------------------------------------------
def seg_launch(n_rows, H):
    """fabind_segment_sum (csrc/gcl.hip)  ->  dict(heavy_min, rpw, U, nslab).
      rpw:        `int rpw = 1024; while (rpw > 64 && (n_rows + rpw - 1) / rpw < 256) rpw >>= 1;`
      heavy_min:  `const int heavy_min = n_rows < 16384 ? 32 : 128;`
      nslab, U:   `if (H <= 512)` launches <1>, else <2>; both kernels call ss_accum<NSLAB, 8 / NSLAB>."""
    rpw = 1024
    while rpw > 64 and (n_rows + rpw - 1) // rpw < 256:
        rpw >>= 1
    nslab = 1 if H <= 512 else 2
    return dict(heavy_min=32 if n_rows < 16384 else 128, rpw=rpw, U=8 // nslab, nslab=nslab)


HEAVY_WAVES = 16          # segment_sum_heavy_kernel: __launch_bounds__(1024), stride 16 from rowptr[r] + w


def heavy_wave_edges(L):
    """Edges each of the 16 waves of the cooperative kernel owns in a row of L edges (e = e0 + w, e0 + w + 16, ...)."""
    return [max(0, (L - w + HEAVY_WAVES - 1) // HEAVY_WAVES) for w in range(HEAVY_WAVES)]


def accum_class(n, U):
    """Which part of ss_accum a walk of n edges runs: the full-group loop (n >= U), the predicated ragged group (n % U != 0)."""
    return "0" if n == 0 else "<U" if n < U else "=U" if n == U else ">U"


def nchunk_mul_dact_colsum(R):
    """kernels._nchunk_fused (mul_dact_colsum / mul_dropmask_colsum): `max(1, min(4096, (rows + 63) // 64))`."""
    return max(1, min(4096, (R + 63) // 64))


def nchunk_gcl_pre(E):
    """kernels.gcl_pre_bwd: `nchunk = max(1, min(2048, (E + 255) // 256))`."""
    return max(1, min(2048, (E + 255) // 256))


def nchunk_colsum(R):
    """kernels._nchunk (colsum, rowdot_bwd): `max(1, min(1024, (rows + 255) // 256))`."""
    return max(1, min(1024, (R + 255) // 256))


def chunk_rows(R, nchunk):
    """Rows of every chunk: `rows_per = (R + nchunk - 1) / nchunk; r0 = k * rows_per; r1 = min(R, r0 + rows_per)` (bwd.hip / gemm.hip)."""
    per = max(1, (R + nchunk - 1) // nchunk)
    return [max(0, min(R, k * per + per) - k * per) for k in range(nchunk)]


def rows4_class(rows):
    """The 4-row-lane loops of mul_dact_colsum_kernel / colsum_part_kernel over a chunk of `rows` rows (lane q starts at r0 + q):
    `for (; r + 12 < r1; r += 16)` then `for (; r < r1; r += 4)`  ->  set of (row-lane ran the 4-in-flight loop, row-lane ran the tail)."""
    out = set()
    for q in range(4):
        r, unrolled, tail = q, False, False
        while r + 12 < rows:
            r, unrolled = r + 16, True
        while r < rows:
            r, tail = r + 4, True
        out.add((unrolled, tail))
    return out


def sum_chunks_class(nchunk):
    """sum_chunks_kernel (bwd.hip): row-lane q of 16 runs `for (k = q; k + 48 < nchunk; k += 64)` then `for (; k < nchunk; k += 16)`
    ->  set of (trips of the 4-way loop, trips of the tail) over the 16 row-lanes."""
    out = set()
    for q in range(16):
        k, a, b = q, 0, 0
        while k + 48 < nchunk:
            k, a = k + 64, a + 1
        while k < nchunk:
            k, b = k + 16, b + 1
        out.add((a, b))
    return out


def rows_for(nchunk_of, nchunk, last):
    """Smallest R with nchunk_of(R) == nchunk whose last chunk holds `last` rows (None if there is none)."""
    for R in range(1, 64 * nchunk + 1):
        if nchunk_of(R) == nchunk and chunk_rows(R, nchunk)[-1] == last:
            return R
    return None


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def feat(g, *shape):
    """Features with mean 4 and spread 1.5: column sums do not cancel."""
    return torch.randn(*shape, generator=g) * 1.5 + 4.0


def bf_exact(t):
    return t.bfloat16().float()


def preact(g, *shape):
    """Pre-activations around 0 with exact 0.0 and -0.0 elements and bf16-exact values (both signs: SiLU' and ReLU' switch)."""
    t = bf_exact(torch.randn(*shape, generator=g) * 1.5 + 0.5)
    f = t.view(-1)
    if f.numel() >= 2:
        f[0], f[-1] = 0.0, -0.0
    if f.numel() >= 7:
        f[3], f[6] = -0.0, 0.0
    return t


# ------------------------------------------------------------------------------------------------
# segment_sum case table
# ------------------------------------------------------------------------------------------------
def special_lengths(n_rows, H, with_1500=True):
    """The row lengths at the edges of the launch's own thresholds."""
    p = seg_launch(n_rows, H)
    U, hm = p["U"], p["heavy_min"]
    out = [0, 1, U - 1, U, U + 1, 2 * U + 3, hm, hm + 1, hm + 15, 16 * U, 16 * U + 1, 32 * U + 7]
    return out + ([1500] if with_1500 else [])


def seg_lengths(n_rows, H, seed=0):
    """Row lengths of one table: empty first rows, empty rows ahead of the last one, a heavy row at n_rows - 1, the special lengths in
    between and 0-2 edges everywhere else."""
    p = seg_launch(n_rows, H)
    U, hm = p["U"], p["heavy_min"]
    if n_rows == 1:
        return [1500 if H <= 136 else 32 * U + 7]
    if n_rows == 5:
        return [0, hm, hm + 1, 0, 16 * U + 1 if 16 * U + 1 > hm else hm + 15]
    g = torch.Generator().manual_seed(1000 + seed)
    lens = torch.randint(0, 3, (n_rows,), generator=g).tolist()
    sp = special_lengths(n_rows, H, with_1500=H <= 136)
    if n_rows < 1024:
        lens[:2] = [0, 0]
        lens[2:2 + len(sp)] = sp
    elif p["rpw"] < 1024:
        # the 16383 / 16384 pair and the rpw = 128 table: rows of 33 .. 128 edges (one-wave rows at heavy_min = 128, cooperative at 32)
        # next to the lengths at both thresholds, scattered over the work-groups
        lens[:2] = [0, 0]
        for i, L in enumerate(sorted(set(sp + [33, 40, 47, 64, 65, 100, 127, 128, 129, 143, 32, 263]))):
            lens[5 + 37 * i] = L
    else:
        # rpw = 1024: work-group 3 scans rows 3072 .. 4095 and finds heavy rows at its first and last row and two in between;
        # work-group 5 holds the special lengths; every other one but the last has no heavy row
        lens[:2] = [0, 0]
        lens[3072], lens[3500], lens[3501], lens[4095] = hm + 1, 1500, hm + 15, 32 * U + 7
        lens[5 * 1024 + 7:5 * 1024 + 7 + len(sp)] = sp
    lens[-3:] = [0, 0, max(32 * U + 7, hm + 1)]
    return lens


SEG_HS = (8, 32, 136, 512, 520, 1024)
SEG_OUT_FORMS = ("fresh", "dAB_lo", "dAB_hi", "out16", "both")


def _seg_cases():
    cases = []
    i = 0
    for n_rows in (1, 5, 70):
        for H in SEG_HS:
            # (i, i // k) walks: every dtype, leading dimension, activation, permutation and output form comes up with every H class
            cases.append(dict(n_rows=n_rows, H=H, z_dt=(F32, BF)[i % 2], ldz_pad=(0, 8)[(i // 2) % 2], act=(ACT_NONE, ACT_SILU, ACT_RELU)[i % 3],
                              perm=bool((i // 3) % 2), out_form=SEG_OUT_FORMS[i % 5]))
            i += 1
    # every output form and the permuted walk with heavy rows at both slab counts, beyond what the walk above happens to give
    for H in (136, 520):
        for j, form in enumerate(SEG_OUT_FORMS):
            cases.append(dict(n_rows=70, H=H, z_dt=(BF, F32)[j % 2], ldz_pad=(8, 0)[j % 2], act=(ACT_SILU, ACT_RELU, ACT_NONE)[j % 3], perm=j % 2 == 0,
                              out_form=form))
    for n_rows, z_dt, perm, form in ((16383, F32, False, "fresh"), (16384, F32, False, "fresh"), (16384, F32, True, "dAB_hi"),
                                     (40000, F32, True, "fresh"), (262144, BF, False, "both")):
        cases.append(dict(n_rows=n_rows, H=8, z_dt=z_dt, ldz_pad=0, act=ACT_NONE if n_rows != 40000 else ACT_SILU, perm=perm, out_form=form))
    for c in cases:
        c["name"] = "n%d H%d %s ldz+%d %s%s %s" % (c["n_rows"], c["H"], "bf16" if c["z_dt"] == BF else "f32", c["ldz_pad"], ACT_NAMES[c["act"]],
                                                   " perm" if c["perm"] else "", c["out_form"])
    return cases


SEG_CASES = _seg_cases()


def seg_case_lengths(c):
    # 16383 and 16384 share one table: the longer one has one more empty row in front
    if c["n_rows"] == 16384:
        return [0] + seg_lengths(16383, c["H"])
    return seg_lengths(c["n_rows"], c["H"])


# ------------------------------------------------------------------------------------------------
# the other case tables
# ------------------------------------------------------------------------------------------------
GATHER_HS, GATHER_ES = (4, 36, 256, 260, 1024), (1, 5, 1021)
COLSUM_RS = (0, 1, 3, 4, 13, 16, 17, 255, 256, 257, 1000)
COLSUM_CS = (1, 3, 4, 5, 64, 65, 256, 260)
COLSUM_BIG_R = 262145                                                  # with C = 4 only: nchunk capped at 1024, empty trailing chunks
MUL_DACT_NS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)
# (dy, aux, out) dtypes of ops._dpre / _GclPre.backward: fp32 or bf16 cotangent, the saved output or stored derivative in the storage dtype,
# the result in the contraction dtype; aux None: the plain cast (act none reads dy itself)
MUL_DACT_DTYPES = ((F32, F32, F32), (F32, F32, BF), (F32, BF, BF), (BF, BF, BF), (BF, F32, F32), (F32, None, BF), (BF, BF, F32))
MDC_NCHUNKS = (1, 15, 16, 17, 48, 49, 64, 65, 113)
MDC_LAST_ROWS = (1, 3, 4, 13, 16, 17)
MDC_CS = (4, 252, 256, 260)
MDC_BIG_R = 64 * 4096 + 1
DROP_SEED = 0xFFFFFF00                                                 # seed + r * C + c wraps past 2^32 within the first rows
DROP_PS = (0.1, 0.5)
ROWDOT_NS = (4, 128, 132, 256, 260)
GCL_HS, GCL_ES = (4, 36, 256, 260, 1024), (1, 3, 4, 5, 1021)
GCL_BIG_E = 256 * 2048 + 1
SPLIT_SPLITS, SPLIT_NS = (1, 2, 7), (4, 1020, 1024, 1028)
ZER_CS, ZER_ROWS = (1, 63, 64, 65, 130), (1, 5, 70)
SCAN_NS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3000)


def mdc_rows():
    """Row counts of the mul_dact_colsum / mul_dropmask_colsum cases: every nchunk of MDC_NCHUNKS (full last chunk where one exists), every
    last-chunk size of MDC_LAST_ROWS (alone in a single chunk, and as the ragged end of a 17-chunk launch where such an R exists)."""
    rs = []
    for n in MDC_NCHUNKS:
        rs.append(64 * n)
        if n > 1:
            rs.append(64 * (n - 1) + 1)
    for last in MDC_LAST_ROWS:
        rs.append(last)
        R = rows_for(nchunk_mul_dact_colsum, 17, last)
        if R is not None:
            rs.append(R)
    return sorted(set(rs))


def rowdot_cases():
    """(M, nchunk or None = the wrapper's own): small M through ops._rowdot_bwd, the sum_chunks classes through explicit nchunk with
    three rows per chunk and a one-row last chunk."""
    return [(M, None) for M in (1, 3, 4, 13, 16, 17, 257, 1000)] + [(3 * n - 2, n) for n in MDC_NCHUNKS if n > 1]
