"""Plain-torch restatements of the operand-level contracts of the normalisation kernels (csrc/norm.hip: row LayerNorm, row_stats,
edge_ln_concat / edge_concat, the LayerNorm-folded first edge Linear and its adjoint, inter_coord_fold), read from the comment blocks
of that file.  Every function computes in the dtype of its floating-point arguments: float64 is the reference of
tests/test_gpu_norm_forms.py, float32 gives that reference's own rounding at the same shape (`err32`); bf16 operands enter with their
exact values (`cast`).  tests/test_norm_refs_cpu.py pins the folded restatements to the unfolded LayerNorm -> Linear forms and the
adjoint to autograd."""
import torch


def cast(dtype, *ts):
    """Every floating-point tensor as `dtype` on the host (exact for bf16 / fp32 -> float32 / float64); the others unchanged."""
    out = tuple(t.detach().cpu().to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t for t in ts)
    return out if len(out) != 1 else out[0]


def _pad(y, pad_to):
    if pad_to is None or pad_to == y.shape[1]:
        return y
    return torch.cat([y, y.new_zeros(y.shape[0], pad_to - y.shape[1])], 1)


# ------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------
def row_stats(x, eps):
    """(mean, rsqrt(centred variance + eps)) of every row."""
    mu = x.mean(1)
    t = x - mu[:, None]
    return mu, torch.rsqrt((t * t).mean(1) + eps)


def layer_norm_rows(x, w, b, eps, pad_to=None):
    """(x - mean) rsqrt(var + eps) w + b per row, columns [C, pad_to) zero.  Gradients: ordinary autograd."""
    mu, rs = row_stats(x, eps)
    return _pad((x - mu[:, None]) * rs[:, None] * w + b, pad_to)


def edge_concat(h, row, col, rhohat, pad_to=None):
    """[h[row] | h[col] | rhohat | 0 ...]."""
    return _pad(torch.cat([h[row.long()], h[col.long()], rhohat[:, None]], 1), pad_to)


def edge_ln_concat(h, row, col, rhohat, w, b, eps, pad_to=None):
    """LayerNorm over the 2H + 1 columns of [h[row] | h[col] | rhohat], columns [2H + 1, pad_to) zero."""
    return _pad(layer_norm_rows(edge_concat(h, row, col, rhohat), w, b, eps), pad_to)


# ------------------------------------------------------------------------------------------------
# the counter-based dropout mask of the GEMM epilogue and the fold kernels
# ------------------------------------------------------------------------------------------------
def hash32(x):
    """fb_hash32 (csrc/common.h) on int64 tensors holding 32-bit values: xor-shift / multiply mixing with 32-bit wrap-around."""
    x = x & 0xFFFFFFFF
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & 0xFFFFFFFF
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def drop_thr(p):
    """round(p * 65536) as the launchers take it: (uint32)(p * 65536.0f + 0.5f) in fp32."""
    return int(torch.tensor(float(p), dtype=torch.float32) * 65536.0 + 0.5)


def drop_keep(seed, n_rows, width, p):
    """keep[e, c] = fb_hash32(seed + e * width + c) & 0xffff >= round(p * 65536)  (bool [n_rows, width]); all True at p = 0."""
    e = torch.arange(n_rows, dtype=torch.int64)[:, None]
    c = torch.arange(width, dtype=torch.int64)[None, :]
    return (hash32(int(seed) + e * width + c) & 0xFFFF) >= drop_thr(p)


def _keep_scale(v, keep, p_drop):
    if keep is None:
        return v
    return v * keep.to(v.dtype) / (1.0 - drop_thr(p_drop) / 65536.0)


# ------------------------------------------------------------------------------------------------
# LayerNorm-folded first edge Linear (edge_lnfold) and its adjoint
# ------------------------------------------------------------------------------------------------
def _lnfold_edge_terms(AB, Kp, H, row, col, rho, stat, eps, w_r, c_r, c_c):
    r, c = row.long(), col.long()
    m_r, q_r, m_c, q_c = stat[r, 0], stat[r, 1], stat[c, 0], stat[c, 1]
    Cn = 2 * H + 1
    mu = (H * (m_r + m_c) + rho) / Cn
    dr, dc, dq = m_r - mu, m_c - mu, rho - mu
    rs = torch.rsqrt((q_r + q_c + H * (dr * dr + dc * dc) + dq * dq) / Cn + eps)
    u = AB[r, :Kp] + AB[c, Kp:2 * Kp] + dr[:, None] * c_r + dc[:, None] * c_c + dq[:, None] * w_r
    return dr, dc, dq, rs, u


def edge_lnfold(AB, Kp, H, row, col, rho, stat, eps, w_r, c_r, c_c, dvec, keep=None, p_drop=0.0):
    """out[e] = relu(rs_e u_e + dvec) keep / (1 - thr / 65536),  u_e = A[row] + B[col] + dr c_r + dc c_c + dq w_r  with
    [A | B] = AB[:, :Kp] | AB[:, Kp:2Kp], stat[n] = (m, Q) = (mean, centred sum of squares) of node n's H features,
    mu = (H (m_r + m_c) + rho) / Cn, (dr, dc, dq) = (m_r, m_c, rho) - mu, rs = rsqrt((Q_r + Q_c + H (dr^2 + dc^2) + dq^2) / Cn + eps),
    Cn = 2H + 1.  keep: bool [E, Kp] (drop_keep) or None.  -> [E, Kp], not rounded."""
    _, _, _, rs, u = _lnfold_edge_terms(AB, Kp, H, row, col, rho, stat, eps, w_r, c_r, c_c)
    return _keep_scale(torch.relu(rs[:, None] * u + dvec), keep, p_drop)


def edge_lnfold_bwd(AB, Kp, H, row, col, rho, stat, eps, w_r, c_r, c_c, out, dout, p_drop=0.0):
    """Adjoint of edge_lnfold with the mask taken from the saved output, g = dout [out != 0] / (1 - thr / 65536):
      du = rs g;  per edge  d rs = sum_k g u,  d dr = sum_k du c_r,  d dc = sum_k du c_c,  d dq = sum_k du w_r  folded through rs and mu;
      per column  d dvec = sum_e g,  d c_r = sum_e du dr,  d c_c = sum_e du dc,  d w_r = sum_e du dq.
    -> (du [E, Kp] not rounded, es [E, 4] = (d m_r, d Q_r, d m_c, d Q_c), drho [E], vecs [4, Kp] = (d dvec, d c_r, d c_c, d w_r))."""
    dr, dc, dq, rs, u = _lnfold_edge_terms(AB, Kp, H, row, col, rho, stat, eps, w_r, c_r, c_c)
    Cn = 2 * H + 1
    g = dout * (out != 0).to(dout.dtype) / (1.0 - drop_thr(p_drop) / 65536.0)
    du = rs[:, None] * g
    s_gu, s_cr, s_cc, s_wr = (g * u).sum(1), (du * c_r).sum(1), (du * c_c).sum(1), (du * w_r).sum(1)
    dV = -0.5 * rs * rs * rs * s_gu                           # rs = (V + eps)^(-1/2)
    dQ = dV / Cn
    ddr, ddc, ddq = s_cr + dV * 2 * H * dr / Cn, s_cc + dV * 2 * H * dc / Cn, s_wr + dV * 2 * dq / Cn
    dmu = -(ddr + ddc + ddq)
    es = torch.stack([ddr + dmu * H / Cn, dQ, ddc + dmu * H / Cn, dQ], 1)
    drho = ddq + dmu / Cn
    vecs = torch.stack([g.sum(0), (du * dr[:, None]).sum(0), (du * dc[:, None]).sum(0), (du * dq[:, None]).sum(0)])
    return du, es, drho, vecs


def edge_mlp_unfolded(h, row, col, rho, ln_w, ln_b, W1, b1, eps):
    """relu(W1 LN([h_r | h_c | rho]) + b1)  -> [E, 2H + 1]."""
    return torch.relu(edge_ln_concat(h, row, col, rho, ln_w, ln_b, eps) @ W1.T + b1)


def fold_edge(h, ln_w, ln_b, W1, b1, Kp):
    """Host-side composition of edge_lnfold's operands from the module's parameters and the node features:
    W1w = W1 diag(ln_w) zero-padded to Kp rows, [A | B] = (h - m 1^T) [W1w_r | W1w_c]^T, stat = (m, |h - m|^2), c_r / c_c = row sums of
    the two weight blocks, w_r = W1w[:, 2H], dvec = W1 ln_b + b1.  -> dict(AB [N, 2 Kp] (not rounded), stat, w_r, c_r, c_c, dvec)."""
    H, Cn = h.shape[1], 2 * h.shape[1] + 1
    W1w = h.new_zeros(Kp, Cn)
    W1w[:W1.shape[0]] = W1 * ln_w[None, :]
    m = h.mean(1)
    hcen = h - m[:, None]
    dvec = h.new_zeros(Kp)
    dvec[:W1.shape[0]] = W1 @ ln_b + b1
    return dict(AB=hcen @ torch.cat([W1w[:, :H], W1w[:, H:2 * H]]).T, stat=torch.stack([m, (hcen * hcen).sum(1)], 1).contiguous(),
                w_r=W1w[:, 2 * H].contiguous(), c_r=W1w[:, :H].sum(1), c_c=W1w[:, H:2 * H].sum(1), dvec=dvec)


# ------------------------------------------------------------------------------------------------
# coord_mlp of the inter-edge attention with the LayerNorm folded (inter_coord_fold)
# ------------------------------------------------------------------------------------------------
def inter_coord_fold(P, H, col, rho, stat, q_w, eps, u, d, w3, keep=None, p_drop=0.0):
    """s[e] = sum_k w3[k] relu(rs_e (P[col[e], k] + rho[e] u[k]) + d[k]) keep / (1 - thr / 65536),
    rs_e = rsqrt(max(stat[col][0] + 2 rho stat[col][1] + rho^2 q_w, 0) / H + eps)."""
    c = col.long()
    rs = torch.rsqrt((stat[c, 0] + 2 * rho * stat[c, 1] + rho * rho * q_w).clamp(min=0) / H + eps)
    v = torch.relu(rs[:, None] * (P[c, :H] + rho[:, None] * u) + d)
    return (_keep_scale(v, keep, p_drop) * w3).sum(1)


def inter_coord_unfolded(V, col, rho, w_rv, ln_w, ln_b, W1, b1, w3, eps):
    """w3 . relu(W1 LN(V[col] + rho w_rv) + b1)  -> [E]."""
    v_e = V[col.long()] + rho[:, None] * w_rv
    return torch.relu(layer_norm_rows(v_e, ln_w, ln_b, eps) @ W1.T + b1) @ w3


def fold_inter(V, w_rv, ln_w, ln_b, W1, b1):
    """Host-side composition of inter_coord_fold's operands: P = (V - mean 1^T)(W1 diag(ln_w))^T, stat = (|Vc|^2, Vc . wc),
    wc = w_rv - mean(w_rv), q_w = |wc|^2, u = W1 diag(ln_w) wc, d = W1 ln_b + b1.  -> dict(P (not rounded), stat, q_w, u, d)."""
    W1w = W1 * ln_w[None, :]
    Vc, wc = V - V.mean(1, keepdim=True), w_rv - w_rv.mean()
    return dict(P=Vc @ W1w.T, stat=torch.stack([(Vc * Vc).sum(1), Vc @ wc], 1).contiguous(), q_w=float((wc * wc).sum()), u=W1w @ wc,
                d=W1 @ ln_b + b1)


# ------------------------------------------------------------------------------------------------
# comparison of a tensor the kernel rounds to bf16
# ------------------------------------------------------------------------------------------------
def bf16_half_ulp(x):
    """Half an ulp of bf16 (8 significand bits, round-to-nearest-even) at magnitude x: 2^(floor(log2 x) - 8), between 2^-9 x (just below
    a power of two) and 2^-8 x (at one); the normal range's smallest exponent below 2^-126."""
    _, e = torch.frexp(x.double().abs().clamp(min=2.0 ** -126))          # x = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 9)


def bf16_excess(got, ref64, A):
    """max over the elements of |got - ref64| - (half_ulp(|ref64| + A) + A): <= 0 when every element is the round-to-nearest bf16 of a
    value v within A of the reference (|bf16(v) - r| <= half_ulp(v) + |v - r|, |v| <= |r| + A).  The half-ulp is the element's own, not
    its envelope 2^-8 |r|: a result one bf16 step away from the nearest is refused wherever |v - r| is small against the step."""
    ref64 = ref64.double()
    if ref64.numel() == 0:
        return 0.0
    return float(((got.double() - ref64).abs() - (bf16_half_ulp(ref64.abs() + A) + A)).max())


def bf16_excess_literal(got, ref64, A):
    """The same against 2^-9 |ref64| + (1 + 2^-9) A, the lower envelope of the half-ulp taken as if it were the half-ulp: a correctly
    rounded result exceeds it wherever the significand of the reference is below 1.5 or so (tests/test_norm_refs_cpu.py shows it on
    exact inputs); printed by the GPU tests for the record, not asserted."""
    ref64 = ref64.double()
    if ref64.numel() == 0:
        return 0.0
    return float(((got.double() - ref64).abs() - (2.0 ** -9 * ref64.abs() + (1.0 + 2.0 ** -9) * A)).max())
