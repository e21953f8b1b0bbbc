"""Plain-torch restatements of the operand-level contracts of the coordinate-path kernels (ops.edge_geom, ops.coord_update,
ops.las_step, ops.inter_attn), differentiable by ordinary autograd.  Every function computes in the dtype of its floating-point
arguments: float64 is the reference of tests/test_gpu_coord_path.py, float32 gives that reference's own rounding at the same
shape (`err32`).  tests/test_coord_refs_cpu.py pins the one restatement that is new here (inter_attn) to captures of the reference."""
import torch

import fabind_oracle as orc


def rows_of(rowptr):
    """Row index of every CSR edge."""
    rp = rowptr.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])


def edge_geom(x, row, col, batch_id, B):
    """d = x[row] - x[col], rho = |d|^2, rhohat = rho / sqrt(sum over the complex of rho^2)  ->  (d, rhohat)."""
    rhohat, d = orc.coord2radial(row, col, x, batch_id, B)
    return d, rhohat


def coord_update(x, d, s_part, row, mean, clampv):
    """s[e] = sum_k s_part[e, k]; x_out[r] = x[r] + clamp((mean ? 1 / max(deg, 1) : 1) sum_e d[e] s[e], +-clampv)
    ->  (x_out, the pre-clamp update)."""
    n = x.shape[0]
    s = s_part.sum(1)
    t = orc.seg_sum(d * s[:, None], row, n)
    if mean:
        deg = torch.bincount(row, minlength=n).clamp(min=1).to(x.dtype)
        t = t / deg[:, None]
    return x + t.clamp(-clampv, clampv), t


def las_step(x, x_las, las, step, clampv):
    """oracle.las_step  ->  (x_out, the pre-clamp update step * F)."""
    i, j = las[0], las[1]
    dcur = x[i] - x[j]
    force = 2 * ((dcur ** 2).sum(1) - ((x_las[i] - x_las[j]) ** 2).sum(1))[:, None] * (2 * dcur)
    pre = orc.seg_sum(force, j, x.shape[0]) * step
    return orc.las_step(x, x_las, las, step, clampv), pre


def inter_attn(qkv, cv, h, x, d, rhohat, row, col, red_idx, bias_part, w_rk, w_rv, wcr, w3, clampv, s_ext=None, Wc=None, bc=None):
    """The inter-edge attention at the operand level of ops.inter_attn (comment block of inter_attn_fwd_kernel, csrc/attn.hip):
      logit_e = q[r] . (k[c] + rhohat_e w_rk) + sum_k bias_part[red_idx[e], k];   alpha = softmax over the row
      h_out[r] = h[r] + sum_e alpha_e (v[c] + rhohat_e w_rv)
      cp_e     = w3 . silu(cv[c] + rhohat_e wcr) + s_ext[e];   x_out[r] = x[r] + clamp(sum_e alpha_e cp_e d_e, +-clampv)
    with q | k | v the three column blocks of qkv and cv = v Wc^T + bc when (Wc, bc) is given.  Rows without edges pass through.
    ->  (h_out, x_out, alpha, logit, the pre-clamp coordinate update)."""
    n, H = h.shape
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    if cv is None:
        cv = v @ Wc.T + bc
    rh = rhohat[:, None]
    logit = (q[row] * (k[col] + rh * w_rk)).sum(1) + bias_part.sum(1)[red_idx]
    alpha = orc.seg_softmax(logit, row, n)
    h_out = h + orc.seg_sum(alpha[:, None] * (v[col] + rh * w_rv), row, n)
    z = cv[col] + rh * wcr
    cp = (z * torch.sigmoid(z) * w3).sum(1)
    if s_ext is not None:
        cp = cp + s_ext
    pre = orc.seg_sum((alpha * cp)[:, None] * d, row, n)
    return h_out, x + pre.clamp(-clampv, clampv), alpha, logit, pre


def rel_err(got, ref):
    """max|T - T64| / max(max|T64|, 1e-6)."""
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)


FLOOR = 64 * 2.0 ** -23


def bound(err32, extra=0.0):
    """What a float32 kernel may differ from the float64 reference by: 8x the rounding of the same restatement in float32 torch ops
    (another summation order: wave tree and 64-edge batches against a sequential index_add_; the fast exponential), floored where
    float32 torch happens to be exact; `extra`: a derived term of the case (the wide-logit softmax)."""
    return max(8.0 * err32, FLOOR) + extra
