"""Conformers of a ligand against each other: superposed, symmetry-corrected RMSD, greedy RMSD pruning and a superposed ensemble.

`poses.pairwise_rmsd` compares poses that share the protein frame: no centring, no rotation.  `embed.embed_conformers` centres every
conformer and leaves it in an arbitrary orientation, so that function would measure orientation, not shape.  Here
(csrc/conformer_rmsd.hip):

* `aligned_pairwise_rmsd`: D[b, s, t] = the heavy-atom RMSD of conformers s and t of ligand b after the best proper rotation and
  translation, minimised over the ligand's automorphisms -- RDKit's `GetBestRMS`, what `pruneRmsThresh` compares.
* `aligned_rmsd_to`: the same against reference conformers (the crystal ligand: the best-of-N number conformer generators are scored
  by), with the minimising automorphism and the rigid motion on request.
* `superpose`: every conformer moved onto a reference by that motion.
* `prune_conformers`: greedy RMSD pruning in ascending order of a key (e.g. the embedding's energy): `poses.cluster_from_distances`
  read as a pruning rule.

With c the centroids, G = sum_i |x_i - c|^2 and S_k = sum_i (x_s[a_k[i]] - c_s)(y_t[i] - c_t)^T,
D = sqrt(min_k max(0, G_s + G_t - 2 lambda_k) / n), lambda_k the largest eigenvalue of Horn's symmetric 4 x 4 matrix of S_k: proper
rotations only, a mirror image is a different conformer.  All of it in double on the device; D is float32, exactly symmetric with a
+0.0 diagonal, and an entry is the same bits alone, in any batch and among any S / T."""
from dataclasses import dataclass

import torch

from . import kernels as K
from .poses import MAX_POSES, PoseClusters, cluster_from_distances
from .symmetry import _atom_off

MAX_ATOMS = 2048


@dataclass
class Superposition:
    """The fit behind `aligned_rmsd_to`.  rmsd: float32 [B, S, T]; auto_index: int32 [B, S, T], the minimising automorphism (its index
    in the ligand's table, the lowest on equal values; 0 where the table is not used); quat: float64 [B, S, T, 4], the unit quaternion
    (w, x, y, z) of the rotation R; trans: float64 [B, S, T, 3] = c_t - R c_s.  R x_s[a_k[i]] + trans lies on y_t[i]; R x_s[i] + trans
    is x_s superposed on y_t with its atoms in their own order."""
    rmsd: torch.Tensor
    auto_index: torch.Tensor
    quat: torch.Tensor
    trans: torch.Tensor


@dataclass
class Pruned:
    """keep: bool [B, S], the conformers kept; order: int32 [S, B], the kept conformers of ligand b in the order they were kept
    (ascending key), -1 from row n_keep[b] on; n_keep: int32 [B]; cluster: the `poses.PoseClusters` underneath (its leaders are the
    kept conformers followed by the invalid ones that nothing absorbed)."""
    keep: torch.Tensor
    order: torch.Tensor
    n_keep: torch.Tensor
    cluster: PoseClusters


def _need_device(*tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("fabind_amd: conformer ensembles run on a HIP device only (no CPU fallback)")


def _args(coords, atom_off, autos):
    if coords.dim() != 3 or coords.shape[2] != 3:
        raise ValueError("coords must be [S, N, 3]; got %s" % (tuple(coords.shape),))
    dev = coords.device
    p = coords.detach().to(torch.float32).contiguous()
    S, N = p.shape[0], p.shape[1]
    if S > MAX_POSES:
        raise ValueError("at most %d conformers; got %d" % (MAX_POSES, S))
    aoff = _atom_off(atom_off, dev, N)
    B = aoff.numel() - 1
    if autos is None:
        flat_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        use = torch.zeros(B, dtype=torch.int32, device=dev)
        flat = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        if autos.atom_off.numel() != B + 1 or not torch.equal(autos.atom_off.to(device=dev, dtype=torch.int32), aoff):
            raise ValueError("atom_off does not match the ligands of `autos`")
        flat_off = autos.off.to(device=dev, dtype=torch.int32).contiguous()
        use = torch.where(autos.status == 0, autos.count, torch.zeros_like(autos.count)).to(device=dev, dtype=torch.int32).contiguous()
        flat = autos.flat.to(device=dev, dtype=torch.int32).contiguous() if autos.flat.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    max_atoms = int(torch.diff(aoff).max()) if B else 0
    if max_atoms > MAX_ATOMS:
        raise ValueError("at most %d atoms per ligand; got %d" % (MAX_ATOMS, max_atoms))
    return p, aoff, flat_off, use, flat, B, max_atoms


def aligned_pairwise_rmsd(coords, atom_off, autos=None):
    """Superposed RMSD of every pair of the conformers of each ligand.  coords [S, N, 3] (S stacked conformers, the layout of
    `Embedding.coords`); atom_off [B + 1].  autos: `symmetry.Automorphisms` of the batch -> the minimum over each ligand's
    automorphisms, the identity alone for a ligand whose set is not complete (status != 0), as in `poses.pairwise_rmsd`; autos=None ->
    the identity alone for every ligand.  -> D float32 [B, S, S], exactly symmetric, +0.0 on the diagonal; 0 for a ligand without atoms;
    NaN in the rows and columns of a conformer with a non-finite coordinate.  At most 512 conformers and 2048 atoms per ligand."""
    _need_device(coords)
    p, aoff, flat_off, use, flat, B, max_atoms = _args(coords, atom_off, autos)
    S = p.shape[0]
    if B == 0 or S == 0:
        return torch.zeros((B, S, S), dtype=torch.float32, device=p.device)
    return K.conformer_pair_rmsd(p, aoff, flat_off, use, flat, B, max_atoms)


def aligned_rmsd_to(coords, ref, atom_off, autos=None, return_fit=False):
    """Superposed RMSD of every conformer of coords [S, N, 3] to every reference of ref [T, N, 3] (or [N, 3]: T = 1), e.g. the crystal
    ligand: the minimum over s is the best-of-S number conformer generators are scored by.  atom_off, autos as `aligned_pairwise_rmsd`.
    -> D float32 [B, S, T], or with return_fit the `Superposition` (D with the automorphism, rotation and translation behind it)."""
    _need_device(coords, ref)
    p, aoff, flat_off, use, flat, B, max_atoms = _args(coords, atom_off, autos)
    r = ref.detach().to(device=p.device, dtype=torch.float32)
    if r.dim() == 2:
        r = r[None]
    if r.dim() != 3 or tuple(r.shape[1:]) != (p.shape[1], 3):
        raise ValueError("ref must be [%d, 3] or [T, %d, 3]; got %s" % (p.shape[1], p.shape[1], tuple(ref.shape)))
    r = r.contiguous()
    S, T = p.shape[0], r.shape[0]
    if T > MAX_POSES:
        raise ValueError("at most %d reference conformers; got %d" % (MAX_POSES, T))
    if B == 0 or S == 0 or T == 0:
        D = torch.zeros((B, S, T), dtype=torch.float32, device=p.device)
        if not return_fit:
            return D
        q = torch.zeros((B, S, T, 4), dtype=torch.float64, device=p.device)
        q[..., 0] = 1.0
        return Superposition(D, torch.zeros((B, S, T), dtype=torch.int32, device=p.device), q,
                             torch.zeros((B, S, T, 3), dtype=torch.float64, device=p.device))
    D, k, q, t = K.conformer_cross_rmsd(p, r, aoff, flat_off, use, flat, B, max_atoms, bool(return_fit))
    return Superposition(D, k, q, t) if return_fit else D


def quaternion_matrix(quat):
    """Unit quaternions (w, x, y, z) [..., 4] -> rotation matrices [..., 3, 3], the convention of csrc/conformer_fit.h."""
    w, x, y, z = quat.unbind(-1)
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (y * x + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (z * x - w * y), 2 * (z * y + w * x), w * w - x * x - y * y + z * z], dim=-1)
    return R.reshape(quat.shape[:-1] + (3, 3))


def superpose(coords, ref, atom_off, autos=None):
    """Every conformer of coords [S, N, 3] moved rigidly onto ref[0] (ref [N, 3] or [T, N, 3]) by the fit of `aligned_rmsd_to`; atoms
    keep their own order (the automorphism only decides which rotation is best).  One launch for the fit, then torch glue in float64.
    -> float32 [S, N, 3]."""
    _need_device(coords, ref)
    r0 = ref if ref.dim() == 2 else ref[:1]
    fit = aligned_rmsd_to(coords, r0, atom_off, autos, return_fit=True)
    dev = coords.device
    S, N = coords.shape[0], coords.shape[1]
    if S == 0 or N == 0:
        return torch.zeros((S, N, 3), dtype=torch.float32, device=dev)
    n_b = torch.diff(_atom_off(atom_off, dev, N)).long()
    lig = torch.repeat_interleave(torch.arange(n_b.numel(), device=dev), n_b)                # ligand of every atom
    R = quaternion_matrix(fit.quat[:, :, 0])[lig].transpose(0, 1)                            # [S, N, 3, 3]
    t = fit.trans[:, :, 0][lig].transpose(0, 1)                                              # [S, N, 3]
    x = coords.detach().to(torch.float64)
    return ((R * x[:, :, None, :]).sum(-1) + t).to(torch.float32)


def prune_conformers(D, rank_key, threshold=0.5, valid=None):
    """Greedy RMSD pruning, the rule of RDKit's `pruneRmsThresh`: go through the conformers of a ligand in ascending `rank_key` (equal
    keys in conformer order, NaN keys last) and keep a conformer iff no conformer kept before it is STRICTLY within `threshold` of it.
    D [B, S, S] (`aligned_pairwise_rmsd`); rank_key [B, S], smaller = better, e.g. `Embedding.energy`; valid: bool [B, S] or None.

    This is `poses.cluster_from_distances(D, -rank_key, threshold)`: its leaders are exactly the kept set (an absorbed conformer is
    strictly within the threshold of an earlier leader; a leader is within it of none, or an earlier leader would have absorbed it).
    A conformer with valid == False (e.g. `Embedding.status != 0`) is ranked behind every valid one and taken out of `keep` afterwards.
    It can never remove a valid conformer: a conformer absorbs others only at the moment it becomes a leader, and when the first invalid
    one is reached every valid one has been reached before it, so each is already a leader or already absorbed by a VALID leader.
    RDKit prunes in generation order; the order here is the caller's key.  The default of 0.5 A is a commonly used `pruneRmsThresh`,
    not a measured optimum.  A NaN distance removes nothing.  -> Pruned."""
    _need_device(D, rank_key)
    if D.dim() != 3 or D.shape[1] != D.shape[2] or tuple(rank_key.shape) != (D.shape[0], D.shape[1]):
        raise ValueError("D must be [B, S, S] and rank_key [B, S]; got %s and %s" % (tuple(D.shape), tuple(rank_key.shape)))
    if not float(threshold) >= 0.0:
        raise ValueError("threshold must be >= 0; got %r" % (threshold,))
    B, S = D.shape[0], D.shape[1]
    dev = D.device
    if valid is None:
        ok = torch.ones((B, S), dtype=torch.bool, device=dev)
    else:
        ok = torch.as_tensor(valid).to(device=dev, dtype=torch.bool)
        if tuple(ok.shape) != (B, S):
            raise ValueError("valid must be [%d, %d]; got %s" % (B, S, tuple(ok.shape)))
    key = rank_key.detach().to(device=dev, dtype=torch.float32)
    key = torch.where(torch.isnan(key), torch.full_like(key, float("inf")), key)             # a valid NaN key: last of the valid ones
    conf = torch.where(ok, -key, torch.full_like(key, float("nan"))).t().contiguous()        # [S, B]; NaN ranks behind everything
    pc = cluster_from_distances(D, conf, threshold)
    lead = pc.leader.long()                                                                  # [S, B], -1 padded
    lead_ok = (lead >= 0) & torch.gather(ok.t(), 0, lead.clamp(min=0))                       # valid leaders: a prefix of every column
    order = torch.where(lead_ok, pc.leader, torch.full_like(pc.leader, -1))
    keep = torch.zeros((B, S + 1), dtype=torch.bool, device=dev)
    keep.scatter_(1, torch.where(lead_ok, lead, torch.full_like(lead, S)).t(), True)         # column S collects the padding
    return Pruned(keep=keep[:, :S].contiguous(), order=order, n_keep=lead_ok.sum(0).to(torch.int32), cluster=pc)
