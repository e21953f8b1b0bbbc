"""The sampled poses of a complex against each other: pairwise symmetry-corrected RMSD and leader clustering on the GPU.

FABind+ draws S poses per complex and ranks them by the confidence head alone (`plus.metrics.select_by_confidence`); with inference
dropout most of them are one binding mode a few tenths of an angstrom apart.  Here (csrc/pose_cluster.hip, two launches for a batch):

* `pairwise_rmsd`: D[b, s, t] = min over the automorphisms a of ligand b of sqrt(mean_i |x_s[a[i]] - x_t[i]|^2), the definition of
  `symmetry.symmetric_rmsd` (no centring, no superposition: the poses of one complex share the protein frame) for every pose pair.
* `cluster_from_distances`: leader clustering -- the most confident unassigned pose leads the next cluster and takes every unassigned
  pose with D[leader, t] < threshold.
* `cluster_poses`: both.

D is exactly symmetric with a +0.0 diagonal and bit-reproducible: an entry depends on its ligand and its two poses only, not on the
batch or on S.  The clustering is integer and comparison work: exact given D.  `plus.metrics.select_distinct_by_confidence` consumes it."""
from dataclasses import dataclass

import torch

from . import kernels as K
from .symmetry import _atom_off

MAX_POSES = 512


@dataclass
class PoseClusters:
    """Leader clusters of the S poses of B complexes, int32 on the device.  cluster_id [S, B]: the cluster of every pose, 0 = the
    cluster of the most confident pose; leader [S, B]: row k holds the pose index of cluster k's leader (clusters in the confidence order
    of their leaders), -1 from row n_clusters[b] on; size [S, B]: the clusters' populations in the same layout, 0 past the end;
    n_clusters [B]."""
    cluster_id: torch.Tensor
    leader: torch.Tensor
    size: torch.Tensor
    n_clusters: torch.Tensor


def _need_device(*tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("fabind_amd: pose clustering runs on a HIP device only (no CPU fallback)")


def pairwise_rmsd(poses, compound_batch, autos=None):
    """RMSD of every pair of the poses of each complex.  poses [S, N, 3] (S stacked poses, the layout `symmetric_rmsd` takes);
    compound_batch [N]: ligand id per atom, non-decreasing.  autos: `symmetry.Automorphisms` of the batch -> the minimum over each
    ligand's automorphisms, plain RMSD for a ligand whose set is not complete (status != 0), as in `symmetric_rmsd`; compound_batch must
    agree with autos.atom_off.  autos=None -> plain RMSD for every ligand.  -> D float32 [B, S, S].
    At most 512 poses and 2048 atoms per ligand.  S = 1 and B = 0 launch nothing."""
    _need_device(poses)
    if poses.dim() != 3 or poses.shape[2] != 3:
        raise ValueError("poses must be [S, N, 3]; got %s" % (tuple(poses.shape),))
    dev = poses.device
    p = poses.detach().to(torch.float32).contiguous()
    S, N = p.shape[0], p.shape[1]
    cb = torch.as_tensor(compound_batch).to(dev).long().reshape(-1)
    if cb.numel() != N:
        raise ValueError("compound_batch has %d entries for %d atoms" % (cb.numel(), N))
    if S > MAX_POSES:
        raise ValueError("at most %d poses; got %d" % (MAX_POSES, S))
    if autos is None:
        if N and (int(cb.min()) < 0 or bool((torch.diff(cb) < 0).any())):
            raise ValueError("compound_batch must be non-negative and non-decreasing")
        B = int(cb.max()) + 1 if N else 0
        aoff = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        aoff[1:] = torch.cumsum(torch.bincount(cb, minlength=B), 0)
        flat_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        use = torch.zeros(B, dtype=torch.int32, device=dev)
        flat = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        B = autos.atom_off.numel() - 1
        aoff = _atom_off(autos.atom_off, dev, N)
        if N and (int(cb.min()) < 0 or bool((torch.diff(cb) < 0).any())) or \
                not torch.equal(torch.bincount(cb, minlength=B)[:B].to(torch.int32), torch.diff(aoff)):
            raise ValueError("compound_batch does not match the ligands of `autos`")
        flat_off = autos.off.to(device=dev, dtype=torch.int32).contiguous()
        use = torch.where(autos.status == 0, autos.count, torch.zeros_like(autos.count)).to(device=dev, dtype=torch.int32).contiguous()
        flat = autos.flat if autos.flat.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0 or S <= 1:
        return torch.zeros((B, S, S), dtype=torch.float32, device=dev)
    max_atoms = int(torch.diff(aoff).max())
    if max_atoms > 2048:
        raise ValueError("at most 2048 atoms per ligand; got %d" % max_atoms)
    return K.pose_pair_rmsd(p, aoff, flat_off, use, flat, B, max_atoms)


def cluster_from_distances(D, conf, threshold=2.0):
    """Leader clustering of each complex's poses.  D [B, S, S] (`pairwise_rmsd`); conf [S, B], larger = better.  Poses are ranked by
    descending confidence (equal values keep pose order, NaN ranks last); the best unassigned pose becomes the leader of the next
    cluster and every unassigned pose t with D[b, leader, t] < threshold joins it (strict, the project's "RMSD < 2 A"; a NaN distance
    joins nothing).  -> PoseClusters."""
    _need_device(D, conf)
    if D.dim() != 3 or D.shape[1] != D.shape[2] or tuple(conf.shape) != (D.shape[1], D.shape[0]):
        raise ValueError("D must be [B, S, S] and conf [S, B]; got %s and %s" % (tuple(D.shape), tuple(conf.shape)))
    B, S = D.shape[0], D.shape[1]
    if S > MAX_POSES:
        raise ValueError("at most %d poses; got %d" % (MAX_POSES, S))
    dev = D.device
    if B == 0 or S == 0:
        z = torch.zeros((S, B), dtype=torch.int32, device=dev)
        return PoseClusters(z, z - 1, z.clone(), torch.zeros(B, dtype=torch.int32, device=dev))
    if S == 1:                                                        # one pose: one cluster, itself
        z = torch.zeros((1, B), dtype=torch.int32, device=dev)
        one = torch.ones((1, B), dtype=torch.int32, device=dev)
        return PoseClusters(z, z.clone(), one, torch.ones(B, dtype=torch.int32, device=dev))
    d = D.detach().to(torch.float32).contiguous()
    c = conf.detach().to(device=dev, dtype=torch.float32).contiguous()
    return PoseClusters(*K.pose_cluster(d, c, threshold))


def cluster_poses(poses, conf, compound_batch, autos=None, threshold=2.0):
    """`pairwise_rmsd` then `cluster_from_distances`: two launches, no host read-back beyond the argument checks.
    -> (PoseClusters, D [B, S, S])."""
    _need_device(poses, conf)
    D = pairwise_rmsd(poses, compound_batch, autos)
    return cluster_from_distances(D, conf, threshold), D
