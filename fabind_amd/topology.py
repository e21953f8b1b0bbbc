"""Ligand LAS ("local atomic structure") constraint pairs on the GPU, from the bare bond list.

The reference derives them per molecule on the host with RDKit (utils/generation_utils.py:170-187 `get_LAS_distance_constraint_mask`,
identical copies in utils/inference_mol_utils.py and utils/feature_utils.py): a pair of atoms is constrained iff the atoms are bonded,
two bonds apart (`n_hops_adj(adj, 2)`), or members of one ring of `Chem.GetSymmSSSR(mol)`; `dense_to_sparse` of that mask is the
sample field `LAS_edge_index` every coordinate-moving step reads.  Here a whole batch runs in csrc/topology.hip, one work-group per
ligand: all-pairs hop distances, a spanning forest, and the RELEVANT cycles (those whose edge set is no GF(2) sum of strictly shorter
cycles -- the union of all minimum cycle bases) found root by root, length by length, with 64-bit cycle-space vectors.

On fused, spiro and bridged ring systems the relevant cycles are the rings RDKit's symmetrised SSSR lists (norbornane's two 5-rings,
all three 6-rings of bicyclo[2.2.2]octane, all six faces of cubane).  RDKit's own heuristics, which depend on the atom order in some
cages, are not reproduced, and agreement with `GetSymmSSSR` itself is not measured."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .symmetry import _atom_off

MAX_ATOMS = 256
MAX_CHORDS = 64
STATUS = {0: "ok", 3: "more than 256 atoms", 4: "more than 64 non-tree bonds"}


@dataclass
class LASPairs:
    """LAS pairs of a batch of ligands, all on the device.  edge_index: int64 [2, El], GLOBAL atom ids, ligand by ligand and
    row-major inside a ligand (i ascending, then j: the order of `dense_to_sparse`); off: int32 [B + 1], ligand b's pairs at
    [off[b], off[b + 1]); ring_pairs: int32 [B], unordered pairs on a common relevant cycle; status: int32 [B] (0 ok, 3 more than 256
    atoms, 4 more than 64 non-tree bonds: bonded and two-bond pairs only); atom_off: int32 [B + 1]."""
    edge_index: torch.Tensor
    off: torch.Tensor
    ring_pairs: torch.Tensor
    status: torch.Tensor
    atom_off: torch.Tensor


def _neighbour_lists(bond_index, n_atoms):
    """Symmetrised, de-duplicated neighbour lists sorted by (owner, neighbour), self-loops dropped (the code-less sibling of
    `conformer._coded_neighbour_lists`).  -> ptr int32 [N + 1], idx int32 [2 * bonds]."""
    dev = bond_index.device
    lo, hi = torch.minimum(bond_index[0], bond_index[1]), torch.maximum(bond_index[0], bond_index[1])
    keep = lo != hi
    key = torch.unique(lo[keep] * n_atoms + hi[keep])
    lo, hi = torch.div(key, n_atoms, rounding_mode="floor"), key % n_atoms
    owner, other = torch.cat([lo, hi]), torch.cat([hi, lo])
    order = torch.argsort(owner * n_atoms + other)
    ptr_ = torch.zeros(n_atoms + 1, dtype=torch.int32, device=dev)
    ptr_[1:] = torch.cumsum(torch.bincount(owner, minlength=n_atoms), 0).to(torch.int32)
    return ptr_, other[order].to(torch.int32).contiguous()


def _pairs(bi, aoff, N, on_overflow, what):
    """bi: int64 [2, E] on the device, ids in [0, N); aoff: int32 [B + 1] on the device, checked.  Two launches, one read-back."""
    dev = bi.device
    B = aoff.numel() - 1
    nptr, nidx = _neighbour_lists(bi, max(N, 1))
    if B and bi.numel():
        lig = torch.bucketize(bi, aoff[1:].to(torch.int64), right=True)
        cross = (lig[0] != lig[1]).any().to(torch.int64).reshape(1)
    else:
        cross = torch.zeros(1, dtype=torch.int64, device=dev)
    row_count = torch.zeros(N, dtype=torch.int32, device=dev)
    mask_rows = torch.zeros(max(N, 1), 8, dtype=torch.int32, device=dev)
    ring_pairs = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    K.las_pairs(nptr, nidx, aoff, B, row_count, mask_rows, ring_pairs, status)
    row_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    row_off[1:] = torch.cumsum(row_count, 0)
    host = torch.cat([row_off[-1:], cross, status.to(torch.int64)]).cpu().numpy()     # the one read-back: total, bond check, statuses
    if host[1]:
        raise ValueError("%s: a bond joins atoms of two different ligands" % what)
    bad = np.nonzero(host[2:])[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("%s: " % what + "; ".join("ligand %d: status %d (%s)" % (b, host[2 + b], STATUS[int(host[2 + b])])
                                                       for b in bad))
    El = int(host[0])
    if El >= 2 ** 31:
        raise RuntimeError("%s: %d pairs exceed the int32 offsets; split the batch" % (what, El))
    row_off = row_off.to(torch.int32)
    edge_index = torch.empty(2, El, dtype=torch.int64, device=dev)
    if El:
        K.las_pairs(nptr, nidx, aoff, B, row_count, mask_rows, ring_pairs, status, row_off, El, edge_index)
    return LASPairs(edge_index=edge_index, off=row_off[aoff.to(torch.int64)].contiguous(), ring_pairs=ring_pairs, status=status,
                    atom_off=aoff)


def las_pairs(bond_index, atom_off, on_overflow="raise"):
    """The LAS pairs of every ligand of a batch (csrc/topology.hip).

    bond_index: [2, E] GLOBAL atom ids on the HIP device, each bond once, in both directions or repeated, self-loops allowed -- the
    result is the same; bonds never cross ligands (ValueError).  atom_off: [B + 1] atom offsets of the ligands.  A ligand may be
    disconnected or empty.
    on_overflow: "raise" -> RuntimeError naming every ligand of more than 256 atoms (status 3) or more than 64 non-tree bonds
    (status 4); "truncate" -> such a ligand gets the bonded and two-bond pairs only and reports its status.
    -> LASPairs; `edge_index` is what `post_optimize_compound_coords_batched(..., LAS_edge_index=)` and
    `distance_optimize_compound_coords_batched(..., LAS_edge_index=)` take.  Two launches (count, then write): one host read-back
    sizes the output.  A ligand's pairs are the same alone and in any batch."""
    if on_overflow not in ("raise", "truncate"):
        raise ValueError("on_overflow must be 'raise' or 'truncate'")
    if not torch.is_tensor(bond_index) or not bond_index.is_cuda:
        raise RuntimeError("fabind_amd: las_pairs runs on a HIP device only (no CPU fallback)")
    dev = bond_index.device
    bi = bond_index.to(torch.int64).reshape(2, -1).contiguous()
    ao = torch.as_tensor(atom_off)
    N = int(ao[-1]) if ao.dim() == 1 and ao.numel() else -1
    aoff = _atom_off(atom_off, dev, N)
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= N):
        raise ValueError("bond_index holds atom ids outside [0, %d)" % N)
    return _pairs(bi, aoff, N, on_overflow, "las_pairs")


def las_mask(bond_index, n_atoms, on_overflow="raise"):
    """The dense int64 [n, n] mask of ONE ligand -- the return value of the reference's `get_LAS_distance_constraint_mask(mol)` -- from
    bond_index [2, E] (local atom ids, on the HIP device)."""
    n = int(n_atoms)
    p = las_pairs(bond_index, [0, n], on_overflow)
    mask = torch.zeros(n, n, dtype=torch.int64, device=p.edge_index.device)
    mask[p.edge_index[0], p.edge_index[1]] = 1
    return mask
