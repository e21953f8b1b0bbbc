"""Start conformers for inference without RDKit: the counterpart of the reference's utils/inference_mol_utils.py
(`generate_conformation`, :135-144: EmbedMolecule(ETKDGv2) + MMFFOptimizeMolecule), for a whole batch on the GPU."""
from dataclasses import dataclass

import torch

from .. import embed as _embed


def generate_conformation_batched(atomic_numbers, bond_index, bond_codes, atom_off, n_confs=1, seed=0, chiral_sign=None):
    """Distance bounds + embedding (`embed.distance_bounds`, `embed.embed_conformers`) of every ligand of a batch.

    Arguments as `embed.distance_bounds` (bond_index on the HIP device, GLOBAL atom ids).  -> (coords, status):
    n_confs == 1: coords float32 [N, 3], per ligand the first conformer (of one) -- ready to be passed as `rdkit_coords`;
    n_confs > 1: coords float32 [n_confs, N, 3], all of them, and per ligand the conformers with status 0 FIRST, in conformer order (so
    coords[0] holds, for every ligand that has one, its first conformer with status 0).
    status int32 [B, n_confs] in the order of coords (0 ok, 1 tries exhausted: the closest try is returned).  A ligand of more than
    256 atoms or with inconsistent bounds raises (`on_overflow="raise"`).  No force-field pass follows."""
    bounds = _embed.distance_bounds(bond_index, bond_codes, atomic_numbers, atom_off, chiral_sign=chiral_sign, on_overflow="raise")
    emb = _embed.embed_conformers(bounds, n_confs=n_confs, seed=seed)
    if n_confs == 1:
        return emb.coords[0], emb.status
    order = torch.argsort((emb.status != 0).to(torch.int32), dim=1, stable=True)             # [B, S]: status 0 first
    n_b = torch.diff(bounds.atom_off).long()
    lig = torch.repeat_interleave(torch.arange(n_b.numel(), device=n_b.device), n_b)          # ligand of every atom
    src = order[lig].t()                                                                      # [S, N]: conformer to read
    coords = torch.gather(emb.coords, 0, src[:, :, None].expand(-1, -1, 3))
    return coords, torch.gather(emb.status, 1, order)


@dataclass
class DiverseConformers:
    """coords: float32 [n_confs, N, 3], per ligand its kept conformers FIRST, in the order they were kept (ascending embedding energy),
    zero rows behind them; n_keep: int32 [B]; order: int32 [n_confs, B], the embedding's conformer index of every kept slot, -1 behind;
    energy, status: the embedding's float64 / int32 [B, n_confs] in generation order; D: float32 [B, n_confs, n_confs], the superposed
    symmetric RMSD of every pair in generation order; embedding: the `embed.Embedding` (all n_confs conformers, generation order);
    autos: the `symmetry.Automorphisms` the distances were minimised over."""
    coords: torch.Tensor
    n_keep: torch.Tensor
    order: torch.Tensor
    energy: torch.Tensor
    status: torch.Tensor
    D: torch.Tensor
    embedding: object
    autos: object


def generate_diverse_conformations_batched(atomic_numbers, bond_index, bond_codes, atom_off, n_confs=16, seed=0, chiral_sign=None,
                                           threshold=0.5, cap=1000):
    """`n_confs` start conformers of every ligand, pruned to those that differ in shape: the counterpart of RDKit's
    `EmbedMultipleConfs(mol, n_confs, pruneRmsThresh=threshold)`.

    `embed.distance_bounds` -> `embed.embed_conformers(n_confs)` -> `symmetry.ligand_automorphisms` (on the heavy-atom graph, labels of
    `reference_atom_labels`; a ligand with more than `cap` automorphisms is compared by the identity alone) ->
    `ensemble.aligned_pairwise_rmsd` -> `ensemble.prune_conformers` in ascending embedding energy with valid = (status == 0).
    Arguments as `generate_conformation_batched`.  RDKit prunes in generation order, this prunes in energy order; 0.5 A is a commonly
    used `pruneRmsThresh`, not a measured optimum.  A ligand none of whose conformers has status 0 keeps none.
    -> DiverseConformers."""
    from .. import ensemble as _ens
    from .. import symmetry as _sym
    bounds = _embed.distance_bounds(bond_index, bond_codes, atomic_numbers, atom_off, chiral_sign=chiral_sign, on_overflow="raise")
    emb = _embed.embed_conformers(bounds, n_confs=n_confs, seed=seed)
    dev = emb.coords.device
    N = emb.coords.shape[1]
    bi = bond_index.to(torch.int64).reshape(2, -1)
    if not torch.is_tensor(bond_codes) and len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [_sym.bond_code(t) for t in bond_codes]
    codes = torch.as_tensor(bond_codes).to(device=dev, dtype=torch.int64).reshape(-1)
    lo, hi = torch.minimum(bi[0], bi[1]), torch.maximum(bi[0], bi[1])
    pair, inv = torch.unique(lo * max(N, 1) + hi, return_inverse=True)                        # each bond once, whatever the input repeats
    code1 = torch.zeros_like(pair).scatter_reduce(0, inv, codes, "amin", include_self=False)
    once = torch.stack([pair // max(N, 1), pair % max(N, 1)])
    z = torch.as_tensor(atomic_numbers).to(device=dev)
    labels = _sym.reference_atom_labels(z, once, code1)
    autos = _sym.ligand_automorphisms(labels, once, bounds.atom_off, cap=cap, on_overflow="truncate")
    D = _ens.aligned_pairwise_rmsd(emb.coords, bounds.atom_off, autos)
    pr = _ens.prune_conformers(D, emb.energy, threshold=threshold, valid=emb.status == 0)
    n_b = torch.diff(bounds.atom_off).long()
    lig = torch.repeat_interleave(torch.arange(n_b.numel(), device=dev), n_b)                 # ligand of every atom
    src = pr.order.long()[:, lig]                                                             # [S, N]: conformer to read, -1: none
    coords = torch.gather(emb.coords, 0, src.clamp(min=0)[:, :, None].expand(-1, -1, 3))
    coords = torch.where((src >= 0)[:, :, None], coords, torch.zeros_like(coords))
    return DiverseConformers(coords=coords, n_keep=pr.n_keep, order=pr.order, energy=emb.energy, status=emb.status, D=D,
                             embedding=emb, autos=autos)
