"""Start conformers for inference without RDKit: the counterpart of the reference's utils/inference_mol_utils.py
(`generate_conformation`, :135-144: EmbedMolecule(ETKDGv2) + MMFFOptimizeMolecule), for a whole batch on the GPU."""
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
