"""Ligand post-optimisation on the GPU (reference FABind/fabind/utils/post_optim_utils.py:9-64, driven per complex by
fabind_inference.py:285-328).

`post_optimize_compound_coords` keeps the reference's name, arguments and return triple for ONE ligand;
`post_optimize_compound_coords_batched` runs a whole batch of ligands in one kernel launch (csrc/post_optim.hip: one
work-group per ligand, all Adam iterations inside the kernel).  HIP device tensors only -- there is no CPU fallback.
`torsion_fit_compound_coords_batched` has no counterpart in the reference: it moves only what a molecule can move;
`relax_compound_coords_batched` then moves it out of contact with the protein.

Numerics: the objective is non-smooth (|.| and relu) and Adam moves each coordinate by ~lr = 0.1 A per step, so the
iteration is chaotic: the reference's own result changes by ~0.1 A between its two `torch.cdist` code paths (direct
for <= 25 atoms, matmul-based above).  The kernel matches the reference step for step to float rounding (tests pin a short
horizon at 1e-5 A on the direct-cdist path) and reaches the same loss / RMSD level after the full 1000 steps."""
import torch

from .. import _lib
from .._lib import check, ptr, stream


def compute_RMSD(a, b):
    return torch.sqrt((((a - b) ** 2).sum(axis=-1)).mean())


def _neighbour_lists(LAS_edge_index, n_atoms, device):
    """CSR over atoms of the symmetrised, de-duplicated directed edge set: for every distinct (i, j) the list of i holds j
    and the list of j holds i (the dense boolean mask of the reference ignores duplicate edges)."""
    e = torch.unique(LAS_edge_index.to(device=device, dtype=torch.int64), dim=1)
    owner = torch.cat([e[0], e[1]])
    other = torch.cat([e[1], e[0]])
    order = torch.argsort(owner, stable=True)
    ptr_ = torch.zeros(n_atoms + 1, dtype=torch.int32, device=device)
    ptr_[1:] = torch.cumsum(torch.bincount(owner, minlength=n_atoms), 0).to(torch.int32)
    return ptr_, other[order].to(torch.int32).contiguous()


def post_optimize_compound_coords_batched(reference_compound_coords, predict_compound_coords, compound_batch,
                                          total_epoch=1000, LAS_edge_index=None, lr=0.1):
    """All ligands of a batch at once.  reference / predict: [sum Nc, 3]; compound_batch: sorted ligand id per atom;
    LAS_edge_index: [2, E] GLOBAL atom ids (edges never cross ligands) or None.
    -> (x [sum Nc, 3], loss [L] at the last epoch, rmsd [L] to the reference conformer after the last step)."""
    if not predict_compound_coords.is_cuda:
        raise RuntimeError("fabind_amd: post-optimisation runs on a HIP device only (no CPU fallback); got %s"
                           % predict_compound_coords.device)
    dev = predict_compound_coords.device
    x0 = predict_compound_coords.detach().to(torch.float32).contiguous()
    ref = reference_compound_coords.detach().to(device=dev, dtype=torch.float32).contiguous()
    n_atoms = x0.shape[0]
    cnt = torch.bincount(compound_batch.to(dev))
    L = cnt.shape[0]
    off = torch.zeros(L + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    max_atoms = int(cnt.max().item())
    if LAS_edge_index is not None:
        nptr, nidx = _neighbour_lists(LAS_edge_index, n_atoms, dev)
    else:
        nptr = nidx = None
    x = torch.empty_like(x0)
    loss = torch.empty(L, dtype=torch.float32, device=dev)
    rmsd = torch.empty(L, dtype=torch.float32, device=dev)
    check(_lib.load().fabind_post_optimize(ptr(x0), ptr(ref), ptr(off), ptr(nptr), ptr(nidx), L, max_atoms,
                                           0 if LAS_edge_index is not None else 1, int(total_epoch), float(lr), ptr(x),
                                           ptr(loss), ptr(rmsd), stream()), "fabind_post_optimize")
    return x, loss, rmsd


def torsion_fit_compound_coords_batched(reference_compound_coords, predict_compound_coords, compound_batch, plan, max_iters=50, tol=1e-6,
                                        on_overflow="truncate", return_fit=False):
    """The torsion-space counterpart of `post_optimize_compound_coords_batched`: instead of pulling the predicted cloud towards the
    start conformer's LAS distances, the start conformer itself is fitted to the prediction over its rotatable-bond dihedrals and
    one rigid motion (`conformer.fit_conformers`, csrc/conformer_fit.hip), so bond lengths, angles and rings are exactly the start
    conformer's.  reference / predict: [sum Nc, 3] ([S, sum Nc, 3] for S sampled poses); compound_batch: sorted ligand id per atom;
    plan: the `conformer.rotatable_bonds` TorsionPlan of the same ligands.  A ligand beyond the kernel's limits (256 atoms, 58
    torsions) is fitted rigidly (`on_overflow`).
    -> (x like predict, rmsd_to_prediction [L] ([S, L]), rmsd_rigid [L] ([S, L]): the same after the rigid fit alone); with return_fit
    the `conformer.ConformerFit` itself (its angles start `relax_compound_coords_batched`)."""
    from .. import conformer
    if not predict_compound_coords.is_cuda:
        raise RuntimeError("fabind_amd: the torsion-space fit runs on a HIP device only (no CPU fallback); got %s"
                           % predict_compound_coords.device)
    dev = predict_compound_coords.device
    ref = reference_compound_coords.detach().to(device=dev)
    cb = torch.as_tensor(compound_batch).to(dev)
    if cb.dim() != 1 or cb.numel() != ref.shape[0]:
        raise ValueError("compound_batch must be [%d]; got %s" % (ref.shape[0], tuple(cb.shape)))
    if plan is None:
        raise ValueError("torsion_fit_compound_coords_batched needs the TorsionPlan of the ligands (conformer.rotatable_bonds)")
    L = int(plan.atom_off.numel()) - 1
    cb = cb.long()
    if cb.numel() and (int(cb.min()) < 0 or int(cb.max()) >= L or bool((cb[1:] < cb[:-1]).any())
                       or not torch.equal(torch.bincount(cb, minlength=L).cumsum(0), plan.atom_off[1:].to(dev).long())):
        raise ValueError("compound_batch is not sorted or does not match the ligands of `plan`")
    fit = conformer.fit_conformers(ref, predict_compound_coords, plan, max_iters=max_iters, tol=tol, on_overflow=on_overflow)
    if return_fit:
        return fit
    if predict_compound_coords.dim() == 2:
        return fit.coords[0], fit.rmsd[0], fit.rmsd0[0]
    return fit.coords, fit.rmsd, fit.rmsd0


def relax_compound_coords_batched(reference_compound_coords, predict_compound_coords, compound_batch, plan, validity_plan, grid,
                                  fit_iters=50, max_iters=100, tol=1e-6, on_overflow="truncate", **weights):
    """`torsion_fit_compound_coords_batched` followed by the relaxation out of protein and internal clashes (`relax.relax_poses`,
    csrc/pose_relax.hip): the start conformer is fitted to the prediction in torsion space, then moved over the same torsions and one
    rigid motion, held to the prediction and pushed out of contact with all heavy atoms of the protein and with itself.  reference /
    predict: [sum Nc, 3] ([S, sum Nc, 3] for S sampled poses), predict in the frame of the grid; compound_batch: sorted ligand id per
    atom; plan: the `conformer.rotatable_bonds` TorsionPlan, validity_plan: the `validity.validity_plan` ValidityPlan, grid: the
    `validity.protein_grid` ProteinGrid of the same complexes; weights: w_fit, w_prot, w_intra, c_prot, c_intra as `relax_poses` takes
    them.  A ligand beyond the kernels' limits is fitted rigidly and left there (256 atoms) or relaxed rigidly (58 torsions).
    -> (x like predict, energy float64 [L, 3] ([S, L, 3]): the unweighted fit / protein / intra sums at the end, energy0: the same
    at the fitted pose)."""
    from .. import relax
    if validity_plan is None or grid is None:
        raise ValueError("relax_compound_coords_batched needs the ValidityPlan of the ligands and the ProteinGrid of their proteins")
    fit = torsion_fit_compound_coords_batched(reference_compound_coords, predict_compound_coords, compound_batch, plan, max_iters=fit_iters,
                                              tol=tol, on_overflow=on_overflow, return_fit=True)
    res = relax.relax_poses(reference_compound_coords.detach().to(predict_compound_coords.device), predict_compound_coords, plan, validity_plan,
                            grid, angles0=fit.angles, max_iters=max_iters, tol=tol, on_overflow=on_overflow, **weights)
    if predict_compound_coords.dim() == 2:
        return res.coords[0], res.energy[0], res.energy0[0]
    return res.coords, res.energy, res.energy0


def check_compound_coords_batched(predict_compound_coords, compound_batch, plan, pocket_coords=None, pocket_batch=None, **thresholds):
    """The physical-validity check of predicted (or post-optimised, or torsion-fitted) ligand coordinates for the inference scripts:
    `validity.check_poses` (csrc/pose_check.hip) behind the conventions of this module.  predict: [sum Nc, 3] ([S, sum Nc, 3] for S
    sampled poses); compound_batch: sorted ligand id per atom; plan: the `validity.validity_plan` ValidityPlan of the same ligands;
    pocket_coords [R, 3] / pocket_batch [R]: the C-alpha atoms of every complex, or None; thresholds: bond_tol, angle_tol, clash_min,
    flat_max, ca_min as `check_poses` takes them.
    -> (valid bool [L] ([S, L]), flags int32 [L] ([S, L]), stats float32 [L, 9] ([S, L, 9]))."""
    from .. import validity
    if not predict_compound_coords.is_cuda:
        raise RuntimeError("fabind_amd: the validity check runs on a HIP device only (no CPU fallback); got %s"
                           % predict_compound_coords.device)
    if plan is None:
        raise ValueError("check_compound_coords_batched needs the ValidityPlan of the ligands (validity.validity_plan)")
    dev = predict_compound_coords.device
    L = int(plan.atom_off.numel()) - 1
    cb = torch.as_tensor(compound_batch).to(dev).long()
    if cb.dim() != 1 or cb.numel() != predict_compound_coords.shape[-2]:
        raise ValueError("compound_batch must be [%d]; got %s" % (predict_compound_coords.shape[-2], tuple(cb.shape)))
    if cb.numel() and (int(cb.min()) < 0 or int(cb.max()) >= L or bool((cb[1:] < cb[:-1]).any())
                       or not torch.equal(torch.bincount(cb, minlength=L).cumsum(0), plan.atom_off[1:].to(dev).long())):
        raise ValueError("compound_batch is not sorted or does not match the ligands of `plan`")
    res = validity.check_poses(predict_compound_coords, plan, pocket_coords, pocket_batch, **thresholds)
    if predict_compound_coords.dim() == 2:
        return res.valid[:, 0], res.flags[:, 0], res.stats[:, 0]
    return res.valid.t(), res.flags.t(), res.stats.transpose(0, 1)


def check_protein_contacts_batched(predict_compound_coords, compound_batch, plan, grid, **thresholds):
    """Predicted (or post-optimised, or torsion-fitted) ligand coordinates against ALL heavy atoms of their proteins for the inference
    scripts: `validity.check_poses_protein` (csrc/protein_contacts.hip) behind the conventions of this module.  predict: [sum Nc, 3]
    ([S, sum Nc, 3] for S sampled poses); compound_batch: sorted ligand id per atom; plan: the `validity.validity_plan` ValidityPlan of
    the ligands; grid: the `validity.protein_grid` ProteinGrid of the same complexes (`validity.protein_atoms_from_pdb` reads its atoms);
    thresholds: cutoff, clash_min, overlap_max, vdw_scale, spacing as `check_poses_protein` takes them.
    -> (ok bool [L] ([S, L]), flags int32 [L] ([S, L]), stats float32 [L, 3] ([S, L, 3])); `ok & valid` with the `valid` of
    `check_compound_coords_batched` is the "physically valid" of the docking benchmarks."""
    from .. import validity
    if not predict_compound_coords.is_cuda:
        raise RuntimeError("fabind_amd: the protein-contact check runs on a HIP device only (no CPU fallback); got %s"
                           % predict_compound_coords.device)
    if plan is None or grid is None:
        raise ValueError("check_protein_contacts_batched needs the ValidityPlan of the ligands and the ProteinGrid of their proteins")
    dev = predict_compound_coords.device
    L = int(plan.atom_off.numel()) - 1
    cb = torch.as_tensor(compound_batch).to(dev).long()
    if cb.dim() != 1 or cb.numel() != predict_compound_coords.shape[-2]:
        raise ValueError("compound_batch must be [%d]; got %s" % (predict_compound_coords.shape[-2], tuple(cb.shape)))
    if cb.numel() and (int(cb.min()) < 0 or int(cb.max()) >= L or bool((cb[1:] < cb[:-1]).any())
                       or not torch.equal(torch.bincount(cb, minlength=L).cumsum(0), plan.atom_off[1:].to(dev).long())):
        raise ValueError("compound_batch is not sorted or does not match the ligands of `plan`")
    res = validity.check_poses_protein(predict_compound_coords, plan, grid, **thresholds)
    if predict_compound_coords.dim() == 2:
        return res.ok[:, 0], res.flags[:, 0], res.stats[:, 0]
    return res.ok.t(), res.flags.t(), res.stats.transpose(0, 1)


def score_compound_coords_batched(predict_compound_coords, compound_batch, lig_types, grid, prot_types, torsion_plan=None, **options):
    """A Vina-style intermolecular energy of predicted (or fitted, or relaxed) ligand coordinates for the inference scripts:
    `scoring.score_poses` (csrc/pose_score.hip) behind the conventions of this module.  predict: [sum Nc, 3] ([S, sum Nc, 3] for S
    sampled poses) in the frame of the grid; compound_batch: sorted ligand id per atom; lig_types: int [sum Nc] type words
    (`scoring.ligand_types`); grid: the `validity.protein_grid` ProteinGrid of the same complexes built with edge >= cutoff
    (`protein_grid(edge=8.0)`); prot_types: int [M] type words of the grid's atoms (`scoring.protein_types_from_pdb`);
    torsion_plan: the `conformer.rotatable_bonds` TorsionPlan, whose torsion counts scale the total and whose status marks ligands
    that are not scored, or None (no torsions); options: weights, cutoff, torsion_weight, per_atom as `score_poses` takes them.
    -> (total float32 [L] ([S, L]): lower is better, NaN where a pose is not scored, flags int32 [L] ([S, L]), the PoseScores)."""
    from .. import scoring
    if not predict_compound_coords.is_cuda:
        raise RuntimeError("fabind_amd: the pose score runs on a HIP device only (no CPU fallback); got %s"
                           % predict_compound_coords.device)
    if grid is None:
        raise ValueError("score_compound_coords_batched needs the ProteinGrid of the proteins (validity.protein_grid(edge=8.0))")
    dev = predict_compound_coords.device
    L = int(grid.prot_off.numel()) - 1
    cb = torch.as_tensor(compound_batch).to(dev).long()
    if cb.dim() != 1 or cb.numel() != predict_compound_coords.shape[-2]:
        raise ValueError("compound_batch must be [%d]; got %s" % (predict_compound_coords.shape[-2], tuple(cb.shape)))
    if cb.numel() and (int(cb.min()) < 0 or int(cb.max()) >= L or bool((cb[1:] < cb[:-1]).any())):
        raise ValueError("compound_batch is not sorted or names a ligand outside the complexes of `grid`")
    atom_off = torch.zeros(L + 1, dtype=torch.int32, device=dev)
    atom_off[1:] = torch.bincount(cb, minlength=L).cumsum(0).to(torch.int32)
    n_torsions = status = None
    if torsion_plan is not None:
        if not torch.equal(torsion_plan.atom_off.to(dev), atom_off):
            raise ValueError("compound_batch does not match the ligands of `torsion_plan`")
        n_torsions, status = torch.diff(torsion_plan.off), torsion_plan.status
    res = scoring.score_poses(predict_compound_coords, atom_off, lig_types, grid, prot_types, n_torsions=n_torsions, status=status, **options)
    if predict_compound_coords.dim() == 2:
        return res.total[:, 0], res.flags[:, 0], res
    return res.total.t(), res.flags.t(), res


def post_optimize_compound_coords(reference_compound_coords, predict_compound_coords, total_epoch=1000, LAS_edge_index=None,
                                  mode=0):
    """The reference's per-ligand entry point: -> (x [Nc, 3], loss of the last epoch (float), RMSD (float)).  `mode` only
    selects the reference's unused interaction term (post_optim_utils.py:15-23: computed, never added to the loss)."""
    if mode not in (0, 1, 2):
        raise NotImplementedError()
    batch = torch.zeros(predict_compound_coords.shape[0], dtype=torch.int64, device=predict_compound_coords.device)
    x, loss, rmsd = post_optimize_compound_coords_batched(reference_compound_coords, predict_compound_coords, batch, total_epoch,
                                                          LAS_edge_index)
    return x, float(loss[0].item()), float(rmsd[0].item())
