"""Relax sampled ligand poses out of clashes with the protein and with themselves, in torsion space, on the GPU.

`conformer.fit_conformers` turns a predicted coordinate cloud into a real molecule, `validity.check_poses` / `check_poses_protein` say
whether it is still that molecule and whether it sits inside the protein; nothing so far MOVED a pose away from the receptor (the
reference does not either: its `post_optimize_compound_coords` never sees the protein).  `relax_poses` (csrc/pose_relax.hip; DESIGN.md
section 19) is that step: the start conformer moves over its rotatable-bond dihedrals and one rigid motion, held close to the predicted
pose and pushed out of contact with all heavy atoms of the protein (the cell list of `validity.protein_grid`) and with itself (the
PAIR_CLASH pairs and radii of `validity.validity_plan`).  Bond lengths, angles and rings stay exactly the start conformer's.  One wave
per (complex, pose), every pose of a batch in one launch, all iterations inside it."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .conformer import MAX_ATOMS, MAX_FIT_TORSIONS
from .symmetry import _atom_off

STATUS = {0: "ok", 3: "more than 256 atoms", 4: "more than 58 torsions"}
NO_INTRA, NO_PROTEIN = 8, 16          # bits of `status` next to the code status & 7: the ligand's ValidityPlan / the complex's ProteinGrid
STATUS_BITS = {"NO_INTRA": NO_INTRA, "NO_PROTEIN": NO_PROTEIN}      # has status != 0, so that term of E is absent
STOP = {0: "converged", 1: "iteration cap", 2: "rejections", 3: "a non-finite input"}
ENERGY = ("fit", "protein", "intra")


@dataclass
class PoseRelax:
    """What `relax_poses` returns, all on the device.  coords: float32 [S, N, 3], the relaxed poses; angles: float32 [S, T] in
    (-pi, pi], plan order: `perturb_conformers(conformer, plan, angles=angles, relative=True, random_rotation=False, centre=False)` is
    `coords` up to a rigid motion; energy0 / energy: float64 [S, B, 3], the three UNWEIGHTED sums of E (columns ENERGY) at the start
    (the Horn fit under angles0) / at the end; iters: int32 [S, B] accepted steps; stop: int32 [S, B], a key of STOP; status: int32
    [B]: status & 7 is a key of STATUS (3: the Horn image only, the last two sums NaN; 4: relaxed rigidly, zero angles), the bits
    STATUS_BITS say which term was absent; trace: float64 [S, B, max_iters], the weighted E after each accepted step, NaN behind the
    last -- or None."""
    coords: torch.Tensor
    angles: torch.Tensor
    energy0: torch.Tensor
    energy: torch.Tensor
    iters: torch.Tensor
    stop: torch.Tensor
    status: torch.Tensor
    trace: object = None


def _f32(v):
    return float(np.float32(v))


def relax_poses(conformer, target, torsion_plan, validity_plan, grid, angles0=None, w_fit=1.0, w_prot=100.0, w_intra=100.0, c_prot=0.80,
                c_intra=0.75, max_iters=100, tol=1e-6, return_trace=False, on_overflow="raise", out=None):
    """Move the start conformer of every ligand, over its rotatable-bond dihedrals and one rigid motion, close to its target poses and out
    of contact with its protein and with itself.

    conformer: [N, 3] on the HIP device; target: [N, 3] or [S, N, 3], the poses to stay near (normally `ConformerFit.coords` or the
    model's own prediction), matched atom by atom, in the frame of the grid; torsion_plan: the `conformer.rotatable_bonds` TorsionPlan,
    validity_plan: the `validity.validity_plan` ValidityPlan, grid: the `validity.protein_grid` ProteinGrid, all of the same complexes.
    Damped Gauss-Newton (csrc/pose_relax.hip) on

        E = w_fit   sum_i |X_i - y_i|^2
          + w_prot  sum_{i, p}  max(0, c_prot  (r_i + r_p) - |X_i - P_p|)^2     p: every kept protein atom of the complex's grid
          + w_intra sum_{i < j} max(0, c_intra (r_i + r_j) - |X_i - X_j|)^2     (i, j): the PAIR_CLASH pairs of the ValidityPlan

    with the radii of the plan and the grid.  c_prot = 0.80 and c_intra = 0.75 sit a margin above the `clash_min` of `check_poses_protein`
    (0.75) and `check_poses` (0.70); the defaults rest on a float64 experiment on the host only.
    angles0: [S, T] (or [T]) start angles, normally `ConformerFit.angles`; None: zeros.  The rigid motion starts as the Horn fit of the
    start conformer under angles0 onto the target.  At most `max_iters` accepted steps, stopped early by an accepted step that lowered E
    by no more than `tol` times itself or by 8 rejected trials in a row; E == 0 at the start means no iteration.
    on_overflow: "raise" -> RuntimeError naming every ligand of more than 256 atoms or more than 58 torsions; "truncate" -> such a
    ligand gets the Horn image only (status 3) / is relaxed rigidly (status 4, zero angles).  A ligand whose ValidityPlan status != 0
    has no intra term, a complex whose ProteinGrid status != 0 no protein term (bits NO_INTRA / NO_PROTEIN of `status`).  A NaN or
    infinite coordinate in a target ends that pose alone: NaN outputs, stop code 3.
    Needs c_prot * (largest ligand radius + grid.max_radius) <= grid.edge: the 27 cells round an atom then hold every partner.  One host
    read-back checks the offsets the kernel indexes with and the ligand radii before the launch.
    out: an optional contiguous float32 [S, N, 3] tensor on the device for the coordinates.  -> PoseRelax."""
    if on_overflow not in ("raise", "truncate"):
        raise ValueError("on_overflow must be 'raise' or 'truncate'")
    if not torch.is_tensor(conformer) or not conformer.is_cuda or not torch.is_tensor(target) or not target.is_cuda:
        raise RuntimeError("fabind_amd: relax_poses runs on a HIP device only (no CPU fallback)")
    if torsion_plan is None or validity_plan is None or grid is None:
        raise ValueError("relax_poses needs the TorsionPlan and the ValidityPlan of the ligands and the ProteinGrid of their proteins")
    dev = conformer.device
    x = conformer.detach().to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("conformer must be [N, 3]; got %s" % (tuple(conformer.shape),))
    N = x.shape[0]
    y = target.detach().to(device=dev, dtype=torch.float32)
    if y.dim() == 2:
        y = y[None]
    if y.dim() != 3 or tuple(y.shape[1:]) != (N, 3) or y.shape[0] < 1 or y.shape[0] > 65535:
        raise ValueError("target must be [%d, 3] or [S, %d, 3] with 1 <= S <= 65535; got %s" % (N, N, tuple(target.shape)))
    y = y.contiguous()
    S = y.shape[0]
    max_iters = int(max_iters)
    if max_iters < 0 or max_iters > 65536:
        raise ValueError("max_iters must be in [0, 65536]")
    tol = float(tol)
    if not (tol >= 0.0 and tol < 1.0):
        raise ValueError("tol must be in [0, 1)")
    weights = tuple(_f32(v) for v in (w_fit, w_prot, w_intra, c_prot, c_intra))
    if not all(0.0 <= v < float("inf") for v in weights):
        raise ValueError("w_fit, w_prot, w_intra, c_prot and c_intra must be finite and >= 0")
    tp, vp = torsion_plan, validity_plan
    aoff = _atom_off(tp.atom_off, dev, N)
    B = aoff.numel() - 1
    T = int(tp.quad.shape[0])
    oh = tp.off.cpu().numpy()
    if (tp.off.dtype != torch.int32 or oh.shape != (B + 1,) or oh[0] != 0 or (np.diff(oh) < 0).any() or int(oh[-1]) != T
            or tuple(tp.quad.shape) != (T, 4) or tuple(tp.side.shape) != (T, 8) or tp.quad.dtype != torch.int32 or tp.side.dtype != torch.int32
            or not (tp.quad.is_contiguous() and tp.side.is_contiguous() and tp.off.is_contiguous())
            or tp.quad.device != dev or tp.side.device != dev or tp.off.device != dev):
        raise ValueError("inconsistent TorsionPlan")
    C, Kk = grid.cell_ptr.numel() - 1, grid.xyz.shape[0]
    ints = (vp.atom_off, vp.status, vp.cls, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr)
    if (any(t.device != dev or not t.is_contiguous() for t in ints + (vp.radii, grid.xyz, grid.radii))
            or any(t.dtype != torch.int32 for t in ints) or any(t.dtype != torch.float32 for t in (vp.radii, grid.xyz, grid.radii))
            or tuple(vp.atom_off.shape) != (B + 1,) or tuple(vp.status.shape) != (B,) or tuple(vp.cls.shape) != (N, 16)
            or tuple(vp.radii.shape) != (N,) or tuple(grid.status.shape) != (B,) or tuple(grid.origin.shape) != (B, 3)
            or tuple(grid.dims.shape) != (B, 3) or tuple(grid.cell_off.shape) != (B + 1,) or tuple(grid.atom_off.shape) != (B + 1,) or C < 0
            or tuple(grid.xyz.shape) != (Kk, 3) or tuple(grid.radii.shape) != (Kk,)):
        raise ValueError("inconsistent ValidityPlan or ProteinGrid (both must hold the complexes of the TorsionPlan's ligands)")
    a0 = None
    if angles0 is not None:
        a0 = torch.as_tensor(angles0).detach().to(device=dev, dtype=torch.float32)
        if a0.dim() == 1:
            a0 = a0[None].expand(S, -1)
        if tuple(a0.shape) != (S, T):
            raise ValueError("angles0 must be [%d, %d]; got %s" % (S, T, tuple(a0.shape)))
        a0 = a0.contiguous()
    if out is not None and not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32
                                and out.is_contiguous() and tuple(out.shape) == (S, N, 3)):
        raise ValueError("out must be a contiguous float32 [%d, %d, 3] tensor on %s" % (S, N, dev))
    # the kernel indexes the ligands, the cells and the sorted atoms with these: checked on the host, one read-back
    rl = vp.radii
    rmax = rl.max().reshape(1) if N else torch.zeros(1, device=dev)
    ok = [torch.equal(vp.atom_off, aoff), (torch.diff(aoff) >= 0).all(),
          (grid.cell_off[0] == 0), (torch.diff(grid.cell_off) >= 0).all(), (grid.cell_off[-1] == C),
          (grid.atom_off[0] == 0), (torch.diff(grid.atom_off) >= 0).all(), (grid.atom_off[-1] == Kk),
          (grid.cell_ptr[0] == 0), (torch.diff(grid.cell_ptr) >= 0).all(), (grid.cell_ptr[-1] == Kk),
          (grid.dims >= 0).all(), (grid.dims.long().prod(1) == torch.diff(grid.cell_off)).all(),
          ((rl >= 0) & (rl < float("inf"))).all() if N else True]
    host = torch.cat([torch.stack([torch.as_tensor(o, device=dev).reshape(()).to(torch.float32) for o in ok]), rmax.to(torch.float32)]).cpu().numpy()
    if not host[:13].all():
        raise ValueError("inconsistent ValidityPlan or ProteinGrid (both must hold the complexes of the TorsionPlan's ligands)")
    if not host[13]:
        raise ValueError("ligand radii must be finite and >= 0")
    reach = weights[3] * (float(host[14]) + float(grid.max_radius))
    if not grid.edge >= reach:
        raise ValueError("the grid's edge (%g) is smaller than c_prot * (largest ligand radius + largest protein radius) = %g: build the "
                         "grid with a larger edge" % (grid.edge, reach))
    counts, tcount = np.diff(aoff.cpu().numpy()), np.diff(oh)
    code = np.where(counts > MAX_ATOMS, 3, np.where(tcount > MAX_FIT_TORSIONS, 4, 0))
    bad = np.nonzero(code)[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("relax_poses: " + "; ".join("ligand %d: status %d (%s)" % (b, code[b], STATUS[int(code[b])]) for b in bad))
    if out is None:
        out = torch.empty(S, N, 3, dtype=torch.float32, device=dev)
    angles = torch.empty(S, T, dtype=torch.float32, device=dev)
    energy0 = torch.empty(S, B, 3, dtype=torch.float64, device=dev)
    energy = torch.empty(S, B, 3, dtype=torch.float64, device=dev)
    iters = torch.empty(S, B, dtype=torch.int32, device=dev)
    stop = torch.empty(S, B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    trace = torch.empty(S, B, max_iters, dtype=torch.float64, device=dev) if return_trace else None
    use_plan = T > 0
    K.pose_relax(x, y, a0 if use_plan else None, aoff, B, tp.off if use_plan else None, tp.quad if use_plan else None,
                 tp.side if use_plan else None, T, int(counts.max()) if B else 0, int(tcount.max()) if B else 0, vp.status, vp.cls, vp.radii,
                 grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr, grid.xyz, grid.radii, grid.edge, reach,
                 weights, max_iters, tol, out, angles, energy0, energy, iters, stop, status, trace)
    return PoseRelax(coords=out, angles=angles, energy0=energy0, energy=energy, iters=iters, stop=stop, status=status, trace=trace)
