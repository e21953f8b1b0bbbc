"""Train-time ligand augmentation on the GPU: rotatable bonds from the bond list, torsion noise and the uniform random rotation.

The reference rotates the start conformer of every training sample (data.py:80-85 -> utils/utils.py:307-311
`uniform_random_rotation`) and, under FABind+'s `--train-ligand-torsion-noise` (utils/utils.py:285-304), first sets every rotatable
bond of the crystal ligand (`get_torsions`, :155-190: RDKit SMARTS) to a uniform random dihedral -- per sample, per epoch, on the host
with RDKit.  Here both run for a whole batch in csrc/conformer.hip:

* `rotatable_bonds`: the torsion plan of every ligand (one wave per candidate bond: a flood fill decides "on no cycle" and
  "which atoms move" at once).  A bond j-k is rotatable iff it is SINGLE, both ends have heavy-atom degree >= 2, neither end has a
  TRIPLE bond, and it is on no cycle -- the reference's SMARTS read literally on the heavy-atom graph.
* `perturb_conformers`: `n_copies` perturbed images of every ligand (one wave per ligand and copy): the torsions set one after
  another, then the rotation M = -(H R).  Random numbers are a counter-based hash of (seed, key of the ligand, copy, draw): a
  ligand's result depends on its key and the seed, never on the batch around it.

RDKit's choice of reference atoms (i, l) and of the moving side is not reproduced: under a uniform target dihedral and a uniform
rotation of the whole ligand neither changes the distribution of the result.

* `fit_conformers` (csrc/conformer_fit.hip) is the inverse of `perturb_conformers`: the dihedral changes and the rigid motion that bring
  the start conformer closest to a target pose, atom by atom -- a predicted coordinate cloud turned into a molecule with the start
  conformer's bond lengths, angles and rings.  One wave per (ligand, pose), all iterations in one launch."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .symmetry import _atom_off, bond_code

MAX_ATOMS = 256
MAX_FIT_TORSIONS = 58
STATUS = {0: "ok", 3: "more than 256 atoms", 4: "more than 58 torsions"}
STOP = {0: "converged", 1: "iteration cap", 2: "rejections"}


@dataclass
class TorsionPlan:
    """Rotatable bonds of a batch of ligands, all on the device.  quad: int32 [T, 4], torsion t = (i, j, k, l) as LOCAL atom ids,
    j < k the bond, i / l the lowest-index neighbour of j other than k / of k other than j; side: int32 [T, 8], the 256-bit set of
    atoms in k's component once j-k is removed (bit a of word a // 32 <=> atom a; read the words as unsigned); off: int32 [B + 1],
    ligand b's torsions at [off[b], off[b + 1]) in ascending (j, k) order; status: int32 [B] (0 ok, 3 more than 256 atoms: no
    torsions); atom_off: int32 [B + 1]."""
    quad: torch.Tensor
    side: torch.Tensor
    off: torch.Tensor
    status: torch.Tensor
    atom_off: torch.Tensor


def _coded_neighbour_lists(bond_index, codes, n_atoms):
    """Symmetrised, de-duplicated neighbour lists sorted by (owner, neighbour), with the bond code of every entry (a bond listed
    several times takes its smallest code; self-loops are dropped).  -> ptr int32 [N + 1], idx, code, owner int32 [2 * bonds]."""
    dev = bond_index.device
    lo, hi = torch.minimum(bond_index[0], bond_index[1]), torch.maximum(bond_index[0], bond_index[1])
    keep = lo != hi
    key, inv = torch.unique(lo[keep] * n_atoms + hi[keep], return_inverse=True)
    c = torch.full((key.numel(),), 2 ** 30, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, codes[keep], "amin")
    lo, hi = torch.div(key, n_atoms, rounding_mode="floor"), key % n_atoms
    owner, other, code = torch.cat([lo, hi]), torch.cat([hi, lo]), torch.cat([c, c])
    order = torch.argsort(owner * n_atoms + other)
    ptr_ = torch.zeros(n_atoms + 1, dtype=torch.int32, device=dev)
    ptr_[1:] = torch.cumsum(torch.bincount(owner, minlength=n_atoms), 0).to(torch.int32)
    i32 = lambda t: t[order].to(torch.int32).contiguous()
    return ptr_, i32(other), i32(code), i32(owner)


def rotatable_bonds(bond_index, bond_codes, atom_off, on_overflow="raise"):
    """The torsion plan of every ligand of a batch (csrc/conformer.hip).

    bond_index: [2, E] GLOBAL atom ids on the HIP device, each bond once, in both directions or repeated -- the plan is the same;
    bonds never cross ligands.  bond_codes: [E] aligned with bond_index, `symmetry.bond_code` coding (AROMATIC 1, TRIPLE 2, DOUBLE 3,
    SINGLE 4, other 5; names are accepted).  atom_off: [B + 1] atom offsets of the ligands.
    on_overflow: "raise" -> RuntimeError naming every ligand of more than 256 atoms; "truncate" -> such a ligand gets no torsions
    (status 3) and is only rotated by `perturb_conformers`.
    -> TorsionPlan.  Two launches (count, then write): one host read-back sizes the output."""
    if on_overflow not in ("raise", "truncate"):
        raise ValueError("on_overflow must be 'raise' or 'truncate'")
    if not torch.is_tensor(bond_index) or not bond_index.is_cuda:
        raise RuntimeError("fabind_amd: rotatable_bonds runs on a HIP device only (no CPU fallback)")
    dev = bond_index.device
    bi = bond_index.to(torch.int64).reshape(2, -1)
    if not torch.is_tensor(bond_codes) and len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [bond_code(t) for t in bond_codes]
    codes = torch.as_tensor(bond_codes).to(device=dev, dtype=torch.int64).reshape(-1)
    if codes.numel() != bi.shape[1]:
        raise ValueError("rotatable_bonds: %d bonds but %d bond codes" % (bi.shape[1], codes.numel()))
    ao = torch.as_tensor(atom_off)
    N = int(ao[-1]) if ao.dim() == 1 and ao.numel() else -1
    aoff = _atom_off(atom_off, dev, N)
    B = aoff.numel() - 1
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= N):
        raise ValueError("bond_index holds atom ids outside [0, %d)" % N)
    nptr, nidx, ncode, nown = _coded_neighbour_lists(bi, codes, max(N, 1))
    E2 = nidx.numel()
    flag = torch.empty(max(E2, 1), dtype=torch.int32, device=dev)
    sq = torch.empty(max(E2, 1) * 4, dtype=torch.int32, device=dev)
    ss = torch.empty(max(E2, 1) * 8, dtype=torch.int32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    check(lib.fabind_torsion_plan(ptr(nptr), ptr(nidx), ptr(ncode), ptr(nown), ptr(aoff), B, E2, ptr(flag), ptr(sq), ptr(ss),
                                  ptr(count), ptr(status), None, None, None, stream()), "fabind_torsion_plan(count)")
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(count, 0)
    host = torch.cat([off[-1:], status]).cpu().numpy()               # the one read-back: total torsions and the statuses
    bad = np.nonzero(host[1:])[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("rotatable_bonds: " + "; ".join("ligand %d: status %d (%s)" % (b, host[1 + b], STATUS[int(host[1 + b])])
                                                            for b in bad))
    T = int(host[0])
    quad = torch.empty(T, 4, dtype=torch.int32, device=dev)
    side = torch.empty(T, 8, dtype=torch.int32, device=dev)
    if T:
        check(lib.fabind_torsion_plan(ptr(nptr), ptr(nidx), ptr(ncode), ptr(nown), ptr(aoff), B, E2, ptr(flag), ptr(sq), ptr(ss),
                                      ptr(count), ptr(status), ptr(off), ptr(quad), ptr(side), stream()), "fabind_torsion_plan(write)")
    return TorsionPlan(quad=quad, side=side, off=off, status=status, atom_off=aoff)


def random_rotation_matrix(uniforms):
    """M = -(H R) of the reference's `uniform_random_rotation` (utils/utils.py:58-78) from uniforms [..., 3] = (x1, x2, x3) in
    [0, 1): R the rotation by 2 pi x1 about z, H = I - 2 v v^T with v = (cos(2 pi x2) sqrt(x3), sin(2 pi x2) sqrt(x3), sqrt(1 - x3)).
    Row-vector convention: rotated = x @ M.  Plain tensor arithmetic on the device (and dtype) of `uniforms`; for callers who rotate
    a pocket together with the ligand."""
    u = torch.as_tensor(uniforms)
    x1, x2, x3 = u[..., 0], u[..., 1], u[..., 2]
    c1, s1 = torch.cos(2 * np.pi * x1), torch.sin(2 * np.pi * x1)
    z, o = torch.zeros_like(x1), torch.ones_like(x1)
    R = torch.stack([torch.stack([c1, -s1, z], -1), torch.stack([s1, c1, z], -1), torch.stack([z, z, o], -1)], -2)
    v = torch.stack([torch.cos(2 * np.pi * x2) * torch.sqrt(x3), torch.sin(2 * np.pi * x2) * torch.sqrt(x3), torch.sqrt(1 - x3)], -1)
    H = torch.eye(3, dtype=u.dtype, device=u.device) - 2 * v[..., :, None] * v[..., None, :]
    return -(H @ R)


def perturb_conformers(coords, plan=None, n_copies=1, seed=0, keys=None, torsion_noise=True, random_rotation=True, centre=True,
                       angles=None, relative=False, uniforms=None, atom_off=None, compound_batch=None, out=None):
    """`n_copies` perturbed conformers of every ligand: coords [N, 3] on the HIP device -> float32 [n_copies, N, 3].

    torsion_noise: every torsion of `plan` (a TorsionPlan of the same ligands) is set, one after another in plan order, to a target
    dihedral 2 pi u -- or rotated BY the target when `relative`; `angles` [n_copies, T] (radians, plan order) replaces the draws.
    random_rotation: then out = (x - mean) @ M + mean @ M with M = `random_rotation_matrix`(x1, x2, x3); `uniforms`
    [n_copies, B, 3] = (x1, x2, x3) replaces the draws.  centre: the term mean @ M is dropped, the output centroid is the origin
    (where the reference's CanonicalizeConformer followed by the rotation leaves it).
    plan=None needs torsion_noise=False and `atom_off` [B + 1] or a sorted `compound_batch` [N]: rotation only.
    keys: int [B], the identity of each ligand for the random draws (default: its position in the batch); together with `seed` it
    fixes the ligand's result whatever batch it sits in.  Draws: u(seed, key, copy, draw), draw = 0 .. T_b - 1 for the torsions,
    then x2, x3, x1.  A ligand of more than 256 atoms has no torsions and is rotated only.
    out: an optional contiguous float32 [n_copies, N, 3] tensor on the device to write into (else a new one)."""
    if not torch.is_tensor(coords) or not coords.is_cuda:
        raise RuntimeError("fabind_amd: perturb_conformers runs on a HIP device only (no CPU fallback)")
    dev = coords.device
    x = coords.detach().to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("coords must be [N, 3]; got %s" % (tuple(coords.shape),))
    N, S = x.shape[0], int(n_copies)
    if S < 1 or S > 65535:
        raise ValueError("n_copies must be in [1, 65535]")
    if plan is None:
        if torsion_noise:
            raise ValueError("torsion_noise=True needs a TorsionPlan (rotatable_bonds); pass torsion_noise=False for rotation only")
        if atom_off is None:
            if compound_batch is None:
                raise ValueError("without a plan pass atom_off or compound_batch")
            cb = torch.as_tensor(compound_batch).to(dev).long()
            atom_off = torch.zeros(int(cb.max()) + 2 if cb.numel() else 1, dtype=torch.int64, device=dev)
            atom_off[1:] = torch.cumsum(torch.bincount(cb), 0)
        aoff = _atom_off(atom_off, dev, N)
    else:
        aoff = _atom_off(plan.atom_off, dev, N)
        if atom_off is not None and not torch.equal(aoff, _atom_off(atom_off, dev, N)):
            raise ValueError("atom_off does not match the ligands of `plan`")
    B = aoff.numel() - 1
    use_plan = plan is not None and torsion_noise
    T = int(plan.quad.shape[0]) if use_plan else 0
    if use_plan:                                                      # the kernel indexes quad / side / angles with these offsets
        oh = plan.off.cpu().numpy()
        if (plan.off.dtype != torch.int32 or oh.shape != (B + 1,) or oh[0] != 0 or (np.diff(oh) < 0).any() or int(oh[-1]) != T
                or tuple(plan.quad.shape) != (T, 4) or tuple(plan.side.shape) != (T, 8) or plan.quad.dtype != torch.int32
                or plan.side.dtype != torch.int32 or not (plan.quad.is_contiguous() and plan.side.is_contiguous() and plan.off.is_contiguous())
                or plan.quad.device != dev or plan.side.device != dev or plan.off.device != dev):
            raise ValueError("inconsistent TorsionPlan")
    f32 = lambda t, shape, what: _shaped(torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous(), shape, what)
    ang = f32(angles, (S, T), "angles") if (angles is not None and use_plan) else None
    uni = f32(uniforms, (S, B, 3), "uniforms") if (uniforms is not None and random_rotation) else None
    k = None
    if keys is not None:
        k = torch.as_tensor(keys).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(k.shape) != (B,):
            raise ValueError("keys must be [%d]" % B)
    if out is None:
        out = torch.empty(S, N, 3, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (S, N, 3)):
        raise ValueError("out must be a contiguous float32 [%d, %d, 3] tensor on %s" % (S, N, dev))
    check(_lib.load().fabind_conformer_perturb(ptr(x), ptr(aoff), B, N, S, ptr(plan.off) if use_plan else None,
                                               ptr(plan.quad) if use_plan else None, ptr(plan.side) if use_plan else None, ptr(ang), T,
                                               ptr(uni), ptr(k), int(seed) & 0xFFFFFFFF, int(bool(relative)), int(bool(random_rotation)),
                                               int(bool(centre)), ptr(out), stream()), "fabind_conformer_perturb")
    return out


@dataclass
class ConformerFit:
    """What `fit_conformers` returns, all on the device.  coords: float32 [S, N, 3], the fitted poses; angles: float32 [S, T] in
    (-pi, pi], plan order: `perturb_conformers(conformer, plan, angles=angles, relative=True, random_rotation=False, centre=False)`
    is `coords` up to a rigid motion; rmsd0 / rmsd: float32 [S, B], to the target after the rigid fit alone / at the end; iters:
    int32 [S, B] accepted steps; stop: int32 [S, B], a key of STOP; status: int32 [B], a key of STATUS (3 / 4: rigid fit only);
    trace: float64 [S, B, max_iters] E = n rmsd^2 after each accepted step, NaN behind the last -- or None."""
    coords: torch.Tensor
    angles: torch.Tensor
    rmsd0: torch.Tensor
    rmsd: torch.Tensor
    iters: torch.Tensor
    stop: torch.Tensor
    status: torch.Tensor
    trace: object = None


def fit_conformers(conformer, target, plan=None, max_iters=50, tol=1e-6, return_trace=False, on_overflow="raise", atom_off=None,
                   compound_batch=None, out=None):
    """Fit the start conformer of every ligand to target poses over its rotatable-bond dihedrals and one rigid motion.

    conformer: [N, 3] on the HIP device; target: [N, 3] or [S, N, 3], matched atom by atom; plan: the TorsionPlan of the same ligands.
    Damped Gauss-Newton on sum |pose(a) - target|^2 (csrc/conformer_fit.hip), at most `max_iters` accepted steps, stopped early by an
    accepted step that lowered the sum by no more than `tol` times itself or by 8 rejected trials in a row.  The defaults rest on a
    float64 experiment on the host only.
    plan=None needs `atom_off` [B + 1] or a sorted `compound_batch` [N]: the rigid fit (Horn's quaternion method, a proper rotation
    always) of every ligand onto every target, angles [S, 0].
    on_overflow: "raise" -> RuntimeError naming every ligand of more than 256 atoms or more than 58 torsions; "truncate" -> such a
    ligand gets the rigid fit only (status 3 / 4, zero angles).
    out: an optional contiguous float32 [S, N, 3] tensor on the device for the coordinates.  -> ConformerFit."""
    if on_overflow not in ("raise", "truncate"):
        raise ValueError("on_overflow must be 'raise' or 'truncate'")
    if not torch.is_tensor(conformer) or not conformer.is_cuda or not torch.is_tensor(target) or not target.is_cuda:
        raise RuntimeError("fabind_amd: fit_conformers runs on a HIP device only (no CPU fallback)")
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
    if plan is None:
        if atom_off is None:
            if compound_batch is None:
                raise ValueError("without a plan pass atom_off or compound_batch")
            cb = torch.as_tensor(compound_batch).to(dev).long()
            atom_off = torch.zeros(int(cb.max()) + 2 if cb.numel() else 1, dtype=torch.int64, device=dev)
            atom_off[1:] = torch.cumsum(torch.bincount(cb), 0)
        aoff = _atom_off(atom_off, dev, N)
    else:
        aoff = _atom_off(plan.atom_off, dev, N)
        if atom_off is not None and not torch.equal(aoff, _atom_off(atom_off, dev, N)):
            raise ValueError("atom_off does not match the ligands of `plan`")
    B = aoff.numel() - 1
    ah = aoff.cpu().numpy()
    counts = np.diff(ah)
    T, tcount = 0, np.zeros(B, np.int64)
    if plan is not None:
        T = int(plan.quad.shape[0])
        oh = plan.off.cpu().numpy()
        if (plan.off.dtype != torch.int32 or oh.shape != (B + 1,) or oh[0] != 0 or (np.diff(oh) < 0).any() or int(oh[-1]) != T
                or tuple(plan.quad.shape) != (T, 4) or tuple(plan.side.shape) != (T, 8) or plan.quad.dtype != torch.int32
                or plan.side.dtype != torch.int32 or not (plan.quad.is_contiguous() and plan.side.is_contiguous() and plan.off.is_contiguous())
                or plan.quad.device != dev or plan.side.device != dev or plan.off.device != dev):
            raise ValueError("inconsistent TorsionPlan")
        tcount = np.diff(oh)
    code = np.where(counts > MAX_ATOMS, 3, np.where(tcount > MAX_FIT_TORSIONS, 4, 0))
    bad = np.nonzero(code)[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("fit_conformers: " + "; ".join("ligand %d: status %d (%s)" % (b, code[b], STATUS[int(code[b])]) for b in bad))
    if out is None:
        out = torch.empty(S, N, 3, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (S, N, 3)):
        raise ValueError("out must be a contiguous float32 [%d, %d, 3] tensor on %s" % (S, N, dev))
    angles = torch.empty(S, T, dtype=torch.float32, device=dev)
    rmsd0 = torch.empty(S, B, dtype=torch.float32, device=dev)
    rmsd = torch.empty(S, B, dtype=torch.float32, device=dev)
    iters = torch.empty(S, B, dtype=torch.int32, device=dev)
    stop = torch.empty(S, B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    trace = torch.empty(S, B, max_iters, dtype=torch.float64, device=dev) if return_trace else None
    use_plan = plan is not None and T > 0
    check(_lib.load().fabind_conformer_fit(ptr(x), ptr(y), ptr(aoff), B, N, S, ptr(plan.off) if use_plan else None,
                                           ptr(plan.quad) if use_plan else None, ptr(plan.side) if use_plan else None, T,
                                           int(counts.max()) if B else 0, int(tcount.max()) if B else 0, max_iters, tol, ptr(out),
                                           ptr(angles), ptr(rmsd0), ptr(rmsd), ptr(iters), ptr(stop), ptr(status), ptr(trace), stream()),
          "fabind_conformer_fit")
    return ConformerFit(coords=out, angles=angles, rmsd0=rmsd0, rmsd=rmsd, iters=iters, stop=stop, status=status, trace=trace)


def _shaped(t, shape, what):
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s; got %s" % (what, tuple(shape), tuple(t.shape)))
    return t
