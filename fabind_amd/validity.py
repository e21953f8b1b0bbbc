"""Physical validity of sampled ligand poses on the GPU: is a predicted coordinate cloud still the molecule?

The reference has no such step (its sampling evaluation, test_sampling_fabind.py:159-191, ranks by confidence and reports RMSD); the
checks are those docking benchmarks report since PoseBusters next to "RMSD < 2 A", restated so that a whole batch runs in
csrc/pose_check.hip:

* `validity_plan`: per ligand, once, from the bond list and the start conformer: the hop class of every atom pair (bonded, angle, clash,
  exempt), the reference distances of the bonded and angle pairs, the planar groups (aromatic systems, double bonds) and the stereo
  centres with their signed volumes.  Count pass, one host read-back, write pass -- as `conformer.rotatable_bonds`.
* `check_poses`: nine statistics and a flag word for every (ligand, pose) of [S, N, 3] poses, one launch whatever S.
* `protein_grid` / `check_poses_protein` (csrc/protein_contacts.hip): the same poses against ALL heavy atoms of
  the protein through a cell list built once per protein -- smallest distance as a fraction of the radius sum, share of the ligand's
  volume inside the protein; `protein_atoms_from_pdb` reads the atoms.

Where this differs from PoseBusters: bond lengths and 1-3 distances are RATIOS to the start conformer's (PoseBusters compares with the
bounds of RDKit's distance geometry); the clash test runs over pairs four or more bonds apart and over different fragments (1-4 pairs are
exempt: with bonds and angles intact their distance is bounded by the cis geometry, and crystal 1-4 contacts reach 0.73 of the radius
sum); flatness is the largest distance from the least-squares plane, as there; chirality is the sign of a signed volume against the
start conformer's instead of CIP labels; the protein check is the distance to C-alpha atoms only and has no default threshold.
Aromatic systems are read from AROMATIC-coded bonds: a Kekulised bond list (alternating SINGLE / DOUBLE) has no aromatic group, its ring
double bonds are then checked as double-bond groups.  DESIGN.md section 17 has the definitions and the error bounds."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .conformer import _coded_neighbour_lists
from .symmetry import _atom_off, bond_code

MAX_ATOMS = 256
STATUS = {0: "ok", 3: "more than 256 atoms", 5: "two bonded or 1-3 atoms at distance 0 in the start conformer"}
STATS = ("bond_lo", "bond_hi", "angle_lo", "angle_hi", "clash", "flat_aromatic", "flat_double", "chirality", "ca_dist")
BOND, ANGLE, CLASH, AROMATIC_FLAT, DOUBLE_FLAT, CHIRALITY, PROTEIN, NONFINITE, UNCHECKED = 1, 2, 4, 8, 16, 32, 64, 128, 256
FLAGS = {"BOND": BOND, "ANGLE": ANGLE, "CLASH": CLASH, "AROMATIC_FLAT": AROMATIC_FLAT, "DOUBLE_FLAT": DOUBLE_FLAT, "CHIRALITY": CHIRALITY,
         "PROTEIN": PROTEIN, "NONFINITE": NONFINITE, "UNCHECKED": UNCHECKED}
PAIR_EXEMPT, PAIR_BONDED, PAIR_ANGLE, PAIR_CLASH = 0, 1, 2, 3


@dataclass
class ValidityPlan:
    """What `check_poses` needs of a batch of ligands, all on the device; atom ids are LOCAL to their ligand, so a ligand's entries are
    the same bits alone and in any batch.
    atom_off: int32 [B + 1]; status: int32 [B], a key of STATUS (a ligand with status != 0 has no entries and is not checked).
    cls: int32 [N, 16], the pair classes of atom i's row, two bits per partner j at bit 2 (j % 16) of word j // 16 (read the words as
    unsigned): PAIR_BONDED 1 (one bond apart), PAIR_ANGLE 2 (two), PAIR_CLASH 3 (four or more, or another fragment), PAIR_EXEMPT 0
    (three bonds apart, i itself, ids beyond the ligand).  radii: float32 [N].
    offs: int32 [4, B + 1], ligand b's slots in the four lists below: rows 0 pairs, 1 groups, 2 group atoms, 3 centres.
    pair_ij: int32 [P, 2], the bonded and angle pairs i < j in ascending (i, j); pair_kind: int32 [P] (1 / 2); pair_d0: float64 [P],
    their distance in the start conformer (float32 differences, float64 sum and root).
    group: int32 [G, 3] = (0 aromatic / 1 double bond, first position within the ligand's slot of group_atoms, atoms), ordered by key
    atom (the lowest atom of an aromatic system, the lower end of a double bond), aromatic before double at one key, double bonds of one
    key by their other end; group_atoms: int32 [A], ascending within a group.
    centre: int32 [C, 5] = (c, n1, n2, n3, n4 or -1), neighbours ascending, centres ascending; centre_v0: float64 [C], the signed
    volume in the start conformer.  max_atoms: the largest ligand of status 0 (a python int, from the plan's one read-back)."""
    atom_off: torch.Tensor
    status: torch.Tensor
    cls: torch.Tensor
    radii: torch.Tensor
    offs: torch.Tensor
    pair_ij: torch.Tensor
    pair_kind: torch.Tensor
    pair_d0: torch.Tensor
    group: torch.Tensor
    group_atoms: torch.Tensor
    centre: torch.Tensor
    centre_v0: torch.Tensor
    max_atoms: int = 0


@dataclass
class PoseValidity:
    """stats: float32 [B, S, 9], columns STATS; flags: int32 [B, S], bits FLAGS; valid: bool [B, S] = no flag, or UNCHECKED alone."""
    stats: torch.Tensor
    flags: torch.Tensor
    valid: torch.Tensor


def validity_plan(bond_index, bond_codes, atomic_numbers, coords0, atom_off, autos=None, radii=None, min_volume=1.0, on_overflow="raise"):
    """The validity plan of every ligand of a batch (csrc/pose_check.hip), on the heavy-atom graph.

    bond_index: [2, E] GLOBAL atom ids on the HIP device, each bond once, in both directions or repeated; bonds never cross ligands.
    bond_codes: [E], `symmetry.bond_code` coding (AROMATIC 1, TRIPLE 2, DOUBLE 3, SINGLE 4, other 5; names are accepted).
    atomic_numbers: int [N]; coords0: [N, 3], the start conformer (`rdkit_coords`); atom_off: [B + 1].
    radii: float [N] van der Waals radii, or None for Bondi's by atomic number (B 1.92, C 1.70, N 1.55, O 1.52, F 1.47, Si 2.10, P 1.80,
    S 1.80, Cl 1.75, Se 1.90, Br 1.85, I 1.98, any other 2.00).
    Planar groups: every connected component of the AROMATIC-coded bonds with at least 4 atoms (a fused system is one group, biphenyl
    two; a Kekulised bond list has none); every DOUBLE-coded bond whose ends are both C, N or O with at most three neighbours each,
    together with all their neighbours, when that makes at least 4 atoms (S=O and P=O are excluded).
    Stereo centres: an atom with three or four neighbours, no AROMATIC, DOUBLE or TRIPLE bond, no nitrogen unless it has four neighbours,
    whose signed volume in the start conformer has |V0| >= min_volume (A^3; V = det[n1 - c, n2 - c, n3 - c] for three neighbours,
    det[n1 - n4, n2 - n4, n3 - n4] for four, neighbours in ascending id).  autos: a `symmetry.Automorphisms` of the same ligands: a
    centre is dropped when some automorphism fixes it and permutes its neighbours oddly (inverting it gives the same molecule: an
    isopropyl carbon); only complete automorphism sets (status 0) are used.  With autos=None EVERY centre is kept, such
    pseudo-centres included, and a pose that swaps two identical substituents is flagged CHIRALITY.
    on_overflow: "raise" -> RuntimeError naming every ligand with status != 0 (3: more than 256 atoms; 5: two bonded or 1-3 atoms at
    distance 0 in coords0); "skip" -> such ligands keep their status, have no entries and `check_poses` reports them UNCHECKED.
    -> ValidityPlan.  Two launches (count, then write): one host read-back sizes the lists."""
    if on_overflow not in ("raise", "skip"):
        raise ValueError("on_overflow must be 'raise' or 'skip'")
    if not torch.is_tensor(bond_index) or not bond_index.is_cuda:
        raise RuntimeError("fabind_amd: validity_plan runs on a HIP device only (no CPU fallback)")
    dev = bond_index.device
    bi = bond_index.to(torch.int64).reshape(2, -1)
    if not torch.is_tensor(bond_codes) and len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [bond_code(t) for t in bond_codes]
    codes = torch.as_tensor(bond_codes).to(device=dev, dtype=torch.int64).reshape(-1)
    if codes.numel() != bi.shape[1]:
        raise ValueError("validity_plan: %d bonds but %d bond codes" % (bi.shape[1], codes.numel()))
    x0 = torch.as_tensor(coords0).detach().to(device=dev, dtype=torch.float32).contiguous()
    if x0.dim() != 2 or x0.shape[1] != 3:
        raise ValueError("coords0 must be [N, 3]; got %s" % (tuple(x0.shape),))
    N = x0.shape[0]
    z = torch.as_tensor(atomic_numbers).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(z.shape) != (N,):
        raise ValueError("atomic_numbers must be [%d]; got %s" % (N, tuple(z.shape)))
    rin = None
    if radii is not None:
        rin = torch.as_tensor(radii).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(rin.shape) != (N,):
            raise ValueError("radii must be [%d]; got %s" % (N, tuple(rin.shape)))
    if not float(min_volume) >= 0.0:
        raise ValueError("min_volume must be >= 0")
    aoff = _atom_off(atom_off, dev, N)
    B = aoff.numel() - 1
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= N):
        raise ValueError("bond_index holds atom ids outside [0, %d)" % N)
    aflat = aoffs = acnt = None
    if autos is not None:
        if not torch.equal(autos.atom_off.to(dev), aoff):
            raise ValueError("atom_off does not match the ligands of `autos`")
        aflat, aoffs = autos.flat.contiguous(), autos.off.contiguous()
        acnt = torch.where(autos.status == 0, autos.count, torch.zeros_like(autos.count)).contiguous()
    nptr, nidx, ncode, _ = _coded_neighbour_lists(bi, codes, max(N, 1))
    counts = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    K.validity_plan_pass(nptr, nidx, ncode, aoff, B, z, x0, rin, min_volume, aflat, aoffs, acnt, counts, status)
    offs = torch.zeros(4, B + 1, dtype=torch.int32, device=dev)
    offs[:, 1:] = torch.cumsum(counts.t(), 1)
    n_b = torch.diff(aoff)
    top = torch.where(status == 0, n_b, torch.zeros_like(n_b)).max().reshape(1) if B else torch.zeros(1, dtype=torch.int32, device=dev)
    host = torch.cat([offs[:, -1], top, status]).cpu().numpy()       # the one read-back: the four totals, the largest ligand, statuses
    bad = np.nonzero(host[5:])[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("validity_plan: " + "; ".join("ligand %d: status %d (%s)" % (b, host[5 + b], STATUS[int(host[5 + b])])
                                                          for b in bad))
    P, G, A, C = (int(v) for v in host[:4])
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    plan = ValidityPlan(atom_off=aoff, status=status, cls=torch.zeros(N, 16, dtype=torch.int32, device=dev),
                        radii=torch.zeros(N, dtype=torch.float32, device=dev), offs=offs, pair_ij=i32(P, 2), pair_kind=i32(P),
                        pair_d0=torch.empty(P, dtype=torch.float64, device=dev), group=i32(G, 3), group_atoms=i32(A), centre=i32(C, 5),
                        centre_v0=torch.empty(C, dtype=torch.float64, device=dev), max_atoms=int(host[4]))
    if B:
        K.validity_plan_pass(nptr, nidx, ncode, aoff, B, z, x0, rin, min_volume, aflat, aoffs, acnt, counts, status, offs, plan.cls,
                             plan.radii, plan.pair_ij, plan.pair_kind, plan.pair_d0, plan.group, plan.group_atoms, plan.centre,
                             plan.centre_v0)
    return plan


def _pair(v, what):
    lo, hi = (float(x) for x in v)
    if not lo <= hi:
        raise ValueError("%s must be (low, high) with low <= high" % what)
    return lo, hi


def check_poses(poses, plan, pocket_xyz=None, pocket_batch=None, bond_tol=(0.75, 1.25), angle_tol=(0.75, 1.25), clash_min=0.7,
                flat_max=0.25, ca_min=None):
    """The validity statistics and flags of every pose of every ligand (csrc/pose_check.hip), one launch whatever S.

    poses: [S, N, 3] (or [N, 3]) on the HIP device, the layout `poses.pairwise_rmsd` takes; plan: the `validity_plan` of the same
    ligands.  pocket_xyz: [R, 3] C-alpha coordinates with pocket_batch: sorted complex id per residue [R] (a complex may have none).
    stats [B, S, 9] (an empty set gives the value in brackets):
      0 bond_lo / 1 bond_hi    min / max of d / d0 over the bonded pairs                                  [+inf / -inf]
      2 angle_lo / 3 angle_hi  the same over the pairs two bonds apart                                    [+inf / -inf]
      4 clash                  min over the clash pairs of d / (r_i + r_j)                                [+inf]
      5 flat_aromatic          largest distance of an atom of an aromatic system from the system's least-squares plane (through
      6 flat_double            the centroid, normal = eigenvector of the smallest eigenvalue of the covariance); double-bond groups [0]
      7 chirality              min over the stereo centres of V_pose / V0: 1 unchanged, negative inverted   [+inf]
      8 ca_dist                min distance of a ligand atom to a C-alpha atom of its complex              [+inf]
    flags: BOND 1 (bond_lo < bond_tol[0] or bond_hi > bond_tol[1]), ANGLE 2 (likewise under angle_tol), CLASH 4 (clash < clash_min),
    AROMATIC_FLAT 8 / DOUBLE_FLAT 16 (> flat_max), CHIRALITY 32 (chirality <= 0), PROTEIN 64 (ca_min is not None and ca_dist < ca_min),
    NONFINITE 128 (a NaN or infinite coordinate: every statistic NaN, no other bit), UNCHECKED 256 (plan status != 0: every
    statistic NaN, no other bit).  The defaults are PoseBusters' thresholds, applied to ratios against the start conformer; ca_min
    has none because this project has measured no value for it.  One host read-back checks the plan's offsets and pocket_batch (the
    kernel indexes with them) before the launch.  -> PoseValidity."""
    if not torch.is_tensor(poses) or not poses.is_cuda:
        raise RuntimeError("fabind_amd: check_poses runs on a HIP device only (no CPU fallback)")
    dev = poses.device
    p = poses.detach().to(torch.float32)
    if p.dim() == 2:
        p = p[None]
    N = int(plan.cls.shape[0])
    if p.dim() != 3 or tuple(p.shape[1:]) != (N, 3):
        raise ValueError("poses must be [S, %d, 3] or [%d, 3]; got %s" % (N, N, tuple(poses.shape)))
    p = p.contiguous()
    S, B = p.shape[0], plan.atom_off.numel() - 1
    P, G, A, C = plan.pair_ij.shape[0], plan.group.shape[0], plan.group_atoms.shape[0], plan.centre.shape[0]
    lists = (plan.atom_off, plan.status, plan.cls, plan.radii, plan.offs, plan.pair_ij, plan.pair_kind, plan.pair_d0, plan.group,
             plan.group_atoms, plan.centre, plan.centre_v0)
    if (any(t.device != dev or not t.is_contiguous() for t in lists) or tuple(plan.offs.shape) != (4, B + 1) or plan.offs.dtype != torch.int32
            or tuple(plan.status.shape) != (B,) or tuple(plan.cls.shape) != (N, 16) or tuple(plan.radii.shape) != (N,)
            or tuple(plan.pair_ij.shape) != (P, 2) or tuple(plan.pair_kind.shape) != (P,) or tuple(plan.pair_d0.shape) != (P,)
            or tuple(plan.group.shape) != (G, 3) or tuple(plan.centre.shape) != (C, 5) or tuple(plan.centre_v0.shape) != (C,)
            or plan.pair_d0.dtype != torch.float64 or plan.centre_v0.dtype != torch.float64 or plan.radii.dtype != torch.float32
            or any(t.dtype != torch.int32 for t in (plan.atom_off, plan.status, plan.cls, plan.pair_ij, plan.pair_kind, plan.group,
                                                    plan.group_atoms, plan.centre))
            or not 0 <= int(plan.max_atoms) <= MAX_ATOMS):
        raise ValueError("inconsistent ValidityPlan")
    blo, bhi = _pair(bond_tol, "bond_tol")
    alo, ahi = _pair(angle_tol, "angle_tol")
    pocket = poff = None
    if pocket_xyz is not None:
        if pocket_batch is None:
            raise ValueError("pocket_xyz needs pocket_batch")
        pocket = torch.as_tensor(pocket_xyz).detach().to(device=dev, dtype=torch.float32).contiguous()
        pb = torch.as_tensor(pocket_batch).to(dev).long().reshape(-1)
        if pocket.dim() != 2 or pocket.shape[1] != 3 or pb.numel() != pocket.shape[0]:
            raise ValueError("pocket_xyz must be [R, 3] and pocket_batch [R]; got %s and %s" % (tuple(pocket.shape), tuple(pb.shape)))
        poff = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        if pb.numel():
            cnt = torch.bincount(pb.clamp(min=0), minlength=B)        # (validated by the read-back below)
            poff[1:] = torch.cumsum(cnt[:B], 0).to(torch.int32)
    stats = torch.full((B, S, 9), float("nan"), dtype=torch.float32, device=dev)
    flags = torch.full((B, S), UNCHECKED, dtype=torch.int32, device=dev)
    if B and S:
        # the kernel indexes the four lists with offs and the residues with pocket_off: checked on the host, one read-back
        ok = [(plan.offs[:, 0] == 0).all(), (plan.offs[:, 1:] >= plan.offs[:, :-1]).all(),
              (plan.offs[:, -1] == torch.tensor([P, G, A, C], dtype=torch.int32, device=dev)).all(),
              (plan.status != 0).all()]
        if pocket is not None and pocket.shape[0]:
            ok += [(pb >= 0).all(), (pb < B).all(), (pb[1:] >= pb[:-1]).all()]
        ok = torch.stack(ok).cpu().numpy()
        if not ok[:3].all():
            raise ValueError("inconsistent ValidityPlan")
        if len(ok) > 4 and not ok[4:].all():
            raise ValueError("pocket_batch must be sorted complex ids in [0, %d)" % B)
        if not ok[3]:                                                 # at least one ligand is checked (else: the prefill stands)
            K.pose_check(p, plan.atom_off, B, plan.max_atoms, plan.status, plan.cls, plan.radii, plan.offs, plan.pair_ij, plan.pair_kind,
                         plan.pair_d0, plan.group, plan.group_atoms, plan.centre, plan.centre_v0, pocket, poff,
                         (blo, bhi, alo, ahi, clash_min, flat_max, 0.0 if ca_min is None else ca_min), ca_min is not None, stats, flags)
    return PoseValidity(stats=stats, flags=flags, valid=(flags == 0) | (flags == UNCHECKED))


# ------------------------------------------------------------------------------------------------ poses against the whole protein
GRID_STATUS = {0: "ok", 6: "a non-finite protein coordinate", 7: "a cell box of more than 2^20 cells"}
MAX_CELLS = 1 << 20
CELL_CLAMP = 1 << 29
PROTEIN_STATS = ("prot_clash", "prot_dist", "overlap")
PROTEIN_COUNTS = ("n_close", "n_lig", "n_both")
PROTEIN_CLASH, PROTEIN_OVERLAP = 1, 2
PROTEIN_FLAGS = {"PROTEIN_CLASH": PROTEIN_CLASH, "PROTEIN_OVERLAP": PROTEIN_OVERLAP, "NONFINITE": NONFINITE, "UNCHECKED": UNCHECKED}
MAX_LATTICE_REACH = 16.0      # vdw_scale * (largest ligand radius) / spacing: bounds the candidates of one atom's bounding cube


@dataclass
class ProteinGrid:
    """The cell list of the kept (Z > 1) atoms of every complex's protein, all on the device (`protein_grid`).  The cell of an atom along
    an axis is floor(float64(x) / float64(edge)), clamped to +-2^29; a complex's box is origin (the lowest cell) and dims, its cells are
    numbered x fastest.
    prot_off: int32 [B + 1] as given; status: int32 [B], a key of GRID_STATUS (a complex with status != 0 has origin = dims = 0, no
    cells and no entries; its poses are UNCHECKED).  origin, dims: int32 [B, 3].  cell_off: int32 [B + 1], the complex's slot of cells;
    atom_off: int32 [B + 1], its slot of kept atoms.  cell_ptr: int32 [cells + 1]: cell c of complex b holds the sorted atoms
    cell_ptr[cell_off[b] + c] .. cell_ptr[cell_off[b] + c + 1] (positions in xyz / radii / atom_id; minus atom_off[b] they are local).
    xyz: float32 [K, 3], radii: float32 [K], atom_id: int32 [K] (the id within the complex, hydrogens counted): the kept atoms ordered
    by (complex, cell, id).  Ids, origin and dims are LOCAL to the complex: its entries are the same bits alone and in any batch.
    edge: the float32 cell edge as a python float; max_radius: the largest radius (python float, from the one read-back)."""
    prot_off: torch.Tensor
    status: torch.Tensor
    origin: torch.Tensor
    dims: torch.Tensor
    cell_off: torch.Tensor
    atom_off: torch.Tensor
    cell_ptr: torch.Tensor
    xyz: torch.Tensor
    radii: torch.Tensor
    atom_id: torch.Tensor
    edge: float = 5.0
    max_radius: float = 0.0


@dataclass
class ProteinContacts:
    """stats: float32 [B, S, 3], columns PROTEIN_STATS; counts: int32 [B, S, 3], columns PROTEIN_COUNTS; pair: int32 [B, S, 2] = the
    (ligand atom, protein atom) of the prot_clash minimum, ids local to the complex, (-1, -1) without a pair; flags: int32 [B, S], bits
    PROTEIN_FLAGS; ok: bool [B, S] = no flag, or UNCHECKED alone."""
    stats: torch.Tensor
    counts: torch.Tensor
    pair: torch.Tensor
    flags: torch.Tensor
    ok: torch.Tensor


def _f32(v):
    return float(np.float32(v))


def protein_grid(prot_xyz, prot_z, prot_off, radii=None, edge=5.0, on_overflow="raise"):
    """The cell list of every complex's protein heavy atoms (csrc/protein_contacts.hip), built once per protein: the poses of every
    sampling round reuse it.

    prot_xyz: float32 [M, 3] on the HIP device, in the frame of the poses; prot_z: int [M] atomic numbers (atoms with Z <= 1 are
    dropped); prot_off: [B + 1], a complex may have no atoms (`protein_atoms_from_pdb` reads the three from a PDB file).
    radii: float [M] or None for Bondi's by atomic number, the table of `validity_plan` (pass covalent radii for ions if wanted); finite
    and >= 0.  edge: the cell edge (A), rounded to float32; at least the `cutoff` of `check_poses_protein` and vdw_scale times the
    largest radius.
    on_overflow: "raise" -> RuntimeError naming every complex with status != 0 (6: a non-finite coordinate, of any atom; 7: a box of more
    than 2^20 cells); "skip" -> such complexes keep their status, have no entries and their poses are reported UNCHECKED.
    -> ProteinGrid.  Two native calls (count, then write): one host read-back sizes the lists."""
    if on_overflow not in ("raise", "skip"):
        raise ValueError("on_overflow must be 'raise' or 'skip'")
    if not torch.is_tensor(prot_xyz) or not prot_xyz.is_cuda:
        raise RuntimeError("fabind_amd: protein_grid runs on a HIP device only (no CPU fallback)")
    dev = prot_xyz.device
    x = prot_xyz.detach().to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("prot_xyz must be [M, 3]; got %s" % (tuple(x.shape),))
    M = x.shape[0]
    z = torch.as_tensor(prot_z).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(z.shape) != (M,):
        raise ValueError("prot_z must be [%d]; got %s" % (M, tuple(z.shape)))
    rin = None
    if radii is not None:
        rin = torch.as_tensor(radii).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(rin.shape) != (M,):
            raise ValueError("radii must be [%d]; got %s" % (M, tuple(rin.shape)))
    edge = _f32(edge)
    if not 0.0 < edge < float("inf"):
        raise ValueError("edge must be positive and finite")
    poff = _atom_off(prot_off, dev, M)
    B = poff.numel() - 1
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    origin, dims, status, counts = i32(B, 3), i32(B, 3), i32(B), i32(B, 2)
    K.protein_grid_pass(x, z, poff, B, rin, edge, origin, dims, status, counts)
    cell_off, kept_off = K.exclusive_scan(counts[:, 0].contiguous()), K.exclusive_scan(counts[:, 1].contiguous())
    rbad = torch.zeros(1, dtype=torch.int32, device=dev) if rin is None else (~((rin >= 0) & (rin < float("inf")))).any().to(torch.int32).reshape(1)
    host = torch.cat([cell_off[-1:], kept_off[-1:], rbad, status]).cpu().numpy()   # the one read-back: two totals, the radii, the statuses
    if host[2]:
        raise ValueError("radii must be finite and >= 0")
    bad = np.nonzero(host[3:])[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("protein_grid: " + "; ".join("complex %d: status %d (%s)" % (b, host[3 + b], GRID_STATUS[int(host[3 + b])])
                                                         for b in bad))
    C, Kk = int(host[0]), int(host[1])
    grid = ProteinGrid(prot_off=poff, status=status, origin=origin, dims=dims, cell_off=cell_off, atom_off=kept_off, cell_ptr=i32(C + 1),
                       xyz=torch.zeros(Kk, 3, dtype=torch.float32, device=dev), radii=torch.zeros(Kk, dtype=torch.float32, device=dev),
                       atom_id=i32(Kk), edge=edge)
    if B:
        K.protein_grid_pass(x, z, poff, B, rin, edge, origin, dims, status, None, cell_off, kept_off, C, Kk, i32(max(M, 1)), i32(max(C, 1)),
                            i32(max(Kk, 1)), grid.cell_ptr, grid.xyz, grid.radii, grid.atom_id)
    grid.max_radius = float(grid.radii.max()) if Kk else 0.0
    return grid


def check_poses_protein(poses, plan, grid, cutoff=5.0, clash_min=0.75, overlap_max=0.075, vdw_scale=0.8, spacing=0.5):
    """Every pose of every ligand against ALL heavy atoms of its protein (csrc/protein_contacts.hip), one launch whatever S: does the
    pose sit inside the protein?

    poses: [S, N, 3] (or [N, 3]) on the HIP device; plan: the `validity_plan` of the same ligands (its atom_off, radii and status are
    used); grid: the `protein_grid` of the same complexes, in the same frame.
    stats [B, S, 3] (an empty set gives the value in brackets):
      0 prot_clash  min of d / (r_i + r_j) over the ligand-protein pairs with d^2 < cutoff^2 (compared in float64)          [+inf]
      1 prot_dist   min of d over the same pairs                                                                           [+inf]
      2 overlap     n_both / n_lig on the lattice of the points spacing * k, k an integer vector: a point is a ligand point when
                    d^2 <= (vdw_scale * r_i)^2 for some ligand atom, a protein point when the same holds for some kept protein atom;
                    n_lig counts every ligand point once, n_both those that are protein points as well                     [0]
    counts [B, S, 3] = (n_close: the pairs with ratio < clash_min, n_lig, n_both); pair [B, S, 2]: the pair of the prot_clash
    minimum, ties to the lowest ligand id, then the lowest protein id (its id within the complex, hydrogens counted).
    flags: PROTEIN_CLASH 1 (prot_clash < clash_min), PROTEIN_OVERLAP 2 (overlap > overlap_max), NONFINITE 128 (a NaN or infinite
    coordinate: every statistic NaN, no other bit), UNCHECKED 256 (plan status or grid status != 0: every statistic NaN, no other
    bit); bits of PROTEIN_FLAGS, a table apart from FLAGS.  ok = no flag, or UNCHECKED alone.
    The defaults are PoseBusters' (0.75 of the radius sum, 7.5 % of the volume, radii scaled by 0.8, 0.5 A lattice).  Where this differs
    from PoseBusters: Bondi radii instead of RDKit's table; ONE set of atoms instead of separate protein / organic cofactor / inorganic
    cofactor / water tests with thresholds of their own (pass the atoms wanted, and covalent radii for ions); the lattice is anchored at
    the origin of the complex's frame instead of the molecule's bounding box, so a result does not depend on the batch (and moves with
    the frame by up to the lattice's resolution); hydrogens take no part.  Needs cutoff <= grid.edge and vdw_scale * (largest protein
    radius) <= grid.edge (the 27 cells around a point then hold every atom that can reach it), and vdw_scale * (largest ligand radius)
    <= 16 spacing.  One host read-back checks the grid's offsets (the kernel indexes with them) and the ligand radii before the launch.
    Combine with the molecule's own checks as `PoseValidity.valid & ProteinContacts.ok`; the selectors of `plus.metrics` take
    `(validity.valid & contacts.ok).t()` as their [S, B] `valid` mask.  DESIGN.md section 18.  -> ProteinContacts."""
    if not torch.is_tensor(poses) or not poses.is_cuda:
        raise RuntimeError("fabind_amd: check_poses_protein runs on a HIP device only (no CPU fallback)")
    dev = poses.device
    p = poses.detach().to(torch.float32)
    if p.dim() == 2:
        p = p[None]
    N = int(plan.radii.shape[0])
    if p.dim() != 3 or tuple(p.shape[1:]) != (N, 3):
        raise ValueError("poses must be [S, %d, 3] or [%d, 3]; got %s" % (N, N, tuple(poses.shape)))
    p = p.contiguous()
    S, B = p.shape[0], plan.atom_off.numel() - 1
    cutoff, clash_min, overlap_max, vdw_scale, spacing = (_f32(v) for v in (cutoff, clash_min, overlap_max, vdw_scale, spacing))
    if not 0.0 <= cutoff < float("inf"):
        raise ValueError("cutoff must be finite and >= 0")
    if grid.edge < cutoff:
        raise ValueError("the grid's edge (%g) is smaller than cutoff (%g): build the grid with edge >= cutoff" % (grid.edge, cutoff))
    if not (0.0 < spacing < float("inf") and 0.0 <= vdw_scale < float("inf")):
        raise ValueError("spacing must be positive and vdw_scale >= 0, both finite")
    if not vdw_scale * grid.max_radius <= grid.edge:
        raise ValueError("vdw_scale * the largest protein radius (%g) exceeds the grid's edge (%g)" % (vdw_scale * grid.max_radius, grid.edge))
    C, Kk = grid.cell_ptr.numel() - 1, grid.xyz.shape[0]
    ints = (plan.atom_off, plan.status, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr, grid.atom_id)
    if (any(t.device != dev or not t.is_contiguous() for t in ints + (plan.radii, grid.xyz, grid.radii))
            or any(t.dtype != torch.int32 for t in ints) or any(t.dtype != torch.float32 for t in (plan.radii, grid.xyz, grid.radii))
            or tuple(plan.status.shape) != (B,) or not 0 <= int(plan.max_atoms) <= MAX_ATOMS
            or tuple(grid.status.shape) != (B,) or tuple(grid.origin.shape) != (B, 3) or tuple(grid.dims.shape) != (B, 3)
            or tuple(grid.cell_off.shape) != (B + 1,) or tuple(grid.atom_off.shape) != (B + 1,) or C < 0
            or tuple(grid.xyz.shape) != (Kk, 3) or tuple(grid.radii.shape) != (Kk,) or tuple(grid.atom_id.shape) != (Kk,)):
        raise ValueError("inconsistent ValidityPlan or ProteinGrid (the grid must hold the complexes of the plan's ligands)")
    stats = torch.full((B, S, 3), float("nan"), dtype=torch.float32, device=dev)
    counts = torch.zeros((B, S, 3), dtype=torch.int32, device=dev)
    pair = torch.full((B, S, 2), -1, dtype=torch.int32, device=dev)
    flags = torch.full((B, S), UNCHECKED, dtype=torch.int32, device=dev)
    if B and S:
        # the kernel indexes the cells and the sorted atoms with these: checked on the host, one read-back
        live = (plan.status == 0) & (grid.status == 0)
        n_b = torch.diff(plan.atom_off)
        rl = plan.radii
        ok = [(plan.atom_off[0] == 0), (n_b >= 0).all(), (plan.atom_off[-1] == N),
              (grid.cell_off[0] == 0), (torch.diff(grid.cell_off) >= 0).all(), (grid.cell_off[-1] == C),
              (grid.atom_off[0] == 0), (torch.diff(grid.atom_off) >= 0).all(), (grid.atom_off[-1] == Kk),
              (grid.cell_ptr[0] == 0), (torch.diff(grid.cell_ptr) >= 0).all(), (grid.cell_ptr[-1] == Kk),
              (grid.dims >= 0).all(), (grid.dims.long().prod(1) == torch.diff(grid.cell_off)).all(),
              ((rl >= 0) & (vdw_scale * rl <= MAX_LATTICE_REACH * spacing)).all() if rl.numel() else torch.ones((), dtype=torch.bool, device=dev),
              live.any()]
        ok = torch.stack([o.reshape(()) for o in ok]).cpu().numpy()
        if not ok[:14].all():
            raise ValueError("inconsistent ValidityPlan or ProteinGrid (the grid must hold the complexes of the plan's ligands)")
        if not ok[14]:
            raise ValueError("ligand radii must be finite, >= 0 and vdw_scale * radius <= %g * spacing" % MAX_LATTICE_REACH)
        if ok[15]:                                                    # at least one complex is checked (else: the prefill stands)
            K.pose_protein_check(p, plan.atom_off, B, plan.max_atoms, plan.status, plan.radii, grid.status, grid.origin, grid.dims,
                                 grid.cell_off, grid.atom_off, grid.cell_ptr, grid.xyz, grid.radii, grid.atom_id, grid.edge,
                                 (cutoff, clash_min, overlap_max, vdw_scale, spacing), grid.max_radius, stats, counts, pair, flags)
    return ProteinContacts(stats=stats, counts=counts, pair=pair, flags=flags, ok=(flags == 0) | (flags == UNCHECKED))


_PDB_ELEMENTS = ("H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar", "K", "Ca", "Sc", "Ti", "V",
                 "Cr", "Mn", "Fe", "Co", "Ni", "Cu", "Zn", "Ga", "Ge", "As", "Se", "Br", "Kr", "Rb", "Sr", "Y", "Zr", "Nb", "Mo", "Tc", "Ru", "Rh",
                 "Pd", "Ag", "Cd", "In", "Sn", "Sb", "Te", "I", "Xe", "Cs", "Ba", "La", "Ce", "Pr", "Nd", "Pm", "Sm", "Eu", "Gd", "Tb", "Dy", "Ho",
                 "Er", "Tm", "Yb", "Lu", "Hf", "Ta", "W", "Re", "Os", "Ir", "Pt", "Au", "Hg", "Tl", "Pb", "Bi")
_PDB_Z = {s.upper(): i + 1 for i, s in enumerate(_PDB_ELEMENTS)}
_PDB_Z["D"] = 1
_PDB_WATER = ("HOH", "WAT", "H2O", "DOD", "D2O", "TIP", "TIP3", "SOL")


def _pdb_element(line, hetero):
    sym = line[76:78].strip().upper() if len(line) >= 78 else ""
    if sym in _PDB_Z:
        return _PDB_Z[sym]
    name = line[12:16]
    letters = "".join(c for c in name if c.isalpha()).upper()
    if not letters:
        return 0
    # the atom name: an element of two letters starts in column 13 (" CA " is a carbon, "CA  " calcium; "FE  ", "ZN  "); in ATOM
    # records a letter in column 13 before a one-letter element is a remoteness or hydrogen prefix ("HG21", "1HB ")
    if name[0].isalpha() and hetero and letters[:2] in _PDB_Z:
        return _PDB_Z[letters[:2]]
    if name[0].isalpha() and not hetero and letters[0] in ("H", "D"):
        return 1
    if name[0].isdigit() and letters[0] in ("H", "D"):
        return 1
    return _PDB_Z.get(letters[0], 0)


def protein_atoms_from_pdb(text, keep_water=False, keep_hydrogens=False):
    """The atoms of the ATOM / HETATM records of a PDB file's text, read by fixed columns (pure Python): coordinates from columns
    31-54, the element from columns 77-78, falling back to the atom name (columns 13-16).  Only the first MODEL is read; of alternate
    locations (column 17) the blank one, "A" or "1" is kept.  Waters (HOH, WAT, DOD, ...) and hydrogens are dropped unless asked for.
    An element that cannot be read gives Z = 0, which `protein_grid` drops like a hydrogen.
    -> (xyz float32 [M, 3], z int32 [M], is_hetero bool [M]) numpy arrays, ready for `protein_grid` once on the device."""
    xyz, zs, het = [], [], []
    for line in text.splitlines():
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec not in ("ATOM  ", "HETATM"):
            continue
        if len(line) < 54 or line[16] not in " A1":
            continue
        hetero = rec == "HETATM"
        if not keep_water and line[17:20].strip().upper() in _PDB_WATER:
            continue
        zi = _pdb_element(line, hetero)
        if zi == 1 and not keep_hydrogens:
            continue
        try:
            c = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
        except ValueError:
            raise ValueError("protein_atoms_from_pdb: unreadable coordinates in %r" % line)
        xyz.append(c)
        zs.append(zi)
        het.append(hetero)
    return (np.asarray(xyz, dtype=np.float32).reshape(-1, 3), np.asarray(zs, dtype=np.int32), np.asarray(het, dtype=bool))
