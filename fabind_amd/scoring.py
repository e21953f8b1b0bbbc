"""A Vina-style intermolecular energy of sampled poses on the device (csrc/pose_score.hip; no counterpart in
the reference, whose only ranking signal is FABind+'s confidence head).

The steps of sections 15-21 filter and repair sampled poses; this one gives every surviving pose a physics-based number: AutoDock
Vina 1.1.2's intermolecular function (Trott, Olson 2010) over heavy atoms, with X-Score atom roles (Wang, Lai, Wang 2002).  Energies
only: no gradients, no pose moves, no intramolecular term.

* `ligand_types` / `hydrogen_counts_from_sdf`: the type word of every ligand atom from the bond list (torch index operations).
* `protein_types_from_pdb` / `protein_types_from_elements`: the type word of every protein atom, from a (residue, atom name) table of
  the 20 standard residues or from the element alone (pure Python / numpy).
* `score_poses`: the energy of every (complex, pose), one launch whatever S, through the cell list of `validity.protein_grid`.

A type word is an int32: bits 0-3 the radius class (RADIUS_CLASSES / RADII), HYDROPHOBIC 16, DONOR 32, ACCEPTOR 64.

The constants are the published ones, written down from the literature; no Vina binary exists where this project runs, so agreement
with Vina itself is NOT measured.  The float64 restatement of tests/score_refs.py is the definition the kernel is held to."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .conformer import _coded_neighbour_lists
from .symmetry import bond_code
from .validity import NONFINITE, UNCHECKED, MAX_ATOMS, _PDB_WATER, _PDB_Z, _f32, _pdb_element

RADIUS_CLASSES = ("C", "N", "O", "P", "S", "F", "Cl", "Br", "I", "metal")
RADII = (1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2)            # A, X-Score; every other element is scored as a metal
CLASS_MASK, HYDROPHOBIC, DONOR, ACCEPTOR = 15, 16, 32, 64
METAL_CLASS = 9
TERMS = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
VINA_WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
SCORE_FLAGS = {"NONFINITE": NONFINITE, "UNCHECKED": UNCHECKED}
_CLASS_OF_Z = {6: 0, 7: 1, 8: 2, 15: 3, 16: 4, 9: 5, 17: 6, 35: 7, 53: 8}
HALOGENS = (9, 17, 35, 53)
# the elements scored as metals WITH the donor role (an element outside every list has the metal radius and no role)
METALS = (3, 4, 11, 12, 13, 19, 20) + tuple(range(21, 32)) + (37, 38) + tuple(range(39, 51)) + (55, 56) + tuple(range(57, 84))
_MAX_Z = 118


def _element_table():
    """int32 [_MAX_Z + 1]: the type word of an element before any rule that needs the bonds: the radius class, halogens hydrophobic,
    metals donors, O an acceptor.  Carbon and nitrogen carry no role here: `ligand_types` and the residue table add theirs."""
    t = np.full(_MAX_Z + 1, METAL_CLASS, np.int32)
    for z, c in _CLASS_OF_Z.items():
        t[z] = c
    for z in HALOGENS:
        t[z] |= HYDROPHOBIC
    for z in METALS:
        t[z] |= DONOR
    t[8] |= ACCEPTOR
    return t


_ELEMENT_TABLE = _element_table()


# ------------------------------------------------------------------------------------------------ ligand typing
def ligand_types(bond_index, bond_codes, atomic_numbers, atom_off, n_hydrogens=None, formal_charge=None):
    """The type word of every ligand atom (heavy atoms; a hydrogen in the list would be scored as an atom of the metal radius).

    bond_index: [2, E] GLOBAL atom ids, each bond once, in both directions or repeated; bond_codes: [E], `symmetry.bond_code` coding
    (AROMATIC 1 = order 1.5, TRIPLE 2 = 3, DOUBLE 3 = 2, SINGLE 4 and anything else = 1; names are accepted); atomic_numbers: int [N];
    atom_off: [B + 1], only its last entry is looked at when it is given on the host (bonds never cross ligands, so the typing does
    not need the offsets); n_hydrogens: int [N] hydrogens on every atom, or None; formal_charge: int [N] or None (0).
    Rules: carbon is HYDROPHOBIC iff no bonded atom has Z other than 1 and 6; F, Cl, Br, I are HYDROPHOBIC; a metal is a DONOR; every O
    is an ACCEPTOR; N or O with at least one hydrogen is a DONOR, the hydrogen count being n_hydrogens when given, else the hydrogens
    bonded in the list plus max(0, v0 + charge - floor(sum of bond orders)) with v0 = 3 for N and 2 for O; N is an ACCEPTOR iff it has
    no hydrogen, charge <= 0, floor(sum of orders) <= 3 and it is aromatic or has a double or triple bond (pyridine, imine, nitrile:
    amines and amide nitrogens are not acceptors).  A documented limit: an aromatic-CODED N-H (a pyrrole written with aromatic bonds)
    comes out without its hydrogen, hence as an acceptor, unless n_hydrogens is passed; Kekule input is unambiguous.
    -> int32 [N] on the device of atomic_numbers.  torch index operations only, nothing is read back."""
    z = torch.as_tensor(atomic_numbers)
    dev = z.device
    z = z.to(torch.int64).reshape(-1)
    N = z.numel()
    if not torch.is_tensor(atom_off) and len(atom_off) and int(atom_off[-1]) != N:
        raise ValueError("atom_off ends at %d but there are %d atoms" % (int(atom_off[-1]), N))
    bi = torch.as_tensor(bond_index).to(device=dev, dtype=torch.int64).reshape(2, -1)
    if not torch.is_tensor(bond_codes) and len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [bond_code(t) for t in bond_codes]
    codes = torch.as_tensor(bond_codes).to(device=dev, dtype=torch.int64).reshape(-1)
    if codes.numel() != bi.shape[1]:
        raise ValueError("ligand_types: %d bonds but %d bond codes" % (bi.shape[1], codes.numel()))
    charge = torch.zeros(N, dtype=torch.int64, device=dev) if formal_charge is None else \
        torch.as_tensor(formal_charge).to(device=dev, dtype=torch.int64).reshape(-1)
    if charge.numel() != N:
        raise ValueError("formal_charge must be [%d]" % N)
    # every bond once per direction, a bond listed several times taking its smallest code
    _, other, code, owner = _coded_neighbour_lists(bi, codes, max(N, 1))
    owner, other, code = owner.long(), other.long(), code.long()
    twice = torch.where(code == 1, 3, torch.where(code == 2, 6, torch.where(code == 3, 4, 2)))      # twice the bond order: integers
    zero = torch.zeros(N, dtype=torch.int64, device=dev)
    order2 = zero.clone().index_add_(0, owner, twice)
    zo = z[other]
    hetero = zero.clone().index_add_(0, owner, ((zo != 1) & (zo != 6)).to(torch.int64)) > 0
    multiple = zero.clone().index_add_(0, owner, (code <= 3).to(torch.int64)) > 0
    floor_order = torch.div(order2, 2, rounding_mode="floor")
    if n_hydrogens is None:
        bonded_h = zero.clone().index_add_(0, owner, (zo == 1).to(torch.int64))
        v0 = torch.where(z == 7, 3, 2)
        nh = bonded_h + torch.clamp(v0 + charge - floor_order, min=0)
    else:
        nh = torch.as_tensor(n_hydrogens).to(device=dev, dtype=torch.int64).reshape(-1)
        if nh.numel() != N:
            raise ValueError("n_hydrogens must be [%d]" % N)
    table = torch.as_tensor(_ELEMENT_TABLE, device=dev).to(torch.int64)
    t = table[z.clamp(0, _MAX_Z)]
    is_n, is_o = z == 7, z == 8
    t = t | torch.where((z == 6) & ~hetero, HYDROPHOBIC, 0)
    t = t | torch.where((is_n | is_o) & (nh > 0), DONOR, 0)
    t = t | torch.where(is_n & (nh == 0) & (charge <= 0) & (floor_order <= 3) & multiple, ACCEPTOR, 0)
    return t.to(torch.int32)


def hydrogen_counts_from_sdf(text):
    """The explicit-hydrogen count of every heavy atom of the first molecule of an SDF / MOL file's text (V2000, fixed columns; pure
    Python), in the atom order of `embed.molecule_from_sdf`: the `n_hydrogens` of `ligand_types` for a file that lists its hydrogens.
    -> int32 [n] numpy array."""
    lines = text.splitlines()
    if len(lines) < 4:
        raise ValueError("hydrogen_counts_from_sdf: no counts line")
    counts = lines[3]
    if "V3000" in counts:
        raise ValueError("hydrogen_counts_from_sdf: V3000 files are not read")
    try:
        na, nbd = int(counts[0:3]), int(counts[3:6])
    except ValueError:
        raise ValueError("hydrogen_counts_from_sdf: unreadable counts line %r" % counts)
    if len(lines) < 4 + na + nbd:
        raise ValueError("hydrogen_counts_from_sdf: the file ends inside the atom or bond block")
    zs = [_PDB_Z.get(ln[31:34].strip().upper(), 0) for ln in lines[4:4 + na]]
    nh = [0] * na
    for ln in lines[4 + na:4 + na + nbd]:
        try:
            a, b = int(ln[0:3]) - 1, int(ln[3:6]) - 1
        except ValueError:
            raise ValueError("hydrogen_counts_from_sdf: unreadable bond line %r" % ln)
        if not (0 <= a < na and 0 <= b < na):
            raise ValueError("hydrogen_counts_from_sdf: a bond to an atom outside the atom block in %r" % ln)
        if zs[a] == 1 and zs[b] != 1:
            nh[b] += 1
        if zs[b] == 1 and zs[a] != 1:
            nh[a] += 1
    return np.asarray([nh[i] for i in range(na) if zs[i] != 1], np.int32)


# ------------------------------------------------------------------------------------------------ protein typing
# side-chain heavy-atom bonds of the 20 standard residues (the backbone's N-CA, CA-C, C-O, C-OXT and CA-CB are added to each)
_SIDE_BONDS = {
    "ALA": "", "GLY": "",
    "ARG": "CB-CG CG-CD CD-NE NE-CZ CZ-NH1 CZ-NH2",
    "ASN": "CB-CG CG-OD1 CG-ND2",
    "ASP": "CB-CG CG-OD1 CG-OD2",
    "CYS": "CB-SG",
    "GLN": "CB-CG CG-CD CD-OE1 CD-NE2",
    "GLU": "CB-CG CG-CD CD-OE1 CD-OE2",
    "HIS": "CB-CG CG-ND1 CG-CD2 ND1-CE1 CD2-NE2 CE1-NE2",
    "ILE": "CB-CG1 CB-CG2 CG1-CD1",
    "LEU": "CB-CG CG-CD1 CG-CD2",
    "LYS": "CB-CG CG-CD CD-CE CE-NZ",
    "MET": "CB-CG CG-SD SD-CE",
    "PHE": "CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ",
    "PRO": "CB-CG CG-CD CD-N",
    "SER": "CB-OG",
    "THR": "CB-OG1 CB-CG2",
    "TRP": "CB-CG CG-CD1 CG-CD2 CD1-NE1 NE1-CE2 CD2-CE2 CD2-CE3 CE2-CZ2 CE3-CZ3 CZ2-CH2 CZ3-CH2",
    "TYR": "CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ CZ-OH",
    "VAL": "CB-CG1 CB-CG2",
}
_SIDE_DONORS = {"ARG": ("NE", "NH1", "NH2"), "ASN": ("ND2",), "GLN": ("NE2",), "LYS": ("NZ",), "TRP": ("NE1",), "HIS": ("ND1", "NE2"),
                "SER": ("OG",), "THR": ("OG1",), "TYR": ("OH",)}
_SIDE_N_ACCEPTORS = {"HIS": ("ND1", "NE2")}                              # (every O is an acceptor by its element)


def _residue_table():
    """{(residue, atom name): type word} of the heavy atoms of the 20 standard residues at pH 7, from their standard topology: backbone
    N a donor (not in PRO), O / OXT acceptors, the side-chain donors of _SIDE_DONORS, HIS ND1 and NE2 donor AND acceptor (a stated
    convention: the tautomer is unknown), hydroxyl O donor and acceptor, carboxylate and amide O acceptors, S without a role, and a
    carbon hydrophobic iff the topology bonds it to no N, O or S."""
    table = {}
    for res, side in _SIDE_BONDS.items():
        bonds = [("N", "CA"), ("CA", "C"), ("C", "O"), ("C", "OXT")] + ([("CA", "CB")] if res != "GLY" else [])
        bonds += [tuple(b.split("-")) for b in side.split()]
        nbrs = {}
        for a, b in bonds:
            nbrs.setdefault(a, []).append(b)
            nbrs.setdefault(b, []).append(a)
        for name, others in nbrs.items():
            el = name[0]
            t = int(_ELEMENT_TABLE[_PDB_Z[el]])
            if el == "C" and not any(o[0] in "NOS" for o in others):
                t |= HYDROPHOBIC
            if name == "N" and res != "PRO":
                t |= DONOR
            if name in _SIDE_DONORS.get(res, ()):
                t |= DONOR
            if name in _SIDE_N_ACCEPTORS.get(res, ()):
                t |= ACCEPTOR
            table[(res, name)] = t
    return table


RESIDUE_TYPES = _residue_table()


def protein_types_from_elements(prot_z):
    """The conservative type word by element alone, for callers who have arrays only, and for every atom outside the residue table:
    carbon is NOT hydrophobic, N has no role, O is an acceptor, halogens are hydrophobic, metals are donors, P and S have no role, any
    other element has the metal radius and no role.  prot_z: int [M], a numpy array (-> numpy int32 [M]) or a torch tensor (-> int32
    [M] on its device)."""
    if torch.is_tensor(prot_z):
        z = prot_z.to(torch.int64).reshape(-1).clamp(0, _MAX_Z)
        return torch.as_tensor(_ELEMENT_TABLE, device=z.device)[z].to(torch.int32)
    z = np.clip(np.asarray(prot_z, np.int64).reshape(-1), 0, _MAX_Z)
    return _ELEMENT_TABLE[z].astype(np.int32)


def protein_types_from_pdb(text, keep_water=False):
    """The heavy atoms of a PDB file's text with their type words: the records are filtered exactly as in
    `validity.protein_atoms_from_pdb` with hydrogens kept out, so the first three outputs equal that function's.  An ATOM record of one
    of the 20 standard residues whose atom name is in RESIDUE_TYPES (and whose element agrees) takes the table's word; every other atom
    (HETATM, non-standard residues, unknown names) takes `protein_types_from_elements`'.
    -> (xyz float32 [M, 3], z int32 [M], is_hetero bool [M], types int32 [M]) numpy arrays."""
    xyz, zs, het, types = [], [], [], []
    for line in text.splitlines():
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec not in ("ATOM  ", "HETATM"):
            continue
        if len(line) < 54 or line[16] not in " A1":
            continue
        hetero = rec == "HETATM"
        res = line[17:20].strip().upper()
        if not keep_water and res in _PDB_WATER:
            continue
        zi = _pdb_element(line, hetero)
        if zi == 1:
            continue
        try:
            c = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
        except ValueError:
            raise ValueError("protein_types_from_pdb: unreadable coordinates in %r" % line)
        name = line[12:16].strip().upper()
        t = None if hetero else RESIDUE_TYPES.get((res, name))
        if t is None or 0 <= zi <= _MAX_Z and (t & CLASS_MASK) != (int(_ELEMENT_TABLE[zi]) & CLASS_MASK):
            t = int(_ELEMENT_TABLE[min(max(zi, 0), _MAX_Z)])
        xyz.append(c)
        zs.append(zi)
        het.append(hetero)
        types.append(t)
    return (np.asarray(xyz, dtype=np.float32).reshape(-1, 3), np.asarray(zs, dtype=np.int32), np.asarray(het, dtype=bool),
            np.asarray(types, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the energy
@dataclass
class PoseScores:
    """terms: float32 [B, S, 5], the unweighted sums in the order of TERMS; inter: float32 [B, S] = sum_k w_k term_k; total: float32
    [B, S] = inter / (1 + torsion_weight * n_torsions); n_pairs: int32 [B, S], the pairs within the cutoff; per_atom: float32 [S, N],
    the weighted energy of every ligand atom, or None; flags: int32 [B, S], bits SCORE_FLAGS."""
    terms: torch.Tensor
    inter: torch.Tensor
    total: torch.Tensor
    n_pairs: torch.Tensor
    per_atom: torch.Tensor
    flags: torch.Tensor


def score_poses(poses, atom_off, lig_types, grid, prot_types, n_torsions=None, status=None, weights=VINA_WEIGHTS, cutoff=8.0,
                torsion_weight=0.0585, per_atom=False):
    """The Vina-style intermolecular energy of every pose of every ligand against ALL heavy atoms of its protein
    (csrc/pose_score.hip), one launch whatever S.  Lower is better.

    poses: [S, N, 3] (or [N, 3]) on the HIP device, in the frame of the grid; atom_off: [B + 1] atom offsets of the ligands (at most 256
    atoms each); lig_types: int [N] type words (`ligand_types`); grid: the `validity.protein_grid` ProteinGrid of the same complexes,
    built with edge >= cutoff -- `protein_grid(edge=8.0)` for the default; prot_types: int [M] type words of ALL protein atoms in the
    order the grid was built from, hydrogens included (`protein_types_from_pdb`, `protein_types_from_elements`); n_torsions: int [B]
    rotatable bonds per ligand, or None (0); status: int [B] or None, a ligand with status != 0 is not scored (UNCHECKED).
    Pairs: every (ligand atom i, kept protein atom j) with r^2 < cutoff^2, compared in float64 on the float32 inputs (strict).  With
    d = r - R_i - R_j (radii by class, RADII) the five terms summed over the pairs are
      gauss1 exp(-(d / 0.5)^2), gauss2 exp(-((d - 3) / 2)^2), repulsion d^2 for d < 0,
      hydrophobic (both atoms HYDROPHOBIC): 1 for d < 0.5, 1.5 - d up to 1.5, 0 beyond,
      hbond (a DONOR with an ACCEPTOR, either way): 1 for d < -0.7, -d / 0.7 up to 0, 0 beyond;
    inter = sum_k weights[k] term_k, total = inter / (1 + torsion_weight * n_torsions).  per_atom=True also gives the weighted energy
    of every ligand atom (its sum over a ligand's atoms is inter up to rounding).
    flags: NONFINITE 128 (a NaN or infinite coordinate: every number of that pose NaN, no other pose affected), UNCHECKED 256 (the
    ligand's status or the grid's status != 0: NaN, no pairs).  Not in this: hydrogens as atoms, the intramolecular term, gradients
    and refinement; agreement with Vina itself is not measured.
    One host read-back checks the offsets and ids the kernel indexes with; when no complex is live the prefilled outputs stand.
    -> PoseScores."""
    if not torch.is_tensor(poses) or not poses.is_cuda:
        raise RuntimeError("fabind_amd: score_poses runs on a HIP device only (no CPU fallback)")
    dev = poses.device
    p = poses.detach().to(torch.float32)
    if p.dim() == 2:
        p = p[None]
    lt = torch.as_tensor(lig_types).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    N = lt.numel()
    if p.dim() != 3 or tuple(p.shape[1:]) != (N, 3):
        raise ValueError("poses must be [S, %d, 3] or [%d, 3]; got %s" % (N, N, tuple(poses.shape)))
    p = p.contiguous()
    aoff = torch.as_tensor(atom_off).to(device=dev, dtype=torch.int32).contiguous()
    if aoff.dim() != 1 or aoff.numel() < 1:
        raise ValueError("atom_off must be a [B + 1] offset vector")
    S, B = p.shape[0], aoff.numel() - 1
    cutoff = _f32(cutoff)
    if not 0.0 <= cutoff < float("inf"):
        raise ValueError("cutoff must be finite and >= 0")
    if grid.edge < cutoff:
        raise ValueError("the grid's edge (%g) is smaller than cutoff (%g): build the grid with protein_grid(edge=%.1f)"
                         % (grid.edge, cutoff, max(cutoff, 8.0)))
    w = [float(v) for v in weights]
    if len(w) != 5 or not all(np.isfinite(w)) or not np.isfinite(float(torsion_weight)) or float(torsion_weight) < 0.0:
        raise ValueError("weights must be five finite numbers and torsion_weight finite and >= 0")
    pt = torch.as_tensor(prot_types).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    st = torch.zeros(B, dtype=torch.int32, device=dev) if status is None else \
        torch.as_tensor(status).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    nt = None if n_torsions is None else torch.as_tensor(n_torsions).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    C, Kk = grid.cell_ptr.numel() - 1, grid.xyz.shape[0]
    ints = (grid.prot_off, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr, grid.atom_id)
    if (any(t.device != dev or not t.is_contiguous() for t in ints + (grid.xyz,)) or any(t.dtype != torch.int32 for t in ints)
            or grid.xyz.dtype != torch.float32 or tuple(st.shape) != (B,) or (nt is not None and tuple(nt.shape) != (B,))
            or tuple(grid.prot_off.shape) != (B + 1,) or tuple(grid.status.shape) != (B,) or tuple(grid.origin.shape) != (B, 3)
            or tuple(grid.dims.shape) != (B, 3) or tuple(grid.cell_off.shape) != (B + 1,) or tuple(grid.atom_off.shape) != (B + 1,)
            or C < 0 or tuple(grid.xyz.shape) != (Kk, 3) or tuple(grid.atom_id.shape) != (Kk,)):
        raise ValueError("inconsistent ligands or ProteinGrid (the grid must hold the complexes of the ligands)")
    nan = float("nan")
    terms = torch.full((B, S, 5), nan, dtype=torch.float32, device=dev)
    inter = torch.full((B, S), nan, dtype=torch.float32, device=dev)
    total = torch.full((B, S), nan, dtype=torch.float32, device=dev)
    n_pairs = torch.zeros((B, S), dtype=torch.int32, device=dev)
    flags = torch.full((B, S), UNCHECKED, dtype=torch.int32, device=dev)
    pa = torch.full((S, N), nan, dtype=torch.float32, device=dev) if per_atom else None
    if B and S:
        # the kernel indexes the cells, the sorted atoms and the type words with these: checked on the host, one read-back
        live = (st == 0) & (grid.status == 0)
        n_b = torch.diff(aoff)
        M = pt.numel()
        # the complex of every kept atom, to bound its id by the size of that complex
        per_cplx = torch.diff(grid.atom_off).long()
        size_of = torch.repeat_interleave(torch.diff(grid.prot_off).long(), per_cplx.clamp(min=0)) if Kk else None
        ok = [(aoff[0] == 0) & (n_b >= 0).all() & (aoff[-1] == N),
              (grid.prot_off[0] == 0), (torch.diff(grid.prot_off) >= 0).all(), (grid.prot_off[-1] == M),
              (grid.cell_off[0] == 0), (torch.diff(grid.cell_off) >= 0).all(), (grid.cell_off[-1] == C),
              (grid.atom_off[0] == 0), (per_cplx >= 0).all(), (grid.atom_off[-1] == Kk),
              (grid.cell_ptr[0] == 0), (torch.diff(grid.cell_ptr) >= 0).all(), (grid.cell_ptr[-1] == Kk),
              (grid.dims >= 0).all(), (grid.dims.long().prod(1) == torch.diff(grid.cell_off)).all(),
              ((grid.atom_id >= 0) & (grid.atom_id < size_of)).all() if Kk and size_of.numel() == Kk
              else torch.full((), Kk == 0, dtype=torch.bool, device=dev),
              (nt >= 0).all() if nt is not None else torch.ones((), dtype=torch.bool, device=dev),
              live.any()]
        host = torch.stack([o.reshape(()).long() for o in ok] + [n_b.max().long()]).cpu().numpy()
        ok, max_atoms = host[:-1] != 0, int(host[-1])
        if not ok[0]:
            raise ValueError("atom_off must be a non-decreasing [B + 1] offset vector from 0 to %d" % N)
        if max_atoms > MAX_ATOMS:
            raise ValueError("score_poses takes ligands of at most %d atoms" % MAX_ATOMS)
        if not ok[1:4].all():
            raise ValueError("prot_types must hold one word per protein atom the grid was built from (%d given)" % M)
        if not ok[4:16].all():
            raise ValueError("inconsistent ligands or ProteinGrid (the grid must hold the complexes of the ligands)")
        if not ok[16]:
            raise ValueError("n_torsions must be >= 0")
        if ok[17]:                                                    # at least one complex is scored (else: the prefill stands)
            params = torch.tensor(w + [float(torsion_weight)], dtype=torch.float64, device=dev)
            K.pose_score(p, aoff, B, max_atoms, st, lt, nt, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off,
                         grid.cell_ptr, grid.xyz, grid.atom_id, grid.prot_off, pt, grid.edge, cutoff, params, terms, inter, total, n_pairs,
                         pa, flags)
    return PoseScores(terms=terms, inter=inter, total=total, n_pairs=n_pairs, per_atom=pa, flags=flags)
