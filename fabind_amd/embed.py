"""Start conformers from the bond list on the GPU, by distance geometry: the input `rdkit_coords` without RDKit.

The reference makes the start conformer with `AllChem.EmbedMolecule(mol, ETKDGv2())` + `MMFFOptimizeMolecule`
(utils/inference_mol_utils.py:135-144).  Here (csrc/embed.hip):

* `distance_bounds`: per ligand, once, from the bond list and the atomic numbers: lower and upper bounds on every atom-atom distance
  (1-2 from covalent radii, 1-3 from the class angle of the centre, 1-4 from the cis and trans geometry, van der Waals sums beyond),
  triangle-smoothed, plus the signed-volume terms that keep trigonal atoms, double bonds and aromatic rings flat and stereo centres on
  the asked hand.  Count pass, one host read-back, write pass -- as `validity.validity_plan`.
* `embed_conformers`: `n_confs` conformers of every ligand in one launch: random distances inside the bounds, metric-matrix embedding
  in four dimensions, conjugate-gradient minimisation of the violation function, retried with new draws until the bounds hold.
* `molecule_from_sdf`, `chiral_signs_from_coords`: the inputs from an SDF read as text and from given coordinates.

What this is NOT: no torsion preferences (the "K" of ETKDG), no force-field pass, no hydrogens, no macrocycle heuristics; E/Z at double
bonds cannot be specified and stereo centres come out on either hand unless `chiral_sign` says which.  Agreement with RDKit's
conformers is not measured (RDKit is not importable where this project runs); what is tested is the bounds against crystal ligands, the
invariants of the result and its flags under `validity.check_poses`."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .conformer import _coded_neighbour_lists
from .symmetry import _atom_off, bond_code

MAX_ATOMS = 256
STATUS = {0: "ok", 1: "tries exhausted", 3: "more than 256 atoms", 6: "inconsistent bounds"}
TETRA, TRIGONAL, LINEAR = 0, 1, 2
# the intervals of the signed volumes (A^3): flat terms [-V_FLAT, V_FLAT], stereo terms sign * [V_MIN, V_MAX]
V_FLAT, V_MIN, V_MAX = 0.2, 1.0, 100.0
# the defaults of `embed_conformers`: they rest on the host experiment of DESIGN.md section 20 only
MAX_TRIES, MAX_STEPS, VIOL_TOL, V_TOL, W_V, W_4, POWER_ITERS = 8, 1000, 0.1, 0.2, 0.1, 0.1, 100


@dataclass
class DistanceBounds:
    """The distance bounds of a batch of ligands, all on the device; atom ids are LOCAL to their ligand, so a ligand's entries are the
    same bits alone and in any batch.
    atom_off: int32 [B + 1]; status: int32 [B], a key of STATUS (3: no entries; 6: some lower bound above its upper bound after
    smoothing -- the block is kept for inspection, nothing is embedded).
    bounds: float32, one n_b x n_b block per ligand at mat_off[b] (int64 [B + 1]): the upper bound of the pair (i, j) at
    (min, max), the lower bound at (max, min), the diagonal 0.  geom: int32 [N], 0 TETRA / 1 TRIGONAL / 2 LINEAR.
    quads: int32 [Q, 4] with quad_lo, quad_hi float32 [Q] and quad_off int32 [B + 1]: V = det[p1 - p0, p2 - p0, p3 - p0] is wanted in
    [quad_lo, quad_hi].  Listed by atom t ascending: its flat term (t, n1, n2, n3) if t is TRIGONAL with three neighbours; the 1-4
    quadruples (i, t, b, j) of its DOUBLE- or AROMATIC-coded bonds t-b, b > t ascending, i then j ascending; its stereo term
    (t, n1, n2, n3) for three neighbours, (n4, n1, n2, n3) for four."""
    atom_off: torch.Tensor
    status: torch.Tensor
    mat_off: torch.Tensor
    bounds: torch.Tensor
    geom: torch.Tensor
    quad_off: torch.Tensor
    quads: torch.Tensor
    quad_lo: torch.Tensor
    quad_hi: torch.Tensor

    def block(self, b):
        """(upper [n, n], lower [n, n]) of ligand b as symmetric float32 tensors (a host read of two offsets)."""
        m0, m1 = (int(v) for v in self.mat_off[b:b + 2])
        n = int(self.atom_off[b + 1]) - int(self.atom_off[b])
        if m1 - m0 != n * n:
            z = torch.zeros(0, 0, dtype=torch.float32, device=self.bounds.device)
            return z, z
        p = self.bounds[m0:m1].reshape(n, n)
        u, l = torch.triu(p, 1), torch.tril(p, -1)
        return u + u.t(), l + l.t()


@dataclass
class Embedding:
    """coords: float32 [S, N, 3], every (ligand, conformer) centred on its centroid (zero rows where status is 3 or 6);
    status: int32 [B, S], a key of STATUS (1: the try with the smallest largest violation is returned); tries, steps: int32 [B, S]
    (tries made; evaluations of E by the minimiser in the returned try); viol: float64 [B, S], the largest max(l - d, d - u, 0) over the
    pairs (A); energy: float64 [B, S], E -- both of the RETURNED float32 coordinates.  trace: float64 [B, S, max_steps + 1] or None: E
    after each step of the last try made, NaN behind the last."""
    coords: torch.Tensor
    status: torch.Tensor
    tries: torch.Tensor
    steps: torch.Tensor
    viol: torch.Tensor
    energy: torch.Tensor
    trace: torch.Tensor = None


def _bond_args(name, bond_index, bond_codes, atomic_numbers, atom_off):
    if not torch.is_tensor(bond_index) or not bond_index.is_cuda:
        raise RuntimeError("fabind_amd: %s runs on a HIP device only (no CPU fallback)" % name)
    dev = bond_index.device
    bi = bond_index.to(torch.int64).reshape(2, -1)
    if not torch.is_tensor(bond_codes) and len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [bond_code(t) for t in bond_codes]
    codes = torch.as_tensor(bond_codes).to(device=dev, dtype=torch.int64).reshape(-1)
    if codes.numel() != bi.shape[1]:
        raise ValueError("%s: %d bonds but %d bond codes" % (name, bi.shape[1], codes.numel()))
    z = torch.as_tensor(atomic_numbers).to(device=dev, dtype=torch.int32).contiguous()
    if z.dim() != 1:
        raise ValueError("atomic_numbers must be [N]; got %s" % (tuple(z.shape),))
    N = z.shape[0]
    aoff = _atom_off(atom_off, dev, N)
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= N):
        raise ValueError("bond_index holds atom ids outside [0, %d)" % N)
    return dev, bi, codes, z, N, aoff


def distance_bounds(bond_index, bond_codes, atomic_numbers, atom_off, chiral_sign=None, on_overflow="raise"):
    """The distance bounds and signed-volume terms of every ligand of a batch (csrc/embed.hip), on the heavy-atom graph.

    bond_index: [2, E] GLOBAL atom ids on the HIP device, each bond once, in both directions or repeated; bonds never cross ligands.
    bond_codes: [E], `symmetry.bond_code` coding (AROMATIC 1, TRIPLE 2, DOUBLE 3, SINGLE 4, other 5; names are accepted).
    atomic_numbers: int [N]; atom_off: [B + 1].
    chiral_sign: int [N] or None.  An atom that is a stereo centre by `validity_plan`'s topological definition (three or four
    neighbours, no AROMATIC, DOUBLE or TRIPLE bond, no nitrogen unless it has four neighbours) and whose entry is +1 or -1 gets a
    term that holds its signed volume (that definition's determinant and neighbour order) to that sign; `chiral_signs_from_coords`
    reads the signs off given coordinates.  With None there are no stereo terms and EITHER hand may come out.  The configuration (E/Z)
    of a double bond cannot be specified: both come out.
    on_overflow: "raise" -> RuntimeError naming every ligand with status != 0 (3: more than 256 atoms; 6: inconsistent bounds);
    "skip" -> such ligands keep their status and `embed_conformers` returns zero rows for them.
    The rules (tests/embed_refs.py restates them and must agree bit for bit): a geometry class per atom; 1-2
    distances from covalent radii and the bond code, +-0.01; 1-3 by the law of cosines with the class angle of the centre (60 / 90 /
    108 degrees on a 3- / 4- / 5-ring), +-0.04; 1-4 between the cis and the trans distance, -+0.06 (cis for both on a six-ring whose
    two middle atoms are TRIGONAL); beyond, the sum of the Bondi radii as the lower bound (0.8 of it at four bonds); different fragments
    are held within 10 A of each other -- an arbitrary value that only keeps them together.  Then triangle smoothing in float32.
    -> DistanceBounds.  Two launches (count, then write) with one host read-back that sizes the lists, and under "raise" a second
    read-back of the statuses (inconsistent bounds show only after smoothing)."""
    if on_overflow not in ("raise", "skip"):
        raise ValueError("on_overflow must be 'raise' or 'skip'")
    dev, bi, codes, z, N, aoff = _bond_args("distance_bounds", bond_index, bond_codes, atomic_numbers, atom_off)
    B = aoff.numel() - 1
    cs = None
    if chiral_sign is not None:
        cs = torch.as_tensor(chiral_sign).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(cs.shape) != (N,):
            raise ValueError("chiral_sign must be [%d]; got %s" % (N, tuple(cs.shape)))
    nptr, nidx, ncode, _ = _coded_neighbour_lists(bi, codes, max(N, 1))
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    vol = (V_FLAT, V_MIN, V_MAX)
    K.embed_bounds_pass(nptr, nidx, ncode, aoff, B, z, cs, vol, counts, status)
    n_b = torch.diff(aoff).to(torch.int64)
    mat_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    mat_off[1:] = torch.cumsum(torch.where(status == 3, torch.zeros_like(n_b), n_b * n_b), 0)
    quad_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    quad_off[1:] = torch.cumsum(counts, 0)
    host = torch.cat([quad_off[-1:].to(torch.int64), mat_off[-1:], status.to(torch.int64)]).cpu().numpy()   # the one read-back
    Q, M = int(host[0]), int(host[1])
    out = DistanceBounds(atom_off=aoff, status=status, mat_off=mat_off, bounds=torch.zeros(M, dtype=torch.float32, device=dev),
                         geom=torch.zeros(N, dtype=torch.int32, device=dev), quad_off=quad_off,
                         quads=torch.zeros(Q, 4, dtype=torch.int32, device=dev), quad_lo=torch.zeros(Q, dtype=torch.float32, device=dev),
                         quad_hi=torch.zeros(Q, dtype=torch.float32, device=dev))
    if B:
        K.embed_bounds_pass(nptr, nidx, ncode, aoff, B, z, cs, vol, counts, status, quad_off, mat_off, out.bounds, out.geom, out.quads,
                            out.quad_lo, out.quad_hi)
    if on_overflow == "raise":
        st = status.cpu().numpy()                                     # status 6 shows only after smoothing
        bad = np.nonzero(st)[0]
        if len(bad):
            raise RuntimeError("distance_bounds: " + "; ".join("ligand %d: status %d (%s)" % (b, st[b], STATUS[int(st[b])]) for b in bad))
    return out


def embed_conformers(bounds, n_confs=1, seed=0, keys=None, max_tries=MAX_TRIES, max_steps=MAX_STEPS, viol_tol=VIOL_TOL, v_tol=V_TOL,
                     w_v=W_V, w_4=W_4, power_iters=POWER_ITERS, return_trace=False):
    """`n_confs` conformers of every ligand under its `distance_bounds` (csrc/embed.hip): one work-group per (ligand, conformer), every
    try and every minimisation step inside ONE launch.

    Per try: (1) a random distance d_ij = l + u01 (u - l) for every pair, u01 from the counter hash of `conformer.perturb_conformers`
    keyed (seed, keys[b], conformer, try, pair index i n + j); (2) the metric matrix g_ij = (d_i0^2 + d_j0^2 - d_ij^2) / 2 in float64;
    (3) its FOUR largest eigenpairs by `power_iters` power iterations with deflation from a hashed start vector, coordinates
    sqrt(lambda) v (an axis whose eigenvalue is not positive takes hashed draws in [-1, 1] A: RDKit's fallback) -- the fourth
    coordinate lets atoms pass each other and is driven to zero by the minimiser; (4) Polak-Ribiere+ conjugate gradients with a
    backtracking line search (at most `max_steps` evaluations) on
        E = sum_{i<j} e(d_ij) + w_v sum_quads (V - clamp(V, lo, hi))^2 + w_4 sum_i x_i4^2,
    e = (d^2 / u^2 - 1)^2 above u, (2 l^2 / (l^2 + d^2) - 1)^2 below l, else 0 (RDKit's distance-violation terms, d over all four
    coordinates, V over the first three); (5) the first three coordinates, centred and rounded to float32, are accepted when every pair
    has max(l - d, d - u) <= viol_tol and every V is inside its interval widened by v_tol; else the next try.  After `max_tries` the
    try with the smallest largest violation is returned with status 1.
    keys: int [B] or None for the ligand's index -- a ligand's conformer c is the same bits alone, in any batch, among any n_confs
    and on a repeat when its key is the same.  viol_tol, v_tol, w_v, w_4 are rounded to float32.  There is no force-field step.
    -> Embedding."""
    if not isinstance(bounds, DistanceBounds) or not bounds.bounds.is_cuda:
        raise RuntimeError("fabind_amd: embed_conformers needs the DistanceBounds of `distance_bounds` on a HIP device (no CPU fallback)")
    dev = bounds.bounds.device
    B, N, Q = bounds.atom_off.numel() - 1, int(bounds.geom.shape[0]), int(bounds.quads.shape[0])
    S = int(n_confs)
    if S < 1:
        raise ValueError("n_confs must be >= 1")
    if not (1 <= int(max_tries) <= 1024 and 0 <= int(max_steps) <= 1000000 and 1 <= int(power_iters) <= 100000):
        raise ValueError("max_tries in [1, 1024], max_steps in [0, 1e6], power_iters in [1, 1e5]")
    tol = [float(np.float32(v)) for v in (viol_tol, v_tol, w_v, w_4)]
    if not all(0.0 <= v < float("inf") for v in tol):
        raise ValueError("viol_tol, v_tol, w_v and w_4 must be finite and >= 0")
    ints = (bounds.atom_off, bounds.status, bounds.quad_off, bounds.quads, bounds.geom)
    if (any(t.device != dev or not t.is_contiguous() for t in ints + (bounds.mat_off, bounds.bounds, bounds.quad_lo, bounds.quad_hi))
            or any(t.dtype != torch.int32 for t in ints) or bounds.mat_off.dtype != torch.int64 or bounds.bounds.dtype != torch.float32
            or bounds.quad_lo.dtype != torch.float32 or bounds.quad_hi.dtype != torch.float32
            or tuple(bounds.status.shape) != (B,) or tuple(bounds.quad_off.shape) != (B + 1,) or tuple(bounds.mat_off.shape) != (B + 1,)
            or tuple(bounds.quads.shape) != (Q, 4) or tuple(bounds.quad_lo.shape) != (Q,) or tuple(bounds.quad_hi.shape) != (Q,)):
        raise ValueError("inconsistent DistanceBounds")
    if keys is None:
        keys = torch.arange(B, dtype=torch.int64, device=dev)
    kk = torch.as_tensor(keys).to(device=dev, dtype=torch.int64).reshape(-1)
    if kk.numel() != B:
        raise ValueError("keys must be [%d]; got %s" % (B, tuple(kk.shape)))
    kk = kk & 0xFFFFFFFF                                               # the kernel reads the keys as unsigned 32-bit words
    kk = torch.where(kk >= 2 ** 31, kk - 2 ** 32, kk).to(torch.int32).contiguous()
    coords = torch.zeros(S, N, 3, dtype=torch.float32, device=dev)
    status = torch.zeros(B, S, dtype=torch.int32, device=dev)
    tries, steps = torch.zeros_like(status), torch.zeros_like(status)
    viol = torch.zeros(B, S, dtype=torch.float64, device=dev)
    energy = torch.zeros_like(viol)
    trace = torch.full((B, S, int(max_steps) + 1), float("nan"), dtype=torch.float64, device=dev) if return_trace else None
    if B:
        # the kernel indexes the blocks and the lists with these: checked on the host, one read-back
        n_b = torch.diff(bounds.atom_off).to(torch.int64)
        want = torch.where(bounds.status == 3, torch.zeros_like(n_b), n_b * n_b)     # (a ligand of status 6 keeps its block)
        ok = torch.stack([(bounds.atom_off[0] == 0), (n_b >= 0).all(), (bounds.atom_off[-1] == N), (bounds.mat_off[0] == 0),
                          (torch.diff(bounds.mat_off) == want).all(), (bounds.mat_off[-1] == bounds.bounds.numel()),
                          (bounds.quad_off[0] == 0), (torch.diff(bounds.quad_off) >= 0).all(), (bounds.quad_off[-1] == Q),
                          ((n_b <= MAX_ATOMS) | (bounds.status == 3)).all()]).cpu().numpy()
        if not ok.all():
            raise ValueError("inconsistent DistanceBounds")
        K.embed_conformers(bounds.bounds, bounds.mat_off, bounds.atom_off, B, N, S, bounds.status, bounds.quad_off, bounds.quads,
                           bounds.quad_lo, bounds.quad_hi, kk, seed, max_tries, max_steps, power_iters, tol, coords, status, tries, steps, viol,
                           energy, trace)
    return Embedding(coords=coords, status=status, tries=tries, steps=steps, viol=viol, energy=energy, trace=trace)


def chiral_signs_from_coords(bond_index, bond_codes, atomic_numbers, coords, atom_off):
    """The sign (+1 / -1; 0: not a centre, or a volume of exactly 0) of every topological stereo centre's signed volume in given
    coordinates, e.g. a crystal pose -- the `chiral_sign` of `distance_bounds`.  The definition is `validity_plan`'s: three or four
    neighbours, no AROMATIC, DOUBLE or TRIPLE bond, no nitrogen unless it has four neighbours; V = det[n1 - c, n2 - c, n3 - c] for
    three neighbours, det[n1 - n4, n2 - n4, n3 - n4] for four, neighbours in ascending id, float32 differences, float64 determinant.
    Thin torch glue on the device of bond_index.  -> int32 [N]."""
    dev, bi, codes, z, N, aoff = _bond_args("chiral_signs_from_coords", bond_index, bond_codes, atomic_numbers, atom_off)
    x = torch.as_tensor(coords).detach().to(device=dev, dtype=torch.float32)
    if tuple(x.shape) != (N, 3):
        raise ValueError("coords must be [%d, 3]; got %s" % (N, tuple(x.shape)))
    out = torch.zeros(N, dtype=torch.int32, device=dev)
    if N == 0:
        return out
    nptr, nidx, ncode, nown = _coded_neighbour_lists(bi, codes, N)
    nptr, nidx, nown = nptr.long(), nidx.long(), nown.long()
    deg = torch.diff(nptr)
    multi = torch.zeros(N, dtype=torch.bool, device=dev)
    multi[nown[(ncode >= 1) & (ncode <= 3)]] = True
    centre = ((deg == 3) | (deg == 4)) & ~multi & ((z != 7) | (deg == 4))
    c = torch.nonzero(centre).reshape(-1)
    if c.numel() == 0:
        return out
    nb = nidx[(nptr[c][:, None] + torch.arange(4, device=dev)[None, :]).clamp(max=max(nidx.numel() - 1, 0))]   # ascending neighbours
    four = deg[c] == 4
    origin = torch.where(four, nb[:, 3], c)
    d = (x[nb[:, :3]] - x[origin][:, None, :]).to(torch.float64)
    v = torch.linalg.det(d)
    out[c] = torch.sign(v).to(torch.int32)
    return out


_ELEMENTS = ("H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar", "K", "Ca", "Sc", "Ti", "V",
             "Cr", "Mn", "Fe", "Co", "Ni", "Cu", "Zn", "Ga", "Ge", "As", "Se", "Br", "Kr", "Rb", "Sr", "Y", "Zr", "Nb", "Mo", "Tc", "Ru", "Rh",
             "Pd", "Ag", "Cd", "In", "Sn", "Sb", "Te", "I", "Xe")
_Z = {s.upper(): i + 1 for i, s in enumerate(_ELEMENTS)}
_Z["D"] = 1
_V2000_CODE = {1: 4, 2: 3, 3: 2, 4: 1}                                # SINGLE, DOUBLE, TRIPLE, AROMATIC in `symmetry.bond_code` coding


def molecule_from_sdf(text):
    """The heavy atoms of the first molecule of an SDF / MOL file's text (V2000, read by fixed columns; pure Python): the counterpart
    of `validity.protein_atoms_from_pdb`.  Hydrogens (H, D) and the bonds to them are dropped; an element that cannot be read gives
    Z = 0; a bond type other than 1 / 2 / 3 / 4 gets code 5.
    -> dict(atomic_numbers int32 [n], bonds int64 [E, 2] (ids among the heavy atoms, each bond once), bond_codes int64 [E], coords
    float32 [n, 3] -- all zeros in a file without coordinates) of numpy arrays."""
    lines = text.splitlines()
    if len(lines) < 4:
        raise ValueError("molecule_from_sdf: no counts line")
    counts = lines[3]
    if "V3000" in counts:
        raise ValueError("molecule_from_sdf: V3000 files are not read")
    try:
        na, nbd = int(counts[0:3]), int(counts[3:6])
    except ValueError:
        raise ValueError("molecule_from_sdf: unreadable counts line %r" % counts)
    if len(lines) < 4 + na + nbd:
        raise ValueError("molecule_from_sdf: the file ends inside the atom or bond block")
    zs, xyz = [], []
    for ln in lines[4:4 + na]:
        try:
            xyz.append((float(ln[0:10]), float(ln[10:20]), float(ln[20:30])))
        except ValueError:
            raise ValueError("molecule_from_sdf: unreadable coordinates in %r" % ln)
        zs.append(_Z.get(ln[31:34].strip().upper(), 0))
    heavy = [i for i, zi in enumerate(zs) if zi != 1]
    new = {old: i for i, old in enumerate(heavy)}
    bonds, codes = [], []
    for ln in lines[4 + na:4 + na + nbd]:
        try:
            a, b, t = int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])
        except ValueError:
            raise ValueError("molecule_from_sdf: unreadable bond line %r" % ln)
        if a in new and b in new:
            bonds.append((new[a], new[b]))
            codes.append(_V2000_CODE.get(t, 5))
    return dict(atomic_numbers=np.asarray([zs[i] for i in heavy], np.int32), bonds=np.asarray(bonds, np.int64).reshape(-1, 2),
                bond_codes=np.asarray(codes, np.int64), coords=np.asarray([xyz[i] for i in heavy], np.float32).reshape(-1, 3))
