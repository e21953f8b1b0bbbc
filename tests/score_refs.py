"""float64 numpy restatement of fabind_amd.scoring (typing and csrc/pose_score.hip), written from the definitions of DESIGN.md section
22 and sharing no code with the device path or with the package: the energy is BRUTE FORCE over every kept protein atom, with no cell
list.  tests/test_score_refs_cpu.py pins this module by hand-worked numbers; tests/test_gpu_score.py compares the device with it.

r^2 = ((dx dx) + (dy dy)) + (dz dz) of float64 differences of the float32 inputs and d = (sqrt(r^2) - R_i) - R_j: the device's
operations in the device's order (its source is compiled without contraction, sqrt is correctly rounded on both sides), so d, the pair
set and the three piecewise terms of a pair are the same bits on both sides; only the two exponentials and the order of the sums
differ (`bound`)."""
import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -52
HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64
NONFINITE, UNCHECKED = 128, 256
C_, N_, O_, P_, S_, F_, CL_, BR_, I_, METAL_ = range(10)
RADII = np.array([1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2] + [1.2] * 6)
WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
TERMS = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
CLASS_OF = {6: C_, 7: N_, 8: O_, 15: P_, 16: S_, 9: F_, 17: CL_, 35: BR_, 53: I_}
METALS = {3, 4, 11, 12, 13, 19, 20, 37, 38, 55, 56} | set(range(21, 32)) | set(range(39, 51)) | set(range(57, 84))
ORDER = {1: 1.5, 2: 3.0, 3: 2.0}                                        # symmetry.bond_code: AROMATIC 1, TRIPLE 2, DOUBLE 3, else single


# ------------------------------------------------------------------------------------------------ typing
def element_word(z):
    """The word of an element alone: class, halogens hydrophobic, metals donors, O an acceptor; anything unknown a metal without a role."""
    z = int(z)
    t = CLASS_OF.get(z, METAL_)
    if z in (9, 17, 35, 53):
        t |= HYDROPHOBIC
    if z in METALS:
        t |= DONOR
    if z == 8:
        t |= ACCEPTOR
    return t


def ligand_types(n, bonds, codes, z, n_hydrogens=None, charge=None):
    """Atom by atom in plain Python.  bonds: [(i, j)] each bond once; codes aligned; z [n]."""
    charge = [0] * n if charge is None else list(charge)
    nbrs = [[] for _ in range(n)]
    for (i, j), c in zip(bonds, codes):
        nbrs[i].append((j, int(c)))
        nbrs[j].append((i, int(c)))
    out = []
    for a in range(n):
        za = int(z[a])
        t = element_word(za)
        total = sum(ORDER.get(c, 1.0) for _, c in nbrs[a])
        if za == 6 and all(int(z[j]) in (1, 6) for j, _ in nbrs[a]):
            t |= HYDROPHOBIC
        if za in (7, 8):
            if n_hydrogens is not None:
                nh = int(n_hydrogens[a])
            else:
                nh = sum(int(z[j]) == 1 for j, _ in nbrs[a]) + max(0, (3 if za == 7 else 2) + charge[a] - int(np.floor(total)))
            if nh > 0:
                t |= DONOR
            if za == 7 and nh == 0 and charge[a] <= 0 and int(np.floor(total)) <= 3 and any(c in (1, 2, 3) for _, c in nbrs[a]):
                t |= ACCEPTOR
        out.append(t)
    return np.asarray(out, np.int32)


# ------------------------------------------------------------------------------------------------ the energy
def pair_terms(d, ti, tj):
    """The five terms of pairs at surface distances d (float64 array) between atoms of words ti, tj (int arrays)."""
    d = np.asarray(d, np.float64)
    ti, tj = np.asarray(ti, np.int64), np.asarray(tj, np.int64)
    u1, u2 = d / 0.5, (d - 3.0) / 2.0
    g1, g2 = np.exp(-(u1 * u1)), np.exp(-(u2 * u2))
    rep = np.where(d < 0.0, d * d, 0.0)
    hyd = np.where((ti & tj & HYDROPHOBIC) != 0, np.where(d < 0.5, 1.0, np.where(d < 1.5, 1.5 - d, 0.0)), 0.0)
    pair_hb = (((ti & DONOR) != 0) & ((tj & ACCEPTOR) != 0)) | (((ti & ACCEPTOR) != 0) & ((tj & DONOR) != 0))
    hb = np.where(pair_hb, np.where(d < -0.7, 1.0, np.where(d < 0.0, -d / 0.7, 0.0)), 0.0)
    return np.stack([g1, g2, rep, hyd, hb], -1)


def score(pose, lig_types, prot_xyz, prot_z, prot_types, n_torsions=0, lig_status=0, grid_status=0, weights=WEIGHTS, cutoff=8.0,
          torsion_weight=0.0585):
    """One (complex, pose), brute force.  prot_xyz / prot_z / prot_types: ALL atoms of the protein (Z <= 1 are dropped here).
    -> dict(terms [5], inter, total, n_pairs, per_atom [n], flags; abs_terms [5]: the sums of |term| (= terms, all are >= 0),
    abs_inter: sum over pairs and terms of |w_k term_k|, abs_total: the same scaled as total is, abs_atom [n]: the same per ligand
    atom, pairs_atom [n]: pairs per atom,
    cut_margin: the smallest |r^2 - cutoff^2| over all pairs (inf without one))."""
    pose = np.asarray(pose, np.float32).reshape(-1, 3)
    n = len(pose)
    nan5 = np.full(5, np.nan)
    none = dict(terms=nan5, inter=np.nan, total=np.nan, n_pairs=0, per_atom=np.full(n, np.nan), abs_terms=nan5, abs_inter=np.nan,
                abs_total=np.nan, abs_atom=np.full(n, np.nan), pairs_atom=np.zeros(n, np.int64), cut_margin=np.inf)
    if lig_status != 0 or grid_status != 0:
        return dict(none, flags=UNCHECKED)
    if not np.isfinite(pose).all():
        return dict(none, flags=NONFINITE)
    w = np.asarray([float(v) for v in weights], np.float64)
    keep = np.nonzero(np.asarray(prot_z).reshape(-1) > 1)[0]
    px = np.asarray(prot_xyz, np.float32).reshape(-1, 3)[keep].astype(np.float64)
    pt = np.asarray(prot_types, np.int64).reshape(-1)[keep]
    lt = np.asarray(lig_types, np.int64).reshape(-1)
    terms, per_atom, abs_atom, pairs_atom = np.zeros(5), np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    abs_inter, margin = 0.0, np.inf
    c = np.float64(np.float32(cutoff))
    if n and len(px):
        a = pose.astype(np.float64)
        dx, dy, dz = (a[:, None, k] - px[None, :, k] for k in range(3))
        r2 = (dx * dx + dy * dy) + dz * dz
        margin = np.abs(r2 - c * c).min()
        ii, jj = np.nonzero(r2 < c * c)
        d = (np.sqrt(r2[ii, jj]) - RADII[lt[ii] & 15]) - RADII[pt[jj] & 15]
        t = pair_terms(d, lt[ii], pt[jj])                                # [P, 5]
        terms = t.sum(0)
        e = (((w[0] * t[:, 0] + w[1] * t[:, 1]) + w[2] * t[:, 2]) + w[3] * t[:, 3]) + w[4] * t[:, 4]
        ea = np.abs(w[None] * t).sum(1)
        per_atom = np.bincount(ii, weights=e, minlength=n)
        abs_atom = np.bincount(ii, weights=ea, minlength=n)
        pairs_atom = np.bincount(ii, minlength=n)
        abs_inter = ea.sum()
    inter = (((w[0] * terms[0] + w[1] * terms[1]) + w[2] * terms[2]) + w[3] * terms[3]) + w[4] * terms[4]
    scale = 1.0 + float(torsion_weight) * float(n_torsions)
    total = inter / scale
    return dict(terms=terms, inter=inter, total=total, n_pairs=int(pairs_atom.sum()), per_atom=per_atom, flags=0, abs_terms=terms.copy(),
                abs_inter=abs_inter, abs_total=abs_inter / scale, abs_atom=abs_atom, pairs_atom=pairs_atom, cut_margin=margin)


def bound(pairs, a, value):
    """|device float32 - this float64| <= (P + 16) 2^-52 A + 2^-24 |value|: P the pairs of the sum, A the sum of
    its absolute (weighted) terms.  First part: the reordered float64 sum of P terms, each within about 1 ulp of the other side's (the
    two exp implementations; the five products and four additions of a weighted pair are in the 16); second part: the float32 store."""
    return (pairs + 16) * EPS * a + U * abs(value)


def exact32(pairs, a, value):
    """True when every float64 within (P + 16) 2^-52 A of `value` rounds to the same float32: then two float64 sums of the same terms in
    different orders must agree as float32, and the comparison may be exact."""
    s = (pairs + 16) * EPS * a
    return np.float32(value - s) == np.float32(value + s)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def random_words(n, rng):
    """Random type words: every class, every combination of the three role bits."""
    return (rng.randint(0, 10, size=n) | (rng.randint(0, 8, size=n) << 4)).astype(np.int32)
