"""float64 numpy restatement of fabind_amd.validity.protein_grid / check_poses_protein (csrc/protein_contacts.hip), written from their
definitions and sharing no code with the device path: the statistics are BRUTE FORCE over every kept protein atom, with no cell list;
the cell list is restated separately (`grid`).  tests/test_contact_refs_cpu.py pins this module (against scipy's cKDTree, hand cases
and the margins of the GPU inputs); tests/test_gpu_protein_contacts.py compares the device with it.

Every sum of squares is ((dx * dx) + (dy * dy)) + (dz * dz) of float64 differences of the float32 inputs, the device's order (its
source is compiled without contraction), so counts are compared exactly; `bound` gives the bounds of the float32 stores."""
import numpy as np

U = 2.0 ** -24
MAX_CELLS = 1 << 20
CLAMP = float(1 << 29)
CLASH, OVERLAP, NONFINITE, UNCHECKED = 1, 2, 128, 256
DEFAULTS = dict(cutoff=5.0, clash_min=0.75, overlap_max=0.075, vdw_scale=0.8, spacing=0.5)
_BONDI = {5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 34: 1.90, 35: 1.85, 53: 1.98}


def bondi(z):
    return np.asarray([_BONDI.get(int(v), 2.00) for v in np.asarray(z).reshape(-1)], np.float32)


def cell_index(x, edge):
    """floor(float64(x) / float64(float32(edge))) clamped to +-2^29, as int64; x: float32 values."""
    with np.errstate(invalid="ignore"):
        q = np.floor(np.asarray(x, np.float32).astype(np.float64) / np.float64(np.float32(edge)))
    return np.clip(q, -CLAMP, CLAMP).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the cell list
def grid(xyz, z, radii=None, edge=5.0):
    """The cell list of ONE complex: dict(status, origin [3], dims [3], cell_ptr [cells + 1] LOCAL positions, xyz [K, 3] float32,
    radii [K] float32, atom_id [K]); kept atoms (Z > 1) ordered by (cell, original id), cells by linear id with x fastest."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    z = np.asarray(z, np.int64).reshape(-1)
    r = bondi(z) if radii is None else np.asarray(radii, np.float32).reshape(-1)
    empty = dict(status=0, origin=np.zeros(3, np.int32), dims=np.zeros(3, np.int32), cell_ptr=np.zeros(1, np.int32),
                 xyz=np.zeros((0, 3), np.float32), radii=np.zeros(0, np.float32), atom_id=np.zeros(0, np.int32))
    if not np.isfinite(xyz).all():
        return dict(empty, status=6)
    keep = np.nonzero(z > 1)[0]
    if len(keep) == 0:
        return empty
    c = cell_index(xyz[keep], edge)
    lo, hi = c.min(0), c.max(0)
    d = hi - lo + 1
    if int(d[0]) * int(d[1]) * int(d[2]) > MAX_CELLS:
        return dict(empty, status=7)
    lin = ((c[:, 2] - lo[2]) * d[1] + (c[:, 1] - lo[1])) * d[0] + (c[:, 0] - lo[0])
    order = np.lexsort((keep, lin))                                    # by cell, then by original id
    cells = int(d.prod())
    ptr = np.concatenate([[0], np.cumsum(np.bincount(lin, minlength=cells))]).astype(np.int32)
    return dict(status=0, origin=lo.astype(np.int32), dims=d.astype(np.int32), cell_ptr=ptr, xyz=xyz[keep][order], radii=r[keep][order],
                atom_id=keep[order].astype(np.int32))


def batch_grid(grids):
    """The per-complex grids in the layout of a ProteinGrid (cell_ptr as positions into the batch's sorted atoms)."""
    cell_off = np.concatenate([[0], np.cumsum([len(g["cell_ptr"]) - 1 for g in grids])]).astype(np.int32)
    atom_off = np.concatenate([[0], np.cumsum([len(g["atom_id"]) for g in grids])]).astype(np.int32)
    ptr = [np.zeros(1, np.int32)] + [g["cell_ptr"][1:] + atom_off[b] for b, g in enumerate(grids)]
    cat = lambda k, tail, dt: np.concatenate([g[k] for g in grids] + [np.zeros((0,) + tail, dt)])
    return dict(status=np.asarray([g["status"] for g in grids], np.int32).reshape(-1),
                origin=np.asarray([g["origin"] for g in grids], np.int32).reshape(-1, 3),
                dims=np.asarray([g["dims"] for g in grids], np.int32).reshape(-1, 3), cell_off=cell_off, atom_off=atom_off,
                cell_ptr=np.concatenate(ptr).astype(np.int32), xyz=cat("xyz", (3,), np.float32), radii=cat("radii", (), np.float32),
                atom_id=cat("atom_id", (), np.int32))


# ------------------------------------------------------------------------------------------------ the statistics
def _d2(a, b):
    """[len(a), len(b)] squared distances: float64 differences of float32 points, ((dx dx) + (dy dy)) + (dz dz)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def kept(prot_xyz, prot_z, prot_r=None):
    """(xyz float32 [K, 3], radii float32 [K], original ids [K]) of the protein atoms with Z > 1."""
    prot_xyz = np.asarray(prot_xyz, np.float32).reshape(-1, 3)
    z = np.asarray(prot_z, np.int64).reshape(-1)
    r = bondi(z) if prot_r is None else np.asarray(prot_r, np.float32).reshape(-1)
    k = np.nonzero(z > 1)[0]
    return prot_xyz[k], r[k], k


def close_pairs(pose, pxyz, cutoff):
    """(i, j, d2) of every (ligand atom i, kept protein atom j -- a position in pxyz) with d^2 < cutoff^2 in float64, brute force."""
    if len(pose) == 0 or len(pxyz) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    d2 = _d2(np.asarray(pose, np.float32), pxyz)
    c = np.float64(np.float32(cutoff))
    i, j = np.nonzero(d2 < c * c)
    return i, j, d2[i, j]


def _ahead(r1, i1, j1, r2, i2, j2):
    """The order of the minimum: NaN first, then the smaller ratio, then the lower ligand id, then the lower protein id."""
    n1, n2 = r1 != r1, r2 != r2
    if n1 != n2:
        return n1
    if not n1 and r1 != r2:
        return r1 < r2
    return (i1, j1) < (i2, j2)


def lattice_points(xyz, radii, vdw_scale, spacing):
    """The integer vectors k [P, 3] (each once, sorted) with |spacing k - x_i|^2 <= (vdw_scale r_i)^2 for some atom i, and the smallest
    |d^2 - R^2| met on the way (the margin of the membership tests)."""
    sp, sc = np.float64(np.float32(spacing)), np.float64(np.float32(vdw_scale))
    out, margin = [np.zeros((0, 3), np.int64)], np.inf
    for x, r in zip(np.asarray(xyz, np.float32).astype(np.float64), np.asarray(radii, np.float32).astype(np.float64)):
        R = sc * r
        lo, hi = np.floor((x - R) / sp).astype(np.int64) - 1, np.ceil((x + R) / sp).astype(np.int64) + 1
        k = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
        g = sp * k.astype(np.float64)
        dx, dy, dz = g[:, 0] - x[0], g[:, 1] - x[1], g[:, 2] - x[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        margin = min(margin, np.abs(d2 - R * R).min())
        out.append(k[d2 <= R * R])
    return np.unique(np.concatenate(out), axis=0), margin


def contacts(pose, lig_r, prot_xyz, prot_z, prot_r=None, plan_status=0, grid_status=0, cutoff=5.0, clash_min=0.75, overlap_max=0.075,
             vdw_scale=0.8, spacing=0.5):
    """One (complex, pose): dict(stats float64 [3], counts [3], pair [2], flags, margins) with margins = dict(cutoff: the smallest
    |d - cutoff| over ALL ligand-protein pairs, lattice: the smallest |d^2 - R^2| of a membership test, close: the smallest
    |ratio - clash_min| of a pair within the cutoff)."""
    pose = np.asarray(pose, np.float32).reshape(-1, 3)
    lig_r = np.asarray(lig_r, np.float32).reshape(-1)
    nan3 = np.full(3, np.nan)
    none = dict(stats=nan3, counts=np.zeros(3, np.int64), pair=np.array([-1, -1]), margins=dict(cutoff=np.inf, lattice=np.inf, close=np.inf))
    if plan_status != 0 or grid_status != 0:
        return dict(none, flags=UNCHECKED)
    if not np.isfinite(pose).all():
        return dict(none, flags=NONFINITE)
    pxyz, pr, pid = kept(prot_xyz, prot_z, prot_r)
    margins = dict(cutoff=np.inf, lattice=np.inf, close=np.inf)
    i, j, d2 = close_pairs(pose, pxyz, cutoff)
    if len(pose) and len(pxyz):
        margins["cutoff"] = np.abs(np.sqrt(_d2(pose, pxyz)) - np.float64(np.float32(cutoff))).min()
    best, bi, bj, dmin = np.inf, None, None, np.inf
    n_close = 0
    if len(i):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.sqrt(d2) / (lig_r[i].astype(np.float64) + pr[j].astype(np.float64))
        cm = np.float64(np.float32(clash_min))
        n_close = int((ratio < cm).sum())
        margins["close"] = np.nanmin(np.abs(ratio - cm)) if not np.isnan(ratio).all() else np.inf
        dmin = np.sqrt(d2.min())
        for r, a, b in zip(ratio, i, pid[j]):
            if bi is None or _ahead(r, a, b, best, bi, bj):
                best, bi, bj = r, int(a), int(b)
    pts, m1 = lattice_points(pose, lig_r, vdw_scale, spacing)
    margins["lattice"] = m1
    n_lig, n_both = len(pts), 0
    if n_lig and len(pxyz):
        sp, sc = np.float64(np.float32(spacing)), np.float64(np.float32(vdw_scale))
        g = sp * pts.astype(np.float64)
        R = sc * pr.astype(np.float64)
        inside = np.zeros(n_lig, bool)
        for s in range(0, n_lig, 2048):
            dd = _d2(g[s:s + 2048], pxyz)
            margins["lattice"] = min(margins["lattice"], np.abs(dd - (R * R)[None]).min())
            inside[s:s + 2048] = (dd <= (R * R)[None]).any(1)
        n_both = int(inside.sum())
    overlap = n_both / n_lig if n_lig else 0.0
    stats = np.array([best, dmin, overlap])
    flags = 0
    with np.errstate(invalid="ignore"):
        if np.float32(best) < np.float32(clash_min):
            flags |= CLASH
        if np.float32(overlap) > np.float32(overlap_max):
            flags |= OVERLAP
    return dict(stats=stats, counts=np.array([n_close, n_lig, n_both]), pair=np.array([-1, -1] if bi is None else [bi, bj]), flags=flags,
                margins=margins)


def bound(col, v):
    """The bound of the device's float32 statistic against this float64 one: the device's float64 arithmetic is the restatement's up to
    a few 2^-53, so only the store rounds (U |v|); prot_clash and prot_dist are given 4 U |v|, overlap U |v|."""
    return (4.0 if col < 2 else 1.0) * U * abs(v)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def synthetic_protein(n, seed, density=0.06, min_sep=1.2, hydrogens=0.0, origin=(0.0, 0.0, 0.0)):
    """n heavy atoms (C, N, O, S) at protein-like density in a cube, no two closer than min_sep, by seeded sequential insertion; with
    hydrogens > 0 that share of extra Z = 1 atoms is interleaved at random places.  -> (xyz float32 [M, 3], z int64 [M])."""
    rng = np.random.RandomState(seed)
    side = (n / density) ** (1.0 / 3.0)
    pts = np.zeros((0, 3))
    while len(pts) < n:
        c = rng.uniform(0.0, side, size=(1, 3))
        if len(pts) == 0 or ((pts - c) ** 2).sum(1).min() >= min_sep * min_sep:
            pts = np.concatenate([pts, c])
    z = rng.choice([6, 6, 6, 7, 8, 16], size=n)
    nh = int(round(hydrogens * n))
    if nh:
        at = np.sort(rng.randint(0, n + 1, size=nh))
        pts = np.insert(pts, at, rng.uniform(0.0, side, size=(nh, 3)), axis=0)
        z = np.insert(z, at, 1)
    return (pts + np.asarray(origin)).astype(np.float32), z.astype(np.int64)


POSE_KINDS = ("inside", "surface", "coincident", "outside+x", "outside-x", "outside+y", "outside-y", "outside+z-corner", "beyond")


def poses_for(x0, prot_xyz, prot_z, seed, edge=5.0):
    """Nine rigid placements [9, n, 3] float32 of the conformer x0 around a synthetic protein, one per POSE_KINDS: its centroid at the
    protein's centre; at the middle of the +z face; the same with atom 0 moved onto a kept protein atom; wholly outside the cell box
    (of cells of `edge`) but within 0.5 A of one of four of its faces, so that the neighbouring cells fall out of range on that side
    while pairs within the cutoff remain; 8 A beyond a corner of the box; and 100 A away (the empty-set values)."""
    rng = np.random.RandomState(seed)
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    heavy = np.asarray(prot_xyz, np.float64)[np.asarray(prot_z) > 1]
    lo, hi = heavy.min(0), heavy.max(0)
    box_lo, box_hi = np.floor(lo / edge) * edge, (np.floor(hi / edge) + 1.0) * edge
    mid = 0.5 * (lo + hi)
    rel = x0 - x0.mean(0) if len(x0) else x0
    reach = np.abs(rel).max() if len(x0) else 0.0
    out = []
    for kind in POSE_KINDS:
        c = mid.copy()
        if kind in ("surface", "coincident"):
            c[2] = hi[2] + 1.0
        elif kind == "outside+z-corner":
            c = box_hi + 8.0 + reach
        elif kind.startswith("outside"):
            ax, sign = "xyz".index(kind[-1]), 1.0 if kind[-2] == "+" else -1.0
            c[ax] = (box_hi[ax] + 0.3 + reach) if sign > 0 else (box_lo[ax] - 0.3 - reach)
        elif kind == "beyond":
            c = hi + 100.0
        p = rel + c + rng.uniform(0.0, 0.2, size=3) * (np.sign(c - mid) + (c == mid))
        if kind == "coincident" and len(p):
            p[0] = heavy[np.argmin(((heavy - p[0]) ** 2).sum(1))]
        out.append(p.astype(np.float32))
    return np.stack(out) if len(x0) else np.zeros((len(POSE_KINDS), 0, 3), np.float32)


def stat_cases():
    """The complexes of the GPU statistics test: ligands of 1, 2, 63, 64 and 65 atoms (carbon chains) and two fixture ligands of
    tests/golden/conformer_ligands.npz, each with a synthetic protein of 600 heavy atoms (hydrogens interleaved) and the nine poses of
    `poses_for`; the last complex is the first fixture ligand again in a frame offset by (50, -50, 50) A.
    -> [dict(name, mol (with 'x'), z, prot_xyz, prot_z, poses [9, n, 3])]."""
    import conformer_refs as R
    from helpers import load_npz
    g = load_npz("conformer_ligands")
    mols = []
    for n in (1, 2, 63, 64, 65):
        m = R.chain(n)
        m["x"] = R.embed(m, seed=100 + n)
        mols.append((m, np.full(n, 6, np.int64)))
    fixtures = [(m, np.asarray(g[m["name"] + "_z"], np.int64)) for m in R.fixture_molecules(g)[:2]]
    mols += fixtures + [(dict(fixtures[0][0], name=fixtures[0][0]["name"] + "+50"), fixtures[0][1])]
    out = []
    for k, (m, z) in enumerate(mols):
        shift = (50.0, -50.0, 50.0) if k == len(mols) - 1 else (-7.5, -3.0, 0.0)      # (negative coordinates in every case)
        pxyz, pz = synthetic_protein(600, seed=300 + k, hydrogens=0.5, origin=shift)
        out.append(dict(name=m["name"], mol=m, z=z, prot_xyz=pxyz, prot_z=pz, poses=poses_for(m["x"], pxyz, pz, seed=500 + k)))
    return out
