"""Numpy restatement of fabind_amd.relax.relax_poses (csrc/pose_relax.hip): the start conformer moved over its rotatable-bond dihedrals
and one explicit rigid motion (a unit quaternion and a translation), held to a target pose and pushed out of contact with the protein
and with itself -- damped Gauss-Newton on

    E = w_fit sum_i |X_i - y_i|^2 + w_prot sum_{i,p} max(0, c_prot (r_i + r_p) - |X_i - P_p|)^2
      + w_intra sum_{i<j clash pairs} max(0, c_intra (r_i + r_j) - |X_i - X_j|)^2.

float64 by default; with dt=np.float32 the coordinates (the centred start conformer, the torsion pass, the pose, the angles) are rounded
to float32 as the kernel holds them, everything else stays float64.  The protein term is BRUTE FORCE over every kept protein atom, with
no cell list.  Molecules and plans come from conformer_refs / fit_refs / validity_refs, proteins from contact_refs; none is changed."""
import numpy as np

import conformer_refs as R
import contact_refs as C
import fit_refs as F
import validity_refs as V

MAX_ATOMS, MAX_TORSIONS = F.MAX_ATOMS, F.MAX_TORSIONS
STOP_CONVERGED, STOP_CAP, STOP_REJECTED, STOP_NONFINITE = 0, 1, 2, 3
STATUS_ATOMS, STATUS_TORSIONS, NO_INTRA, NO_PROTEIN = 3, 4, 8, 16
LAM0, LAM_MIN, MAX_REJECT = 1e-3, 1e-9, 8
DEFAULTS = dict(w_fit=1.0, w_prot=100.0, w_intra=100.0, c_prot=0.80, c_intra=0.75)
U = 2.0 ** -24


def _w(kw):
    """The five weights as the device reads them: float32 values in float64 arithmetic."""
    d = dict(DEFAULTS)
    d.update(kw)
    return {k: np.float64(np.float32(v)) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the objective
def terms(X, yc, P, rp, rl, clash, **weights):
    """The three unweighted sums, and per ligand atom A_i [n, 3, 3] and b_i [n, 3] with H = sum J_i^T A_i J_i, g = sum J_i^T b_i (and
    grad E = -2 g exactly).  X, yc: [n, 3]; P [K, 3], rp [K]: the kept protein atoms in the frame of X (None: no protein term); rl [n];
    clash: bool [n, n] symmetric, the PAIR_CLASH pairs (None: no intra term).  A pair is active iff d < reach; at d = 0 it has an energy
    and no direction.  For the intra pairs A holds the majorant 2 w n n^T on both atoms in place of the cross terms."""
    w = _w(weights)
    X, yc = np.asarray(X, np.float64), np.asarray(yc, np.float64)
    n = len(X)
    r = yc - X
    sums = np.array([(r * r).sum(), 0.0, 0.0])
    A = np.tile(w["w_fit"] * np.eye(3), (n, 1, 1))
    b = w["w_fit"] * r
    rl = np.asarray(rl, np.float32).astype(np.float64)

    def push(e, reach, mask, count, wt, mult):
        d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        act = mask & (d < reach)
        rho = np.where(act, reach - d, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            nv = np.where((act & (d > 0))[..., None], e / d[..., None], 0.0)
        return (rho[count] ** 2).sum(), mult * wt * np.einsum("ipa,ipb->iab", nv, nv), wt * (rho[..., None] * nv).sum(1)
    if P is not None and len(P) and n:
        P = np.asarray(P, np.float64)
        reach = w["c_prot"] * (rl[:, None] + np.asarray(rp, np.float32).astype(np.float64)[None])
        every = np.ones(reach.shape, bool)
        sums[1], dA, db = push(X[:, None, :] - P[None], reach, every, every, w["w_prot"], 1.0)
        A, b = A + dA, b + db
    if clash is not None and n:
        reach = w["c_intra"] * (rl[:, None] + rl[None])
        sums[2], dA, db = push(X[:, None, :] - X[None], reach, np.asarray(clash, bool), np.triu(np.asarray(clash, bool), 1), w["w_intra"], 2.0)
        A, b = A + dA, b + db
    return sums, A, b


def total(sums, **weights):
    w = _w(weights)
    return float((w["w_fit"] * sums[0] + w["w_prot"] * sums[1]) + w["w_intra"] * sums[2])


def normal_equations(X, A, b, quad, side, moving=None):
    """H [M, M] and g [M], M = T + 6, with the Jacobian of fit_refs (torsions, three translations, three rotations about the centroid)."""
    n = len(X)
    J = F.jacobian(X, quad, side, moving).reshape(n, 3, -1)
    return np.einsum("iac,iab,ibd->cd", J, A, J), np.einsum("iac,ia->c", J, b)


# ------------------------------------------------------------------------------------------------ the rigid motion
def horn_quat(P, Y):
    """(unit quaternion q, cp, cy) of fit_refs.horn: image = R(q) (P - cp) + cy."""
    P, Y = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Y, np.float64).reshape(-1, 3)
    cp, cy = P.mean(0), Y.mean(0)
    S = (P - cp).T @ (Y - cy)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, v = F.jacobi_eigh4(N)
    q = v[:, int(np.argmax(w))]
    return q / np.linalg.norm(q), cp, cy


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_exp(omega):
    th = float(np.sqrt(omega @ omega))
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) / th * omega])


def rigid_step(q, t, c, tau, omega):
    """R' = exp(omega) R, t' = c + exp(omega) (t - c) + tau; the quaternion renormalised."""
    qe = quat_exp(np.asarray(omega, np.float64))
    q2 = quat_mul(qe, q)
    q2 = q2 / np.sqrt(q2 @ q2)
    return q2, c + F.quaternion_rotation(qe) @ (t - c) + tau


def pose(x0c, quad, side, a, q, t, dt=np.float64, moving=None):
    """X(a, R, t) = R torsions(x0c, a) + t: the torsion pass in dt, the rigid motion in float64, the result rounded to dt."""
    p = F.apply_torsions(x0c, quad, side, a, dt, moving).astype(np.float64)
    return (p @ F.quaternion_rotation(q).T + t).astype(dt)


# ------------------------------------------------------------------------------------------------ the relaxation
def relax_one(x0, y, quad, side, cls, radii, prot_xyz=None, prot_r=None, angles0=None, vstatus=0, gstatus=0, max_iters=100, tol=1e-6,
              dt=np.float64, **weights):
    """One (complex, pose).  x0, y: [n, 3]; quad / side: the ligand's torsions; cls [n, n] pair classes and radii [n] of its validity
    plan (vstatus != 0: no intra term); prot_xyz [K, 3] / prot_r [K]: the KEPT protein atoms in the frame of y (gstatus != 0: no protein
    term).  -> dict(coords [n, 3] float64, angles [T], energy0 [3], energy [3], iters, stop, trace, status, X (centred frame), cy)."""
    x0, y = np.asarray(x0, np.float64).reshape(-1, 3), np.asarray(y, np.float64).reshape(-1, 3)
    n, T = len(x0), len(quad)
    tol = float(np.float32(tol))
    nan3 = np.full(3, np.nan)
    status = (NO_INTRA if vstatus != 0 else 0) | (NO_PROTEIN if gstatus != 0 else 0)
    status |= STATUS_ATOMS if n > MAX_ATOMS else STATUS_TORSIONS if T > MAX_TORSIONS else 0
    base = dict(angles=np.zeros(T), iters=0, stop=STOP_CONVERGED if max_iters > 0 else STOP_CAP, trace=[], status=status)
    if n == 0:
        return dict(base, coords=np.zeros((0, 3)), energy0=np.zeros(3), energy=np.zeros(3))
    if not (np.isfinite(y).all() and np.isfinite(x0).all()):
        return dict(base, coords=np.full((n, 3), np.nan), angles=np.full(T, np.nan), energy0=nan3, energy=nan3, stop=STOP_NONFINITE)
    if n > MAX_ATOMS:
        X = F.rigid_image(x0, y).astype(dt).astype(np.float64)
        e = np.array([((X - y) ** 2).sum(), np.nan, np.nan])
        return dict(base, coords=X, energy0=e, energy=e)
    a = np.zeros(T, dt) if angles0 is None else np.asarray(angles0, np.float64).astype(dt)
    if T > MAX_TORSIONS:
        quad, side, a = quad[:0], side[:0], a[:0]
    cy = y.mean(0)
    yc = y - cy
    x0c = (x0 - x0.mean(0)).astype(dt)
    mv = F.moving_atoms(quad, side, n)
    P = rp = clash = None
    if gstatus == 0 and prot_xyz is not None:
        P, rp = np.asarray(prot_xyz, np.float32).astype(np.float64) - cy, np.asarray(prot_r, np.float32)
    if vstatus == 0:
        clash = np.asarray(cls) == 3
    p0 = F.apply_torsions(x0c, quad, side, a, dt, mv)
    q, cp, cyc = horn_quat(p0, yc)
    t = cyc - F.quaternion_rotation(q) @ cp
    X = pose(x0c, quad, side, a, q, t, dt, mv)
    sums, A, b = terms(X, yc, P, rp, radii, clash, **weights)
    E = total(sums, **weights)
    sums0, lam, iters, stop, trace = sums, LAM0, 0, base["stop"], []
    done = max_iters <= 0 or E == 0.0
    while not done:
        X64 = X.astype(np.float64)
        H, g = normal_equations(X64, A, b, quad, side, mv)
        c = X64.mean(0)
        rejected = 0
        while True:
            Et = np.inf
            try:
                L = np.linalg.cholesky(H + lam * np.diag(np.diag(H) + 1e-12))
                d = np.linalg.solve(L.T, np.linalg.solve(L, g))
                at = F.wrap(a.astype(np.float64) + d[:len(quad)]).astype(dt)
                qt, tt = rigid_step(q, t, c, d[len(quad):len(quad) + 3], d[len(quad) + 3:])
                Xt = pose(x0c, quad, side, at, qt, tt, dt, mv)
                st, At, bt = terms(Xt, yc, P, rp, radii, clash, **weights)
                Et = total(st, **weights)
            except np.linalg.LinAlgError:
                pass
            if Et < E:
                small = E - Et <= tol * E
                E, a, q, t, X, sums, A, b = Et, at, qt, tt, Xt, st, At, bt
                lam = max(lam / 10.0, LAM_MIN)
                iters += 1
                trace.append(E)
                if small:
                    stop, done = STOP_CONVERGED, True
                elif iters >= max_iters:
                    stop, done = STOP_CAP, True
                break
            lam *= 10.0
            rejected += 1
            if rejected >= MAX_REJECT:
                stop, done = STOP_REJECTED, True
                break
    angles = np.zeros(T)
    angles[:len(a)] = a
    return dict(coords=X.astype(np.float64) + cy, angles=angles, energy0=sums0, energy=sums, iters=iters, stop=stop, trace=trace,
                status=status, X=X.astype(np.float64), cy=cy, quat=q, trans=t)


def energy_of(coords, y, cls, radii, prot_xyz=None, prot_r=None, vstatus=0, gstatus=0, **weights):
    """The three sums of E on given coordinates, in the frame of the target's centroid as `relax_one` forms it, and the 1-norm of
    dE/dX (the sensitivity of E to a perturbation of every coordinate): -> (sums [3], |dE/dX|_1)."""
    y = np.asarray(y, np.float64).reshape(-1, 3)
    cy = y.mean(0)
    P = rp = None
    if gstatus == 0 and prot_xyz is not None:
        P, rp = np.asarray(prot_xyz, np.float32).astype(np.float64) - cy, prot_r
    sums, _, b = terms(np.asarray(coords, np.float64) - cy, y - cy, P, rp, radii, (np.asarray(cls) == 3) if vstatus == 0 else None, **weights)
    return sums, 2.0 * float(np.abs(b).sum())


# ------------------------------------------------------------------------------------------------ statistics of the two checks
def prot_clash(coords, lig_r, prot_xyz, prot_r):
    """min d / (r_i + r_p) over all ligand-protein pairs (inf without one)."""
    if not len(coords) or prot_xyz is None or not len(prot_xyz):
        return np.inf
    d = np.sqrt(C._d2(np.asarray(coords, np.float64), np.asarray(prot_xyz, np.float32)))
    return float((d / (np.asarray(lig_r, np.float64)[:, None] + np.asarray(prot_r, np.float64)[None])).min())


def clash(coords, lig_r, cls):
    """min d / (r_i + r_j) over the PAIR_CLASH pairs (inf without one)."""
    ii, jj = np.nonzero(np.triu(np.asarray(cls) == 3, 1))
    if not len(ii):
        return np.inf
    x, r = np.asarray(coords, np.float64), np.asarray(lig_r, np.float64)
    return float((np.sqrt(((x[ii] - x[jj]) ** 2).sum(1)) / (r[ii] + r[jj])).min())


# ------------------------------------------------------------------------------------------------ the committed cases
CARVE, TARGETS_PER_MOLECULE = 0.95, 3
AMP, ROT_SIGMA, SHIFT_SIGMA = 0.3, 0.1, 0.5
OFFSET = np.array([50.0, -50.0, 50.0])


def atomic_numbers(m, g):
    if m["name"] + "_z" in g:
        return np.asarray(g[m["name"] + "_z"], np.int64)
    return np.asarray(V.HAND_Z.get(m["name"], [6] * m["n"]), np.int64)


def carve(prot_xyz, prot_z, lig_x, lig_r, frac=CARVE):
    """The protein without every heavy atom with d / (r_i + r_p) < frac to some ligand atom (hydrogens stay): a snug pocket."""
    prot_xyz, prot_z = np.asarray(prot_xyz, np.float32), np.asarray(prot_z, np.int64)
    pr = C.bondi(prot_z).astype(np.float64)
    d = np.sqrt(C._d2(np.asarray(lig_x, np.float32), prot_xyz))
    hit = ((d / (np.asarray(lig_r, np.float64)[:, None] + pr[None])) < frac).any(0) & (prot_z > 1)
    return prot_xyz[~hit], prot_z[~hit]


def complexes(g):
    """The 13 molecules of fit_refs.molecules_with_torsions, each placed at the centre of contact_refs.synthetic_protein(600,
    seed=300 + k) (hydrogens interleaved) with its pocket carved, plus the first recorded ligand again in a frame offset by
    (50, -50, 50) A.  -> [dict(name, mol (x = the start conformer), z, vplan, placed float32 [n, 3], prot_xyz, prot_z, kept (xyz, r))]."""
    mols = F.molecules_with_torsions(g)
    first = [k for k, m in enumerate(mols) if m["name"] + "_z" in g][0]
    out = []
    for k, m in enumerate(mols + [dict(mols[first], name=mols[first]["name"] + "+50")]):
        z = atomic_numbers(mols[first] if k == len(mols) else m, g)
        origin = OFFSET if k == len(mols) else np.array([-7.5, -3.0, 0.0])
        pxyz, pz = C.synthetic_protein(600, seed=300 + k, hydrogens=0.5, origin=tuple(origin))
        heavy = pxyz[pz > 1].astype(np.float64)
        x = np.asarray(m["x"], np.float64)
        placed = (x - x.mean(0) + 0.5 * (heavy.min(0) + heavy.max(0))).astype(np.float32)
        vp = V.plan(m, z, np.asarray(m["x"], np.float32))
        pxyz, pz = carve(pxyz, pz, placed, vp["radii"])
        kx, kr, _ = C.kept(pxyz, pz)
        out.append(dict(name=m["name"], mol=m, z=z, vplan=vp, placed=placed, prot_xyz=pxyz, prot_z=pz, kept=(kx, kr)))
    return out


def make_target(c, seed):
    """The placement with every torsion changed by a uniform angle in +-0.3 rad, rotated about its centroid by a rotation vector of
    0.1 sigma rad and shifted by 0.5 A sigma; float32, as the device reads it."""
    rng = np.random.RandomState(seed)
    m = c["mol"]
    ang = rng.uniform(-AMP, AMP, len(m["quad"]))
    p = R.perturb_one(c["placed"].astype(np.float64), m["quad"], m["side"], ang, (0, 0, 0), relative=True, rotate=False, centre=False)
    Rm = F.quaternion_rotation(quat_exp(ROT_SIGMA * rng.randn(3)))
    ctr = p.mean(0)
    return ((p - ctr) @ Rm.T + ctr + SHIFT_SIGMA * rng.randn(3)).astype(np.float32)


def target_seed(k, s):
    return 7000 + 10 * k + s


# (complex, target) of `complexes` / `make_target(c, target_seed(k, s))`: the cases of the comparison with the device.  Chosen once, by
# the float64 and the float32-pose restatement alone: both end within 1e-3 A RMSD of each other (test_relax_refs_cpu.py asserts it).
CASES = ((0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 2), (3, 1), (4, 0), (4, 1), (4, 2), (6, 0), (6, 1), (6, 2), (7, 1), (8, 1), (9, 0), (9, 1),
         (9, 2), (10, 0), (10, 1), (11, 0), (12, 0), (12, 2), (13, 0), (13, 2))
ALL_TARGETS = tuple((k, s) for k in range(13) for s in range(TARGETS_PER_MOLECULE))    # the 39 targets of the host experiment


class Results:
    """The restatement on the committed cases, each run once per precision and shared by the tests of a module."""

    def __init__(self, g):
        self.cx = complexes(g)
        self._runs = {}

    def run(self, k, s, dt=np.float64, **kw):
        key = (k, s, dt, tuple(sorted(kw.items())))
        if key not in self._runs:
            self._runs[key] = run_case(self.cx, k, s, dt, **kw)
        return self._runs[key]

    def row(self, k, s, **kw):
        """dict(E64, E32, d32: RMSD between the two results, prot0 / prot1, clash0 / clash1: the two checks' statistics at the fitted
        pose and at the float64 result, rmsd: the float64 result to the target, flagged0, clean1)."""
        c = self.cx[k]
        y, fit, o64 = self.run(k, s, **kw)
        _, _, o32 = self.run(k, s, np.float32, **kw)
        r, cl = c["vplan"]["radii"], c["vplan"]["cls"]
        row = dict(E64=total(o64["energy"], **kw), E32=total(o32["energy"], **kw), d32=F.rmsd(o64["coords"], o32["coords"]),
                   prot0=prot_clash(fit["coords"], r, *c["kept"]), prot1=prot_clash(o64["coords"], r, *c["kept"]),
                   clash0=clash(fit["coords"], r, cl), clash1=clash(o64["coords"], r, cl), rmsd=F.rmsd(o64["coords"], y))
        row["flagged0"] = row["prot0"] < 0.75 or row["clash0"] < 0.70
        row["clean1"] = row["prot1"] >= 0.75 + 1e-3 and row["clash1"] >= 0.70 + 1e-3
        return row


def run_case(cx, k, s, dt=np.float64, fit_iters=50, **kw):
    """Case (k, s): the float64 fit's angles (`fit_refs.fit_one`), rounded to float32, as the start, then the relaxation in dt.  -> (target, fit result, relax result)."""
    c = cx[k]
    m = c["mol"]
    y = make_target(c, target_seed(k, s))
    fit = F.fit_one(m["x"], y, m["quad"], m["side"], max_iters=fit_iters)
    out = relax_one(m["x"], y, m["quad"], m["side"], c["vplan"]["cls"], c["vplan"]["radii"], c["kept"][0], c["kept"][1],
                    angles0=fit["angles"].astype(np.float32), dt=dt, **kw)
    return y, fit, out
