"""Numpy restatement of fabind_amd.conformer.fit_conformers (csrc/conformer_fit.hip): fit the start conformer to a target pose over
its rotatable-bond dihedrals and one rigid motion -- damped Gauss-Newton (Levenberg-Marquardt) on E(a) = sum |pose(a) - y|^2, the
rigid part solved exactly inside `pose` by Horn's quaternion method.  float64 by default; with dt=np.float32 the coordinates (the
centred start conformer, the torsion pass, the pose after the rigid fit, the angles) are rounded to float32 as the kernel holds them,
while the rigid fit, the normal matrix and its solve stay in float64.  Molecules, plans and `perturb_one` come from conformer_refs."""
import numpy as np

import conformer_refs as R

MAX_ATOMS, MAX_TORSIONS = 256, 58
STOP_CONVERGED, STOP_CAP, STOP_REJECTED = 0, 1, 2
STATUS_OK, STATUS_ATOMS, STATUS_TORSIONS = 0, 3, 4
JACOBI_SWEEPS = 16
LAM0, LAM_MIN, MAX_REJECT = 1e-3, 1e-9, 8


# ------------------------------------------------------------------------------------------------ rigid fit
def jacobi_eigh4(A):
    """Eigenvalues and eigenvectors (columns) of a symmetric 4 x 4 matrix by cyclic Jacobi, at most JACOBI_SWEEPS sweeps over the six
    pairs in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a rotation whose off-diagonal entry no longer changes either diagonal
    entry zeroes it instead."""
    a = np.array(A, np.float64)
    v = np.eye(4)
    for _ in range(JACOBI_SWEEPS):
        off = sum(abs(a[p, q]) for p in range(4) for q in range(p + 1, 4))
        if off == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                g = 100.0 * abs(apq)
                if abs(a[p, p]) + g == abs(a[p, p]) and abs(a[q, q]) + g == abs(a[q, q]):
                    a[p, q] = a[q, p] = 0.0
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                G = np.eye(4)
                G[p, p] = G[q, q] = c
                G[p, q], G[q, p] = s, -s
                a = G.T @ a @ G
                a[p, q] = a[q, p] = 0.0
                v = v @ G
    return np.diag(a).copy(), v


def quaternion_rotation(q):
    q0, qx, qy, qz = q / np.linalg.norm(q)
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                     [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                     [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])


def horn(P, Y):
    """The proper rotation Rm and the centroids (cp, cy) with sum |Rm (P_i - cp) + cy - Y_i|^2 minimal (Horn 1987): the eigenvector of
    the largest eigenvalue (the first of equal ones) of the 4 x 4 matrix of the cross-covariance, as a unit quaternion."""
    P, Y = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Y, np.float64).reshape(-1, 3)
    cp, cy = P.mean(0), Y.mean(0)
    S = (P - cp).T @ (Y - cy)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, v = jacobi_eigh4(N)
    return quaternion_rotation(v[:, int(np.argmax(w))]), cp, cy


def rigid_image(P, Y):
    """P moved rigidly onto Y (float64)."""
    Rm, cp, cy = horn(P, Y)
    return (np.asarray(P, np.float64) - cp) @ Rm.T + cy


def kabsch_svd(P, Y):
    """The same image by the SVD route with the determinant correction: an independent check of `horn`."""
    P, Y = np.asarray(P, np.float64), np.asarray(Y, np.float64)
    cp, cy = P.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Y - cy))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    return (P - cp) @ (U @ D @ Vt) + cy


# ------------------------------------------------------------------------------------------------ pose and Jacobian
def wrap(a):
    """Angles to (-pi, pi]."""
    a = np.asarray(a, np.float64)
    return a - 2.0 * np.pi * np.ceil((a - np.pi) / (2.0 * np.pi))


def moving_atoms(quad, side, n):
    """Per torsion the atoms it moves (side without k), or None for a torsion that names an atom outside the ligand."""
    out = []
    for q, w in zip(quad, side):
        ok = all(0 <= int(v) < n for v in q)
        out.append(np.asarray([i for i in R.side_atoms(w) if i < n and i != int(q[2])], np.int64) if ok else None)
    return out


def apply_torsions(x0, quad, side, a, dt=np.float64, moving=None):
    """The torsions applied one after another as relative rotations by a[t]: the rule of conformer_perturb_kernel."""
    p = np.array(x0, dtype=dt)
    n = len(p)
    moving = moving_atoms(quad, side, n) if moving is None else moving
    for t in range(len(quad)):
        q = [int(v) for v in quad[t]]
        if moving[t] is None:
            continue
        axis = p[q[2]] - p[q[1]]
        l2 = dt(axis @ axis)
        if l2 == 0:
            continue
        u = (axis / np.sqrt(l2)).astype(dt)
        cs, sn = dt(np.cos(dt(a[t]))), dt(np.sin(dt(a[t])))
        idx = moving[t]
        if len(idx):
            v = p[idx] - p[q[1]]
            d = (v @ u)[:, None].astype(dt) * (dt(1) - cs)
            p[idx] = (p[q[1]] + (v * cs + np.cross(u[None, :], v).astype(dt) * sn + u[None, :] * d)).astype(dt)
    return p


def pose(x0c, yc, quad, side, a, dt=np.float64, moving=None):
    """pose(a) in the frame of the centred target yc: torsions on the centred start conformer, then the optimal rigid motion."""
    p = apply_torsions(x0c, quad, side, a, dt, moving)
    return rigid_image(p, yc).astype(dt)


def jacobian(X, quad, side, moving=None):
    """J [3 n, T + 6] of pose at X: torsion t -> u_t x (X_i - X_j) on the moving side (k excepted), three translations, three rotations
    e_d x (X_i - centroid)."""
    X = np.asarray(X, np.float64)
    n, T = len(X), len(quad)
    J = np.zeros((n, 3, T + 6))
    moving = moving_atoms(quad, side, n) if moving is None else moving
    for t in range(T):
        q = [int(v) for v in quad[t]]
        if moving[t] is None:
            continue
        axis = X[q[2]] - X[q[1]]
        l2 = axis @ axis
        if l2 == 0:
            continue
        u = axis / np.sqrt(l2)
        idx = moving[t]
        if len(idx):
            J[idx, :, t] = np.cross(u[None, :], X[idx] - X[q[1]])
    c = X.mean(0)
    for d in range(3):
        e = np.zeros(3)
        e[d] = 1.0
        J[:, :, T + d] = e
        J[:, :, T + 3 + d] = np.cross(e[None, :], X - c)
    return J.reshape(3 * n, T + 6)


# ------------------------------------------------------------------------------------------------ the fit
def fit_one(x0, y, quad, side, max_iters=50, tol=1e-6, dt=np.float64):
    """One (ligand, pose).  -> dict(coords [n, 3] float64, angles [T], rmsd0, rmsd, iters, stop, trace [iters], status)."""
    x0, y = np.asarray(x0, np.float64).reshape(-1, 3), np.asarray(y, np.float64).reshape(-1, 3)
    n, T = len(x0), len(quad)
    if n == 0:
        return dict(coords=np.zeros((0, 3)), angles=np.zeros(T), rmsd0=0.0, rmsd=0.0, iters=0, stop=STOP_CONVERGED, trace=[], status=STATUS_OK)
    status = STATUS_ATOMS if n > MAX_ATOMS else STATUS_TORSIONS if T > MAX_TORSIONS else STATUS_OK
    if status != STATUS_OK:
        quad, side = quad[:0], side[:0]
    cy = y.mean(0)
    yc = y - cy
    x0c = (x0 - x0.mean(0)).astype(dt)
    a = np.zeros(len(quad), dt)
    mv = moving_atoms(quad, side, n)
    X = pose(x0c, yc, quad, side, a, dt, mv)
    E = float(((X.astype(np.float64) - yc) ** 2).sum())
    E0, lam, iters, stop, trace = E, LAM0, 0, STOP_CONVERGED, []
    if max_iters <= 0:
        stop = STOP_CAP
    done = len(quad) == 0 or n <= 2 or max_iters <= 0
    while not done:
        X64 = X.astype(np.float64)
        J = jacobian(X64, quad, side, mv)
        r = (yc - X64).reshape(-1)
        H, g = J.T @ J, J.T @ r
        rejected = 0
        while True:
            A = H + lam * np.diag(np.diag(H) + 1e-12)
            Et = np.inf
            try:
                L = np.linalg.cholesky(A)
                d = np.linalg.solve(L.T, np.linalg.solve(L, g))
                at = wrap(a.astype(np.float64) + d[:len(quad)]).astype(dt)
                Xt = pose(x0c, yc, quad, side, at, dt, mv)
                Et = float(((Xt.astype(np.float64) - yc) ** 2).sum())
            except np.linalg.LinAlgError:
                pass
            if Et < E:
                small = E - Et <= tol * E
                E, a, X = Et, at, Xt
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
    return dict(coords=X.astype(np.float64) + cy, angles=angles, rmsd0=float(np.sqrt(E0 / n)), rmsd=float(np.sqrt(E / n)), iters=iters,
                stop=stop, trace=trace, status=status)


def rmsd(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max(len(a), 1)))


# ------------------------------------------------------------------------------------------------ cases
def random_rotation(rng):
    q = rng.randn(4)
    return quaternion_rotation(q)


def molecules_with_torsions(fixture):
    """The molecules of the recovery experiment: hand molecules, chains of 8 / 20 / 40 atoms and the recorded ligands, those with at
    least one torsion, each with its coordinates, plan and name."""
    hand = [m for _, (m, _) in sorted(R.hand_molecules().items())]
    out = []
    for i, m in enumerate(hand + [R.chain(8), R.chain(20), R.chain(40)] + R.fixture_molecules(fixture)):
        q, s, st = R.plan(m["n"], m["bonds"], m["codes"])
        if st == 0 and len(q):
            x = np.asarray(m["x"] if "x" in m else R.embed(m, seed=17 + i), np.float64)
            out.append(dict(m, x=x, quad=q, side=s))
    return out


def make_target(m, rng, amp, noise=0.0):
    """The start conformer with every torsion changed by a uniform angle in +-amp, a random rotation and shift [and Gaussian noise].
    -> (target, the noise-free target, the angles)."""
    ang = rng.uniform(-amp, amp, len(m["quad"]))
    p = R.perturb_one(m["x"], m["quad"], m["side"], ang, (0, 0, 0), relative=True, rotate=False, centre=False)
    clean = p @ random_rotation(rng).T + rng.uniform(-10, 10, 3)
    return clean + noise * rng.randn(*clean.shape), clean, ang
