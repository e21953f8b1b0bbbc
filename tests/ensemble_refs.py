"""Float64 numpy restatements for fabind_amd/ensemble.py (csrc/conformer_rmsd.hip): the superposed, symmetry-corrected RMSD formulated
independently of the kernel (SVD Kabsch with the determinant correction, the rotation applied, the residual summed explicitly, the minimum
over an automorphism list), the same value through Horn's quaternion eigenvalue, greedy RMSD pruning as the prose rule, the bound of the
GPU tests and the case builders.  Imported by the CPU and the GPU tests: every case is built once and shared."""
import functools

import numpy as np

from pose_cluster_refs import _rot, chain_autos, fixture_autos, leader_cluster_ref, ring_autos  # noqa: F401  (re-exported)

THRESHOLD = 0.5
MARGIN = 1e-3          # the mode generator keeps every float64 distance this far from the threshold
NOISES = (0.0, 1e-4, 0.3)


def centred(x):
    x = np.asarray(x, dtype=np.float64)
    return x - x.mean(0) if len(x) else x


def kabsch_e(p, y, allow_mirror=False):
    """p, y [.., n, 3] CENTRED -> (sum_i |R p_i - y_i|^2 summed explicitly, R [.., 3, 3]), R the best proper rotation (any orthogonal
    matrix with allow_mirror) from the SVD of sum_i p_i y_i^T."""
    H = np.einsum("...ni,...nj->...ij", p, y)
    U, _, Vt = np.linalg.svd(H)
    d = np.ones(H.shape[:-2] + (3,))
    if not allow_mirror:
        d[..., 2] = np.sign(np.linalg.det(np.einsum("...ji,...kj->...ik", Vt, U)))      # det(V U^T)
        d[..., 2] = np.where(d[..., 2] == 0, 1.0, d[..., 2])
    R = np.einsum("...ji,...j,...kj->...ik", Vt, d, U)                                   # V diag(d) U^T
    r = np.einsum("...ij,...nj->...ni", R, p) - y
    return (r * r).sum((-1, -2)), R


def horn_matrix(S):
    """S [.., 3, 3] = sum p y^T -> Horn's symmetric 4 x 4 matrix [.., 4, 4]."""
    N = np.zeros(S.shape[:-2] + (4, 4))
    N[..., 0, 0] = S[..., 0, 0] + S[..., 1, 1] + S[..., 2, 2]
    N[..., 1, 1] = S[..., 0, 0] - S[..., 1, 1] - S[..., 2, 2]
    N[..., 2, 2] = -S[..., 0, 0] + S[..., 1, 1] - S[..., 2, 2]
    N[..., 3, 3] = -S[..., 0, 0] - S[..., 1, 1] + S[..., 2, 2]
    N[..., 0, 1] = N[..., 1, 0] = S[..., 1, 2] - S[..., 2, 1]
    N[..., 0, 2] = N[..., 2, 0] = S[..., 2, 0] - S[..., 0, 2]
    N[..., 0, 3] = N[..., 3, 0] = S[..., 0, 1] - S[..., 1, 0]
    N[..., 1, 2] = N[..., 2, 1] = S[..., 0, 1] + S[..., 1, 0]
    N[..., 1, 3] = N[..., 3, 1] = S[..., 2, 0] + S[..., 0, 2]
    N[..., 2, 3] = N[..., 3, 2] = S[..., 1, 2] + S[..., 2, 1]
    return N


def _autos(autos, n):
    return np.arange(n).reshape(1, n) if autos is None or len(autos) == 0 or n == 0 else np.asarray(autos, dtype=np.int64).reshape(-1, n)


def pair_e_all(xs, yt, autos=None, allow_mirror=False):
    """E_k = min over proper rotations of sum_i |R (x_s[a_k[i]] - c_s) - (y_t[i] - c_t)|^2 for every automorphism -> [K]."""
    n = len(xs)
    if n == 0:
        return np.zeros(1)
    a = _autos(autos, n)
    return kabsch_e(centred(xs)[a], centred(yt)[None], allow_mirror)[0]


def pair_e_all_quat(xs, yt, autos=None):
    """The same through the quaternion eigenvalue: max(0, G_s + G_t - 2 lambda_k)."""
    n = len(xs)
    if n == 0:
        return np.zeros(1)
    a = _autos(autos, n)
    p, y = centred(xs), centred(yt)
    S = np.einsum("kni,nj->kij", p[a], y)
    lam = np.linalg.eigvalsh(horn_matrix(S))[..., -1]
    return np.maximum(0.0, (p * p).sum() + (y * y).sum() - 2.0 * lam)


def aligned_rmsd_ref(X, Y=None, autos=None, e_fn=pair_e_all):
    """X [S, n, 3] against Y [T, n, 3] (Y=None: X against itself, s < t computed and mirrored, zero diagonal).
    -> dict(D [S, T], k [S, T] the argmin (lowest index on ties), gap [S, T]: second-smallest E minus smallest (inf for K = 1),
    G [S, T] = G_s + G_t)."""
    X = np.asarray(X, dtype=np.float64)
    pair = Y is None
    Y = X if pair else np.asarray(Y, dtype=np.float64)
    S, T, n = len(X), len(Y), X.shape[1]
    D, k, gap = np.zeros((S, T)), np.zeros((S, T), np.int64), np.full((S, T), np.inf)
    g = lambda x: float((centred(x) ** 2).sum())                                         # noqa: E731
    G = np.array([[g(X[s]) + g(Y[t]) for t in range(T)] for s in range(S)]).reshape(S, T)
    for s in range(S):
        for t in range(s + 1 if pair else 0, T):
            E = e_fn(X[s], Y[t], autos)
            o = np.argsort(E, kind="stable")
            D[s, t], k[s, t] = np.sqrt(E[o[0]] / max(n, 1)), o[0]
            if len(E) > 1:
                gap[s, t] = E[o[1]] - E[o[0]]
            if pair:
                D[t, s], k[t, s], gap[t, s] = D[s, t], k[s, t], gap[s, t]
    return dict(D=D, k=k, gap=gap, G=G)


def bound_d2(n, G, D):
    """|D_dev^2 - D_ref^2| <= (4 n + 64) 2^-53 (G_s + G_t) / n + 2^-22 D_ref^2."""
    return (4 * n + 64) * 2.0 ** -53 * np.asarray(G) / max(n, 1) + 2.0 ** -22 * np.asarray(D) ** 2


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (y * x + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (z * x - w * y), 2 * (z * y + w * x), w * w - x * x - y * y + z * z]])


def fit_rmsd(xs, yt, a, q, trans):
    """The RMSD of R(q) x_s[a[i]] + trans against y_t[i], recomputed in float64."""
    xs, yt = np.asarray(xs, np.float64), np.asarray(yt, np.float64)
    if len(xs) == 0:
        return 0.0
    r = xs[a] @ quat_matrix(q).T + trans - yt
    return float(np.sqrt((r * r).sum() / len(xs)))


def prune_ref(D, key, thr, valid=None):
    """The prose rule on one ligand: go through the valid conformers in ascending key (ties in conformer order, NaN keys last); keep a
    conformer iff no conformer kept before it is strictly within thr.  -> (keep bool [S], kept indices in the order they were kept)."""
    D, key = np.asarray(D), np.asarray(key, dtype=np.float64)
    S = len(key)
    valid = np.ones(S, bool) if valid is None else np.asarray(valid, bool)
    key = np.where(np.isnan(key), np.inf, key)
    kept = []
    for c in sorted(np.nonzero(valid)[0], key=lambda i: (key[i], i)):
        if not any(D[u, c] < thr for u in kept):
            kept.append(int(c))
    keep = np.zeros(S, bool)
    keep[kept] = True
    return keep, kept


def random_conformers(rng, S, n, autos=None, shift=None, n_shapes=3):
    """S conformers of n atoms: random rigid images of `n_shapes` base shapes under a random automorphism, plus noise of 0, 1e-4 or
    0.3 A (conformer s: shape s mod n_shapes, noise NOISES[(s // n_shapes) mod 3]); `shift` moves the whole frame.  float32 [S, n, 3]."""
    a_all = _autos(autos, n)
    shapes = [rng.normal(scale=2.0, size=(n, 3)) for _ in range(n_shapes)]
    out = []
    for s in range(S):
        x = shapes[s % n_shapes][a_all[rng.integers(len(a_all))]] if n else np.zeros((0, 3))
        x = x + rng.normal(scale=NOISES[(s // n_shapes) % 3] / np.sqrt(3.0), size=(n, 3)) if NOISES[(s // n_shapes) % 3] else x
        x = x @ _rot(rng).T + rng.normal(scale=3.0, size=3)
        out.append(x + (0.0 if shift is None else np.asarray(shift)))
    return np.asarray(out, dtype=np.float32).reshape(S, n, 3)


# (two atoms are superposed equally well both ways round: every entry of that case ties, so it is kept small)
SPEC = [("single_atom n1 K1 S7", "single_atom", 7), ("chain n2 K2 S2", 2, 2), ("chain n3 K2 S8", 3, 8), ("chain_mixed n4 K1 S9", "chain_mixed", 9),
        ("neopentane n5 K24 S8", "neopentane", 8), ("benzene n6 K12 S17", "benzene", 17), ("c60 n60 K120 S3", "c60", 3),
        ("druglike_61 S9", "druglike_61", 9), ("ring n63 K126 S3", -63, 3), ("ring n64 K128 S2", -64, 2), ("ring n65 K130 S3", -65, 3),
        ("chain n255 K2 S3", 255, 3), ("chain n256 K2 S3", 256, 3), ("chain n257 K2 S3", 257, 3), ("plain n300 Knone S2", None, 2),
        ("far benzene n6 K12 S7", "benzene", 7), ("far chain n65 K2 S3", 65, 3)]


def _spec_autos(a):
    if a is None:
        return None, 300
    if isinstance(a, str):
        t = fixture_autos(a)
    else:
        t = chain_autos(a) if a > 0 else ring_autos(-a)
    return t, t.shape[1]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(X float32 [S, n, 3], Y float32 [3, n, 3], autos [K, n] or None, n, pair / cross: the `aligned_rmsd_ref` dicts).
    n in 1, 2 (collinear), 3 (planar), 4, 5, 6, 60, 61, 63 / 64 / 65, 255 / 256 / 257, 300; S in 2, 3, 7, 8, 9, 17; T = 3 (its first
    column is T = 1); K none, 1, 2, 12, 24, 120 and beyond; two cases 1000 A from the origin."""
    rng = np.random.default_rng(20241021)
    out = {}
    for name, a, S in SPEC:
        autos, n = _spec_autos(a)
        shift = (1000.0, -1000.0, 1000.0) if name.startswith("far") else None
        Z = random_conformers(rng, S + 3, n, autos, shift)
        X, Y = Z[:S], Z[S:]
        out[name] = dict(X=X, Y=Y, autos=autos, n=n, pair=aligned_rmsd_ref(X, None, autos), cross=aligned_rmsd_ref(X, Y, autos))
    return out


def make_modes(rng, autos, n, sizes, thr=THRESHOLD, margin=MARGIN):
    """len(sizes) shapes of one ligand, sizes[m] conformers of shape m: each a random rigid image of the shape under a random
    automorphism plus jitter of about 0.1 A; the conformers in random order.  Redrawn until every float64 distance is at least `margin`
    from `thr`, below it inside a mode and above it between modes.  -> (X float32 [S, n, 3], mode [S], D float64 [S, S])."""
    a_all = _autos(autos, n)
    for _ in range(50):
        shapes = [rng.normal(scale=2.0, size=(n, 3)) for _ in sizes]
        X, mode = [], []
        for m, cnt in enumerate(sizes):
            for _ in range(cnt):
                x = shapes[m][a_all[rng.integers(len(a_all))]] + rng.normal(scale=0.1 / np.sqrt(3.0), size=(n, 3))
                X.append(x @ _rot(rng).T + rng.normal(scale=3.0, size=3))
                mode.append(m)
        perm = rng.permutation(len(mode))
        X, mode = np.asarray(X, dtype=np.float32)[perm], np.asarray(mode)[perm]
        D = aligned_rmsd_ref(X, None, autos)["D"]
        same = mode[:, None] == mode[None, :]
        off = ~np.eye(len(mode), dtype=bool)
        if (np.abs(D - thr)[off] >= margin).all() and (D[same] < thr).all() and (D[~same] > thr).all():
            return X, mode, D
    raise RuntimeError("make_modes: no draw met the margin condition")


MODE_SPEC = (("benzene", "benzene", (5, 3, 2)), ("druglike_61", "druglike_61", (2, 6, 1, 3)), ("chain n5", 5, (4, 5)),
             ("neopentane", "neopentane", (3, 3, 3)))


@functools.lru_cache(maxsize=None)
def mode_cases():
    """The planted-mode cases of the pruning tests: name -> (X, mode, D float64, autos, key float32 [S], valid bool [S])."""
    rng = np.random.default_rng(505)
    out = {}
    for name, a, sizes in MODE_SPEC:
        autos, n = _spec_autos(a)
        X, mode, D = make_modes(rng, autos, n, sizes)
        key = rng.normal(size=len(mode)).astype(np.float32)
        key[1] = key[0]                                                                  # a tie: conformer order decides
        valid = rng.random(len(mode)) > 0.25
        out[name] = (X, mode, D, autos, key, valid)
    return out


def chiral_pair():
    """A four-neighbour centre with four different arms and its mirror image: (x, mirror) float64 [5, 3]."""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [-1.2, -1.2, 1.2], [-1.4, 1.4, -1.4], [1.7, -1.7, -1.7]])
    return x, x * np.array([1.0, 1.0, -1.0])
