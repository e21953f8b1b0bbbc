"""Restatement of fabind_amd.embed (csrc/embed.hip) in numpy: the definition of record of the distance-geometry rules.

`bounds(m, z, chiral_sign)`: the rules in float64 on tabulated constants (only + - * / sqrt), every value rounded once to float32, then
triangle smoothing in float32 with k ascending -- required to equal the device BIT FOR BIT.  `embed(...)`: the embedding with the same
draws, eigen step, E and optimiser in a chosen dtype (float64: the reference; float32: the yardstick of the parity bound).
DESIGN.md section 20 lists every rule."""
import numpy as np

from conformer_refs import AROMATIC, DOUBLE, SINGLE, TRIPLE, hash32, mol, chain

M32 = 0xFFFFFFFF
MAX_ATOMS = 256
TETRA, TRIGONAL, LINEAR = 0, 1, 2
# (cos, sin) of the class angles 109.47 / 120 / 180 degrees and of the ring angles 60 / 90 / 108 degrees: table entries, never evaluated
ANGLE = [(-0.3333333333333333, 0.9428090415820634), (-0.5, 0.8660254037844386), (-1.0, 0.0),
         (0.5, 0.8660254037844386), (0.0, 1.0), (-0.30901699437494745, 0.9510565162951535)]
COVALENT = {5: 0.85, 6: 0.75, 7: 0.71, 8: 0.63, 9: 0.64, 14: 1.16, 15: 1.11, 16: 1.03, 17: 0.99, 34: 1.16, 35: 1.14, 53: 1.33}
COVALENT_OTHER = 1.20
CODE_SHIFT = {AROMATIC: -0.11, TRIPLE: -0.30, DOUBLE: -0.16, SINGLE: 0.0}
CONJ_SHIFT = 0.05
TOL12, TOL13, TOL14 = 0.01, 0.04, 0.06
BONDI = {5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 34: 1.90, 35: 1.85, 53: 1.98}
HOP4_SCALE = 0.8
UPPER_FAR, UPPER_FRAGMENT = 1000.0, 10.0
V_FLAT, V_MIN, V_MAX = float(np.float32(0.2)), 1.0, 100.0
# (the tolerances and weights as the device receives them: rounded to float32)
DEFAULTS = dict(max_tries=8, max_steps=1000, viol_tol=float(np.float32(0.1)), v_tol=float(np.float32(0.2)), w_v=float(np.float32(0.1)),
                w4=float(np.float32(0.1)), power_iters=100)
LS_C1, LS_MAX = 1e-4, 10
SMOOTH_PASSES = 16


def f32(v):
    return np.float32(v)


# ------------------------------------------------------------------------------------------------ topology
def adjacency(m):
    n = m["n"]
    code = {}
    for (a, b), c in zip(m["bonds"], m["codes"]):
        a, b, c = int(a), int(b), int(c)
        if a == b:
            continue
        k = (min(a, b), max(a, b))
        code[k] = min(code.get(k, 1 << 30), c)                         # a bond listed several times takes its smallest code
    nb = [[] for _ in range(n)]
    for (a, b) in code:
        nb[a].append(b)
        nb[b].append(a)
    return [sorted(v) for v in nb], code


def hop_matrix(n, nb, cap=5):
    """Bonds between every pair, capped: cap = "cap or more in the same fragment", cap + 1 = another fragment."""
    h = np.full((n, n), cap + 1, np.int64)
    for s in range(n):
        dist = {s: 0}
        todo = [s]
        while todo:
            nxt = []
            for u in todo:
                for v in nb[u]:
                    if v not in dist:
                        dist[v] = dist[u] + 1
                        nxt.append(v)
            todo = nxt
        for v, d in dist.items():
            h[s, v] = min(d, cap)
    return h


def geometry(n, nb, code, z):
    bc = lambda a, b: code[(min(a, b), max(a, b))]
    multi = [any(bc(a, b) in (AROMATIC, DOUBLE, TRIPLE) for b in nb[a]) for a in range(n)]
    g = np.zeros(n, np.int32)
    for a in range(n):
        deg = len(nb[a])
        nd = sum(bc(a, b) == DOUBLE for b in nb[a])
        ht = any(bc(a, b) == TRIPLE for b in nb[a])
        if deg >= 4:
            g[a] = TETRA
        elif deg <= 2 and (ht or nd >= 2):
            g[a] = LINEAR
        elif multi[a]:
            g[a] = TRIGONAL
        elif int(z[a]) in (7, 8) and any(multi[b] for b in nb[a]):
            g[a] = TRIGONAL
        else:
            g[a] = TETRA
    return g, multi


def bounds(m, z, chiral_sign=None, smooth=True):
    """-> dict(status, n, bounds float32 [n, n] packed (upper at (min, max), lower at (max, min)), geom int32 [n], quads int32 [Q, 4],
    quad_lo / quad_hi float32 [Q]); with smooth=False the bounds before triangle smoothing."""
    n = m["n"]
    empty = dict(n=n, bounds=np.zeros((0, 0), np.float32), geom=np.zeros(n, np.int32), quads=np.zeros((0, 4), np.int32),
                 quad_lo=np.zeros(0, np.float32), quad_hi=np.zeros(0, np.float32))
    if n > MAX_ATOMS:
        return dict(empty, status=3)
    nb, code = adjacency(m)
    z = [int(v) for v in z]
    bc = lambda a, b: code[(min(a, b), max(a, b))]
    geom, multi = geometry(n, nb, code, z)
    h = hop_matrix(n, nb)
    adj = [set(v) for v in nb]

    def d0(i, j):
        d = (COVALENT.get(z[i], COVALENT_OTHER) + COVALENT.get(z[j], COVALENT_OTHER)) + CODE_SHIFT.get(bc(i, j), 0.0)
        if bc(i, j) == SINGLE and geom[i] == TRIGONAL and geom[j] == TRIGONAL:
            d = d - CONJ_SHIFT
        return d

    def angle(a, i, k):
        """The angle class of i-a-k: the ring angle when the three lie on a 3-, 4- or 5-ring, else the class of a."""
        if k in adj[i]:
            return 3
        if (adj[i] & adj[k]) - {a}:
            return 4
        for x in nb[i]:
            if x != a and x != k and (adj[x] & adj[k]) - {a, i}:
                return 5
        return int(geom[a])

    U = np.zeros((n, n), np.float64)
    L = np.zeros((n, n), np.float64)
    for i in range(n):
        ri = np.float64(np.float32(BONDI.get(z[i], 2.00)))
        for j in range(i + 1, n):
            hop = h[i, j]
            if hop == 1:
                d = d0(i, j)
                lo, up = d - TOL12, d + TOL12
            elif hop == 2:
                lo, up = np.inf, -np.inf
                for a in sorted(adj[i] & adj[j]):
                    x, y = d0(a, i), d0(a, j)
                    c = ANGLE[angle(a, i, j)][0]
                    d = np.sqrt((x * x + y * y) - ((2.0 * x) * y) * c)
                    lo, up = min(lo, d - TOL13), max(up, d + TOL13)
            elif hop == 3:
                lo, up = np.inf, -np.inf
                for a in nb[i]:
                    for b in nb[j]:
                        if b not in adj[a]:
                            continue
                        d1, d2, d3 = d0(i, a), d0(a, b), d0(b, j)
                        c1, s1 = ANGLE[angle(a, i, b)]
                        c2, s2 = ANGLE[angle(b, a, j)]
                        xx = d2 - (d3 * c2 + d1 * c1)
                        ys, yi = d3 * s2, d1 * s1
                        cis = np.sqrt(xx * xx + (ys - yi) * (ys - yi))
                        trans = np.sqrt(xx * xx + (ys + yi) * (ys + yi))
                        # a planar six-ring: both centres TRIGONAL and a path i-x-y-j that avoids a and b
                        flat = geom[a] == TRIGONAL and geom[b] == TRIGONAL and any(
                            (adj[x] & adj[j]) - {a, b} for x in nb[i] if x != a and x != b)
                        lo, up = min(lo, cis - TOL14), max(up, (cis if flat else trans) + TOL14)
            else:
                rs = ri + np.float64(np.float32(BONDI.get(z[j], 2.00)))
                lo = rs * HOP4_SCALE if hop == 4 else rs
                up = UPPER_FRAGMENT if hop == 6 else UPPER_FAR
            U[i, j] = U[j, i] = np.float64(np.float32(up))
            L[i, j] = L[j, i] = np.float64(np.float32(lo))
    U, L = U.astype(np.float32), L.astype(np.float32)
    if smooth:
        U, L = smooth_bounds(U, L)
    status = 6 if (np.triu(L > U, 1)).any() else 0
    # ---- signed-volume terms, by atom: its trigonal term, the 1-4 quadruples of its DOUBLE / AROMATIC bonds to higher atoms, its stereo term
    quads, qlo, qhi = [], [], []
    for t in range(n):
        deg = len(nb[t])
        if geom[t] == TRIGONAL and deg == 3:
            quads.append([t] + nb[t]); qlo.append(-V_FLAT); qhi.append(V_FLAT)
        for b in nb[t]:
            if b > t and bc(t, b) in (DOUBLE, AROMATIC):
                for i in nb[t]:
                    for j in nb[b]:
                        if i != b and j != t and i != j:
                            quads.append([i, t, b, j]); qlo.append(-V_FLAT); qhi.append(V_FLAT)
        if chiral_sign is not None and deg in (3, 4) and not multi[t] and (z[t] != 7 or deg == 4) and int(chiral_sign[t]) in (1, -1):
            quads.append([t] + nb[t] if deg == 3 else [nb[t][3]] + nb[t][:3])
            lo, hi = (V_MIN, V_MAX) if int(chiral_sign[t]) > 0 else (-V_MAX, -V_MIN)
            qlo.append(lo); qhi.append(hi)
    return dict(status=status, n=n, bounds=pack_bounds(U, L), geom=geom, quads=np.asarray(quads, np.int32).reshape(-1, 4),
                quad_lo=np.asarray(qlo, np.float32), quad_hi=np.asarray(qhi, np.float32))


def smooth_bounds(U, L, passes=None):
    """Triangle smoothing in float32: passes over k ascending, uppers first (u_ij = min(u_ij, u_ik + u_kj)), then lowers (l_ij =
    max(l_ij, l_ik - u_kj, l_jk - u_ki)), each repeated until a whole pass changes nothing (at most SMOOTH_PASSES): a later k can lower
    a sum that an earlier k has used by a rounding, and only at the fixed point do the triangle inequalities hold in float32 exactly
    and is smoothing idempotent.  Within one k neither row k nor column k changes, so the vectorised update equals the sequential one."""
    U, L = U.astype(np.float32).copy(), L.astype(np.float32).copy()
    n = len(U)
    count = [0, 0]
    for _ in range(SMOOTH_PASSES):
        before = U.copy()
        for k in range(n):
            U = np.minimum(U, U[:, k, None] + U[None, k, :])
            np.fill_diagonal(U, 0)
        count[0] += 1
        if np.array_equal(before, U):
            break
    for _ in range(SMOOTH_PASSES):
        before = L.copy()
        for k in range(n):
            L = np.maximum(L, np.maximum(L[:, k, None] - U[None, k, :], L[None, k, :] - U[:, k, None]))
            np.fill_diagonal(L, 0)
        count[1] += 1
        if np.array_equal(before, L):
            break
    if passes is not None:
        passes.extend(count)
    return U, L


def pack_bounds(U, L):
    return (np.triu(U, 1) + np.tril(L, -1)).astype(np.float32)


def unpack_bounds(P):
    U = np.triu(P, 1)
    L = np.tril(P, -1)
    return U + U.T, L + L.T


def chiral_signs(m, z, x):
    """The sign (+1 / -1, 0 = no centre) of every topological stereo centre's signed volume in the coordinates x (`validity_plan`'s
    definition and determinant)."""
    nb, code = adjacency(m)
    _, multi = geometry(m["n"], nb, code, z)
    x = np.asarray(x, np.float32)
    out = np.zeros(m["n"], np.int32)
    for t in range(m["n"]):
        deg = len(nb[t])
        if deg in (3, 4) and not multi[t] and (int(z[t]) != 7 or deg == 4):
            o = t if deg == 3 else nb[t][3]
            v = np.linalg.det((x[nb[t][:3]] - x[o]).astype(np.float64))
            out[t] = 1 if v > 0 else -1 if v < 0 else 0
    return out


# ------------------------------------------------------------------------------------------------ draws
def _hash_vec(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def draws(seed, key, conf, t, idx):
    """u01 of (seed, key, conformer, try, draw index): the chain of csrc/conformer.hip with one more round; idx an integer array."""
    h = hash32((int(seed) & M32) + 0x9e3779b9)
    h = hash32((h ^ (int(key) & M32)) + 0x85ebca6b)
    h = hash32((h ^ (int(conf) & M32)) + 0xc2b2ae35)
    h = hash32((h ^ (int(t) & M32)) + 0x165667b1)
    v = _hash_vec((np.uint64(h) ^ (np.asarray(idx).astype(np.uint64) & M32)) + np.uint64(0x27d4eb2f))
    return (v >> np.uint64(8)).astype(np.float64) / 16777216.0


# ------------------------------------------------------------------------------------------------ embedding
def quad_volumes(x, quads):
    x = x[:, :3]
    p0 = x[quads[:, 0]]
    a, b, c = x[quads[:, 1]] - p0, x[quads[:, 2]] - p0, x[quads[:, 3]] - p0
    return a, b, c, np.einsum("qi,qi->q", a, np.cross(b, c))


def evaluate(x, U, L, quads, qlo, qhi, w_v, w4=0.0, dt=np.float64):
    """x [n, 4]: E = sum_{i<j} e(d_ij) over the FOUR-dimensional distances + w_v sum_quads (V - clamp(V, lo, hi))^2 on the first three
    coordinates + w4 sum_i x_i4^2, and its exact gradient; the largest pair violation (A) of the THREE-dimensional distances and the
    largest excess of a volume over its interval."""
    n = len(x)
    x = x.astype(dt)
    d = x[:, None, :] - x[None, :, :]
    d2 = np.einsum("ijk,ijk->ij", d, d).astype(dt)
    u2, l2 = (U.astype(dt)) ** 2, (L.astype(dt)) ** 2
    off = ~np.eye(n, dtype=bool)
    over = off & (d2 > u2)
    under = off & (d2 < l2)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(over, d2 / np.where(over, u2, 1) - 1, 0).astype(dt)
        den = np.where(under, l2 + d2, 1)
        b = np.where(under, 2 * l2 / den - 1, 0).astype(dt)
        coef = np.where(over, 2 * a / np.where(over, u2, 1), 0) + np.where(under, 2 * b * (-2 * l2 / (den * den)), 0)
    E = dt(0.5) * (np.sum(a * a, dtype=dt) + np.sum(b * b, dtype=dt)) + dt(w4) * np.sum(x[:, 3] * x[:, 3], dtype=dt)
    g = (2 * np.einsum("ij,ijk->ik", coef.astype(dt), d)).astype(dt)
    g[:, 3] += 2 * dt(w4) * x[:, 3]
    viol, _ = violations(x[:, :3], U, L, quads, qlo, qhi)
    vex = 0.0
    if len(quads):
        a3, b3, c3, V = quad_volumes(x, quads)
        r = (V - np.clip(V, qlo.astype(dt), qhi.astype(dt))).astype(dt)
        E = E + dt(w_v) * np.sum(r * r, dtype=dt)
        vex = float(np.abs(r).max())
        k = (2 * dt(w_v) * r)[:, None]
        g1, g2, g3 = k * np.cross(b3, c3), k * np.cross(c3, a3), k * np.cross(a3, b3)
        g3d = np.zeros((n, 3), dt)
        np.add.at(g3d, quads[:, 1], g1); np.add.at(g3d, quads[:, 2], g2); np.add.at(g3d, quads[:, 3], g3)
        np.add.at(g3d, quads[:, 0], -(g1 + g2 + g3))
        g[:, :3] += g3d
    return dt(E), g.astype(dt), viol, vex


def violations(x3, U, L, quads, qlo, qhi):
    """In float64 from coordinates [n, 3]: the largest max(l - d, d - u, 0) over the pairs, the largest excess of a volume."""
    x3 = np.asarray(x3, np.float64)
    n = len(x3)
    if n < 2:
        return 0.0, 0.0
    dist = np.sqrt(((x3[:, None, :] - x3[None, :, :]) ** 2).sum(-1))
    v = np.maximum(np.maximum(dist - U.astype(np.float64), L.astype(np.float64) - dist), 0.0)
    np.fill_diagonal(v, 0.0)
    vex = 0.0
    if len(quads):
        V = quad_volumes(x3, np.asarray(quads, np.int64))[3]
        vex = float(np.abs(V - np.clip(V, qlo.astype(np.float64), qhi.astype(np.float64))).max())
    return float(v.max()), vex


def energy3(x3, U, L, quads, qlo, qhi, w_v):
    """E of coordinates [n, 3] (no fourth coordinate), float64."""
    x4 = np.concatenate([np.asarray(x3, np.float64), np.zeros((len(x3), 1))], 1)
    return float(evaluate(x4, U, L, np.asarray(quads, np.int64), qlo, qhi, w_v, 0.0)[0])


def initial_coords(pl, seed, key, conf, t, power_iters, dt=np.float64):
    """Random distances, the metric matrix and its FOUR largest eigenpairs by power iteration with deflation -> x [n, 4]."""
    n = pl["n"]
    U, L = unpack_bounds(pl["bounds"])
    iu = np.triu_indices(n, 1)
    u01 = draws(seed, key, conf, t, iu[0] * n + iu[1])
    D = np.zeros((n, n), dt)
    D[iu] = (L[iu].astype(dt) + u01.astype(dt) * (U[iu].astype(dt) - L[iu].astype(dt)))
    D = D + D.T
    D2 = D * D
    d0 = D2.sum(1, dtype=dt) / dt(n) - (D2[iu].sum(dtype=dt)) / dt(n * n)
    G = ((d0[:, None] + d0[None, :] - D2) / dt(2)).astype(dt)
    x = np.zeros((n, 4), dt)
    vecs, lams = [], []
    for a in range(4):
        v = (2 * draws(seed, key, conf, t, n * n + a * n + np.arange(n)) - 1).astype(dt)
        lam = dt(0)
        nrm = np.sqrt(np.sum(v * v, dtype=dt))
        if nrm > 0:
            v = v / nrm
        for _ in range(power_iters):
            y = G @ v
            for vp, lp in zip(vecs, lams):
                y = y - (lp * np.sum(vp * v, dtype=dt)) * vp
            lam = np.sum(v * y, dtype=dt)
            nrm = np.sqrt(np.sum(y * y, dtype=dt))
            if not nrm > 0:
                break
            v = (y / nrm).astype(dt)
        vecs.append(v); lams.append(lam)
        if lam > 0:
            x[:, a] = np.sqrt(lam) * v
        else:
            x[:, a] = 2 * draws(seed, key, conf, t, n * n + (4 + a) * n + np.arange(n)) - 1
    return x.astype(dt)


def embed(pl, seed=0, key=0, conf=0, dt=np.float64, **kw):
    """One conformer of one ligand from its bounds plan -> dict(coords [n, 3] centred, status, tries, steps, viol, energy, trace).
    Polak-Ribiere+ conjugate gradients with a backtracking line search (quadratic interpolation), one evaluation of E per step."""
    p = dict(DEFAULTS, **kw)
    n = pl["n"]
    if pl["status"] != 0 or n == 0:
        return dict(coords=np.zeros((n, 3), dt), status=pl["status"], tries=0, steps=0, viol=0.0, energy=0.0, trace=[])
    U, L = unpack_bounds(pl["bounds"])
    quads, qlo, qhi = pl["quads"].astype(np.int64), pl["quad_lo"], pl["quad_hi"]
    dot = lambda a, b: dt(np.sum((a * b).sum(1, dtype=dt), dtype=dt))
    best = None
    for t in range(p["max_tries"]):
        x = initial_coords(pl, seed, key, conf, t, p["power_iters"], dt)
        E, g, viol, vex = evaluate(x, U, L, quads, qlo, qhi, p["w_v"], p["w4"], dt)
        tr = [float(E)]
        gg = dot(g, g)
        d, gd = -g, -gg
        alpha = dt(1) / max(dt(1), np.sqrt(gg))
        steps, fails, trial = 0, 0, 0
        while True:
            ok = viol <= p["viol_tol"] and vex <= p["v_tol"]
            if ok or steps >= p["max_steps"]:
                break
            if not gd < 0:
                d, gd = -g, -gg
                if gd == 0:
                    break
            xn = (x + alpha * d).astype(dt)
            En, gn, vn, vxn = evaluate(xn, U, L, quads, qlo, qhi, p["w_v"], p["w4"], dt)
            steps += 1
            if En <= E + dt(LS_C1) * alpha * gd:
                ggn = dot(gn, gn)
                beta = max(dt(0), (ggn - dot(gn, g)) / gg)
                gd = -ggn + beta * dot(gn, d)
                d = (-gn + beta * d).astype(dt)
                x, E, g, gg, viol, vex = xn, En, gn, ggn, vn, vxn
                if trial == 0:
                    alpha = dt(alpha * 2)
                fails, trial = 0, 0
            else:
                den = dt(2) * (En - E - gd * alpha)
                an = -gd * alpha * alpha / den if den > 0 else dt(0.5) * alpha
                alpha = dt(min(max(an, dt(0.1) * alpha), dt(0.5) * alpha))
                trial += 1
                if trial >= LS_MAX:
                    if fails:
                        tr.append(float(E))
                        break
                    d, gd, fails, trial = -g, -gg, 1, 0
            tr.append(float(E))
        # the result: the first three coordinates centred (and rounded to `out_dt`); E, the violations and the acceptance are those of
        # the returned coordinates, the fourth coordinate dropped
        x3 = x[:, :3]
        x3 = (x3 - x3.sum(0, dtype=dt) / dt(n)).astype(p.get("out_dt", dt))
        x4 = np.concatenate([x3.astype(dt), np.zeros((n, 1), dt)], 1)
        E, _, viol, vex = evaluate(x4, U, L, quads, qlo, qhi, p["w_v"], p["w4"], dt)
        ok = viol <= p["viol_tol"] and vex <= p["v_tol"]
        res = dict(coords=x3, status=0 if ok else 1, tries=t + 1, steps=steps, viol=viol, energy=float(E), trace=tr)
        if ok:
            return res
        if best is None or viol < best["viol"]:
            best = res
    best["tries"] = p["max_tries"]
    return best


# ------------------------------------------------------------------------------------------------ molecules
def hand_molecules():
    """name -> (molecule, atomic numbers): the CPU cases, which are also the GPU shapes."""
    S, D, T, A = SINGLE, DOUBLE, TRIPLE, AROMATIC
    ring = lambda k, o=0: [(o + i, o + (i + 1) % k) for i in range(k)]
    C = lambda n: [6] * n
    out = {
        "empty": (mol(0, []), []),
        "atom": (mol(1, []), C(1)),
        "ethane": (chain(2), C(2)),
        "propane": (chain(3), C(3)),
        "butane": (chain(4), C(4)),
        "cyclopropane": (mol(3, ring(3)), C(3)),
        "cyclobutane": (mol(4, ring(4)), C(4)),
        "cyclopentane": (mol(5, ring(5)), C(5)),
        "benzene": (mol(6, ring(6), [A] * 6), C(6)),
        "biphenyl": (mol(12, ring(6) + ring(6, 6) + [(0, 6)], [A] * 12 + [S]), C(12)),
        "naphthalene": (mol(10, ring(6) + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 0)], [A] * 11), C(10)),
        "norbornane": (mol(7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 6), (6, 3)]), C(7)),
        "spiro": (mol(9, ring(5) + [(0, 5), (5, 6), (6, 7), (7, 8), (8, 0)]), C(9)),
        # CH3-C(=O)-NH2: C0 C1 O2 N3
        "acetamide": (mol(4, [(0, 1), (1, 2), (1, 3)], [S, D, S]), [6, 6, 8, 7]),
        # CH3-C#N
        "acetonitrile": (mol(3, [(0, 1), (1, 2)], [S, T]), [6, 6, 7]),
        # CH3-S(=O)(=O)-CH3
        "sulfone": (mol(5, [(0, 1), (1, 2), (1, 3), (1, 4)], [S, D, D, S]), [6, 16, 8, 8, 6]),
        "two-fragment": (mol(9, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7), (7, 8)]), C(9)),
    }
    for k in (64, 65, 255, 256, 257):
        out["chain%d" % k] = (chain(k), C(k))
    for k, (m, _) in out.items():
        m["name"] = k
    return out
