"""GPU: fabind_amd.scoring.score_poses (csrc/pose_score.hip) against the float64 numpy restatement of tests/score_refs.py (pinned on the
CPU by tests/test_score_refs_cpu.py), on random type words and coordinates and on the 25 carved-pocket cases of
tests/golden/relax_cases.npz.

Equal exactly: n_pairs and flags (r^2 and d are the same bits on both sides), and the three piecewise sums wherever equality can be
proved: both sides add the same float64 terms in different orders, so the float32 results must agree when every float64 within the
reordering error of the restatement's sum rounds to one float32 (score_refs.exact32; otherwise the value is held to the bound below,
and the tests count how often that happens).
Within the bound (score_refs.bound): gauss1, gauss2, inter, total and per_atom, each within
(P + 16) 2^-52 A + 2^-24 |value|.  The tests print the largest observed fraction of the bound."""
import numpy as np
import pytest
import torch

import conformer_refs as R
import contact_refs as C
import relax_refs as X
import score_refs as SR
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIELDS = ("terms", "inter", "total", "n_pairs", "flags", "per_atom")
_CACHE = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class _Batch:
    """Complexes on the device.  cases: [dict(name, lig_types [n], poses [S, n, 3], prot_xyz [M, 3], prot_z [M], prot_types [M],
    n_torsions, status)]."""

    def __init__(self, cases, edge=8.0):
        from fabind_amd import validity
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["lig_types"]) for c in cases])]).astype(np.int32)
        self.poff = np.concatenate([[0], np.cumsum([len(c["prot_z"]) for c in cases])]).astype(np.int32)
        self.lt = _t(np.concatenate([np.asarray(c["lig_types"], np.int32) for c in cases] + [np.zeros(0, np.int32)]))
        self.pt = _t(np.concatenate([np.asarray(c["prot_types"], np.int32) for c in cases] + [np.zeros(0, np.int32)]))
        self.nt = _t(np.asarray([c["n_torsions"] for c in cases], np.int32))
        self.st = _t(np.asarray([c["status"] for c in cases], np.int32))
        pxyz = np.concatenate([np.asarray(c["prot_xyz"], np.float32).reshape(-1, 3) for c in cases] + [np.zeros((0, 3), np.float32)])
        pz = np.concatenate([np.asarray(c["prot_z"], np.int64) for c in cases] + [np.zeros(0, np.int64)])
        self.grid = validity.protein_grid(_t(pxyz), _t(pz), self.poff, edge=edge, on_overflow="skip")
        self.poses = np.concatenate([c["poses"] for c in cases], 1).astype(np.float32)     # [S, N, 3]

    def score(self, poses=None, **kw):
        from fabind_amd import scoring
        kw.setdefault("per_atom", True)
        res = scoring.score_poses(_t(self.poses if poses is None else poses), self.off, self.lt, self.grid, self.pt, n_torsions=self.nt,
                                  status=self.st, **kw)
        return {f: getattr(res, f).cpu().numpy() for f in FIELDS if getattr(res, f) is not None}

    def want(self, b, s, **kw):
        c = self.cases[b]
        gs = 0 if np.isfinite(np.asarray(c["prot_xyz"], np.float32)).all() else 6
        return SR.score(c["poses"][s], c["lig_types"], c["prot_xyz"], c["prot_z"], c["prot_types"], n_torsions=c["n_torsions"],
                        lig_status=c["status"], grid_status=gs, **kw)


def _cloud(n, rng):
    """n points at ligand-like density in a ball (no chemistry is needed: the energy reads coordinates and type words)."""
    rad = 1.2 * max(n, 1) ** (1.0 / 3.0)
    v = rng.randn(n, 3)
    return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9) * rad * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)).astype(np.float32)


def _case(name, n, nprot, seed, origin=(-7.5, -3.0, 0.0), status=0, n_torsions=0):
    rng = np.random.RandomState(seed)
    pxyz, pz = C.synthetic_protein(max(nprot, 1), seed=seed + 1, hydrogens=0.5 if nprot > 1 else 0.0, origin=origin)
    if nprot == 0:
        pxyz, pz = pxyz[:0], pz[:0]
        poses = np.stack([_cloud(n, rng) + np.float32(k) for k in range(9)]) if n else np.zeros((9, 0, 3), np.float32)
    else:
        poses = C.poses_for(_cloud(n, rng), pxyz, pz, seed=seed + 2, edge=8.0)
    return dict(name=name, lig_types=SR.random_words(n, rng), poses=poses, prot_xyz=pxyz, prot_z=pz, prot_types=SR.random_words(len(pz), rng),
                n_torsions=n_torsions, status=status)


def _special_cases():
    rng = np.random.RandomState(77)
    # more than 64 atoms in one cell of 8 A: 100 of 150 atoms in the cell (1, 1, 1), hydrogens among them
    crowd = rng.uniform(-7.9, 23.9, size=(150, 3)).astype(np.float32)
    crowd[20:120] = rng.uniform(8.01, 15.99, size=(100, 3))
    cz = rng.choice([1, 6, 7, 8, 16], size=150)
    lig = (rng.uniform(9.0, 15.0, size=(8, 3))).astype(np.float32)
    crowded = dict(name="crowded-cell", lig_types=SR.random_words(8, rng), poses=np.stack([lig + np.float32(0.25 * k) for k in range(9)]),
                   prot_xyz=crowd, prot_z=cz, prot_types=SR.random_words(150, rng), n_torsions=3, status=0)
    # ligand atoms ON cell faces (x = 8 = the edge, -0.0, a negative multiple) and protein atoms at r = 8 EXACTLY on three axes
    lig = np.array([[8.0, 0.0, 0.0], [-0.0, 16.0, -8.0], [24.0, 8.0, 8.0]], np.float32)
    prot = np.array([[0.0, 0.0, 0.0], [16.0, 0.0, 0.0], [8.0, 8.0, 0.0], [8.0, 0.0, -8.0], [8.0, 7.5, 0.0], [0.0, 16.0, 0.0], [0.0, 8.0, -8.0],
                     [24.0, 8.0, 0.0], [24.0, 8.0, 15.999999], [30.0, 8.0, 8.0], [1.0, 1.0, 1.0]], np.float32)
    pz = np.array([6, 6, 8, 7, 6, 6, 1, 6, 8, 6, 6])
    faces = dict(name="faces-and-r8", lig_types=SR.random_words(3, rng), poses=np.stack([lig] * 9), prot_xyz=prot, prot_z=pz,
                 prot_types=SR.random_words(len(pz), rng), n_torsions=0, status=0)
    bad = _case("grid-status-6", 5, 64, seed=901)
    bad["prot_xyz"] = bad["prot_xyz"].copy()
    bad["prot_xyz"][7, 2] = np.inf
    return [crowded, faces, bad]


def _shape_setup():
    if "shape" not in _CACHE:
        cases = [_case("lig0-prot64", 0, 64, 10), _case("lig1-prot1", 1, 1, 20, n_torsions=1), _case("lig2-prot0", 2, 0, 30),
                 _case("lig63-prot65", 63, 65, 40, n_torsions=7), _case("lig64-prot2000", 64, 2000, 50, n_torsions=12),
                 _case("lig65-prot64", 65, 64, 60), _case("lig256-prot2000", 256, 2000, 70, n_torsions=30),
                 _case("status-3", 20, 64, 80, status=3), _case("lig30-offset-1000", 30, 600, 90, origin=(1000.0, -1000.0, 1000.0), n_torsions=4)]
        cases[1]["poses"][:, 0] = cases[1]["prot_xyz"][0] + np.float32([3.5, 0.5, -0.25])      # the one protein atom within reach
        cases += _special_cases()
        b = _Batch(cases)
        want = [[b.want(k, s) for s in range(9)] for k in range(len(cases))]
        _CACHE["shape"] = (b, want)
    return _CACHE["shape"]


def _compare(got, b, s, a0, w, what, worst, proved):
    """One (complex, pose) of a host result against the restatement; a0: the ligand's first atom."""
    assert int(got["n_pairs"][b, s]) == w["n_pairs"], (what, "n_pairs", got["n_pairs"][b, s], w["n_pairs"])
    assert int(got["flags"][b, s]) == w["flags"], (what, "flags")
    n = len(w["per_atom"])
    pa = got["per_atom"][s, a0:a0 + n] if "per_atom" in got else None
    if w["flags"] != 0:
        assert np.isnan(got["terms"][b, s]).all() and np.isnan(got["inter"][b, s]) and np.isnan(got["total"][b, s]), what
        assert pa is None or np.isnan(pa).all(), what
        return
    P = w["n_pairs"]
    for col in range(5):
        g, v, A = float(got["terms"][b, s, col]), float(w["terms"][col]), float(w["abs_terms"][col])
        if col >= 2 and SR.exact32(P, A, v):
            assert g == float(np.float32(v)), (what, SR.TERMS[col], g, v)
            proved[0] += 1
        else:
            proved[1] += col >= 2
            bd = SR.bound(P, A, v)
            assert abs(g - v) <= bd, (what, SR.TERMS[col], g, v, bd)
            if bd > 0 and col < 2:
                worst[SR.TERMS[col]] = max(worst.get(SR.TERMS[col], 0.0), abs(g - v) / bd)
    for name, A in (("inter", w["abs_inter"]), ("total", w["abs_total"])):
        g, v = float(got[name][b, s]), float(w[name])
        bd = SR.bound(P, A, v)
        assert abs(g - v) <= bd, (what, name, g, v, bd)
        if bd > 0:
            worst[name] = max(worst.get(name, 0.0), abs(g - v) / bd)
    if pa is not None:
        bds = np.array([SR.bound(int(w["pairs_atom"][i]), float(w["abs_atom"][i]), float(w["per_atom"][i])) for i in range(n)])
        err = np.abs(pa.astype(np.float64) - w["per_atom"])
        assert (err <= bds).all(), (what, "per_atom", int(np.argmax(err - bds)))
        if n and (bds > 0).any():
            worst["per_atom"] = max(worst.get("per_atom", 0.0), float((err[bds > 0] / bds[bds > 0]).max()))
        # per_atom sums to inter: both are within their bounds of the same exact number
        assert abs(pa.astype(np.float64).sum() - float(got["inter"][b, s])) <= bds.sum() + SR.bound(P, w["abs_inter"], w["inter"]), (what, "sum")


def _report(title, worst, proved):
    print("%s: largest observed fraction of the bound: %s; piecewise sums equal exactly where provable: %d, held to the bound instead: %d"
          % (title, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), proved[0], proved[1]))


@pytest.mark.parametrize("S", [1, 3, 8, 9])
def test_energies_pairs_and_flags(S):
    b, want = _shape_setup()
    got = b.score(b.poses[:S])
    B = len(b.cases)
    assert got["terms"].shape == (B, S, 5) and got["terms"].dtype == np.float32 and got["inter"].shape == (B, S) and got["total"].dtype == np.float32
    assert got["n_pairs"].dtype == np.int32 and got["flags"].dtype == np.int32 and got["per_atom"].shape == (S, b.off[-1])
    worst, proved = {}, [0, 0]
    for k, c in enumerate(b.cases):
        for s in range(S):
            _compare(got, k, s, b.off[k], want[k][s], (c["name"], C.POSE_KINDS[s]), worst, proved)
    names = [c["name"] for c in b.cases]
    assert (got["flags"][names.index("status-3")] == SR.UNCHECKED).all() and (got["flags"][names.index("grid-status-6")] == SR.UNCHECKED).all()
    assert (got["n_pairs"][names.index("lig0-prot64")] == 0).all() and (got["inter"][names.index("lig0-prot64")] == 0).all()
    assert (got["n_pairs"][names.index("lig2-prot0")] == 0).all() and (got["terms"][names.index("lig2-prot0")] == 0).all()
    assert proved[1] * 50 <= proved[0]                                   # equality is provable for all but a few sums
    _report("pose score, S = %d" % S, worst, proved)


def test_the_inputs_reach_every_branch():
    b, want = _shape_setup()
    names = [c["name"] for c in b.cases]
    live = [w for row in want for w in row if w["flags"] == 0]
    tot = np.sum([w["terms"] for w in live], 0)
    assert (tot > 0).all()                                               # every term is met, the role-gated ones included
    assert max(w["n_pairs"] for w in live) > 5000
    h = {f: getattr(b.grid, f).cpu().numpy() for f in ("cell_ptr", "atom_id", "atom_off", "status", "dims")}
    assert np.diff(h["cell_ptr"]).max() > 64                             # a cell with more than 64 atoms
    k = names.index("lig64-prot2000")
    ids = h["atom_id"][h["atom_off"][k]:h["atom_off"][k + 1]]
    assert len(ids) == 2000 and (ids != np.arange(2000)).any()           # hydrogens interleaved: atom_id differs from the stored position
    f = want[names.index("faces-and-r8")][0]
    assert f["cut_margin"] == 0.0 and f["n_pairs"] == 4                  # pairs at r = 8 exactly exist and are excluded
    assert h["status"].tolist().count(6) == 1
    assert any(w["n_pairs"] == 0 for w in want[names.index("lig63-prot65")])          # "beyond": the empty sums
    assert want[names.index("lig30-offset-1000")][0]["n_pairs"] > 100


def test_same_bits_alone_elsewhere_among_other_poses_and_on_a_repeat():
    b, want = _shape_setup()
    full, again = b.score(), b.score()
    for f in full:
        assert full[f].tobytes() == again[f].tobytes(), f
    pick, sel = [6, 9, 3, 4], [7, 0, 4]                                  # four complexes in another order, three of the nine poses
    sub_b = _Batch([dict(b.cases[i], poses=b.cases[i]["poses"][sel]) for i in pick])
    sub = sub_b.score()
    for pos, i in enumerate(pick):
        for f in ("terms", "inter", "total", "n_pairs", "flags"):
            assert sub[f][pos].tobytes() == np.ascontiguousarray(full[f][i][sel]).tobytes(), (b.cases[i]["name"], f)
        a, a2 = slice(b.off[i], b.off[i + 1]), slice(sub_b.off[pos], sub_b.off[pos + 1])
        assert np.ascontiguousarray(sub["per_atom"][:, a2]).tobytes() == np.ascontiguousarray(full["per_atom"][sel][:, a]).tobytes()
    i = 4
    solo_b = _Batch([dict(b.cases[i], poses=b.cases[i]["poses"][5:6])])
    solo = solo_b.score()
    for f in ("terms", "inter", "total", "n_pairs", "flags"):
        assert solo[f][0, 0].tobytes() == np.ascontiguousarray(full[f][i, 5]).tobytes(), f
    assert solo["per_atom"][0].tobytes() == np.ascontiguousarray(full["per_atom"][5, b.off[i]:b.off[i + 1]]).tobytes()
    plain = b.score(per_atom=False)                                      # the per-atom output changes nothing else
    assert "per_atom" not in plain
    for f in plain:
        assert plain[f].tobytes() == full[f].tobytes(), f


def test_nan_in_one_pose_leaves_every_other_pose_unchanged():
    b, want = _shape_setup()
    clean = b.score(b.poses[:8])
    dirty = b.poses[:8].copy()
    k = 4
    dirty[3, b.off[k] + 7, 1] = np.nan
    dirty[5, b.off[k] + 2, 0] = np.inf
    got = b.score(dirty)
    keep = np.ones(got["flags"].shape, bool)
    for s in (3, 5):
        assert got["flags"][k, s] == SR.NONFINITE and np.isnan(got["terms"][k, s]).all() and np.isnan(got["inter"][k, s]) and np.isnan(got["total"][k, s])
        assert got["n_pairs"][k, s] == 0 and np.isnan(got["per_atom"][s, b.off[k]:b.off[k + 1]]).all()
        keep[k, s] = False
    for f in ("terms", "inter", "total", "n_pairs", "flags"):
        assert got[f][keep].tobytes() == clean[f][keep].tobytes(), f
    pa_keep = np.ones(got["per_atom"].shape, bool)
    pa_keep[3, b.off[k]:b.off[k + 1]] = pa_keep[5, b.off[k]:b.off[k + 1]] = False
    assert got["per_atom"][pa_keep].tobytes() == clean["per_atom"][pa_keep].tobytes()


def test_c_abi_fills_only_its_rows():
    """Through the C ABI wrapper: outputs prefilled with a sentinel, one sentinel row past the end survives, every row is written."""
    from fabind_amd import kernels as K
    b, want = _shape_setup()
    B, S, N = len(b.cases), 3, int(b.off[-1])
    f32 = lambda *shape: torch.full(shape, 12345.0, dtype=torch.float32, device=DEV)
    i32 = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=DEV)
    terms, inter, total, n_pairs, flags, pa = f32(B * S + 1, 5), f32(B * S + 1), f32(B * S + 1), i32(B * S + 1), i32(B * S + 1), f32(S + 1, N)
    params = torch.tensor(list(SR.WEIGHTS) + [0.0585], dtype=torch.float64, device=DEV)
    g = b.grid
    K.pose_score(_t(b.poses[:S]), _t(b.off), B, 256, b.st, b.lt, b.nt, g.status, g.origin, g.dims, g.cell_off, g.atom_off, g.cell_ptr, g.xyz,
                 g.atom_id, g.prot_off, b.pt, g.edge, 8.0, params, terms, inter, total, n_pairs, pa, flags)
    assert terms[-1].cpu().tolist() == [12345.0] * 5 and float(inter[-1]) == 12345.0 and float(total[-1]) == 12345.0
    assert int(n_pairs[-1]) == -77 and int(flags[-1]) == -77 and (pa[-1] == 12345.0).all()
    got = dict(terms=terms[:-1].reshape(B, S, 5).cpu().numpy(), inter=inter[:-1].reshape(B, S).cpu().numpy(),
               total=total[:-1].reshape(B, S).cpu().numpy(), n_pairs=n_pairs[:-1].reshape(B, S).cpu().numpy(),
               flags=flags[:-1].reshape(B, S).cpu().numpy(), per_atom=pa[:-1].cpu().numpy())
    assert (got["n_pairs"] >= 0).all() and (got["flags"] >= 0).all() and not (got["terms"] == 12345.0).any() and not (got["per_atom"] == 12345.0).any()
    worst, proved = {}, [0, 0]
    for k, c in enumerate(b.cases):
        for s in range(S):
            _compare(got, k, s, b.off[k], want[k][s], (c["name"], s), worst, proved)


def test_other_weights_cutoff_and_torsion_weight():
    b, want = _shape_setup()
    kw = dict(weights=(-0.05, 0.01, 1.25, -0.02, -0.75), cutoff=6.5, torsion_weight=0.1)
    got = b.score(b.poses[:2], **kw)
    worst, proved = {}, [0, 0]
    for k in (3, 4, 9, 10):
        for s in range(2):
            _compare(got, k, s, b.off[k], b.want(k, s, **kw), (b.cases[k]["name"], s, "custom"), worst, proved)
    assert got["n_pairs"][4, 0] < want[4][0]["n_pairs"]


def test_refusals():
    from fabind_amd import scoring
    b, want = _shape_setup()
    small = _Batch(b.cases[:3], edge=5.0)
    with pytest.raises(ValueError, match=r"protein_grid\(edge=8"):
        small.score()
    with pytest.raises(ValueError, match="edge"):
        b.score(cutoff=8.5)
    args = (_t(b.poses[:1]), b.off, b.lt, b.grid, b.pt)
    with pytest.raises(ValueError):
        scoring.score_poses(_t(b.poses[:1, :-1]), b.off, b.lt, b.grid, b.pt)
    with pytest.raises(ValueError, match="prot_types"):
        scoring.score_poses(args[0], b.off, b.lt, b.grid, b.pt[:-1])
    with pytest.raises(ValueError):
        scoring.score_poses(args[0], b.off[:-1], b.lt, b.grid, b.pt)
    with pytest.raises(ValueError):
        scoring.score_poses(*args, weights=(1.0, 2.0))
    with pytest.raises(ValueError, match="256"):
        scoring.score_poses(_t(np.zeros((1, 300, 3), np.float32)), [0, 300], _t(np.zeros(300, np.int32)), _Batch(b.cases[1:2]).grid,
                            _t(b.cases[1]["prot_types"]))
    none = _Batch([b.cases[7]]).score()                                  # nothing is live: the prefilled outputs stand
    assert (none["flags"] == SR.UNCHECKED).all() and np.isnan(none["terms"]).all() and np.isnan(none["per_atom"]).all() and (none["n_pairs"] == 0).all()


# ------------------------------------------------------------------------------------------------ the committed relax cases
def _relax_setup():
    if "relax" not in _CACHE:
        g, gold = load_npz("conformer_ligands"), load_npz("relax_cases")
        cx = X.complexes(g)
        cases = []
        for i, (k, s) in enumerate(gold["cases"]):
            c = cx[k]
            m = c["mol"]
            y = X.make_target(c, X.target_seed(k, s))
            a0 = gold["angles0"][gold["angle_off"][i]:gold["angle_off"][i + 1]]
            fitted = X.relax_one(m["x"], y, m["quad"], m["side"], c["vplan"]["cls"], c["vplan"]["radii"], c["kept"][0], c["kept"][1],
                                 angles0=a0, max_iters=0)["coords"]
            relaxed = gold["coords64"][gold["atom_off"][i]:gold["atom_off"][i + 1]]
            cases.append(dict(name="relax-%d-%d" % (k, s), mol=m, z=c["z"], lig_types=SR.ligand_types(m["n"], m["bonds"], m["codes"], c["z"]),
                              poses=np.stack([fitted, relaxed]).astype(np.float32), prot_xyz=c["prot_xyz"], prot_z=c["prot_z"],
                              prot_types=np.asarray([SR.element_word(v) for v in c["prot_z"]], np.int32), n_torsions=len(m["quad"]), status=0))
        _CACHE["relax"] = _Batch(cases)
    return _CACHE["relax"]


def test_committed_relax_cases_and_device_typing():
    from fabind_amd import scoring
    b = _relax_setup()
    assert len(b.cases) == 25
    x, bi, codes, off = R.pack([c["mol"] for c in b.cases], [c["poses"][0] for c in b.cases])
    z = np.concatenate([c["z"] for c in b.cases])
    lt = scoring.ligand_types(_t(bi), _t(codes), _t(z), off)
    assert lt.dtype == torch.int32 and lt.cpu().numpy().tolist() == b.lt.cpu().numpy().tolist()       # the device typing is the restatement's
    pz = np.concatenate([c["prot_z"] for c in b.cases])
    assert scoring.protein_types_from_elements(_t(pz)).cpu().numpy().tolist() == b.pt.cpu().numpy().tolist()
    got = b.score()
    worst, proved = {}, [0, 0]
    rows = []
    for k, c in enumerate(b.cases):
        for s in range(2):
            w = b.want(k, s)
            _compare(got, k, s, b.off[k], w, (c["name"], ("fitted", "relaxed")[s]), worst, proved)
        rows.append((got["terms"][k, 0, 2], got["terms"][k, 1, 2], got["total"][k, 0], got["total"][k, 1]))
    assert (got["flags"] == 0).all() and (got["n_pairs"] > 0).all()
    r = np.asarray(rows, np.float64)
    _report("pose score, the 25 relax cases", worst, proved)
    print("pose score, the 25 relax cases (recorded, not asserted): repulsion fitted mean %.4f median %.4f -> relaxed mean %.4f median %.4f; "
          "total fitted mean %.4f median %.4f -> relaxed mean %.4f median %.4f; total lower after relaxation in %d of 25"
          % (r[:, 0].mean(), np.median(r[:, 0]), r[:, 1].mean(), np.median(r[:, 1]), r[:, 2].mean(), np.median(r[:, 2]), r[:, 3].mean(),
             np.median(r[:, 3]), int((r[:, 3] < r[:, 2]).sum())))


def test_batched_wrapper_agrees_with_the_direct_call():
    from fabind_amd import conformer, scoring
    from fabind_amd.utils.post_optim_utils import score_compound_coords_batched
    b = _relax_setup()
    x, bi, codes, off = R.pack([c["mol"] for c in b.cases], [c["poses"][0] for c in b.cases])
    tp = conformer.rotatable_bonds(_t(bi), _t(codes), off, on_overflow="truncate")
    assert torch.diff(tp.off).cpu().tolist() == [c["n_torsions"] for c in b.cases]
    cb = _t(np.repeat(np.arange(len(b.cases)), np.diff(b.off)))
    direct = scoring.score_poses(_t(b.poses), b.off, b.lt, b.grid, b.pt, n_torsions=b.nt)
    total, flags, res = score_compound_coords_batched(_t(b.poses), cb, b.lt, b.grid, b.pt, torsion_plan=tp)
    assert tuple(total.shape) == (2, len(b.cases)) and torch.equal(flags, direct.flags.t())
    assert total.cpu().numpy().tobytes() == direct.total.t().contiguous().cpu().numpy().tobytes() and res.per_atom is None
    t1, f1, _ = score_compound_coords_batched(_t(b.poses[1]), cb, b.lt, b.grid, b.pt, torsion_plan=tp)
    assert tuple(t1.shape) == (len(b.cases),) and t1.cpu().numpy().tobytes() == direct.total[:, 1].contiguous().cpu().numpy().tobytes()
    t0, _, _ = score_compound_coords_batched(_t(b.poses[1]), cb, b.lt, b.grid, b.pt)                  # no plan: no torsion scaling
    assert t0.cpu().numpy().tobytes() == direct.inter[:, 1].contiguous().cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        score_compound_coords_batched(_t(b.poses[1]), cb.flip(0), b.lt, b.grid, b.pt)
