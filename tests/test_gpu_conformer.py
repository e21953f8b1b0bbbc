"""GPU: fabind_amd.conformer (csrc/conformer.hip) -- the torsion plan, torsion noise and the uniform rotation -- against the numpy
restatement of tests/conformer_refs.py (checked on the CPU by tests/test_conformer_refs_cpu.py), the invariants the reference's
RDKit path guarantees, and the augmentation options of fabind_amd.data.build_batch.

Error bound of the perturbation tests (`bound` below): the restatement is run in float32 numpy on the same inputs; the largest
float32-vs-float64 deviation over all cases is the yardstick and the device must stay within 4 x that (another sincos, another
operation order -- not another algorithm).  Measured figures: DESIGN.md section 13."""
import itertools

import numpy as np
import pytest
import torch

import conformer_refs as R
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _plan_of(mols, on_overflow="raise", form="once"):
    from fabind_amd import conformer
    x, bi, codes, off = R.pack(mols)
    if form == "both":
        bi, codes = np.concatenate([bi, bi[::-1]], 1), np.tile(codes, 2)
    elif form == "dup":
        bi, codes = np.concatenate([bi[::-1], bi, bi], 1), np.tile(codes, 3)
    return conformer.rotatable_bonds(_t(bi), _t(codes), off, on_overflow=on_overflow), x, off


def _assert_plan_equal(p, mols):
    q, s, off, st = R.batch_plan(mols)
    assert np.array_equal(p.off.cpu().numpy(), off) and np.array_equal(p.status.cpu().numpy(), st)
    assert np.array_equal(p.quad.cpu().numpy(), q)
    assert np.array_equal(p.side.cpu().numpy().view(np.uint32), s)
    assert np.array_equal(p.atom_off.cpu().numpy(), np.concatenate([[0], np.cumsum([m["n"] for m in mols])]))


def _all_molecules():
    g = load_npz("conformer_ligands")
    hand = [m for _, (m, _) in sorted(R.hand_molecules().items())]
    chains = [R.chain(n) for n in (1, 2, 3, 4, 63, 64, 65, 128, 129, 256)]
    return hand, R.fixture_molecules(g), chains


# ------------------------------------------------------------------------------------------------ 1. the plan
def test_plan_equals_restatement_molecule_by_molecule():
    hand, fix, chains = _all_molecules()
    for m in hand + fix + chains:
        p, _, _ = _plan_of([m])
        _assert_plan_equal(p, [m])
    p, _, _ = _plan_of([R.chain(256)])
    assert p.quad.shape[0] == 253                                       # crosses every lane and word boundary


@pytest.mark.parametrize("form", ["once", "both", "dup"])
def test_plan_of_a_mixed_batch_in_every_bond_list_form(form):
    hand, fix, chains = _all_molecules()
    mols = hand[:5] + [R.chain(257)] + fix[:2] + chains + hand[5:] + fix[2:]
    p, _, _ = _plan_of(mols, on_overflow="truncate", form=form)
    _assert_plan_equal(p, mols)
    assert p.status.cpu().tolist().count(3) == 1


def test_more_than_256_atoms():
    from fabind_amd import conformer
    mols = [R.chain(4), R.chain(257), R.chain(5)]
    with pytest.raises(RuntimeError, match=r"ligand 1: status 3 \(more than 256 atoms\)"):
        _plan_of(mols)
    p, _, _ = _plan_of(mols, on_overflow="truncate")
    assert p.status.cpu().tolist() == [0, 3, 0] and p.off.cpu().tolist() == [0, 1, 1, 3]
    x, bi, codes, off = R.pack(mols)
    with pytest.raises(ValueError):
        conformer.rotatable_bonds(_t(bi), _t(codes[:-1]), off)
    with pytest.raises(ValueError):
        conformer.rotatable_bonds(_t(bi + 1), _t(codes), off)
    with pytest.raises(RuntimeError, match="HIP device"):
        conformer.rotatable_bonds(torch.as_tensor(bi), codes, off)


# ------------------------------------------------------------------------------------------------ 2./3. perturbation
class _Cases:
    """Every perturbation case run once on the device and once per precision on the host, shared by the tests below."""

    def __init__(self):
        from fabind_amd import conformer
        g = load_npz("conformer_ligands")
        fix = R.fixture_molecules(g)
        batches = {"ligands": fix + [R.chain(1), R.chain(2)], "chains": [R.chain(256), R.chain(257)]}
        rng = np.random.RandomState(11)
        self.cases, self.f32_dev, self.gpu_dev = [], 0.0, 0.0
        for name, mols in batches.items():
            p, x, off = _plan_of(mols, on_overflow="truncate")
            q, s, toff, _ = R.batch_plan(mols)
            for S, relative, centre in itertools.product((1, 3), (False, True), (True, False)):
                ang = rng.uniform(0, 2 * np.pi, (S, len(q))).astype(np.float32)
                uni = rng.uniform(0, 1, (S, len(mols), 3)).astype(np.float32)
                got = conformer.perturb_conformers(_t(x), p, n_copies=S, angles=_t(ang), uniforms=_t(uni), relative=relative,
                                                   centre=centre).cpu().numpy()
                r64 = R.perturb(x, off, q, s, toff, ang, uni, relative, True, centre, np.float64)
                r32 = R.perturb(x, off, q, s, toff, ang, uni, relative, True, centre, np.float32)
                c = dict(name=name, mols=mols, x=x, off=off, quad=q, side=s, toff=toff, ang=ang, S=S, relative=relative, centre=centre,
                         got=got, r64=r64, e32=float(np.abs(r32 - r64).max()), egpu=float(np.abs(got - r64).max()))
                print("%s S=%d relative=%d centre=%d: float32 numpy vs float64 %.3e, device vs float64 %.3e" % (
                    name, S, relative, centre, c["e32"], c["egpu"]))
                self.cases.append(c)
        self.f32_dev = max(c["e32"] for c in self.cases)
        self.gpu_dev = max(c["egpu"] for c in self.cases)
        self.bound = 4.0 * self.f32_dev
        print("largest float32-vs-float64 deviation %.3e, largest device deviation %.3e, ratio %.2f" % (
            self.f32_dev, self.gpu_dev, self.gpu_dev / self.f32_dev))


@pytest.fixture(scope="module")
def cases():
    return _Cases()


def test_perturbation_within_four_times_the_float32_deviation(cases):
    assert len(cases.cases) == 16 and cases.f32_dev > 0
    for c in cases.cases:
        assert c["egpu"] <= cases.bound, (c["name"], c["S"], c["relative"], c["centre"], c["egpu"], cases.bound)


def _dist(z, pr):
    return np.linalg.norm(z[pr[:, 0]] - z[pr[:, 1]], axis=1)


def test_invariants_of_the_torsion_path(cases):
    """Bonded and 1-3 distances and the distances inside every rigid fragment survive; with relative=False every dihedral is at its
    target (mod 2 pi); with centre the centroid is the origin -- all within the float32-derived bound."""
    tol = cases.bound
    for c in cases.cases:
        for b, m in enumerate(c["mols"]):
            a0, a1, t0, t1 = c["off"][b], c["off"][b + 1], c["toff"][b], c["toff"][b + 1]
            x = c["x"][a0:a1].astype(np.float64)
            pr = R.bonded_and_13_pairs(m)
            lab = R.rigid_fragments(m, c["quad"][t0:t1])
            ii, jj = np.triu_indices(m["n"], 1)
            same = lab[ii] == lab[jj]
            frag = np.stack([ii[same], jj[same]], 1)
            for s in range(c["S"]):
                y = c["got"][s, a0:a1].astype(np.float64)
                if len(pr):
                    assert np.abs(_dist(y, pr) - _dist(x, pr)).max() <= tol
                if len(frag):
                    assert np.abs(_dist(y, frag) - _dist(x, frag)).max() <= tol
                if not c["relative"]:
                    for q, t in zip(c["quad"][t0:t1], c["ang"][s, t0:t1]):
                        d, deg = R.dihedral(y, q)
                        assert not deg and abs((d - float(t) + np.pi) % (2 * np.pi) - np.pi) <= tol
                if c["centre"]:
                    assert np.abs(y.mean(0)).max() <= tol


def test_rotation_only_keeps_every_distance_and_the_handedness(cases):
    """plan=None: all pair distances kept, the signed volume of a fixed atom quadruple keeps sign and size (det M = +1), the centroid
    goes where the reference's formula puts it (mean @ M) or to the origin."""
    from fabind_amd import conformer
    tol = cases.bound
    g = load_npz("conformer_ligands")
    mols = R.fixture_molecules(g) + [R.chain(257), R.chain(1)]
    x, _, _, off = R.pack(mols)
    uni = np.random.RandomState(5).uniform(0, 1, (2, len(mols), 3)).astype(np.float32)
    cb = np.repeat(np.arange(len(mols)), np.diff(off))
    for centre, how in ((False, dict(atom_off=off)), (True, dict(compound_batch=_t(cb)))):
        got = conformer.perturb_conformers(_t(x), None, n_copies=2, torsion_noise=False, uniforms=_t(uni), centre=centre, **how).cpu().numpy()
        none_q, none_s = np.zeros((0, 4), np.int32), np.zeros((0, 8), np.uint32)
        ref = R.perturb(x, off, none_q, none_s, np.zeros(len(mols) + 1, np.int32), np.zeros((2, 0), np.float32), uni, centre=centre)
        assert np.abs(got - ref).max() <= tol
        for b, m in enumerate(mols):
            xb = x[off[b]:off[b + 1]].astype(np.float64)
            ii, jj = np.triu_indices(m["n"], 1)
            pr = np.stack([ii, jj], 1)
            for s in range(2):
                y = got[s, off[b]:off[b + 1]].astype(np.float64)
                if len(pr):
                    assert np.abs(_dist(y, pr) - _dist(xb, pr)).max() <= tol
                if m["n"] >= 4:
                    vol = lambda z: np.linalg.det(z[1:4] - z[0]) / 6.0
                    e = xb[:4]
                    areas = sum(0.5 * np.linalg.norm(np.cross(e[(i + 1) % 4] - e[(i + 2) % 4], e[(i + 3) % 4] - e[(i + 2) % 4])) for i in range(4))
                    # a vertex displaced by d changes the volume by at most |d| * (opposite face area) / 3; |d| <= sqrt(3) * tol
                    assert abs(vol(y[:4]) - vol(e)) <= np.sqrt(3.0) * tol * areas / 3.0 and vol(y[:4]) * vol(e) > 0
                if centre:
                    assert np.abs(y.mean(0)).max() <= tol
    with pytest.raises(ValueError):
        conformer.perturb_conformers(_t(x), None, atom_off=off)                      # torsion noise without a plan
    with pytest.raises(RuntimeError, match="HIP device"):
        conformer.perturb_conformers(torch.as_tensor(x), None, torsion_noise=False, atom_off=off)


# ------------------------------------------------------------------------------------------------ 4. keys, not positions
def test_result_depends_on_key_and_seed_only():
    from fabind_amd import conformer
    g = load_npz("conformer_ligands")
    fix = R.fixture_molecules(g)
    target = fix[2]
    n = target["n"]

    def run(mols, pos, seed, keys, out=None):
        p, x, off = _plan_of(mols)
        y = conformer.perturb_conformers(_t(x), p, n_copies=3, seed=seed, keys=_t(np.asarray(keys, np.int32)), out=out)
        return y[:, off[pos]:off[pos] + n].clone(), p, x, off
    alone, p1, x1, _ = run([target], 0, 9, [7])
    mid, _, _, _ = run([fix[0], R.chain(64), target, fix[3], R.chain(5)], 2, 9, [1, 2, 7, 3, 4])
    last, _, _, _ = run([R.chain(30), fix[1], fix[0], R.chain(2), target], 4, 9, [7, 7, 5, 0, 7])
    assert torch.equal(alone, mid) and torch.equal(alone, last)
    again, _, _, _ = run([target], 0, 9, [7])
    assert torch.equal(alone, again)                                   # repeats are bit-identical
    other_seed, _, _, _ = run([target], 0, 10, [7])
    other_key, _, _, _ = run([target], 0, 9, [8])
    assert not torch.equal(alone, other_seed) and not torch.equal(alone, other_key)
    assert not torch.equal(alone[0], alone[1])                         # copies differ
    # the draws are the restated hash: explicit angles / uniforms computed on the host give the same bits
    T = int(p1.quad.shape[0])
    ang, uni = R.drawn_inputs(9, [7], 3, [T])
    explicit = conformer.perturb_conformers(_t(x1), p1, n_copies=3, angles=_t(ang), uniforms=_t(uni))
    assert torch.equal(explicit, alone)
    # default keys = the position in the batch
    assert torch.equal(conformer.perturb_conformers(_t(x1), p1, n_copies=3, seed=9), run([target], 0, 9, [0])[0])
    # sentinels on both sides of the output
    buf = torch.full((3 * n * 3 + 128,), -777.0, device=DEV)
    out = buf[64:64 + 3 * n * 3].view(3, n, 3)
    got, _, _, _ = run([target], 0, 9, [7], out=out)
    assert torch.equal(got, alone) and bool((buf[:64] == -777.0).all()) and bool((buf[-64:] == -777.0).all())


# ------------------------------------------------------------------------------------------------ 5. distribution
def test_draws_are_uniform():
    """4096 copies of a 4-atom chain: the rotated first bond direction is uniform on the sphere (|mean| < 0.045 per component,
    |E[z^2] - 1/3| < 0.03: 5 sigma) and the drawn dihedral uniform on the circle (mean resultant length < 4 / sqrt(4096))."""
    from fabind_amd import conformer
    S = 4096
    m = R.chain(4)
    p, x, off = _plan_of([m])
    y = conformer.perturb_conformers(_t(x), p, n_copies=S, seed=R.DIST_SEED).cpu().numpy().astype(np.float64)
    d = y[:, 1] - y[:, 0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.abs(d.mean(0)).max() < 0.045 and abs((d[:, 2] ** 2).mean() - 1.0 / 3.0) < 0.03
    phi = np.array([R.dihedral(y[s], (0, 1, 2, 3))[0] for s in range(S)])
    assert abs(np.exp(1j * phi).mean()) < 4.0 / np.sqrt(S)
    ang, _ = R.drawn_inputs(R.DIST_SEED, [0], S, [1])
    assert np.abs((phi - ang[:, 0] + np.pi) % (2 * np.pi) - np.pi).max() < 1e-4      # the dihedrals ARE the restated draws


# ------------------------------------------------------------------------------------------------ 6. build_batch
def _raw(with_codes=True):
    g = load_npz("data_builder")
    out = []
    for i in range(int(g["n"])):
        s = dict(protein_node_xyz=g["raw%d_protein_node_xyz" % i], protein_esm2_feat=g["raw%d_protein_esm2_feat" % i],
                 coords=g["raw%d_coords" % i], compound_node_features=g["raw%d_compound_node_features" % i],
                 input_atom_edge_list=g["raw%d_input_atom_edge_list" % i], LAS_edge_index=g["raw%d_LAS_edge_index" % i],
                 rdkit_coords=g["raw%d_rdkit_coords" % i], pdb="x%d" % i)
        if with_codes:                                                  # bond orders are not in the fixture: all SINGLE (rings are found by the flood fill)
            s["bond_codes"] = np.full(len(s["input_atom_edge_list"]), R.SINGLE, np.int64)
        out.append(s)
    return out


def _tensors(batch):
    for key, st in list(batch._stores.items()) + [("", batch._glob)]:
        for f, v in st.items():
            if torch.is_tensor(v):
                yield (key, f), v


def _lig_rows(batch, name="complex"):
    st = batch[name]
    return (st.segment == 0) & ~st.is_global


def test_build_batch_defaults_are_untouched():
    from fabind_amd.data import build_batch
    base = dict(_tensors(build_batch(_raw(False), DEV)))
    for kw, raw in ((dict(random_rotation=False, torsion_noise=False, augment_seed=5, augment_keys=[3, 2, 1, 0]), _raw(False)), ({}, _raw(True))):
        got = dict(_tensors(build_batch(raw, DEV, **kw)))
        assert set(got) == set(base) and len(base) >= 35
        for k in base:
            assert torch.equal(got[k], base[k]), k


def test_build_batch_random_rotation():
    from fabind_amd.data import build_batch
    base = build_batch(_raw(False), DEV)
    aug = build_batch(_raw(False), DEV, random_rotation=True, augment_seed=3)
    cb = base["compound"].batch.cpu().numpy()
    r0, r1 = base["compound"].rdkit_coords.cpu().numpy().astype(np.float64), aug["compound"].rdkit_coords.cpu().numpy().astype(np.float64)
    # float32 rotation of coordinates of size c: each output component is a 3-term product sum with |M| <= 1 after a mean subtraction and
    # before an offset addition, M itself carries a few ulp from sincos / sqrt and its products: 64 eps c covers both end points of a pair
    tol = 64 * np.finfo(np.float32).eps * max(np.abs(r0).max(), np.abs(aug["compound"].node_coords.cpu().numpy()).max())
    assert np.abs(r1 - r0).max() > 0.1
    for b in range(int(cb.max()) + 1):
        a, c = r0[cb == b], r1[cb == b]
        ii, jj = np.triu_indices(len(a), 1)
        pr = np.stack([ii, jj], 1)
        assert np.abs(_dist(c, pr) - _dist(a, pr)).max() <= tol
        init = aug["compound"].node_coords.cpu().numpy().astype(np.float64)[cb == b]
        assert np.abs(init.mean(0) - aug.pocket_residue_center[b].cpu().numpy()).max() <= tol
        assert np.abs(_dist(init, pr) - _dist(a, pr)).max() <= tol
    for name in ("complex", "complex_whole_protein"):
        assert torch.equal(aug[name].node_coords_LAS[_lig_rows(aug, name)], aug["compound"].rdkit_coords)
        assert torch.equal(aug[name, "c2c", name].edge_index, base[name, "c2c", name].edge_index)
        assert torch.equal(aug[name, "LAS", name].edge_index, base[name, "LAS", name].edge_index)
    assert torch.equal(aug["complex"].node_coords[_lig_rows(aug)], aug["compound"].node_coords)
    for f in ("coords", "dis_map", "pocket_idx", "node_xyz", "node_xyz_whole", "coords_center", "pocket_residue_center"):
        assert torch.equal(getattr(aug, f), getattr(base, f)), f
    for f in ("node_feats", "keepNode", "batch"):
        assert torch.equal(aug["pocket"][f], base["pocket"][f]), f
    assert torch.equal(aug["compound", "LAS", "compound"].edge_index, base["compound", "LAS", "compound"].edge_index)
    assert torch.equal(aug["compound_atom_edge_list"].x, base["compound_atom_edge_list"].x)
    again = build_batch(_raw(False), DEV, random_rotation=True, augment_seed=3)
    assert torch.equal(again["compound"].rdkit_coords, aug["compound"].rdkit_coords)
    keyed = build_batch(_raw(False), DEV, random_rotation=True, augment_seed=3, augment_keys=[5, 6, 7, 8])
    assert not torch.equal(keyed["compound"].rdkit_coords, aug["compound"].rdkit_coords)


def test_build_batch_torsion_noise():
    from fabind_amd.data import build_batch
    # (the fixture's start conformers share the native ligands' local geometry: stretch them by 10 % so that the two can be told apart)
    raw = [dict(s, rdkit_coords=1.1 * np.asarray(s["rdkit_coords"])) for s in _raw(True)]
    base = build_batch(raw, DEV)
    aug = build_batch(raw, DEV, torsion_noise=True, augment_seed=4)
    cb = base["compound"].batch.cpu().numpy()
    lig = base.coords.cpu().numpy()
    new = aug["compound"].rdkit_coords.cpu().numpy()
    # the restatement on the same source (the native ligand as the builder holds it), drawn inputs: keys = positions
    mols = [R.mol(len(s["coords"]), np.asarray(s["input_atom_edge_list"])[:, :2], s["bond_codes"]) for s in raw]
    q, sd, toff, st = R.batch_plan(mols)
    assert (st == 0).all() and len(q) > 0
    off = np.concatenate([[0], np.cumsum([m["n"] for m in mols])])
    ang, uni = R.drawn_inputs(4, list(range(len(mols))), 1, list(np.diff(toff)))
    r64 = R.perturb(lig, off, q, sd, toff, ang, uni, dt=np.float64)[0]
    r32 = R.perturb(lig, off, q, sd, toff, ang, uni, dt=np.float32)[0]
    tol = 4 * np.abs(r32 - r64).max()
    print("build_batch torsion noise: float32 numpy vs float64 %.3e, device vs float64 %.3e" % (np.abs(r32 - r64).max(), np.abs(new - r64).max()))
    assert np.abs(new - r64).max() <= tol
    moved = 0.0
    for b, m in enumerate(mols):
        pr = R.bonded_and_13_pairs(m)
        y = new[cb == b].astype(np.float64)
        assert np.abs(_dist(y, pr) - _dist(lig[cb == b].astype(np.float64), pr)).max() <= tol      # the crystal ligand's local geometry
        moved = max(moved, np.abs(_dist(y, pr) - _dist(raw[b]["rdkit_coords"].astype(np.float64), pr)).max())
        assert np.abs(y.mean(0)).max() <= tol
    assert moved > 1e-3                                                 # ... not the input conformer's
    for name in ("complex", "complex_whole_protein"):
        assert torch.equal(aug[name].node_coords_LAS[_lig_rows(aug, name)], aug["compound"].rdkit_coords)
    assert torch.equal(aug.coords, base.coords) and torch.equal(aug.dis_map, base.dis_map)
    with pytest.raises(ValueError, match="bond_codes"):
        build_batch(_raw(False), DEV, torsion_noise=True)
    keyed = [dict(s, augment_key=100 + i) for i, s in enumerate(raw)]   # keys from the samples: the same complexes in another order
    a = build_batch(keyed, DEV, torsion_noise=True, augment_seed=4)
    b = build_batch(keyed[::-1], DEV, torsion_noise=True, augment_seed=4)
    n0 = mols[0]["n"]
    assert torch.equal(a["compound"].rdkit_coords[:n0], b["compound"].rdkit_coords[-n0:])


def test_feeder_augments_on_its_side_stream(monkeypatch):
    from fabind_amd import conformer
    from fabind_amd.data import DeviceFeeder
    raw = _raw(True)
    groups = [raw[:2], raw[2:]]
    seen = []
    real = conformer.perturb_conformers

    def spy(*a, **k):
        seen.append(torch.cuda.current_stream(DEV) != torch.cuda.default_stream(DEV))
        return real(*a, **k)
    monkeypatch.setattr(conformer, "perturb_conformers", spy)

    def epoch(seed):
        return [b["compound"].node_coords.clone() for b in DeviceFeeder(groups, DEV, torsion_noise=True, random_rotation=True, augment_seed=seed)]
    e1, e1b, e2 = epoch(1), epoch(1), epoch(2)
    assert len(e1) == 2 and all(torch.equal(a, b) for a, b in zip(e1, e1b))
    assert all(not torch.equal(a, b) for a, b in zip(e1, e2))
    assert len(seen) == 6 and all(seen)
