"""GPU: fabind_amd.validity (csrc/pose_check.hip) -- the validity plan and the per-pose statistics and flags -- against the float64 numpy
restatement of tests/validity_refs.py (pinned on the CPU by tests/test_validity_refs_cpu.py, which also asserts that no statistic of
the poses used here lies within 16 bounds of a threshold, so the flags must be equal exactly).

Bounds (validity_refs.bound; U = 2^-24; derivations in DESIGN.md section 17): ratios and ca_dist 4 U |v|, flatness 2 U |v| + 1e-7 A,
chirality 2 U |v| + 1e-9; infinite neutral values are equal exactly.  The statistics test prints its largest observed fraction."""
import numpy as np
import pytest
import torch

import conformer_refs as R
import validity_refs as V
from helpers import load_npz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PLAN_FIELDS = ("status", "cls", "radii", "offs", "pair_ij", "pair_kind", "pair_d0", "group", "group_atoms", "centre", "centre_v0")


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _device_plan(mols, on_overflow="skip", autos=None, **kw):
    """mols: [(molecule with 'x', z)] -> the ValidityPlan of the batch."""
    from fabind_amd import validity
    x, bi, codes, off = R.pack([m for m, _ in mols], [m["x"] for m, _ in mols])
    z = np.concatenate([np.asarray(zz, np.int64) for _, zz in mols] + [np.zeros(0, np.int64)])
    return validity.validity_plan(_t(bi), _t(codes), _t(z), _t(x), off, autos=autos, on_overflow=on_overflow, **kw)


def _host(plan):
    out = {f: getattr(plan, f).cpu().numpy() for f in PLAN_FIELDS}
    out["cls"] = out["cls"].view(np.uint32)
    return out


def _slices(h, b, aoff):
    """Ligand b's part of a host plan: its bits must not depend on the batch."""
    o = h["offs"]
    return dict(status=h["status"][b:b + 1], cls=h["cls"][aoff[b]:aoff[b + 1]], radii=h["radii"][aoff[b]:aoff[b + 1]],
                pair_ij=h["pair_ij"][o[0, b]:o[0, b + 1]], pair_kind=h["pair_kind"][o[0, b]:o[0, b + 1]],
                pair_d0=h["pair_d0"][o[0, b]:o[0, b + 1]], group=h["group"][o[1, b]:o[1, b + 1]],
                group_atoms=h["group_atoms"][o[2, b]:o[2, b + 1]], centre=h["centre"][o[3, b]:o[3, b + 1]],
                centre_v0=h["centre_v0"][o[3, b]:o[3, b + 1]])


def _plan_molecules():
    g = load_npz("conformer_ligands")
    out = []
    for k, name in enumerate(sorted(R.hand_molecules())):
        m, z = V.hand(name)
        m["x"] = R.embed(m, seed=20 + k)
        out.append((m, z))
    out += [(m, np.asarray(g[m["name"] + "_z"], np.int64)) for m in R.fixture_molecules(g)]
    out.append(V.isopentane())
    for n in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257):
        m = R.chain(n)
        m["x"] = R.embed(m, seed=n)
        out.append((m, np.full(n, 6, np.int64)))
    out.insert(7, (dict(R.mol(0, [], name="empty"), x=np.zeros((0, 3), np.float32)), np.zeros(0, np.int64)))
    m = R.chain(5)
    m["name"], m["x"] = "zero-distance", R.embed(m, seed=77)
    m["x"][3] = m["x"][2]                                              # a bonded pair at distance 0
    out.append((m, np.full(5, 6, np.int64)))
    return out


def _assert_plan_equal(got, want, what):
    for f in PLAN_FIELDS:
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        if f in ("pair_d0", "centre_v0"):
            tol = 4 * 2.0 ** -53 * np.abs(want[f]) if f == "pair_d0" else 1e-12 * (1 + np.abs(want[f]))
            assert (np.abs(got[f] - want[f]) <= tol).all(), (what, f)
        else:
            np.testing.assert_array_equal(got[f], want[f], err_msg="%s: %s" % (what, f))


def test_plan_equals_the_restatement_alone_and_in_a_shuffled_batch():
    mols = _plan_molecules()
    want = [V.plan(m, z, m["x"]) for m, z in mols]
    assert [w["status"] for w in want].count(3) == 1 and [w["status"] for w in want].count(5) == 1
    alone = []
    for (m, z), w in zip(mols, want):
        h = _host(_device_plan([(m, z)]))
        _assert_plan_equal(h, V.batch_plan([w]), m["name"])
        alone.append(_slices(h, 0, [0, m["n"]]))
    order = np.random.RandomState(3).permutation(len(mols))
    assert (order != np.arange(len(mols))).any()
    batch = _host(_device_plan([mols[i] for i in order]))
    _assert_plan_equal(batch, V.batch_plan([want[i] for i in order]), "shuffled batch")
    aoff = np.concatenate([[0], np.cumsum([mols[i][0]["n"] for i in order])])
    for pos, i in enumerate(order):
        part = _slices(batch, pos, aoff)
        for f, v in alone[i].items():
            assert np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(part[f]).tobytes(), (mols[i][0]["name"], f)


def test_overflow_raises_by_name_and_skip_keeps_the_status():
    from fabind_amd import validity
    mols = [m for m in _plan_molecules() if m[0]["name"] in ("butane", "chain257", "zero-distance")]
    assert len(mols) == 3
    pos = {m[0]["name"]: i for i, m in enumerate(mols)}
    with pytest.raises(RuntimeError) as e:
        _device_plan(mols, on_overflow="raise")
    assert "ligand %d: status 3" % pos["chain257"] in str(e.value) and "ligand %d: status 5" % pos["zero-distance"] in str(e.value)
    assert "ligand %d" % pos["butane"] not in str(e.value)
    plan = _device_plan(mols, on_overflow="skip")
    assert plan.status.cpu().tolist() == [{"butane": 0, "chain257": 3, "zero-distance": 5}[m[0]["name"]] for m in mols]
    assert plan.max_atoms == 4
    with pytest.raises(ValueError):
        _device_plan(mols, on_overflow="truncate")
    assert validity.STATUS[3] and validity.STATUS[5]


def test_automorphisms_drop_the_isopropyl_centre():
    from fabind_amd import symmetry
    m, z = V.isopentane()
    g = load_npz("conformer_ligands")
    f = R.fixture_molecules(g)[0]
    mols = [(f, np.asarray(g[f["name"] + "_z"], np.int64)), (m, z)]
    x, bi, codes, off = R.pack([a for a, _ in mols], [a["x"] for a, _ in mols])
    zz = np.concatenate([a for _, a in mols])
    labels = symmetry.reference_atom_labels(_t(zz), _t(bi), _t(codes))
    autos = symmetry.ligand_automorphisms(labels, _t(bi), off)
    lists = symmetry.to_isomorphism_lists(autos)
    assert len(lists[1]) == 2
    with_autos, without = _host(_device_plan(mols, autos=autos)), _host(_device_plan(mols))
    _assert_plan_equal(with_autos, V.batch_plan([V.plan(a, b, a["x"], autos=l) for (a, b), l in zip(mols, lists)]), "with autos")
    _assert_plan_equal(without, V.batch_plan([V.plan(a, b, a["x"]) for a, b in mols]), "without autos")
    assert without["offs"][3, 2] - without["offs"][3, 1] == 1 and with_autos["offs"][3, 2] - with_autos["offs"][3, 1] == 0
    # radii and min_volume reach the kernel
    rad = np.linspace(1.0, 2.0, len(zz)).astype(np.float32)
    h = _host(_device_plan(mols, radii=_t(rad), min_volume=2.5))
    _assert_plan_equal(h, V.batch_plan([V.plan(a, b, a["x"], radii=rad[off[i]:off[i + 1]], min_volume=2.5) for i, (a, b) in enumerate(mols)]),
                       "radii, min_volume")


class _World:
    """The statistics world, made once: molecules, restated plans, nine poses each, pockets, the float64 statistics and flags, and the
    device's answers for S = 9 with the pocket."""

    def __init__(self):
        from fabind_amd import validity
        g = load_npz("conformer_ligands")
        self.mols = V.world_molecules(g)
        self.B = len(self.mols)
        self.plans = [V.plan(m, z, m["x"]) for m, z in self.mols]
        self.off = np.concatenate([[0], np.cumsum([m["n"] for m, _ in self.mols])])
        self.poses = np.concatenate([V.make_poses(m, pl, seed=100 + b) for b, ((m, _), pl) in enumerate(zip(self.mols, self.plans))], axis=1)
        self.pocket, self.pbatch = V.make_pocket(self.mols, V.POCKET_COUNTS, seed=5)
        self.plan = _device_plan(self.mols)
        self.want = np.zeros((self.B, V.N_POSES, 9))
        self.wflags = np.zeros((self.B, V.N_POSES), np.int64)
        for b, pl in enumerate(self.plans):
            for s in range(V.N_POSES):
                p = self.poses[s, self.off[b]:self.off[b + 1]]
                self.want[b, s] = V.stats(pl, p, self.pocket[self.pbatch == b])
                self.wflags[b, s] = V.flags(pl, p, self.want[b, s], ca_min=V.CA_MIN)
        self.dposes = _t(self.poses)
        self.res = validity.check_poses(self.dposes, self.plan, _t(self.pocket), _t(self.pbatch), ca_min=V.CA_MIN)

    def check(self, stats, flags, want, wflags, what):
        """-> the largest fraction of a bound; asserts the bounds, the exact infinities and NaNs, and the flags."""
        worst = 0.0
        assert stats.shape == want.shape and stats.dtype == np.float32 and flags.dtype == np.int32
        for idx in np.ndindex(*want.shape):
            g, w = float(stats[idx]), float(want[idx])
            if not np.isfinite(w):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (what, idx, g, w)
                continue
            frac = abs(g - w) / V.bound(idx[-1], w)
            worst = max(worst, frac)
            assert frac <= 1.0, (what, idx, V.STATS[idx[-1]], g, w, frac)
        np.testing.assert_array_equal(flags, wflags, err_msg=what)
        return worst


@pytest.fixture(scope="module")
def world():
    return _World()


@pytest.mark.parametrize("S", [1, 3, 8, 9])
def test_statistics_and_flags_against_float64(world, S):
    """S = 9 is one pose more than a work-group of eight waves holds."""
    from fabind_amd import validity
    res = validity.check_poses(world.dposes[:S], world.plan, _t(world.pocket), _t(world.pbatch), ca_min=V.CA_MIN)
    stats, flags = res.stats.cpu().numpy(), res.flags.cpu().numpy()
    worst = world.check(stats, flags, world.want[:, :S], world.wflags[:, :S], "S = %d" % S)
    print("S = %d: largest observed fraction of a bound %.3g" % (S, worst))
    # an entry is the same bits among any S
    assert np.array_equal(stats.view(np.uint32), world.res.stats.cpu().numpy()[:, :S].view(np.uint32))
    assert np.array_equal(flags, world.res.flags.cpu().numpy()[:, :S])
    valid = res.valid.cpu().numpy()
    assert valid.dtype == np.bool_ and np.array_equal(valid, (flags == 0) | (flags == V.UNCHECKED))
    # what the world is made of: every flag but NONFINITE occurs at S = 9, unchecked and empty ligands have their neutral rows
    if S == 9:
        seen = np.bitwise_or.reduce(flags.ravel())
        assert seen == (V.BOND | V.ANGLE | V.CLASH | V.AROMATIC_FLAT | V.DOUBLE_FLAT | V.CHIRALITY | V.PROTEIN | V.UNCHECKED)
        assert (flags[8] == V.UNCHECKED).all() and np.isnan(stats[8]).all() and valid[8].all()
        neutral = np.asarray([np.inf, -np.inf, np.inf, -np.inf, np.inf, 0, 0, np.inf, np.inf], np.float32)
        assert (flags[5] == 0).all() and np.array_equal(stats[5, 0], neutral)


def test_without_a_pocket_and_with_other_thresholds(world):
    from fabind_amd import validity
    res = validity.check_poses(world.dposes[:3], world.plan)
    stats, flags = res.stats.cpu().numpy(), res.flags.cpu().numpy()
    want = world.want[:, :3].copy()
    want[..., 8] = np.where(np.isnan(want[..., 8]), np.nan, np.inf)
    wflags = world.wflags[:, :3] & ~V.PROTEIN
    world.check(stats, flags, want, wflags, "no pocket")
    assert np.array_equal(stats[..., :8].view(np.uint32), world.res.stats.cpu().numpy()[:, :3, :8].view(np.uint32))
    # thresholds are arguments: exact halves and quarters, far from every statistic of the first three poses
    kw = dict(bond_tol=(0.5, 1.125), angle_tol=(0.5, 1.0625), clash_min=0.25, flat_max=0.03125)
    far = all(abs(v - thr) > 16 * max(V.bound(c, v), V.bound(c, thr)) for b in range(world.B) for s in range(3) if world.plans[b]["status"] == 0
              for c, v, thr in V.threshold_gaps(want[b, s], **kw))
    assert far
    res = validity.check_poses(world.dposes[:3], world.plan, **kw)
    wf = np.asarray([[V.flags(world.plans[b], world.poses[s, world.off[b]:world.off[b + 1]], want[b, s], **kw) for s in range(3)]
                     for b in range(world.B)])
    np.testing.assert_array_equal(res.flags.cpu().numpy(), wf)
    assert not np.array_equal(wf, wflags)


def test_nonfinite_pose_is_flagged_alone_and_outputs_stay_in_their_rows(world):
    """Straight through the wrapper of the C ABI into NaN-prefilled outputs with a sentinel row behind [B, S]."""
    from fabind_amd import kernels as K
    S, B, p = 8, world.B, world.plan
    poses = world.dposes[:S].clone()
    a0 = int(world.off[2])
    poses[1, a0 + 3, 1] = float("nan")
    poses[6, a0 + 5, 0] = float("inf")
    poses[4, int(world.off[3]) + 7, 2] = float("-inf")
    stats = torch.full((B * S + 1, 9), float("nan"), device=DEV)
    flags = torch.full((B * S + 1,), -7, dtype=torch.int32, device=DEV)
    stats[-1] = 12345.0
    poff = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    poff[1:] = torch.cumsum(torch.bincount(_t(world.pbatch), minlength=B), 0)
    K.pose_check(poses, p.atom_off, B, p.max_atoms, p.status, p.cls, p.radii, p.offs, p.pair_ij, p.pair_kind, p.pair_d0, p.group,
                 p.group_atoms, p.centre, p.centre_v0, _t(world.pocket), poff, (0.75, 1.25, 0.75, 1.25, 0.7, 0.25, V.CA_MIN), True, stats,
                 flags)
    torch.cuda.synchronize()
    assert (stats[-1] == 12345.0).all() and int(flags[-1]) == -7
    st, fl = stats[:-1].reshape(B, S, 9).cpu().numpy(), flags[:-1].reshape(B, S).cpu().numpy()
    ref_st, ref_fl = world.res.stats.cpu().numpy()[:, :S], world.res.flags.cpu().numpy()[:, :S]
    hit = np.zeros((B, S), bool)
    hit[2, 1] = hit[2, 6] = hit[3, 4] = True
    assert (fl[hit] == V.NONFINITE).all() and np.isnan(st[hit]).all()
    # every other entry -- the neighbours in the same work-group included -- is unchanged bit for bit
    assert np.array_equal(st[~hit].view(np.uint32), ref_st[~hit].view(np.uint32)) and np.array_equal(fl[~hit], ref_fl[~hit])
    assert (fl != -7).all()


def test_a_ligand_is_the_same_bits_alone_elsewhere_in_a_batch_and_on_a_repeat(world):
    from fabind_amd import validity
    b = 3                                                              # 6n93: 48 atoms, an aromatic system, centres, double bonds
    m, z = world.mols[b]
    sl = slice(int(world.off[b]), int(world.off[b + 1]))
    ref = world.res.stats.cpu().numpy()[b].view(np.uint32)
    ref_f = world.res.flags.cpu().numpy()[b]
    pk = world.pocket[world.pbatch == b]
    alone = _device_plan([(m, z)])
    r = validity.check_poses(_t(world.poses[:, sl]), alone, _t(pk), _t(np.zeros(len(pk), np.int64)), ca_min=V.CA_MIN)
    assert np.array_equal(r.stats.cpu().numpy()[0].view(np.uint32), ref) and np.array_equal(r.flags.cpu().numpy()[0], ref_f)
    others = [world.mols[i] for i in (0, 4, 1, 6)]
    batch = others[:3] + [(m, z)] + others[3:]                         # position 3 of 5, other neighbours
    pos = np.concatenate([[0], np.cumsum([a["n"] for a, _ in batch])])
    poses = np.zeros((3, pos[-1], 3), np.float32)
    poses[:, pos[3]:pos[4]] = world.poses[6:9, sl]                     # S = 3: three of the nine
    for i in (0, 1, 2, 4):
        poses[:, pos[i]:pos[i + 1]] = batch[i][0]["x"]
    r = validity.check_poses(_t(poses), _device_plan(batch), _t(pk), _t(np.full(len(pk), 3, np.int64)), ca_min=V.CA_MIN)
    assert np.array_equal(r.stats.cpu().numpy()[3].view(np.uint32), ref[6:9]) and np.array_equal(r.flags.cpu().numpy()[3], ref_f[6:9])
    again = validity.check_poses(world.dposes, world.plan, _t(world.pocket), _t(world.pbatch), ca_min=V.CA_MIN)
    assert torch.equal(again.flags, world.res.flags)
    assert np.array_equal(again.stats.cpu().numpy().view(np.uint32), world.res.stats.cpu().numpy().view(np.uint32))


def test_empty_shapes_and_only_unchecked_ligands():
    from fabind_amd import validity
    m = R.chain(257)
    m["x"] = R.embed(m, seed=1)
    plan = _device_plan([(m, np.full(257, 6, np.int64))] * 2)
    assert plan.max_atoms == 0
    r = validity.check_poses(_t(np.zeros((2, 514, 3), np.float32)), plan)
    assert (r.flags == V.UNCHECKED).all() and torch.isnan(r.stats).all() and r.valid.all() and tuple(r.stats.shape) == (2, 2, 9)
    r = validity.check_poses(torch.zeros(0, 514, 3, device=DEV), plan)
    assert tuple(r.stats.shape) == (2, 0, 9) and tuple(r.flags.shape) == (2, 0) and tuple(r.valid.shape) == (2, 0)
    e = np.zeros((2, 0), np.int64)
    plan = validity.validity_plan(_t(e), _t(np.zeros(0, np.int64)), _t(np.zeros(0, np.int64)), torch.zeros(0, 3, device=DEV), [0])
    r = validity.check_poses(torch.zeros(4, 0, 3, device=DEV), plan)
    assert tuple(r.stats.shape) == (0, 4, 9) and tuple(r.valid.shape) == (0, 4)
    with pytest.raises(RuntimeError):
        validity.check_poses(torch.zeros(1, 0, 3), plan)
    with pytest.raises(ValueError):
        validity.check_poses(torch.zeros(1, 5, 3, device=DEV), plan)


def test_inference_wrapper_and_consumers(world):
    from fabind_amd.utils.post_optim_utils import check_compound_coords_batched
    cb = _t(np.repeat(np.arange(world.B), np.diff(world.off)))
    valid, flags, stats = check_compound_coords_batched(world.dposes, cb, world.plan, _t(world.pocket), _t(world.pbatch), ca_min=V.CA_MIN)
    assert torch.equal(flags, world.res.flags.t()) and torch.equal(valid, world.res.valid.t()) and tuple(stats.shape) == (9, world.B, 9)
    v1, f1, s1 = check_compound_coords_batched(world.dposes[0], cb, world.plan)
    assert tuple(v1.shape) == (world.B,) and torch.equal(f1, world.res.flags[:, 0] & ~V.PROTEIN) and tuple(s1.shape) == (world.B, 9)
    with pytest.raises(ValueError):
        check_compound_coords_batched(world.dposes, cb.flip(0), world.plan)
    V.check_consumers(DEV)
