"""GPU: fabind_amd.validity.protein_grid / check_poses_protein (csrc/protein_contacts.hip) against the float64 numpy restatement of
tests/contact_refs.py (pinned on the CPU by tests/test_contact_refs_cpu.py, which also asserts the margins of the inputs used here: no
pair at the cutoff, no lattice point on a sphere, no statistic within 16 bounds of a threshold -- so counts, pairs and flags must be
equal exactly).

Bounds (contact_refs.bound; U = 2^-24): prot_clash and prot_dist 4 U |v|, overlap U |v|; infinite neutral values
are equal exactly.  The statistics test prints its largest observed fraction of each bound."""
import numpy as np
import pytest
import torch

import conformer_refs as R
import contact_refs as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRID_FIELDS = ("status", "origin", "dims", "cell_off", "atom_off", "cell_ptr", "xyz", "radii", "atom_id")
_CACHE = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _device_plan(mols, on_overflow="skip", **kw):
    from fabind_amd import validity
    x, bi, codes, off = R.pack([m for m, _ in mols], [m["x"] for m, _ in mols])
    z = np.concatenate([np.asarray(zz, np.int64) for _, zz in mols] + [np.zeros(0, np.int64)])
    return validity.validity_plan(_t(bi), _t(codes), _t(z), _t(x), off, on_overflow=on_overflow, **kw)


def _device_grid(prots, on_overflow="skip", radii=None, edge=5.0):
    """prots: [(xyz, z)] -> the ProteinGrid of the batch."""
    from fabind_amd import validity
    off = np.concatenate([[0], np.cumsum([len(z) for _, z in prots])]).astype(np.int32)
    xyz = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x, _ in prots] + [np.zeros((0, 3), np.float32)])
    z = np.concatenate([np.asarray(zz, np.int64) for _, zz in prots] + [np.zeros(0, np.int64)])
    return validity.protein_grid(_t(xyz), _t(z), off, radii=None if radii is None else _t(np.concatenate(radii).astype(np.float32)),
                                 edge=edge, on_overflow=on_overflow)


def _host(grid):
    return {f: getattr(grid, f).cpu().numpy() for f in GRID_FIELDS}


def _part(h, b):
    """Complex b's part of a host grid, positions rebased: its bits must not depend on the batch."""
    c0, c1, a0, a1 = h["cell_off"][b], h["cell_off"][b + 1], h["atom_off"][b], h["atom_off"][b + 1]
    return dict(status=h["status"][b:b + 1], origin=h["origin"][b], dims=h["dims"][b], cell_ptr=h["cell_ptr"][c0:c1 + 1] - a0,
                xyz=h["xyz"][a0:a1], radii=h["radii"][a0:a1], atom_id=h["atom_id"][a0:a1])


def _assert_grid_equal(got, want, what):
    for f in GRID_FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


def _grid_proteins():
    out = [("empty", (np.zeros((0, 3), np.float32), np.zeros(0, np.int64)))]
    for n in (1, 63, 64, 65, 2000):
        out.append(("random%d" % n, C.synthetic_protein(n, seed=n, hydrogens=0.5, origin=(-9.0, -21.0, 3.0))))
    rng = np.random.RandomState(5)
    out.append(("one-cell", (rng.uniform(0.01, 4.99, size=(40, 3)).astype(np.float32) - np.float32(5.0), np.full(40, 6, np.int64))))
    crowd = rng.uniform(-4.9, 9.9, size=(150, 3)).astype(np.float32)
    crowd[20:120] = rng.uniform(5.01, 9.99, size=(100, 3))              # 100 atoms of 150 in the cell (1, 1, 1)
    out.append(("crowded-cell", (crowd, rng.choice([1, 6, 7, 8], size=150))))
    faces = np.array([[-0.0, 0.0, 5.0], [-5.0, -1e-30, 4.9999995], [10.0, -5.0000005, -10.0], [-2.5, 2.5, 0.0], [0.0, 0.0, 0.0],
                      [-10.0, -15.0, -20.0], [15.0, 20.0, 25.0], [-4.9999995, 5.0, -5.0]], np.float32)
    out.append(("faces", (faces, np.array([6, 7, 8, 6, 1, 16, 6, 8]))))
    out.append(("only-hydrogens", (rng.uniform(0, 9, size=(7, 3)).astype(np.float32), np.ones(7, np.int64))))
    bad = C.synthetic_protein(30, seed=9)
    bad[0][17, 1] = np.nan
    out.append(("non-finite", bad))
    out.append(("over-cap", (np.array([[0, 0, 0], [600.0, 600.0, 600.0]], np.float32), np.array([6, 6]))))     # 121^3 cells > 2^20
    return out


def test_grid_equals_the_restatement_alone_and_in_a_shuffled_batch():
    prots = _grid_proteins()
    want = [C.grid(x, z) for _, (x, z) in prots]
    status = [w["status"] for w in want]
    assert status.count(6) == 1 and status.count(7) == 1 and max(np.diff(want[7]["cell_ptr"])) > 64
    alone = []
    for (name, p), w in zip(prots, want):
        h = _host(_device_grid([p]))
        _assert_grid_equal(h, C.batch_grid([w]), name)
        alone.append(_part(h, 0))
    order = np.random.RandomState(3).permutation(len(prots))
    order = np.concatenate([order[order != 0][:4], [0], order[order != 0][4:]])          # the complex without atoms in the middle
    batch = _host(_device_grid([prots[i][1] for i in order]))
    _assert_grid_equal(batch, C.batch_grid([want[i] for i in order]), "shuffled batch")
    for pos, i in enumerate(order):
        part = _part(batch, pos)
        for f, v in alone[i].items():
            assert np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(part[f]).tobytes(), (prots[i][0], f)
    again = _host(_device_grid([prots[i][1] for i in order]))
    _assert_grid_equal(again, batch, "repeat")


def test_grid_overflow_raises_by_name_custom_radii_and_edge():
    prots = dict(_grid_proteins())
    three = [prots["non-finite"], prots["random63"], prots["over-cap"]]
    with pytest.raises(RuntimeError) as e:
        _device_grid(three, on_overflow="raise")
    assert "complex 0: status 6" in str(e.value) and "complex 2: status 7" in str(e.value) and "complex 1" not in str(e.value)
    assert _device_grid(three).status.cpu().tolist() == [6, 0, 7]
    x, z = prots["random65"]
    radii = np.random.RandomState(1).uniform(0.6, 2.4, size=len(z)).astype(np.float32)
    _assert_grid_equal(_host(_device_grid([(x, z)], radii=[radii], edge=3.3)), C.batch_grid([C.grid(x, z, radii, edge=3.3)]), "radii, edge 3.3")
    with pytest.raises(ValueError):
        _device_grid([(x, z)], radii=[-radii])
    with pytest.raises(ValueError):
        _device_grid([(x, z)], edge=0.0)


# ------------------------------------------------------------------------------------------------ statistics
def _stat_setup():
    if "stat" not in _CACHE:
        cases = C.stat_cases()
        plan = _device_plan([(c["mol"], c["z"]) for c in cases])
        grid = _device_grid([(c["prot_xyz"], c["prot_z"]) for c in cases])
        poses = np.concatenate([c["poses"] for c in cases], 1)           # [9, N, 3]
        want = [[C.contacts(p, C.bondi(c["z"]), c["prot_xyz"], c["prot_z"]) for p in c["poses"]] for c in cases]
        _CACHE["stat"] = (cases, plan, grid, poses, want)
    return _CACHE["stat"]


def _host_res(res):
    return dict(stats=res.stats.cpu().numpy(), counts=res.counts.cpu().numpy(), pair=res.pair.cpu().numpy(), flags=res.flags.cpu().numpy(),
                ok=res.ok.cpu().numpy())


def _compare(got, b, s, want, what, worst=None):
    """One (complex, pose) of a host result against the restatement."""
    assert got["counts"][b, s].tolist() == want["counts"].tolist(), (what, "counts", got["counts"][b, s], want["counts"])
    assert got["pair"][b, s].tolist() == want["pair"].tolist(), (what, "pair", got["pair"][b, s], want["pair"])
    assert int(got["flags"][b, s]) == want["flags"], (what, "flags")
    assert bool(got["ok"][b, s]) == (want["flags"] in (0, C.UNCHECKED)), what
    for col in range(3):
        g, w = float(got["stats"][b, s, col]), float(want["stats"][col])
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) if np.isnan(w) else g == w), (what, col, g, w)
            continue
        bd = C.bound(col, w)
        assert abs(g - w) <= bd, (what, col, g, w)
        if worst is not None and bd > 0:
            worst[col] = max(worst[col], abs(g - w) / bd)


@pytest.mark.parametrize("S", [1, 3, 8, 9])
def test_statistics_counts_pairs_and_flags(S):
    from fabind_amd import validity
    cases, plan, grid, poses, want = _stat_setup()
    got = _host_res(validity.check_poses_protein(_t(poses[:S]), plan, grid))
    assert got["stats"].shape == (len(cases), S, 3) and got["stats"].dtype == np.float32 and got["flags"].dtype == np.int32
    worst = [0.0, 0.0, 0.0]
    for b, c in enumerate(cases):
        for s in range(S):
            _compare(got, b, s, want[b][s], (c["name"], C.POSE_KINDS[s]), worst)
    print("protein contacts, S = %d: largest observed fraction of the bound: prot_clash %.3f, prot_dist %.3f, overlap %.3f" % (S, *worst))


def test_same_bits_alone_elsewhere_among_other_poses_and_on_a_repeat():
    from fabind_amd import validity
    cases, plan, grid, poses, want = _stat_setup()
    full = _host_res(validity.check_poses_protein(_t(poses), plan, grid))
    again = _host_res(validity.check_poses_protein(_t(poses), plan, grid))
    for f in full:
        assert full[f].tobytes() == again[f].tobytes(), f
    pick, off = [5, 2, 6], np.concatenate([[0], np.cumsum([c["mol"]["n"] for c in cases])])
    plan2 = _device_plan([(cases[i]["mol"], cases[i]["z"]) for i in pick])
    grid2 = _device_grid([(cases[i]["prot_xyz"], cases[i]["prot_z"]) for i in pick])
    sel = [7, 0, 4]                                                      # three of the nine poses, at other positions of another batch
    sub = _host_res(validity.check_poses_protein(_t(np.concatenate([cases[i]["poses"][sel] for i in pick], 1)), plan2, grid2))
    for pos, i in enumerate(pick):
        for f in full:
            assert sub[f][pos].tobytes() == np.ascontiguousarray(full[f][i][sel]).tobytes(), (cases[i]["name"], f)
    i = 3
    solo = _host_res(validity.check_poses_protein(_t(cases[i]["poses"][4]), _device_plan([(cases[i]["mol"], cases[i]["z"])]),
                                                  _device_grid([(cases[i]["prot_xyz"], cases[i]["prot_z"])])))
    for f in full:
        assert solo[f][0, 0].tobytes() == np.ascontiguousarray(full[f][i, 4]).tobytes(), f
    assert off[-1] == poses.shape[1]


def test_a_tie_resolves_to_the_lowest_ids():
    from fabind_amd import validity
    m = R.chain(2)
    m["x"] = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    prot = (np.array([[0.5, 9, 9], [2, 0, 0], [-2, 0, 0], [12, 0, 0], [0, 0, 2]], np.float32), np.array([1, 6, 6, 6, 6]))
    want = C.contacts(m["x"], C.bondi([6, 6]), *prot)
    assert want["pair"].tolist() == [0, 1] and want["counts"][0] == 4
    got = _host_res(validity.check_poses_protein(_t(m["x"]), _device_plan([(m, [6, 6])]), _device_grid([prot])))
    _compare(got, 0, 0, want, "tie")


def test_nan_in_one_pose_leaves_its_work_group_neighbours_unchanged():
    from fabind_amd import validity
    cases, plan, grid, poses, want = _stat_setup()
    clean = _host_res(validity.check_poses_protein(_t(poses[:8]), plan, grid))
    dirty = poses[:8].copy()
    b, off = 4, int(sum(c["mol"]["n"] for c in cases[:4]))
    dirty[3, off + 7, 1] = np.nan
    got = _host_res(validity.check_poses_protein(_t(dirty), plan, grid))
    assert got["flags"][b, 3] == C.NONFINITE and np.isnan(got["stats"][b, 3]).all() and not got["ok"][b, 3]
    assert got["counts"][b, 3].tolist() == [0, 0, 0] and got["pair"][b, 3].tolist() == [-1, -1]
    keep = np.ones(got["flags"].shape, bool)
    keep[b, 3] = False
    for f in clean:
        assert got[f][keep].tobytes() == clean[f][keep].tobytes(), f


def test_unchecked_for_a_plan_status_and_for_a_grid_status():
    from fabind_amd import validity
    cases = C.stat_cases()[:1]
    zero = R.chain(5)
    zero["x"] = R.embed(zero, seed=77)
    zero["x"][3] = zero["x"][2]                                          # plan status 5
    ok1, ok2 = R.chain(4), R.chain(3)
    ok1["x"], ok2["x"] = R.embed(ok1, seed=1), R.embed(ok2, seed=2)
    mols = [(zero, np.full(5, 6)), (ok1, np.full(4, 6)), (ok2, np.full(3, 6))]
    prot = (cases[0]["prot_xyz"], cases[0]["prot_z"])
    bad = (prot[0].copy(), prot[1])
    bad[0][5, 0] = np.inf                                                # grid status 6
    plan, grid = _device_plan(mols), _device_grid([prot, prot, bad])
    assert plan.status.cpu().tolist() == [5, 0, 0] and grid.status.cpu().tolist() == [0, 0, 6]
    poses = np.stack([np.concatenate([m["x"] for m, _ in mols]) + np.float32(k) for k in range(3)])
    got = _host_res(validity.check_poses_protein(_t(poses), plan, grid))
    for b in (0, 2):
        assert (got["flags"][b] == C.UNCHECKED).all() and np.isnan(got["stats"][b]).all() and got["ok"][b].all()
        assert (got["counts"][b] == 0).all() and (got["pair"][b] == -1).all()
    for s in range(3):
        _compare(got, 1, s, C.contacts(poses[s, 5:9], C.bondi(np.full(4, 6)), *prot), ("checked", s))
    none = _host_res(validity.check_poses_protein(_t(poses[:, :5]), _device_plan(mols[:1]), _device_grid([prot])))
    assert (none["flags"] == C.UNCHECKED).all() and np.isnan(none["stats"]).all()


def test_c_abi_fills_only_its_rows():
    """Through the C ABI wrapper: outputs prefilled with NaN and a sentinel, one sentinel row past the end survives."""
    from fabind_amd import kernels as K
    cases, plan, grid, poses, want = _stat_setup()
    B, S = len(cases), 3
    stats = torch.full((B * S + 1, 3), float("nan"), device=DEV)
    counts = torch.full((B * S + 1, 3), -77, dtype=torch.int32, device=DEV)
    pair = torch.full((B * S + 1, 2), -77, dtype=torch.int32, device=DEV)
    flags = torch.full((B * S + 1,), -77, dtype=torch.int32, device=DEV)
    stats[-1] = 12345.0
    K.pose_protein_check(_t(poses[:S]), plan.atom_off, B, plan.max_atoms, plan.status, plan.radii, grid.status, grid.origin, grid.dims,
                         grid.cell_off, grid.atom_off, grid.cell_ptr, grid.xyz, grid.radii, grid.atom_id, grid.edge,
                         (5.0, 0.75, 0.075, 0.8, 0.5), grid.max_radius, stats, counts, pair, flags)
    assert stats[-1].cpu().tolist() == [12345.0] * 3 and counts[-1].cpu().tolist() == [-77] * 3
    assert pair[-1].cpu().tolist() == [-77, -77] and int(flags[-1]) == -77
    got = dict(stats=stats[:-1].reshape(B, S, 3).cpu().numpy(), counts=counts[:-1].reshape(B, S, 3).cpu().numpy(),
               pair=pair[:-1].reshape(B, S, 2).cpu().numpy(), flags=flags[:-1].reshape(B, S).cpu().numpy())
    got["ok"] = (got["flags"] == 0) | (got["flags"] == C.UNCHECKED)
    assert not np.isnan(got["stats"]).any() and (got["counts"] >= 0).all() and (got["flags"] >= 0).all()
    for b, c in enumerate(cases):
        for s in range(S):
            _compare(got, b, s, want[b][s], (c["name"], s))


def test_custom_radii_on_both_sides_and_other_thresholds():
    from fabind_amd import validity
    cases = C.stat_cases()
    c = cases[5]
    rng = np.random.RandomState(11)
    r_lig = rng.uniform(1.0, 2.2, size=c["mol"]["n"]).astype(np.float32)
    r_prot = rng.uniform(0.7, 2.3, size=len(c["prot_z"])).astype(np.float32)
    plan = _device_plan([(c["mol"], c["z"])], radii=_t(r_lig))
    grid = _device_grid([(c["prot_xyz"], c["prot_z"])], radii=[r_prot], edge=4.5)
    kw = dict(cutoff=4.25, clash_min=0.6, overlap_max=0.2, vdw_scale=0.7, spacing=0.4)
    got = _host_res(validity.check_poses_protein(_t(c["poses"][:3]), plan, grid, **kw))
    for s in range(3):
        want = C.contacts(c["poses"][s], r_lig, c["prot_xyz"], c["prot_z"], r_prot, **kw)
        assert want["margins"]["cutoff"] >= 1e-6 and want["margins"]["lattice"] >= 1e-9 and want["margins"]["close"] >= 1e-9
        _compare(got, 0, s, want, ("custom", s))


def test_refusals():
    from fabind_amd import validity
    cases, plan, grid, poses, want = _stat_setup()
    with pytest.raises(ValueError, match="edge"):
        validity.check_poses_protein(_t(poses[:1]), plan, grid, cutoff=5.5)
    small = _device_grid([(c["prot_xyz"], c["prot_z"]) for c in cases], edge=4.0)
    with pytest.raises(ValueError, match="edge"):
        validity.check_poses_protein(_t(poses[:1]), plan, small)
    with pytest.raises(ValueError):
        validity.check_poses_protein(_t(poses[:1]), plan, small, cutoff=4.0, vdw_scale=3.0)     # a protein sphere wider than a cell
    with pytest.raises(ValueError):
        validity.check_poses_protein(_t(poses[:1]), plan, grid, spacing=0.05)                   # too many lattice points per atom
    with pytest.raises(ValueError):
        validity.check_poses_protein(_t(poses[:1, :-1]), plan, grid)
    with pytest.raises(ValueError):
        validity.check_poses_protein(_t(poses[:1]), plan, _device_grid([(cases[0]["prot_xyz"], cases[0]["prot_z"])]))


def test_batched_wrapper_agrees_with_the_direct_call():
    from fabind_amd import validity
    from fabind_amd.utils.post_optim_utils import check_protein_contacts_batched
    cases, plan, grid, poses, want = _stat_setup()
    cb = _t(np.repeat(np.arange(len(cases)), [c["mol"]["n"] for c in cases]))
    direct = validity.check_poses_protein(_t(poses[:3]), plan, grid, clash_min=0.7)
    ok, flags, stats = check_protein_contacts_batched(_t(poses[:3]), cb, plan, grid, clash_min=0.7)
    assert tuple(ok.shape) == (3, len(cases)) and tuple(stats.shape) == (3, len(cases), 3)
    assert torch.equal(ok, direct.ok.t()) and torch.equal(flags, direct.flags.t())
    assert stats.cpu().numpy().tobytes() == direct.stats.transpose(0, 1).contiguous().cpu().numpy().tobytes()
    ok1, flags1, stats1 = check_protein_contacts_batched(_t(poses[1]), cb, plan, grid, clash_min=0.7)
    assert tuple(ok1.shape) == (len(cases),) and torch.equal(ok1, direct.ok[:, 1]) and torch.equal(flags1, direct.flags[:, 1])
    assert stats1.cpu().numpy().tobytes() == direct.stats[:, 1].contiguous().cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        check_protein_contacts_batched(_t(poses[1]), cb.flip(0), plan, grid)
