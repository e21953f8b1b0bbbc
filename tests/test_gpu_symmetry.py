"""GPU: ligand automorphisms and symmetry-corrected RMSD (fabind_amd/symmetry.py, csrc/symmetry.hip) against the golden sets and
float64 minima of tests/golden/symmetry_graphs.npz (tools/make_golden_symmetry.py), their properties, the designed early exits,
and FABind+'s permutation-invariant loss fed from the device search instead of hand-written lists."""
import numpy as np
import pytest
import torch

from helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 4096


def _graphs():
    g = load_npz("symmetry_graphs")
    return g, [str(s) for s in g["names"]]


def _batch(g, ids):
    """Concatenate fixture graphs: labels [N], bonds [2, E] global, atom_off [B + 1]."""
    labs, bonds, off = [], [], [0]
    for gi in ids:
        lab, e = g["g%d_labels" % gi], g["g%d_bonds" % gi]
        labs.append(lab)
        bonds.append(e.astype(np.int64) + off[-1])
        off.append(off[-1] + len(lab))
    return (torch.from_numpy(np.concatenate(labs)).to(DEV), torch.from_numpy(np.concatenate(bonds, 1)).to(DEV),
            torch.tensor(off, dtype=torch.int32, device=DEV))


def _autos_of(A, b, n):
    lo, hi = int(A.off[b]), int(A.off[b + 1])
    return A.flat[lo:hi].cpu().numpy().reshape(-1, n) if n else np.zeros((int(A.count[b]), 0), np.int32)


def test_search_returns_the_fixture_sets_in_order():
    from fabind_amd.symmetry import ligand_automorphisms
    g, names = _graphs()
    lab, bonds, off = _batch(g, range(len(names)))
    A = ligand_automorphisms(lab, bonds, off, cap=CAP)
    torch.cuda.synchronize()
    assert A.status.cpu().tolist() == [0] * len(names)
    for gi, name in enumerate(names):
        want = g["g%d_autos" % gi]
        assert int(A.count[gi]) == len(want), name
        assert np.array_equal(_autos_of(A, gi, want.shape[1]), want), name
    assert int(A.count[names.index("c60")]) == 120 and int(A.count[names.index("nitrate_salt")]) == 8


def test_count_mode_agrees_with_write_mode_and_bonds_in_either_direction():
    from fabind_amd import _lib
    from fabind_amd.symmetry import _neighbour_lists, ligand_automorphisms
    g, names = _graphs()
    lab, bonds, off = _batch(g, range(len(names)))
    nptr, nidx = _neighbour_lists(bonds, lab.numel(), DEV)
    B = len(names)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    st = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().fabind_sym_automorphisms(lab.data_ptr(), nptr.data_ptr(), nidx.data_ptr(), off.data_ptr(), B, CAP,
                                                    1_000_000, None, None, None, cnt.data_ptr(), st.data_ptr(), _lib.stream()), "count")
    A = ligand_automorphisms(lab, torch.flip(bonds, [0]), off, cap=CAP)          # the reversed bond list: same graph
    assert st.cpu().tolist() == [0] * B and torch.equal(cnt, A.count)
    assert A.count.cpu().tolist() == [len(g["g%d_autos" % i]) for i in range(B)]


def test_early_exits_report_status_and_return():
    from fabind_amd.symmetry import ligand_automorphisms
    lab = torch.full((12,), 600, dtype=torch.int32, device=DEV)                  # 12 isolated identical atoms: 12! automorphisms
    none = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 12], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ligand 0: status 1"):
        ligand_automorphisms(lab, none, off, cap=1000)
    A = ligand_automorphisms(lab, none, off, cap=1000, on_overflow="truncate")
    assert int(A.status[0]) == 1 and int(A.count[0]) == 1000
    a = A.flat.cpu().numpy().reshape(1000, 12)
    assert np.array_equal(a[0], np.arange(12)) and len({tuple(r) for r in a}) == 1000
    assert all(tuple(a[k]) < tuple(a[k + 1]) for k in range(999))
    A = ligand_automorphisms(lab, none, off, cap=1000, max_steps=5, on_overflow="truncate")
    assert int(A.status[0]) == 2 and int(A.count[0]) == 1
    with pytest.raises(RuntimeError, match="status 2"):
        ligand_automorphisms(lab, none, off, cap=1000, max_steps=5)
    big = torch.full((300,), 600, dtype=torch.int32, device=DEV)                 # more than 256 atoms: identity only
    A = ligand_automorphisms(big, none, torch.tensor([0, 300], dtype=torch.int32, device=DEV), on_overflow="truncate")
    assert int(A.status[0]) == 3 and torch.equal(A.flat.cpu(), torch.arange(300, dtype=torch.int32))


def _pose_batch(g):
    from fabind_amd.symmetry import ligand_automorphisms
    lab, bonds, off = _batch(g, g["batch_graph"])
    A = ligand_automorphisms(lab, bonds, off, cap=CAP)
    cb = torch.repeat_interleave(torch.arange(off.numel() - 1, device=DEV), torch.diff(off).long())
    return A, torch.from_numpy(g["pred"]).to(DEV), torch.from_numpy(g["true"]).to(DEV), cb, off


def test_minima_match_the_float64_fixture():
    from fabind_amd.symmetry import symmetric_rmsd
    g, _ = _graphs()
    A, pred, true, cb, _ = _pose_batch(g)
    assert pred.shape[0] == 10 and A.count.numel() == 64
    r, corr, ar, l1, al = symmetric_rmsd(pred, true, cb, A, return_details=True)
    assert r.shape == (10, 64) and bool(corr.all())
    np.testing.assert_allclose(r.cpu().numpy(), g["exp_rmsd"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(l1.cpu().numpy(), g["exp_sl1"], rtol=1e-6, atol=0)
    assert np.array_equal(ar.cpu().numpy(), g["exp_arg_rmsd"]) and np.array_equal(al.cpu().numpy(), g["exp_arg_sl1"])
    r1, _ = symmetric_rmsd(pred[3], true, cb, A)                                 # one pose: [B]
    assert r1.shape == (64,) and torch.equal(r1, r[3])


def test_symmetric_rmsd_properties():
    from fabind_amd.symmetry import symmetric_rmsd
    g, _ = _graphs()
    A, pred, true, cb, off = _pose_batch(g)
    r, _ = symmetric_rmsd(pred, true, cb, A)
    r2, _ = symmetric_rmsd(pred, true, cb, A)
    assert torch.equal(r, r2)                                                    # bit-identical runs
    plain = torch.zeros(pred.shape[0], 64, device=DEV).index_add_(1, cb, ((pred - true) ** 2).sum(-1))
    plain = (plain / torch.diff(off).float()).sqrt()
    assert bool((r <= plain * (1 + 1e-6)).all())
    k1 = torch.tensor([len(g["g%d_autos" % i]) == 1 for i in g["batch_graph"]], device=DEV)
    assert bool(k1.any()) and torch.allclose(r[:, k1], plain[:, k1], rtol=1e-6, atol=0)
    # an automorphism applied to the true pose leaves the symmetric RMSD unchanged
    offh = off.cpu().numpy()
    perm = np.arange(true.shape[0])
    rng = np.random.default_rng(0)
    for b, gi in enumerate(g["batch_graph"]):
        autos = g["g%d_autos" % gi]
        perm[offh[b]:offh[b + 1]] = autos[rng.integers(len(autos))] + offh[b]
    rp, _ = symmetric_rmsd(pred, true[torch.from_numpy(perm).to(DEV)], cb, A)
    torch.testing.assert_close(rp, r, rtol=1e-6, atol=0)
    # a failed ligand falls back to plain RMSD and says so
    from dataclasses import replace
    bad = replace(A, status=A.status.clone())
    bad.status[5] = 2
    rb, corr = symmetric_rmsd(pred, true, cb, bad)
    assert corr.cpu().tolist() == [b != 5 for b in range(64)]
    assert torch.allclose(rb[:, 5], plain[:, 5], rtol=1e-6, atol=0) and torch.equal(rb[:, :5], r[:, :5])


def test_best_automorphism_index_equals_best_isomorphism_index():
    from fabind_amd.plus.models.model import best_isomorphism_index
    from fabind_amd.symmetry import best_automorphism_index, to_isomorphism_lists
    g, _ = _graphs()
    A, pred, true, _, off = _pose_batch(g)
    isos = to_isomorphism_lists(A)
    n = torch.diff(off).tolist()
    for s in (0, 7):
        want = best_isomorphism_index(pred[s], true, n, isos)
        got = best_automorphism_index(pred[s], true, A, off)
        assert got.dtype == torch.int64 and torch.equal(got, want)


def _plus_model_and_batch():
    from fabind_amd import synthetic
    from fabind_amd.plus.models import get_model
    from test_gpu_plus import _args

    class _Log:
        def log_message(self, s):
            pass
    a = _args(64, 2, 1)
    for k, v in dict(pocket_pred_hidden_size=32, pocket_pred_layers=1, pocket_pred_n_iter=1, random_n_iter=False,
                     use_for_radius_pred="ligand", dis_map_thres=15.0, pocket_radius_buffer=5.0, min_pocket_radius=20.0,
                     force_fix_radius=False, use_clustering=False, gs_tau=1.0, gs_hard=False, pocket_radius=20.0,
                     train_pred_pocket_noise=0.0, local_eval=False).items():
        setattr(a, k, v)
    torch.manual_seed(0)
    m = get_model(a, _Log()).to(DEV).eval()
    sizes = [(60, 9), (45, 14), (80, 6), (52, 11)]
    data = synthetic.make_hetero_batch(sizes, seed=3).to(DEV)
    data.ligand_radius = torch.tensor([6.0, 7.0, 5.0, 6.5], device=DEV)
    return m, data, [s[1] for s in sizes]


def test_plus_loss_with_device_isomorphisms_end_to_end():
    from fabind_amd.plus.models import compute_loss
    from fabind_amd.symmetry import ligand_automorphisms, symmetric_rmsd, to_isomorphism_lists
    m, data, num_atoms = _plus_model_and_batch()
    # the compound bond list of the batch (chains; local ids + 1 for the global node) in global ligand-atom ids
    off = torch.tensor(np.concatenate([[0], np.cumsum(num_atoms)]), dtype=torch.int32, device=DEV)
    ex = data["compound_atom_edge_list"]
    bonds = (ex.x.T.long() - 1) + off[ex.batch].long()
    labels = torch.full((int(off[-1]),), 600, dtype=torch.int32, device=DEV)
    A = ligand_automorphisms(labels, bonds, off)
    isos = to_isomorphism_lists(A)
    hand = [[list(range(n)), list(reversed(range(n)))] for n in num_atoms]
    assert [[a.tolist() for a in L] for L in isos] == hand
    with torch.no_grad():
        d = data.clone()
        d.ligand_radius = data.ligand_radius
        out = m(d, train=False)                    # moves d.coords into the frame of the predicted coordinates
        losses = []
        for iso in (hand, isos):
            d.num_atoms, d.isomorphisms = num_atoms, iso
            losses.append(compute_loss(out, d)[0])
    assert torch.equal(losses[0], losses[1])
    coords, cb = out[0], out[1]
    r, corr = symmetric_rmsd(coords, d.coords, cb, A)
    c, t = coords.double().cpu().numpy(), d.coords.double().cpu().numpy()
    want = []
    for b, n in enumerate(num_atoms):
        o = int(off[b])
        ci, ti = c[o:o + n], t[o:o + n]
        want.append(min(np.sqrt(((ci - ti) ** 2).sum(-1).mean()), np.sqrt(((ci[::-1] - ti) ** 2).sum(-1).mean())))
    assert bool(corr.all())
    np.testing.assert_allclose(r.cpu().numpy(), np.array(want), rtol=1e-5, atol=1e-6)
