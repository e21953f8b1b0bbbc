"""GPU: superposed symmetric RMSD of conformers, the fit behind it, greedy pruning and the pruned embedding (fabind_amd/ensemble.py,
csrc/conformer_rmsd.hip, utils.inference_mol_utils.generate_diverse_conformations_batched) against the float64 restatements of
tests/ensemble_refs.py (pinned on the CPU by tests/test_ensemble_refs_cpu.py).

Values: |D_dev^2 - D_ref^2| <= (4 n + 64) 2^-53 (G_s + G_t) / n + 2^-22 D_ref^2 (ensemble_refs.bound_d2; DESIGN.md section 21 derives
it); every case prints its largest fraction of the bound before it asserts (`pytest -s`).  The native calls of this file write into
NaN- / sentinel-prefilled buffers with a guard band on either side of each output."""
import numpy as np
import pytest
import torch

import conformer_refs as C
import embed_refs as E
import ensemble_refs as R
from helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64
U53 = 2.0 ** -53
SKIP_CAP = 0.05
_seen = {"frac": 0.0, "fit_frac": 0.0, "qerr": 0.0, "skipped": 0, "entries": 0}


def _table(autos_list, status=None):
    """`symmetry.Automorphisms` of hand-given lists: one [K_b, n_b] array per ligand."""
    from fabind_amd.symmetry import Automorphisms
    n = [a.shape[1] for a in autos_list]
    off = np.concatenate([[0], np.cumsum([a.size for a in autos_list])])
    flat = np.concatenate([a.reshape(-1) for a in autos_list]) if autos_list else np.zeros(0)
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)          # noqa: E731
    return Automorphisms(flat=i32(flat), off=i32(off), count=i32([len(a) for a in autos_list]),
                         status=i32(status if status is not None else [0] * len(n)), atom_off=i32(np.concatenate([[0], np.cumsum(n)])))


def _ident(n):
    return np.arange(n).reshape(1, n)


def _guarded(shape, dtype, fill):
    """A buffer with a sentinel band on either side of `shape` elements prefilled with `fill` -> (whole, view, check)."""
    size = int(np.prod(shape))
    sent = -7
    buf = torch.full((size + 2 * GUARD,), sent, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + size] = fill
    ok = lambda: bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + size:] == sent).all())   # noqa: E731
    return buf, buf[GUARD:GUARD + size].reshape(shape), ok


def _abi_args(A):
    use = torch.where(A.status == 0, A.count, torch.zeros_like(A.count))
    flat = A.flat if A.flat.numel() else torch.zeros(1, dtype=torch.int32, device=DEV)
    return use, flat, A.atom_off.numel() - 1, int(torch.diff(A.atom_off).max())


def _guarded_pair(x, A, max_atoms=None):
    from fabind_amd import _lib
    S, N = x.shape[0], x.shape[1]
    use, flat, B, ma = _abi_args(A)
    buf, D, ok = _guarded((B, S, S), torch.float32, float("nan"))
    rc = _lib.load().fabind_conformer_pair_rmsd(x.data_ptr(), S, N, A.atom_off.data_ptr(), A.off.data_ptr(), use.data_ptr(), flat.data_ptr(), B,
                                                ma if max_atoms is None else max_atoms, D.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, D, ok


def _guarded_cross(x, y, A, fit=True, max_atoms=None):
    from fabind_amd import _lib
    S, N, T = x.shape[0], x.shape[1], y.shape[0]
    use, flat, B, ma = _abi_args(A)
    _, D, ok_d = _guarded((B, S, T), torch.float32, float("nan"))
    _, k, ok_k = _guarded((B, S, T), torch.int32, -99)
    _, q, ok_q = _guarded((B, S, T, 4), torch.float64, float("nan"))
    _, t, ok_t = _guarded((B, S, T, 3), torch.float64, float("nan"))
    rc = _lib.load().fabind_conformer_cross_rmsd(x.data_ptr(), S, y.data_ptr(), T, N, A.atom_off.data_ptr(), A.off.data_ptr(), use.data_ptr(),
                                                 flat.data_ptr(), B, ma if max_atoms is None else max_atoms, D.data_ptr(),
                                                 k.data_ptr() if fit else None, q.data_ptr() if fit else None,
                                                 t.data_ptr() if fit else None, _lib.stream())
    torch.cuda.synchronize()
    return rc, D, k, q, t, lambda: ok_d() and ok_k() and ok_q() and ok_t()


def _assert_structure(D):
    assert torch.equal(D, D.transpose(1, 2))                                             # bit-symmetric
    diag = torch.diagonal(D, dim1=1, dim2=2)
    assert torch.equal(diag.contiguous().view(torch.int32), torch.zeros_like(diag, dtype=torch.int32))   # +0.0, not -0.0


def _assert_bound(name, D_dev, ref, n, off_diag=False):
    got = D_dev.double().cpu().numpy()
    err, bnd = np.abs(got * got - ref["D"] ** 2), R.bound_d2(n, ref["G"], ref["D"])
    if off_diag:
        err = np.where(np.eye(len(err), dtype=bool), 0.0, err)
    frac = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    _seen["frac"] = max(_seen["frac"], frac)
    print("conformer_rmsd %-26s n %3d shape %-8s max err / bound = %.4f" % (name, n, got.shape, frac))
    assert (err <= bnd).all(), (name, frac)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("name", [s[0] for s in R.SPEC])
def test_values_fit_and_memory_against_float64(name):
    from fabind_amd import ensemble
    c = R.cases()[name]
    n, autos = c["n"], c["autos"]
    A = _table([autos if autos is not None else _ident(n)])
    arg = A if autos is not None else None                                               # the plain case goes through autos=None as well
    x, y = torch.from_numpy(c["X"]).to(DEV), torch.from_numpy(c["Y"]).to(DEV)
    off = A.atom_off
    rc, D, ok = _guarded_pair(x, A)
    assert rc == 0 and ok() and not bool(torch.isnan(D).any())
    _assert_structure(D)
    _assert_bound(name, D[0], c["pair"], n)
    assert torch.equal(_bits(ensemble.aligned_pairwise_rmsd(x, off, arg)), _bits(D))     # the public path, and a repeat: same bits
    rc, Dc, k, q, t, ok = _guarded_cross(x, y, A)
    assert rc == 0 and ok() and not bool(torch.isnan(Dc).any())
    _assert_bound(name + " cross", Dc[0], c["cross"], n)
    fit = ensemble.aligned_rmsd_to(x, y, off, arg, return_fit=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((fit.rmsd, Dc), (fit.quat, q), (fit.trans, t))) and torch.equal(fit.auto_index, k)
    assert torch.equal(_bits(ensemble.aligned_rmsd_to(x, y, off, arg)), _bits(Dc))       # without the fit: the same eigenvalues
    assert torch.equal(_bits(ensemble.aligned_rmsd_to(x, y[0], off, arg)), _bits(Dc[:, :, :1]))      # T = 1, ref as [N, 3]
    # the fit: RMSD recomputed in float64 from (auto_index, quat, trans); |q| = 1; the index against the restatement's argmin
    kh, qh, th = k[0].cpu().numpy(), q[0].cpu().numpy(), t[0].cpu().numpy()
    a_all = autos if autos is not None else _ident(n)
    ref = c["cross"]
    bnd = R.bound_d2(n, ref["G"], ref["D"])
    dev2 = Dc[0].double().cpu().numpy() ** 2
    for s in range(len(c["X"])):
        for u in range(3):
            assert 0 <= kh[s, u] < len(a_all)
            d = R.fit_rmsd(c["X"][s], c["Y"][u], a_all[kh[s, u]], qh[s, u], th[s, u])
            # this recomputation's own rounding: R x + trans - y loses about eight roundings of its largest term per coordinate,
            # an error vector of length <= eps per atom, which moves d^2 by at most 2 d eps + eps^2
            eps = np.sqrt(3.0) * 8 * U53 * (np.abs(c["X"][s]).max() + np.abs(c["Y"][u]).max() + np.abs(th[s, u]).max())
            over = abs(d * d - dev2[s, u]) - (2 * d * eps + eps * eps)
            if bnd[s, u] > 0:
                _seen["fit_frac"] = max(_seen["fit_frac"], over / bnd[s, u])
            assert over <= bnd[s, u], (name, s, u, over, bnd[s, u])
    qn = np.sqrt((qh.astype(np.longdouble) ** 2).sum(-1))
    _seen["qerr"] = max(_seen["qerr"], float(np.abs(qn - 1).max() / U53))
    assert (np.abs(qn - 1) <= 4 * U53).all(), float(np.abs(qn - 1).max() / U53)
    decided = ref["gap"] > 2 * n * bnd
    _seen["skipped"] += int((~decided).sum())
    _seen["entries"] += decided.size
    assert np.array_equal(kh[decided], ref["k"][decided]), name
    # X against one of its own conformers = that column of the pair form, within the same bound
    col = ensemble.aligned_rmsd_to(x, x[1], off, arg)[0, :, 0]
    _assert_bound(name + " col 1", col[:, None], dict(D=c["pair"]["D"][:, 1:2], G=c["pair"]["G"][:, 1:2]), n)


def test_observed_fractions_and_the_share_of_skipped_indices():
    """Runs after the parametrised cases: what they saw.  The share of auto_index entries too close to call is capped at 5 %."""
    share = _seen["skipped"] / max(_seen["entries"], 1)
    print("\nlargest err / bound %.4f; fit RMSD^2 against D^2 / bound %.4f; ||q| - 1| / 2^-53 = %.2f; auto_index skipped %d of %d (%.2f %%)"
          % (_seen["frac"], _seen["fit_frac"], _seen["qerr"], _seen["skipped"], _seen["entries"], 100 * share))
    assert share <= SKIP_CAP


def _batch():
    """A mixed batch: an empty ligand in the middle, a table with status != 0 (identity alone), S = 9 (two tiles, the second partial)."""
    rng = np.random.default_rng(5)
    S = 9
    names = ["benzene", "chain_mixed", "druglike_61", "neopentane", "nitrate_salt"]
    autos = [R.fixture_autos(nm) for nm in names]
    autos.insert(2, np.zeros((1, 0), dtype=np.int64))                                    # n_b = 0 between two non-empty ligands
    status = [0, 0, 0, 0, 1, 0]                                                          # neopentane: its table must not be used
    X = [R.random_conformers(rng, S, a.shape[1], a) for a in autos]
    return S, autos, status, X


def test_mixed_batch_equals_every_ligand_alone():
    from fabind_amd import ensemble
    S, autos, status, X = _batch()
    A = _table(autos, status)
    x = torch.from_numpy(np.concatenate(X, axis=1)).to(DEV)
    rc, D, ok = _guarded_pair(x, A)
    assert rc == 0 and ok()
    _assert_structure(D)
    assert not bool(D[2].any()) and not bool(torch.isnan(D).any())                       # the empty ligand: zeros
    y = x[[4, 0, 7]]
    rc, Dc, k, q, t, ok = _guarded_cross(x, y, A)
    assert rc == 0 and ok()
    assert not bool(Dc[2].any()) and not bool(k[2].any()) and bool((q[2] == torch.tensor([1.0, 0, 0, 0], device=DEV, dtype=torch.float64)).all())
    assert not bool(t[2].any()) and not bool(k[4].any())                                 # status != 0: the identity alone
    for b, a in enumerate(autos):
        n = a.shape[1]
        if n == 0:
            continue
        use = a if status[b] == 0 else None
        _assert_bound("batch[%d]" % b, D[b], R.aligned_rmsd_ref(X[b], None, use), n)
        Ab = _table([a], [status[b]])
        xb = torch.from_numpy(X[b]).to(DEV)
        alone = ensemble.aligned_pairwise_rmsd(xb, Ab.atom_off, Ab)
        assert torch.equal(_bits(alone[0]), _bits(D[b])), b                              # alone = in the batch, bit for bit
        fa = ensemble.aligned_rmsd_to(xb, xb[[4, 0, 7]], Ab.atom_off, Ab, return_fit=True)
        assert torch.equal(_bits(fa.rmsd[0]), _bits(Dc[b])) and torch.equal(fa.auto_index[0], k[b])
        assert torch.equal(_bits(fa.quat[0]), _bits(q[b])) and torch.equal(_bits(fa.trans[0]), _bits(t[b]))
        if status[b]:
            plain = ensemble.aligned_pairwise_rmsd(xb, Ab.atom_off)
            assert torch.equal(_bits(plain[0]), _bits(D[b]))


def test_the_same_bits_among_any_number_of_conformers_in_any_slot_and_with_the_roles_swapped():
    from fabind_amd import ensemble
    c = R.cases()["benzene n6 K12 S17"]
    A = _table([c["autos"]])
    off = A.atom_off
    x = torch.from_numpy(c["X"]).to(DEV)
    D = ensemble.aligned_pairwise_rmsd(x, off, A)
    assert torch.equal(_bits(ensemble.aligned_pairwise_rmsd(x, off, A)), _bits(D))       # a repeat
    for pick in ([2, 9, 16], [0, 8], [7, 8, 15, 16]):                                    # 3 of 17: pairs of two tiles now share one
        sub = ensemble.aligned_pairwise_rmsd(x[pick], off, A)
        assert torch.equal(_bits(sub), _bits(D[:, pick][:, :, pick])), pick
    # the cross form puts the first conformer in the row tile whatever its index: X[:9] against X[9:] = that block of the pair form
    blk = ensemble.aligned_rmsd_to(x[:9], x[9:], off, A)
    assert torch.equal(_bits(blk), _bits(D[:, :9, 9:]))
    # roles swapped.  Identity alone: S becomes its transpose, Horn's matrix changes the sign of its first row and column, and every
    # operation of the Jacobi sweep is odd or even in those signs: the same bits.  With automorphisms the permuted side changes, the
    # sums are taken in another order: the same value within the bound.
    y = torch.from_numpy(c["Y"]).to(DEV)
    ab, ba = ensemble.aligned_rmsd_to(x, y, off), ensemble.aligned_rmsd_to(y, x, off)
    assert torch.equal(_bits(ab), _bits(ba.transpose(1, 2)))
    sw = ensemble.aligned_rmsd_to(y, x, off, A)
    ref = c["cross"]
    _assert_bound("roles swapped", sw[0].t(), ref, c["n"])


def test_nan_and_inf_stay_in_their_conformer():
    from fabind_amd import ensemble
    S, autos, status, X = _batch()
    A = _table(autos, status)
    x = torch.from_numpy(np.concatenate(X, axis=1)).to(DEV)
    D = ensemble.aligned_pairwise_rmsd(x, A.atom_off, A)
    bad = x.clone()
    a0 = A.atom_off.tolist()
    bad[3, a0[0] + 2, 1] = float("nan")                                                  # benzene, conformer 3
    bad[8, a0[3] + 5, 0] = float("inf")                                                  # druglike_61, conformer 8
    Dn = ensemble.aligned_pairwise_rmsd(bad, A.atom_off, A)
    hit = torch.zeros_like(D, dtype=torch.bool)
    hit[0, 3, :] = hit[0, :, 3] = True
    hit[3, 8, :] = hit[3, :, 8] = True
    hit[0, 3, 3] = hit[3, 8, 8] = False                                                  # the diagonal stays +0.0
    assert bool(torch.isnan(Dn[hit]).all()) and torch.equal(_bits(Dn[~hit]), _bits(D[~hit]))
    _assert_structure(torch.nan_to_num(Dn, nan=5.0))
    f = ensemble.aligned_rmsd_to(bad, x[:2], A.atom_off, A, return_fit=True)
    g = ensemble.aligned_rmsd_to(x, x[:2], A.atom_off, A, return_fit=True)
    hc = torch.zeros_like(f.rmsd, dtype=torch.bool)
    hc[0, 3], hc[3, 8] = True, True
    assert bool(torch.isnan(f.rmsd[hc]).all()) and torch.equal(_bits(f.rmsd[~hc]), _bits(g.rmsd[~hc]))
    assert torch.equal(_bits(f.quat[~hc]), _bits(g.quat[~hc])) and torch.equal(f.auto_index[~hc], g.auto_index[~hc])


def test_a_ligand_larger_than_the_staging_and_degenerate_shapes():
    from fabind_amd import ensemble
    rng = np.random.default_rng(8)
    autos = [R.chain_autos(5), R.chain_autos(9)]
    X = [R.random_conformers(rng, 4, a.shape[1], a) for a in autos]
    A = _table(autos)
    x = torch.from_numpy(np.concatenate(X, axis=1)).to(DEV)
    rc, D, ok = _guarded_pair(x, A, max_atoms=5)                                         # sized for 5 atoms: the 9-atom ligand gets NaN
    assert rc == 0 and ok()
    eye = torch.eye(4, dtype=torch.bool, device=DEV)
    assert bool(torch.isnan(D[1][~eye]).all()) and not bool(D[1][eye].any())
    assert torch.equal(_bits(D[0]), _bits(ensemble.aligned_pairwise_rmsd(x, A.atom_off, A)[0]))
    rc, Dc, k, q, t, ok = _guarded_cross(x, x[:1], A, max_atoms=5)
    assert rc == 0 and ok() and bool(torch.isnan(Dc[1]).all()) and bool(torch.isnan(q[1]).all()) and not bool(torch.isnan(Dc[0]).any())
    # one conformer; no ligand; no reference
    one = ensemble.aligned_pairwise_rmsd(x[:1], A.atom_off, A)
    assert one.shape == (2, 1, 1) and torch.equal(_bits(one), torch.zeros(2, 1, 1, dtype=torch.int32, device=DEV))
    self1 = ensemble.aligned_rmsd_to(x[:1], x[0], A.atom_off, A, return_fit=True)
    for b in range(2):                                                                   # a conformer against itself: 0 within the bound
        G2 = 2 * float((R.centred(X[b][0]) ** 2).sum())
        assert float(self1.rmsd[b, 0, 0]) ** 2 <= R.bound_d2(X[b].shape[1], G2, 0.0)
    assert self1.rmsd.shape == (2, 1, 1)
    none = _table([])
    z = torch.zeros(3, 0, 3, device=DEV)
    assert ensemble.aligned_pairwise_rmsd(z, none.atom_off, none).shape == (0, 3, 3)
    assert ensemble.aligned_rmsd_to(z, z[:2], none.atom_off).shape == (0, 3, 2)
    assert ensemble.aligned_rmsd_to(x, x[:0], A.atom_off, A, return_fit=True).quat.shape == (2, 4, 0, 4)


def test_a_ligand_whose_two_tiles_need_more_than_64_kb():
    """1400 atoms: one conformer per tile and 67 KB of centred doubles, past the 64 KB a launch gets without asking; the identity alone."""
    from fabind_amd import ensemble
    rng = np.random.default_rng(9)
    n = 1400
    X = R.random_conformers(rng, 3, n)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    D = ensemble.aligned_pairwise_rmsd(torch.from_numpy(X).to(DEV), off)
    _assert_structure(D)
    _assert_bound("n 1400", D[0], R.aligned_rmsd_ref(X, None, None), n)


def _prune_host(pr, b=0):
    n = int(pr.n_keep[b])
    order = pr.order[:, b].cpu().numpy()
    assert (order[n:] == -1).all()
    return pr.keep[b].cpu().numpy(), [int(v) for v in order[:n]]


def test_pruning_on_planted_modes_equals_the_restatement():
    from fabind_amd import ensemble
    for name, (X, mode, D64, autos, key, valid) in R.mode_cases().items():
        off = ~np.eye(len(mode), dtype=bool)
        assert (np.abs(D64 - R.THRESHOLD)[off] >= R.MARGIN).all(), name                  # the margin condition first
        A = _table([autos])
        x = torch.from_numpy(X).to(DEV)
        D = ensemble.aligned_pairwise_rmsd(x, A.atom_off, A)
        _assert_bound("modes " + name, D[0], R.aligned_rmsd_ref(X, None, autos), X.shape[1])
        kt = torch.from_numpy(key).to(DEV)[None]
        for v in (None, valid):
            pr = ensemble.prune_conformers(D, kt, R.THRESHOLD, None if v is None else torch.from_numpy(v).to(DEV)[None])
            keep, kept = _prune_host(pr)
            w_keep, w_kept = R.prune_ref(D64, key, R.THRESHOLD, v)                       # the restatement on the FLOAT64 distances
            assert np.array_equal(keep, w_keep) and kept == w_kept, name
            Dh = D[0].cpu().numpy()
            assert all(Dh[a, b] >= R.THRESHOLD for a in kept for b in kept if a != b)    # kept conformers are pairwise apart
            ok = np.ones(len(mode), bool) if v is None else v
            for c in np.nonzero(ok & ~keep)[0]:                                          # a dropped valid one: an earlier kept one within
                rank = lambda i: (key[i], i)                                             # noqa: E731
                assert any(Dh[u, c] < R.THRESHOLD and rank(u) < rank(c) for u in kept), (name, c)
            assert not keep[~ok].any()
            if v is not None:                                                            # invalid ones never remove a valid one
                sub = np.nonzero(v)[0]
                alone = ensemble.prune_conformers(D[:, sub][:, :, sub], kt[:, sub], R.THRESHOLD)
                assert np.array_equal(_prune_host(alone)[0], keep[sub]), name
            else:
                assert len(kept) == mode.max() + 1                                       # one per planted shape
        for thr, want in ((0.0, len(mode)), (float("inf"), 1)):
            assert int(ensemble.prune_conformers(D, kt, thr).n_keep[0]) == want


def _molecules():
    """The four crystal ligands and two hand molecules: (bond_index, codes, z, atom_off, crystal x [N, 3] with zeros for the hand ones,
    chiral signs, names)."""
    g = load_npz("conformer_ligands")
    hand = E.hand_molecules()
    cases = [(m["name"], m, np.asarray(g[m["name"] + "_z"], np.int64)) for m in C.fixture_molecules(g)]
    cases += [(k, hand[k][0], np.asarray(hand[k][1], np.int64)) for k in ("biphenyl", "butane")]
    mols = [m for _, m, _ in cases]
    x0 = [m["x"] if "x" in m else np.zeros((m["n"], 3), np.float32) for m in mols]
    x, bi, codes, off = C.pack(mols, x0)
    return bi, codes, np.concatenate([z for _, _, z in cases]), off, x, [k for k, _, _ in cases]


def test_end_to_end_pruned_embedding_against_the_crystal_conformation():
    from fabind_amd import embed, ensemble
    from fabind_amd.utils.inference_mol_utils import generate_diverse_conformations_batched
    bi, codes, z, off, x0, names = _molecules()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)                       # noqa: E731
    signs = embed.chiral_signs_from_coords(t(bi), t(codes), t(z), t(x0), off)
    signs[int(off[4]):] = 0                                                              # the hand molecules have no crystal pose
    run = {S: generate_diverse_conformations_batched(t(z), t(bi), t(codes), off, n_confs=S, seed=0, chiral_sign=signs) for S in (8, 16)}
    d16, d8 = run[16], run[8]
    aoff = d16.autos.atom_off
    ref = t(x0)
    ref[int(off[4]):] = d8.embedding.coords[0, int(off[4]):]                             # the hand molecules: their first conformer
    to16 = ensemble.aligned_rmsd_to(d16.embedding.coords, ref, aoff, d16.autos)[:, :, 0]
    to8 = ensemble.aligned_rmsd_to(d8.embedding.coords, ref, aoff, d8.autos)[:, :, 0]
    assert torch.equal(_bits(to16[:, :8]), _bits(to8))                                   # conformer c is the same bits among any n_confs
    assert bool((to16.min(1).values <= to8.min(1).values).all())                         # hence best-of-16 <= best-of-8, exactly
    nk = d16.n_keep.cpu().numpy()
    print("\nkept of 16:", dict(zip(names, nk.tolist())), "best-of-8 / 16 RMSD to the crystal (A):",
          [round(float(v), 3) for v in to8.min(1).values[:4]], [round(float(v), 3) for v in to16.min(1).values[:4]])
    assert ((nk >= 1) & (nk <= 16)).all()
    assert torch.equal((d16.order >= 0).sum(0).to(torch.int32), d16.n_keep)
    # the kept conformers, padded: slot r of ligand b is conformer order[r, b]
    order = d16.order.cpu().numpy()
    for b in range(len(names)):
        a0, a1 = int(off[b]), int(off[b + 1])
        for r in range(16):
            got = d16.coords[r, a0:a1]
            want = d16.embedding.coords[order[r, b], a0:a1] if order[r, b] >= 0 else torch.zeros_like(got)
            assert torch.equal(got, want), (b, r)
        kept = order[:nk[b], b]
        Dh = d16.D[b].cpu().numpy()
        assert all(Dh[u, v] >= 0.5 for u in kept for v in kept if u != v)
        assert (d16.status[b].cpu().numpy()[kept] == 0).all()
    # superpose: the moved conformers have, without any further alignment, the RMSD to the crystal that aligned_rmsd_to reported
    moved = ensemble.superpose(d16.embedding.coords, ref, aoff, d16.autos)
    assert moved.dtype == torch.float32 and moved.shape == d16.embedding.coords.shape
    mh, rh, th = moved.double().cpu().numpy(), ref.double().cpu().numpy(), to16.double().cpu().numpy()
    A = d16.autos
    flat, foff, cnt = A.flat.cpu().numpy(), A.off.cpu().numpy(), A.count.cpu().numpy()
    assert (A.status.cpu().numpy() == 0).all()
    for b in range(len(names)):
        a0, a1 = int(off[b]), int(off[b + 1])
        n = a1 - a0
        autos = flat[foff[b]:foff[b] + cnt[b] * n].reshape(cnt[b], n)
        # float32 rounding of the moved coordinates (at most 2^-24 of the largest one each) and of the reported distance
        tol = 2 * np.sqrt(3.0) * 2.0 ** -24 * np.abs(rh[a0:a1]).max() + 2.0 ** -22 * th[b].max() + 1e-7
        for s in range(16):
            d = np.sqrt((((mh[s, a0:a1][autos] - rh[a0:a1]) ** 2).sum((1, 2)) / n).min())
            assert abs(d - th[b, s]) <= tol, (names[b], s, d, th[b, s])


def test_argument_errors():
    from fabind_amd import _lib, ensemble
    A = _table([R.chain_autos(3)])
    off = A.atom_off
    x = torch.zeros(4, 3, 3, device=DEV)
    with pytest.raises(RuntimeError, match="HIP device"):
        ensemble.aligned_pairwise_rmsd(x.cpu(), off)
    with pytest.raises(RuntimeError, match="HIP device"):
        ensemble.aligned_rmsd_to(x, x[0].cpu(), off)
    with pytest.raises(RuntimeError, match="HIP device"):
        ensemble.prune_conformers(torch.zeros(1, 4, 4), torch.zeros(1, 4))
    with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
        ensemble.aligned_pairwise_rmsd(x[0], off)
    with pytest.raises(ValueError, match="512"):
        ensemble.aligned_pairwise_rmsd(torch.zeros(513, 3, 3, device=DEV), off)
    with pytest.raises(ValueError, match="512"):
        ensemble.aligned_rmsd_to(x, torch.zeros(513, 3, 3, device=DEV), off)
    with pytest.raises(ValueError, match="2048"):
        ensemble.aligned_pairwise_rmsd(torch.zeros(2, 2049, 3, device=DEV), [0, 2049])
    with pytest.raises(ValueError, match="atom_off"):
        ensemble.aligned_pairwise_rmsd(x, [0, 2])
    with pytest.raises(ValueError, match="autos"):
        ensemble.aligned_pairwise_rmsd(x, [0, 1, 3], A)
    with pytest.raises(ValueError, match="ref must be"):
        ensemble.aligned_rmsd_to(x, torch.zeros(2, 4, 3, device=DEV), off)
    D = torch.zeros(1, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="rank_key"):
        ensemble.prune_conformers(D, torch.zeros(4, 1, device=DEV))
    with pytest.raises(ValueError, match="valid"):
        ensemble.prune_conformers(D, torch.zeros(1, 4, device=DEV), valid=torch.ones(1, 3, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="threshold"):
        ensemble.prune_conformers(D, torch.zeros(1, 4, device=DEV), threshold=-1.0)
    # the library's own refusals: nothing is written
    big = torch.zeros(513, 3, 3, device=DEV)
    rc, Dg, ok = _guarded_pair(big, A)
    assert rc != 0 and b"512" in _lib.load().fabind_last_error() and bool(torch.isnan(Dg).all()) and ok()
    rc, Dg, k, q, t, ok = _guarded_cross(x, big, A)
    assert rc != 0 and b"512" in _lib.load().fabind_last_error() and bool(torch.isnan(Dg).all()) and ok()
    rc, Dg, ok = _guarded_pair(x, A, max_atoms=2049)
    assert rc != 0 and b"2048" in _lib.load().fabind_last_error() and bool(torch.isnan(Dg).all()) and ok()
    _, Dg, ok = _guarded((1, 4, 4), torch.float32, float("nan"))
    _, kg, _ = _guarded((1, 4, 4), torch.int32, -99)
    use, flat, B, ma = _abi_args(A)
    rc = _lib.load().fabind_conformer_cross_rmsd(x.data_ptr(), 4, x.data_ptr(), 4, 3, off.data_ptr(), A.off.data_ptr(), use.data_ptr(),
                                                 flat.data_ptr(), 1, 3, Dg.data_ptr(), kg.data_ptr(), None, None, _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"together" in _lib.load().fabind_last_error() and bool(torch.isnan(Dg).all()) and bool((kg == -99).all())
