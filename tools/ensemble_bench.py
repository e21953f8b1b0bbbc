"""Superposed symmetric RMSD of conformers and greedy pruning on the device: 64 ligands of 20-60 heavy atoms x 64 conformers.

Reports, for `fabind_amd.ensemble`: the median wall time of a synchronised `aligned_pairwise_rmsd` and `prune_conformers` call
(argument checks and torch glue included) and the device time of the pair kernel of csrc/conformer_rmsd.hip and of the clustering
kernel alone (HIP events around the native calls, many calls per window).  Against it: the same [B, S, S] matrix from batched
`torch.linalg.svd` in float64 on the same device (Kabsch: per ligand every (automorphism, s, t) 3 x 3 matrix in one call, automorphisms
in chunks of 32) and the float64 numpy restatement of tests/ensemble_refs.py on the host (the first ligands only, scaled to the batch).
The device sides alternate inside one process; the matrices are compared before anything is timed.  With --best-of it also prints the
best-of-1 / 8 / 64 superposed symmetric RMSD of `embed.embed_conformers` to the crystal conformation of the four fixture ligands.

    python tools/ensemble_bench.py [--ligands 64] [--confs 64] [--reps 10] [--inner 10] [--host-ligands 2] [--best-of] [--out profiles/ensemble.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
import ensemble_refs as ER  # noqa: E402
from fabind_amd import embed, ensemble, kernels as K, symmetry  # noqa: E402
from conformer_bench import random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


def svd_matrix(P, A, chunk=32):
    """The same matrix by batched SVD in float64 on the device: per ligand H[k, s, t] = sum_i p_s[a_k[i]] p_t[i]^T, E = G_s + G_t -
    2 (s1 + s2 + sign(det H) s3), the minimum over k."""
    S = P.shape[0]
    off, foff = A.atom_off.tolist(), A.off.tolist()
    cnt = torch.where(A.status == 0, A.count, torch.zeros_like(A.count)).tolist()
    out = []
    for b in range(len(off) - 1):
        n = off[b + 1] - off[b]
        p = P[:, off[b]:off[b + 1]].double()
        p = p - p.mean(1, keepdim=True)
        G = (p * p).sum((1, 2))
        autos = A.flat[foff[b]:foff[b] + cnt[b] * n].reshape(cnt[b], n).long() if cnt[b] else torch.arange(n, device=P.device)[None]
        best = torch.full((S, S), float("inf"), dtype=torch.float64, device=P.device)
        for k0 in range(0, autos.shape[0], chunk):
            H = torch.einsum("ksni,tnj->kstij", p[:, autos[k0:k0 + chunk]].transpose(0, 1), p)
            sv = torch.linalg.svdvals(H)
            lam = sv[..., 0] + sv[..., 1] + torch.sign(torch.linalg.det(H)) * sv[..., 2]
            best = torch.minimum(best, (G[:, None] + G[None, :] - 2 * lam).clamp(min=0).amin(0))
        out.append(torch.sqrt(best / n).fill_diagonal_(0))
    return torch.stack(out)


def best_of(dev):
    """Best-of-1 / 8 / 64 superposed symmetric RMSD of the embedder to the crystal conformation of the four fixture ligands."""
    from helpers import load_npz
    g = load_npz("conformer_ligands")
    mols = R.fixture_molecules(g)
    x, bi, codes, off = R.pack(mols, [m["x"] for m in mols])
    z = np.concatenate([g[m["name"] + "_z"] for m in mols]).astype(np.int64)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)                     # noqa: E731
    signs = embed.chiral_signs_from_coords(t(bi), t(codes), t(z), t(x), off)
    db = embed.distance_bounds(t(bi), t(codes), t(z), off, chiral_sign=signs)
    em = embed.embed_conformers(db, n_confs=64, seed=0)
    A = symmetry.ligand_automorphisms(symmetry.reference_atom_labels(t(z), t(bi), t(codes)), t(bi), off, on_overflow="truncate")
    D = ensemble.aligned_rmsd_to(em.coords, t(x), db.atom_off, A)[:, :, 0]
    pr = ensemble.prune_conformers(ensemble.aligned_pairwise_rmsd(em.coords, db.atom_off, A), em.energy, valid=em.status == 0)
    rows = ["best-of-N superposed symmetric RMSD of embed_conformers (seed 0, stereo signs from the crystal) to the crystal conformation, A:"]
    for b, m in enumerate(mols):
        rows.append("  %s (%d atoms, %d automorphisms): best-of-1 %.3f, best-of-8 %.3f, best-of-64 %.3f; status 0 in %d of 64; kept at 0.5 A: %d"
                    % (m["name"], m["n"], int(A.count[b]), float(D[b, 0]), float(D[b, :8].min()), float(D[b].min()),
                       int((em.status[b] == 0).sum()), int(pr.n_keep[b])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--confs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-ligands", type=int, default=2)
    ap.add_argument("--best-of", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    mols = [random_ligand(int(rng.randint(20, 61)), rng) for _ in range(a.ligands)]
    x, bi, codes, off = R.pack(mols)
    N, B, S = int(off[-1]), a.ligands, a.confs
    labels = symmetry.reference_atom_labels(np.full(N, 6), bi, codes).to(dev)
    A = symmetry.ligand_automorphisms(labels, torch.from_numpy(bi).to(dev), off, cap=1000, on_overflow="truncate")
    n_b = torch.diff(A.atom_off).long()
    lig = torch.repeat_interleave(torch.arange(B, device=dev), n_b)
    # four shapes per ligand (the conformer plus 0 / 0.6 / 1.2 / 1.8 A of a fixed distortion), every conformer with 0.1 A jitter, centred
    # and turned by its own random rotation: what embed_conformers returns
    gen = torch.Generator().manual_seed(0)
    base = torch.from_numpy(x).double()
    dist = torch.randn(N, 3, generator=gen, dtype=torch.float64) / 3 ** 0.5
    P = base[None] + 0.6 * (torch.arange(S) % 4).double().reshape(S, 1, 1) * dist[None] + 0.1 / 3 ** 0.5 * torch.randn(S, N, 3, generator=gen,
                                                                                                                     dtype=torch.float64)
    q = torch.randn(S, B, 4, generator=gen, dtype=torch.float64)
    Rm = ensemble.quaternion_matrix(q / q.norm(dim=-1, keepdim=True)).to(dev)[:, lig]                      # [S, N, 3, 3]
    P = P.to(dev)
    cen = torch.zeros(S, B, 3, dtype=torch.float64, device=dev).index_add_(1, lig, P) / n_b[None, :, None]
    P = (Rm * (P - cen[:, lig])[:, :, None, :]).sum(-1).float().contiguous()
    key = torch.randn(B, S, generator=gen).to(dev)

    def new_d():
        return ensemble.aligned_pairwise_rmsd(P, A.atom_off, A)

    def base_d():
        return svd_matrix(P, A)

    D, D0 = new_d(), base_d()
    diff = (D.double() - D0).abs().max().item()
    pr = ensemble.prune_conformers(D, key)
    lines = ["ensemble_bench: %d ligands (%d atoms, %d automorphisms kept, %d ligands with more than one), %d conformers on %s" % (
        B, N, int(A.count.sum()), int((A.count > 1).sum()), S, torch.cuda.get_device_name(0)),
        "largest difference of the kernel's matrix and the float64 SVD matrix: %.2e A; kept per ligand at 0.5 A: mean %.2f" % (
            diff, pr.n_keep.double().mean().item())]
    assert diff < 1e-5, diff                                              # float32 store of distances of a few A, the root near 0
    t0 = time.perf_counter()
    hb = min(a.host_ligands, B)
    Ph = P.cpu().numpy()
    fl, fo, cn, ao = A.flat.cpu().numpy(), A.off.cpu().numpy(), A.count.cpu().numpy(), A.atom_off.cpu().numpy()
    for b in range(hb):
        n = ao[b + 1] - ao[b]
        Dh = ER.aligned_rmsd_ref(Ph[:, ao[b]:ao[b + 1]], None, fl[fo[b]:fo[b] + cn[b] * n].reshape(cn[b], n))["D"]
        assert np.abs(Dh - D[b].double().cpu().numpy()).max() < 1e-5
    t_host = (time.perf_counter() - t0) * 1e3
    use = torch.where(A.status == 0, A.count, torch.zeros_like(A.count)).contiguous()
    max_atoms = int(n_b.max())
    conf = (-key).t().contiguous()

    def new_k():
        K.conformer_pair_rmsd(P, A.atom_off, A.off, use, A.flat, B, max_atoms)

    def prune_d():
        return ensemble.prune_conformers(D, key)

    def clus_k():
        K.pose_cluster(D, conf, 0.5)

    for fn in (new_d, base_d, new_k, prune_d, clus_k):                    # warm-up of every timed shape
        fn()
    torch.cuda.synchronize()
    t_new, t_base, k_new, t_pr, k_cl = [], [], [], [], []
    for _ in range(3):                                                    # the sides alternate
        t_new.append(timed(new_d, a.reps))
        t_base.append(timed(base_d, max(a.reps // 5, 2)))
        k_new.append(event_time(new_k, a.reps, a.inner))
        t_pr.append(timed(prune_d, a.reps))
        k_cl.append(event_time(clus_k, a.reps, a.inner))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    pairs = B * S * (S - 1) // 2
    solves = int((torch.clamp(use, min=1).long()).sum()) * S * (S - 1) // 2
    lines += ["aligned_pairwise_rmsd  : 1 native launch, call %.3f ms (median of 3 x %d), pair kernel alone %.4f ms (HIP events): %d pairs, %d"
              " eigen-solves, %.1f ns per solve" % (med(t_new), a.reps, med(k_new), pairs, solves, med(k_new) * 1e6 / solves),
              "batched torch.linalg.svd: float64 on the same device, call %.1f ms (median of 3 x %d)" % (med(t_base), max(a.reps // 5, 2)),
              "numpy restatement       : %.0f ms for the first %d ligand(s) on the host = %.0f ms scaled to %d" % (t_host, hb, t_host * B / hb, B),
              "prune_conformers        : 1 native launch, call %.3f ms with its torch glue, clustering kernel alone %.4f ms" % (med(t_pr), med(k_cl)),
              "ratio svd / kernel call : %.0fx; spread of the three windows: pair kernel %.4f-%.4f ms, svd %.1f-%.1f ms" % (
                  med(t_base) / med(t_new), min(k_new), max(k_new), min(t_base), max(t_base))]
    if a.best_of:
        lines += best_of(dev)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
