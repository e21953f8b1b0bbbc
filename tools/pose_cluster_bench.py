"""Pose clustering on the device against what the scoring kernel alone can do: 64 ligands of 20-60 heavy atoms x 40 poses.

Reports, for `fabind_amd.poses`: the device kernel launches of one `cluster_poses` call (torch.profiler), the median wall time of a
synchronised `pairwise_rmsd` and `cluster_from_distances` call (argument checks included) and the device time of the two kernels of
csrc/pose_cluster.hip alone (HIP events around the native calls, many calls per window).  The baseline is the same [B, S, S] matrix
from S calls of the existing `symmetric_rmsd(poses, poses[t], ...)` -- one reference pose per launch -- timed the same two ways.  The
two sides alternate inside one process; the matrices are compared before anything is timed.

    python tools/pose_cluster_bench.py [--ligands 64] [--poses 40] [--reps 20] [--inner 20] [--out profiles/pose_cluster.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
from fabind_amd import _lib, kernels as K, poses, symmetry  # noqa: E402
from conformer_bench import launches, random_ligand, timed  # noqa: E402


def event_time(fn, reps, inner):
    """Median device time (ms) of one fn() over `reps` windows of `inner` calls each."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--poses", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    mols = [random_ligand(int(rng.randint(20, 61)), rng) for _ in range(a.ligands)]
    x, bi, codes, off = R.pack(mols)
    N, B, S = int(off[-1]), a.ligands, a.poses
    labels = symmetry.reference_atom_labels(np.full(N, 6), bi, codes).to(dev)
    A = symmetry.ligand_automorphisms(labels, torch.from_numpy(bi).to(dev), off, cap=1000, on_overflow="truncate")
    cb = torch.repeat_interleave(torch.arange(B, device=dev), torch.diff(A.atom_off).long())
    # four modes per ligand: the conformer shifted by 0, 4, 8, 12 A, every pose with 0.3 A jitter
    gen = torch.Generator().manual_seed(0)
    shift = 4.0 * (torch.arange(S) % 4).float().reshape(S, 1, 1)
    P = (torch.from_numpy(x)[None] + shift + 0.3 / 3 ** 0.5 * torch.randn(S, N, 3, generator=gen)).to(dev).contiguous()
    conf = torch.randn(S, B, generator=gen).to(dev)

    def new_d():
        return poses.pairwise_rmsd(P, cb, A)

    def base_d():
        return torch.stack([symmetry.symmetric_rmsd(P, P[t], cb, A)[0] for t in range(S)], 0).permute(2, 1, 0)

    D, D0 = new_d(), base_d()
    off_diag = ~torch.eye(S, dtype=torch.bool, device=dev)
    rel = ((D - D0).abs() / D0.clamp(min=1e-30))[:, off_diag].max().item()
    pc = poses.cluster_from_distances(D, conf)
    lines = ["pose_cluster_bench: %d ligands (%d atoms, %d automorphisms kept, %d ligands with more than one), %d poses on %s" % (
        B, N, int(A.count.sum()), int((A.count > 1).sum()), S, torch.cuda.get_device_name(0)),
        "largest relative difference of the two matrices off the diagonal: %.2e; clusters per ligand: mean %.2f" % (
            rel, pc.n_clusters.double().mean().item())]
    assert rel < 2 * (1.5 * 60 + 4) * 2.0 ** -24, rel

    # native calls alone: the arguments as the two wrappers marshal them
    use = torch.where(A.status == 0, A.count, torch.zeros_like(A.count)).contiguous()
    max_atoms = int(torch.diff(A.atom_off).max())
    lib = _lib.load()
    r, l1 = torch.empty(S, B, device=dev), torch.empty(S, B, device=dev)
    ar, al = torch.empty(S, B, dtype=torch.int32, device=dev), torch.empty(S, B, dtype=torch.int32, device=dev)

    def new_k():
        K.pose_pair_rmsd(P, A.atom_off, A.off, use, A.flat, B, max_atoms)

    def base_k():
        for t in range(S):
            lib.fabind_sym_score(P.data_ptr(), S, N, P[t].data_ptr(), A.atom_off.data_ptr(), A.off.data_ptr(), use.data_ptr(), A.flat.data_ptr(),
                                 B, max_atoms, r.data_ptr(), ar.data_ptr(), l1.data_ptr(), al.data_ptr(), None, _lib.stream())

    def clus_k():
        K.pose_cluster(D, conf, 2.0)

    for fn in (new_d, base_d, new_k, base_k, clus_k):                     # warm-up of every timed shape
        fn()
    torch.cuda.synchronize()
    t_new, t_base, k_new, k_base, k_cl = [], [], [], [], []
    for _ in range(3):                                                    # the two sides alternate
        t_new.append(timed(new_d, a.reps))
        t_base.append(timed(base_d, a.reps))
        k_new.append(event_time(new_k, a.reps, a.inner))
        k_base.append(event_time(base_k, max(a.reps // 4, 2), 2))
        k_cl.append(event_time(clus_k, a.reps, a.inner))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    lines += ["cluster_poses: %s kernel launches in all (index checks included), 2 native (pair kernel, clustering)" % launches(
        lambda: poses.cluster_poses(P, conf, cb, A)),
        "pairwise_rmsd            : 1 native launch, call %.3f ms (median of 3 x %d), pair kernel alone %.4f ms (HIP events)" % (
            med(t_new), a.reps, med(k_new)),
        "S x symmetric_rmsd       : %d native launches, calls %.3f ms, scoring kernels alone %.4f ms" % (S, med(t_base), med(k_base)),
        "cluster_from_distances   : 1 native launch, call %.3f ms, kernel alone %.4f ms" % (
            med([timed(lambda: poses.cluster_from_distances(D, conf), a.reps)]), med(k_cl)),
        "ratio baseline / pairwise: calls %.1fx, kernels %.1fx; spread of the three windows: pair kernel %.4f-%.4f ms, baseline kernels %.4f-%.4f ms" % (
            med(t_base) / med(t_new), med(k_base) / med(k_new), min(k_new), max(k_new), min(k_base), max(k_base))]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
