"""Sampled poses against all heavy atoms of the protein on the device: 64 complexes x 40 poses, about 12,000 protein heavy atoms each.

Reports, for `fabind_amd.validity`: the median wall time of a synchronised `protein_grid` call and `check_poses_protein` call (argument
checks and read-backs included), the device time of the check kernel alone (HIP events around the native call, many calls per
window), the device kernel launches of one call of each (torch.profiler), and two baselines on the same inputs that need nothing of
this feature: the minimum ratio alone (prot_clash, no lattice) by `torch.cdist` over all protein atoms on the same device, one complex
at a time in float32, and the float64 numpy restatement of tests/contact_refs.py on the host, timed on a few (complex, pose) and scaled
(it is brute force over every protein atom: a whole batch takes about ten minutes).  The poses that the restatement is timed on
are compared with the device before anything is timed.

The proteins are ONE synthetic protein (protein-like density, 1.2 A minimum separation, hydrogens interleaved) moved rigidly to a
different place per complex: the figures are timings, not chemistry.

    python tools/protein_contact_bench.py [--complexes 64] [--poses 40] [--atoms 12000] [--reps 20] [--inner 20] [--host-poses 4]
                                          [--out profiles/protein_contacts.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
import contact_refs as C  # noqa: E402
from fabind_amd import kernels as K, validity  # noqa: E402
from conformer_bench import launches, random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complexes", type=int, default=64)
    ap.add_argument("--poses", type=int, default=40)
    ap.add_argument("--atoms", type=int, default=12000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-poses", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    B, S = a.complexes, a.poses
    mols = [random_ligand(int(rng.randint(20, 61)), rng) for _ in range(B)]
    x, bi, codes, off = R.pack(mols)
    N = int(off[-1])
    z = rng.choice([6, 6, 6, 7, 8], N)
    p0, pz0 = C.synthetic_protein(a.atoms, seed=1, hydrogens=0.9)
    side = float(p0.max())
    shifts = rng.uniform(-60.0, 60.0, size=(B, 3))
    pxyz = np.concatenate([(p0.astype(np.float64) + shifts[b]).astype(np.float32) for b in range(B)])
    pz = np.tile(pz0, B)
    poff = (np.arange(B + 1) * len(pz0)).astype(np.int32)
    # poses: the conformer about a random point of the protein's cube (some inside, some at the surface), 0.05-0.6 A of jitter per pose
    P = np.zeros((S, N, 3), np.float32)
    for b in range(B):
        xb = x[off[b]:off[b + 1]].astype(np.float64)
        c = rng.uniform(-0.1 * side, 1.1 * side, size=3) + shifts[b]
        for s in range(S):
            P[s, off[b]:off[b + 1]] = xb - xb.mean(0) + c + rng.randn(len(xb), 3) * (0.05 + 0.55 * s / max(S - 1, 1)) / 3 ** 0.5
    d = lambda t: torch.as_tensor(t).to(dev)                                # noqa: E731
    dP, dpx, dpz = d(P), d(pxyz), d(pz)
    plan = validity.validity_plan(d(bi), d(codes), d(z), d(x), off)

    def new_grid():
        return validity.protein_grid(dpx, dpz, poff)

    grid = new_grid()

    def new_check():
        return validity.check_poses_protein(dP, plan, grid)

    res = new_check()
    got = {k: getattr(res, k).cpu().numpy() for k in ("stats", "counts", "pair", "flags")}
    # ---- the host restatement on a few (complex, pose): compared, timed, scaled
    r_lig = C.bondi(z)
    picks = [(int(b), int(s)) for b, s in zip(rng.randint(0, B, a.host_poses), rng.randint(0, S, a.host_poses))]
    worst, t_host = np.zeros(3), 0.0
    for b, s in picks:
        t0 = time.perf_counter()
        w = C.contacts(P[s, off[b]:off[b + 1]], r_lig[off[b]:off[b + 1]], pxyz[poff[b]:poff[b + 1]], pz[poff[b]:poff[b + 1]])
        t_host += time.perf_counter() - t0
        assert got["counts"][b, s].tolist() == w["counts"].tolist() and got["pair"][b, s].tolist() == w["pair"].tolist(), (b, s)
        assert int(got["flags"][b, s]) == w["flags"], (b, s)
        for col in range(3):
            if np.isfinite(w["stats"][col]) and w["stats"][col] != 0:
                worst[col] = max(worst[col], abs(float(got["stats"][b, s, col]) - w["stats"][col]) / C.bound(col, w["stats"][col]))
            else:
                assert got["stats"][b, s, col] == w["stats"][col], (b, s, col)
    assert worst.max() <= 1.0, worst
    t0 = time.perf_counter()
    hg = C.grid(pxyz[:poff[1]], pz[:poff[1]])
    t_hgrid = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(grid.atom_id[:grid.atom_off[1]].cpu().numpy(), hg["atom_id"])
    # ---- the baseline on the device: prot_clash alone by torch.cdist over every kept protein atom, one complex at a time
    keep = dpz > 1
    kxyz, kr = dpx[keep], d(C.bondi(pz))[keep]
    koff = np.concatenate([[0], np.cumsum([int((pz[poff[b]:poff[b + 1]] > 1).sum()) for b in range(B)])])
    rl = plan.radii

    def cdist_clash():
        out = torch.empty(B, S, device=dev)
        for b in range(B):
            a0, a1, k0, k1 = int(off[b]), int(off[b + 1]), int(koff[b]), int(koff[b + 1])
            dist = torch.cdist(dP[:, a0:a1], kxyz[k0:k1].expand(S, -1, -1), compute_mode="donot_use_mm_for_euclid_dist")      # [S, n, M]
            ratio = torch.where(dist < 5.0, dist / (rl[a0:a1][None, :, None] + kr[None, None, k0:k1]), torch.full_like(dist, float("inf")))
            out[b] = ratio.amin((1, 2))
        return out

    base = cdist_clash().cpu().numpy()
    fin = np.isfinite(got["stats"][..., 0])
    both = fin & np.isfinite(base)
    base_same = float((np.isfinite(base) == fin).mean())              # (reported, not asserted: the baseline is not the code under test)
    base_diff = float(np.abs(base[both] - got["stats"][..., 0][both]).max()) if both.any() else 0.0
    stats, counts = torch.empty(B, S, 3, device=dev), torch.empty(B, S, 3, dtype=torch.int32, device=dev)
    pair, fl = torch.empty(B, S, 2, dtype=torch.int32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)

    def check_k():
        K.pose_protein_check(dP, plan.atom_off, B, plan.max_atoms, plan.status, plan.radii, grid.status, grid.origin, grid.dims, grid.cell_off,
                             grid.atom_off, grid.cell_ptr, grid.xyz, grid.radii, grid.atom_id, grid.edge, (5.0, 0.75, 0.075, 0.8, 0.5),
                             grid.max_radius, stats, counts, pair, fl)

    for fn in (new_grid, new_check, check_k, cdist_clash):
        fn()
    torch.cuda.synchronize()
    t_grid, t_check, k_check, t_cdist = [], [], [], []
    for _ in range(3):
        t_grid.append(timed(new_grid, a.reps))
        t_check.append(timed(new_check, a.reps))
        k_check.append(event_time(check_k, a.reps, a.inner))
        t_cdist.append(timed(cdist_clash, max(a.reps // 4, 2)))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    flags = got["flags"]
    lines = ["protein_contact_bench: %d complexes, %d protein atoms (%d kept, %d cells), %d ligand atoms, %d poses on %s" % (
        B, len(pz), grid.xyz.shape[0], grid.cell_ptr.numel() - 1, N, S, torch.cuda.get_device_name(0)),
        "poses ok: %d of %d; PROTEIN_CLASH %d, PROTEIN_OVERLAP %d; pairs within the cutoff for %d poses" % (
            int(res.ok.sum()), B * S, int((flags & 1).astype(bool).sum()), int((flags & 2).astype(bool).sum()), int(fin.sum())),
        "%d (complex, pose) against the restatement: counts, pairs and flags equal; largest observed fraction of the bound: "
        "prot_clash %.3g, prot_dist %.3g, overlap %.3g" % (len(picks), *worst),
        "protein_grid        : 2 native calls (count, write) of %s kernel launches in all, one read-back; call %.3f ms (median of 3 x %d)" % (
            launches(new_grid), med(t_grid), a.reps),
        "check_poses_protein : 1 native launch of %s kernel launches in all (argument checks included), one read-back; call %.3f ms; "
        "check kernel alone %.4f ms (HIP events; spread of the three windows %.4f-%.4f ms)" % (
            launches(new_check), med(t_check), med(k_check), min(k_check), max(k_check)),
        "baseline, prot_clash alone by torch.cdist over all kept protein atoms (float32 differences, no matrix-product form; one complex at a "
        "time): %s kernel launches, %.3f ms; it agrees with prot_clash on which poses have a pair for %.1f %% of the poses, largest difference %.2g" % (
            launches(cdist_clash), med(t_cdist), 100.0 * base_same, base_diff),
        "host restatement (float64 numpy, brute force): %.0f ms per (complex, pose) over %d of them = about %.0f s for the batch; the cell "
        "list of one protein %.0f ms" % (t_host * 1e3 / len(picks), len(picks), t_host / len(picks) * B * S, t_hgrid),
        "note: one synthetic protein moved rigidly per complex and random-graph ligands placed about random points of its cube; the "
        "figures are timings and error fractions, not chemistry"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
