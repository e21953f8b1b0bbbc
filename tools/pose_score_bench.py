"""A Vina-style energy of sampled poses against all heavy atoms of the protein on the device: 64 complexes x 40 poses of 20-60 atoms,
about 12,000 protein heavy atoms each.

Reports, for `fabind_amd.scoring.score_poses`: the median wall time of a synchronised call (argument checks and the read-back
included), the device time of the kernel alone (HIP events around the native call, many calls per window), the device kernel launches
of one call (torch.profiler), and two baselines on the same inputs that need nothing of this feature: the same energy by `torch.cdist`
plus masks over all kept protein atoms on the same device, one complex and eight poses at a time in float32, and the float64 numpy
restatement of tests/score_refs.py on the host, timed on a few (complex, pose) and scaled.  The poses that the restatement is timed on
-- the pose on which the baseline differs most from the kernel among them -- are compared with the device before anything is timed.

The proteins are ONE synthetic protein (protein-like density, 1.2 A minimum separation, hydrogens interleaved) moved rigidly to a
different place per complex, and the type words are random: the figures are timings and error fractions, not chemistry.

    python tools/pose_score_bench.py [--complexes 64] [--poses 40] [--atoms 12000] [--reps 20] [--inner 20] [--host-poses 4]
                                     [--out profiles/pose_score.txt]"""
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
import score_refs as SR  # noqa: E402
from fabind_amd import kernels as K, scoring, validity  # noqa: E402
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
    p0, pz0 = C.synthetic_protein(a.atoms, seed=1, hydrogens=0.9)
    side = float(p0.max())
    shifts = rng.uniform(-60.0, 60.0, size=(B, 3))
    pxyz = np.concatenate([(p0.astype(np.float64) + shifts[b]).astype(np.float32) for b in range(B)])
    pz = np.tile(pz0, B)
    poff = (np.arange(B + 1) * len(pz0)).astype(np.int32)
    lt, pt = SR.random_words(N, rng), SR.random_words(len(pz), rng)
    nt = rng.randint(0, 12, B).astype(np.int32)
    # poses: the conformer about a random point of the protein's cube (some inside, some at the surface), 0.05-0.6 A of jitter per pose
    P = np.zeros((S, N, 3), np.float32)
    for b in range(B):
        xb = x[off[b]:off[b + 1]].astype(np.float64)
        c = rng.uniform(-0.1 * side, 1.1 * side, size=3) + shifts[b]
        for s in range(S):
            P[s, off[b]:off[b + 1]] = xb - xb.mean(0) + c + rng.randn(len(xb), 3) * (0.05 + 0.55 * s / max(S - 1, 1)) / 3 ** 0.5
    d = lambda t: torch.as_tensor(t).to(dev)                                # noqa: E731
    dP, dlt, dpt, dnt = d(P), d(lt), d(pt), d(nt)
    grid = validity.protein_grid(d(pxyz), d(pz), poff, edge=8.0)

    def new_score():
        return scoring.score_poses(dP, off, dlt, grid, dpt, n_torsions=dnt)

    res = new_score()
    got = {k: getattr(res, k).cpu().numpy() for k in ("terms", "inter", "total", "n_pairs", "flags")}
    # ---- the baseline on the device: the same energy by torch.cdist and masks over every kept protein atom, one complex at a time
    keep = d(pz) > 1
    kxyz, kt = d(pxyz)[keep], dpt[keep].long()
    koff = np.concatenate([[0], np.cumsum([int((pz[poff[b]:poff[b + 1]] > 1).sum()) for b in range(B)])])
    radii = torch.tensor(list(scoring.RADII) + [1.2] * 6, dtype=torch.float32, device=dev)
    wts = [float(v) for v in scoring.VINA_WEIGHTS]
    lt64 = dlt.long()
    # eight poses per cdist call: with all 40 poses of a complex in one call (40 x 60 x 12,000 distances) the direct form returned whole
    # poses at distance 0 on the MI355X -- the restatement sided with the kernel on them; in chunks of eight it agrees with inter to 1e-6
    CHUNK = 8

    def cdist_score():
        out = torch.empty(B, S, device=dev)
        for b in range(B):
            a0, a1, k0, k1 = int(off[b]), int(off[b + 1]), int(koff[b]), int(koff[b + 1])
            ti, tj = lt64[a0:a1][None, :, None], kt[k0:k1][None, None, :]
            hb = (((ti & 32) != 0) & ((tj & 64) != 0)) | (((ti & 64) != 0) & ((tj & 32) != 0))
            for s0 in range(0, S, CHUNK):
                dist = torch.cdist(dP[s0:s0 + CHUNK, a0:a1], kxyz[k0:k1].expand(min(CHUNK, S - s0), -1, -1),
                                   compute_mode="donot_use_mm_for_euclid_dist")                          # [chunk, n, M]
                sd = dist - radii[ti & 15] - radii[tj & 15]
                e = wts[0] * torch.exp(-(sd / 0.5) ** 2) + wts[1] * torch.exp(-((sd - 3.0) / 2.0) ** 2) + wts[2] * torch.where(sd < 0, sd * sd, 0.0)
                e = e + wts[3] * torch.where((ti & tj & 16) != 0, (1.5 - sd).clamp(0.0, 1.0), 0.0)
                e = e + wts[4] * torch.where(hb, (-sd / 0.7).clamp(0.0, 1.0), 0.0)
                out[b, s0:s0 + CHUNK] = torch.where(dist < 8.0, e, 0.0).sum((1, 2))
        return out

    base = cdist_score().cpu().numpy()
    base_err = np.abs(base - got["inter"]) / np.maximum(np.abs(got["inter"]), 1.0)
    base_diff, base_rel = float(np.abs(base - got["inter"]).max()), float(base_err.max())
    base_worst = tuple(int(v) for v in np.unravel_index(int(np.argmax(base_err)), base_err.shape))
    # ---- the host restatement on a few (complex, pose): compared, timed, scaled
    # (the pose on which the baseline differs most from the kernel is one of them: the restatement says which of the two is off)
    picks = [(int(b), int(s)) for b, s in zip(rng.randint(0, B, a.host_poses), rng.randint(0, S, a.host_poses))] + [base_worst]
    worst, t_host = {}, 0.0
    for b, s in picks:
        t0 = time.perf_counter()
        w = SR.score(P[s, off[b]:off[b + 1]], lt[off[b]:off[b + 1]], pxyz[poff[b]:poff[b + 1]], pz[poff[b]:poff[b + 1]], pt[poff[b]:poff[b + 1]],
                     n_torsions=int(nt[b]))
        t_host += time.perf_counter() - t0
        assert int(got["n_pairs"][b, s]) == w["n_pairs"] and int(got["flags"][b, s]) == w["flags"], (b, s)
        vals = [(SR.TERMS[k], float(got["terms"][b, s, k]), w["terms"][k], w["abs_terms"][k]) for k in range(5)]
        vals += [("inter", float(got["inter"][b, s]), w["inter"], w["abs_inter"]), ("total", float(got["total"][b, s]), w["total"], w["abs_total"])]
        for name, g, v, A in vals:
            bd = SR.bound(w["n_pairs"], A, v)
            if bd > 0:
                worst[name] = max(worst.get(name, 0.0), abs(g - v) / bd)
            else:
                assert g == v, (b, s, name)
    assert max(worst.values()) <= 1.0, worst
    params = torch.tensor(wts + [0.0585], dtype=torch.float64, device=dev)
    terms, inter, total = torch.empty(B, S, 5, device=dev), torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)
    n_pairs, fl = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)
    doff, st = d(off), torch.zeros(B, dtype=torch.int32, device=dev)
    max_atoms = int(np.diff(off).max())

    def score_k():
        K.pose_score(dP, doff, B, max_atoms, st, dlt, dnt, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr,
                     grid.xyz, grid.atom_id, grid.prot_off, dpt, grid.edge, 8.0, params, terms, inter, total, n_pairs, None, fl)

    for fn in (new_score, score_k, cdist_score):
        fn()
    torch.cuda.synchronize()
    t_score, k_score, t_cdist = [], [], []
    for _ in range(3):
        t_score.append(timed(new_score, a.reps))
        k_score.append(event_time(score_k, a.reps, a.inner))
        t_cdist.append(timed(cdist_score, max(a.reps // 4, 2)))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    pairs = int(got["n_pairs"].astype(np.int64).sum())
    lines = ["pose_score_bench: %d complexes, %d protein atoms (%d kept, %d cells of 8 A), %d ligand atoms, %d poses on %s" % (
        B, len(pz), grid.xyz.shape[0], grid.cell_ptr.numel() - 1, N, S, torch.cuda.get_device_name(0)),
        "poses scored: %d of %d; %d pairs within 8 A in all (%.0f per pose); total from %.3f to %.3f" % (
            int((got["flags"] == 0).sum()), B * S, pairs, pairs / (B * S), float(np.nanmin(got["total"])), float(np.nanmax(got["total"]))),
        "%d (complex, pose) against the restatement, the one where the baseline differs most included: n_pairs and flags equal; largest observed fraction of the bound: %s" % (
            len(picks), ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))),
        "score_poses : 1 native launch of %s kernel launches in all (argument checks included), one read-back; call %.3f ms (median of 3 x %d); "
        "kernel alone %.4f ms (HIP events; spread of the three windows %.4f-%.4f ms) = %.2f ns per pair within the cutoff" % (
            launches(new_score), med(t_score), a.reps, med(k_score), min(k_score), max(k_score), med(k_score) * 1e6 / max(pairs, 1)),
        "baseline, the same energy by torch.cdist and masks over all kept protein atoms (float32, no matrix-product form; one complex and eight "
        "poses at a time): %s kernel launches, %.3f ms; largest difference from inter %.3g (%.3g of max(|inter|, 1)), at complex %d pose %d: "
        "baseline %.6g, kernel %.6g (that pose is among those held to the restatement above)" % (
            launches(cdist_score), med(t_cdist), base_diff, base_rel, base_worst[0], base_worst[1], float(base[base_worst]),
            float(got["inter"][base_worst])),
        "host restatement (float64 numpy, brute force): %.0f ms per (complex, pose) over %d of them = about %.0f s for the batch" % (
            t_host * 1e3 / len(picks), len(picks), t_host / len(picks) * B * S),
        "note: one synthetic protein moved rigidly per complex, random-graph ligands placed about random points of its cube and random "
        "type words; the figures are timings and error fractions, not chemistry"]
    lines.insert(0, "command: python tools/pose_score_bench.py " + " ".join(sys.argv[1:]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
