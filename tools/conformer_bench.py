"""Train-time ligand augmentation, device against a host loop: 64 ligands of 20-60 heavy atoms x 40 copies on one device.

Reports, for `fabind_amd.conformer.rotatable_bonds` (plan) and `perturb_conformers` (torsion noise + rotation): device kernel
launches of one call (torch.profiler) and the median wall time of a synchronised call; and the wall time of the same work as a host
numpy loop (the float64 restatement of tests/conformer_refs.py: plan per ligand, then one perturbation per ligand and copy).

    python tools/conformer_bench.py [--ligands 64] [--copies 40] [--reps 20] [--out profiles/conformer.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conformer_refs as R  # noqa: E402
from fabind_amd import conformer  # noqa: E402


def random_ligand(n, rng):
    """A drug-like heavy-atom graph: a six-ring, then a branching tree grown from recent atoms (every fourth bond DOUBLE)."""
    bonds = [(i, (i + 1) % 6) for i in range(6)]
    codes = [R.AROMATIC] * 6
    for a in range(6, n):
        bonds.append((int(rng.randint(max(0, a - 4), a)), a))
        codes.append(R.DOUBLE if rng.rand() < 0.25 else R.SINGLE)
    return R.mol(n, bonds, codes)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # noqa: BLE001
        return "n/a (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    mols = [random_ligand(int(rng.randint(20, 61)), rng) for _ in range(a.ligands)]
    x, bi, codes, off = R.pack(mols)
    xd, bid, cd = torch.from_numpy(x).to(dev), torch.from_numpy(bi).to(dev), torch.from_numpy(codes).to(dev)
    plan = conformer.rotatable_bonds(bid, cd, off)
    T = int(plan.quad.shape[0])
    do_plan = lambda: conformer.rotatable_bonds(bid, cd, off)
    do_pert = lambda: conformer.perturb_conformers(xd, plan, n_copies=a.copies, seed=1)
    for f in (do_plan, do_pert):
        f()
    lines = ["conformer_bench: %d ligands (%d atoms, %d rotatable bonds) x %d copies on %s" % (
        a.ligands, x.shape[0], T, a.copies, torch.cuda.get_device_name(0))]
    lp, lq = launches(do_plan), launches(do_pert)
    tp, tq = timed(do_plan, a.reps), timed(do_pert, a.reps)
    lines.append("device plan     (rotatable_bonds, incl. its index glue and the one read-back): %s kernel launches, %.3f ms" % (lp, tp))
    lines.append("device perturb  (perturb_conformers: %d conformers): %s kernel launches, %.3f ms" % (a.ligands * a.copies, lq, tq))
    t = time.perf_counter()
    q, s, toff, _ = R.batch_plan(mols)
    t_plan = (time.perf_counter() - t) * 1e3
    ang, uni = R.drawn_inputs(1, list(range(a.ligands)), a.copies, list(np.diff(toff)))
    t = time.perf_counter()
    ref = R.perturb(x, off, q, s, toff, ang, uni)
    t_pert = (time.perf_counter() - t) * 1e3
    got = do_pert().cpu().numpy()
    lines.append("host numpy loop (float64 restatement): plan %.1f ms, perturb %.1f ms" % (t_plan, t_pert))
    lines.append("plan + perturb: device %.3f ms, host loop %.1f ms; max |device - host float64| = %.3e A" % (
        tp + tq, t_plan + t_pert, float(np.abs(got - ref).max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
