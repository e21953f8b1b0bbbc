"""Physical validity of sampled poses on the device against the float64 numpy restatement on the host: 64 ligands of 20-60 heavy atoms
x 40 poses.

Reports, for `fabind_amd.validity`: the median wall time of a synchronised `validity_plan` call and `check_poses` call (argument checks
and read-backs included), the device time of the check kernel alone (HIP events around the native call, many calls per window), the
device kernel launches of one `check_poses` call (torch.profiler), and the time the same plan and statistics take in
tests/validity_refs.py (interpreted numpy, one ligand and pose at a time -- what a host loop per pose costs, not a tuned host
implementation).  Statistics and flags of the two sides are compared before anything is timed and the largest fraction of each
derived bound is reported.

    python tools/pose_check_bench.py [--ligands 64] [--poses 40] [--reps 20] [--inner 20] [--out profiles/pose_check.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
import validity_refs as V  # noqa: E402
from fabind_amd import kernels as K, validity  # noqa: E402
from conformer_bench import launches, random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


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
    z = rng.choice([6, 6, 6, 7, 8], N)
    # poses: the conformer with 0.05-0.6 A of jitter, in the protein frame; 40 C-alpha atoms per complex
    gen = torch.Generator().manual_seed(0)
    amp = torch.linspace(0.05, 0.6, S).reshape(S, 1, 1) / 3 ** 0.5
    P = (torch.from_numpy(x)[None] + amp * torch.randn(S, N, 3, generator=gen) + torch.tensor(V.OFFSET, dtype=torch.float32)).contiguous()
    pocket, pbatch = V.make_pocket([(dict(m, x=x[off[b]:off[b + 1]]), None) for b, m in enumerate(mols)], [40] * B, seed=1)
    d = lambda t: torch.as_tensor(t).to(dev)                                # noqa: E731
    dbi, dcodes, dz, dx, dP, dpk, dpb = d(bi), d(codes), d(z), d(x), P.to(dev), d(pocket), d(pbatch)

    def new_plan():
        return validity.validity_plan(dbi, dcodes, dz, dx, off)

    plan = new_plan()

    def new_check():
        return validity.check_poses(dP, plan, dpk, dpb, ca_min=V.CA_MIN)

    res = new_check()
    t0 = time.perf_counter()
    hplans = [V.plan(m, z[off[b]:off[b + 1]], x[off[b]:off[b + 1]]) for b, m in enumerate(mols)]
    t_hplan = (time.perf_counter() - t0) * 1e3
    Ph = P.numpy()
    t0 = time.perf_counter()
    want = np.stack([np.stack([V.stats(hplans[b], Ph[s, off[b]:off[b + 1]], pocket[pbatch == b]) for s in range(S)]) for b in range(B)])
    t_hcheck = (time.perf_counter() - t0) * 1e3
    got, flags = res.stats.cpu().numpy(), res.flags.cpu().numpy()
    worst = np.zeros(9)
    for idx in np.ndindex(*want.shape):
        if np.isfinite(want[idx]):
            worst[idx[-1]] = max(worst[idx[-1]], abs(float(got[idx]) - want[idx]) / V.bound(idx[-1], want[idx]))
        else:
            assert got[idx] == want[idx], (idx, got[idx], want[idx])
    assert worst.max() <= 1.0, worst
    hp = V.batch_plan(hplans)
    assert all(np.array_equal(getattr(plan, f).cpu().numpy().view(hp[f].dtype), hp[f]) for f in ("offs", "pair_ij", "pair_kind", "group",
                                                                                                  "group_atoms", "centre", "cls"))
    lines = ["pose_check_bench: %d ligands (%d atoms; %d ratio pairs, %d planar groups, %d stereo centres), %d poses, %d C-alpha atoms "
             "on %s" % (B, N, plan.pair_ij.shape[0], plan.group.shape[0], plan.centre.shape[0], S, len(pocket), torch.cuda.get_device_name(0)),
             "valid poses: %d of %d; flag word OR: %d" % (int(res.valid.sum()), B * S, int(np.bitwise_or.reduce(flags.ravel()))),
             "largest observed fraction of the derived bound per statistic: " + ", ".join("%s %.3g" % (n, w) for n, w in zip(V.STATS, worst))]
    poff = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    poff[1:] = torch.cumsum(torch.bincount(dpb, minlength=B), 0)
    stats, fl = torch.empty(B, S, 9, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)

    def check_k():
        K.pose_check(dP, plan.atom_off, B, plan.max_atoms, plan.status, plan.cls, plan.radii, plan.offs, plan.pair_ij, plan.pair_kind,
                     plan.pair_d0, plan.group, plan.group_atoms, plan.centre, plan.centre_v0, dpk, poff,
                     (0.75, 1.25, 0.75, 1.25, 0.7, 0.25, V.CA_MIN), True, stats, fl)

    for fn in (new_plan, new_check, check_k):
        fn()
    torch.cuda.synchronize()
    t_plan, t_check, k_check = [], [], []
    for _ in range(3):
        t_plan.append(timed(new_plan, a.reps))
        t_check.append(timed(new_check, a.reps))
        k_check.append(event_time(check_k, a.reps, a.inner))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    lines += ["validity_plan : 2 native launches (count, write) of %s kernel launches in all, one read-back; call %.3f ms (median of 3 x %d)" % (
        launches(new_plan), med(t_plan), a.reps),
        "check_poses   : 1 native launch of %s kernel launches in all (argument checks included), one read-back; call %.3f ms; "
        "check kernel alone %.4f ms (HIP events; spread of the three windows %.4f-%.4f ms)" % (
            launches(new_check), med(t_check), med(k_check), min(k_check), max(k_check)),
        "host restatement (float64 numpy, one ligand and pose at a time): plan %.0f ms, statistics %.0f ms" % (t_hplan, t_hcheck)]
    lines.append("note: the ligands are random graphs embedded without ring closure, so their start conformers clash and no pose counts as valid; the figures are timings and error fractions, not chemistry")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
