"""The torsion-space fit on the device next to the Cartesian post-optimisation and the host restatement: 64 ligands of 20-60 heavy atoms
x 40 target poses.

Targets: every torsion of the start conformer changed by a uniform angle in +-0.5 rad (perturb_conformers, relative), a random
rotation, a shift and Gaussian noise of 0.3 A per coordinate -- an imitation of 40 sampled predictions per complex.
Reports, for `conformer.fit_conformers`: the median wall time of a synchronised call (argument checks and the plan's read-back
included), the device time of the one kernel of csrc/conformer_fit.hip alone (HIP events around the native call, several calls per
window), iterations, stop codes and RMSDs; next to it the existing `post_optimize_compound_coords_batched` (csrc/post_optim.hip, 1000
Adam steps, LAS pairs from `topology.las_pairs`) on the same inputs, one call per pose, timed the same two ways, with the largest
bond-length error each method leaves; and the float64 numpy restatement (tests/fit_refs.py) on the host for a few cases.  The two
device sides alternate inside one process.  Reported, not gated.

    python tools/conformer_fit_bench.py [--ligands 64] [--poses 40] [--reps 10] [--inner 5] [--host-cases 8] [--out profiles/conformer_fit.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
import fit_refs as F  # noqa: E402
from fabind_amd import _lib, conformer, topology  # noqa: E402
from fabind_amd.utils.post_optim_utils import post_optimize_compound_coords_batched  # noqa: E402
from conformer_bench import random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--poses", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-cases", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    mols = [random_ligand(int(rng.randint(20, 61)), rng) for _ in range(a.ligands)]
    x, bi, codes, off = R.pack(mols)
    N, B, S = int(off[-1]), a.ligands, a.poses
    xd, bid = torch.from_numpy(x).to(dev), torch.from_numpy(bi).to(dev)
    plan = conformer.rotatable_bonds(bid, torch.from_numpy(codes).to(dev), off)
    T = int(plan.quad.shape[0])
    tcount = torch.diff(plan.off).cpu().numpy()
    gen = torch.Generator().manual_seed(0)
    ang = ((torch.rand(S, T, generator=gen) - 0.5) * 1.0).to(dev)
    clean = conformer.perturb_conformers(xd, plan, n_copies=S, seed=3, angles=ang, relative=True, random_rotation=True, centre=True)
    cb = torch.repeat_interleave(torch.arange(B, device=dev), torch.diff(plan.atom_off).long())
    shift = (torch.rand(S, B, 3, generator=gen) * 40 - 20).to(dev)
    clean = clean + shift[:, cb]
    target = (clean + 0.3 * torch.randn(S, N, 3, generator=gen).to(dev)).contiguous()
    las = topology.las_pairs(bid, off).edge_index
    bonds = torch.from_numpy(bi).to(dev)

    def bond_error(c):                                                      # the largest |bond length - the start conformer's|
        d0 = (xd[bonds[0]] - xd[bonds[1]]).norm(dim=-1)
        return ((c[:, bonds[0]] - c[:, bonds[1]]).norm(dim=-1) - d0).abs().max().item()

    def rmsd_to(c, y):
        d2 = ((c - y) ** 2).sum(-1)
        per = torch.zeros(S, B, device=dev).index_add_(1, cb, d2) / torch.diff(plan.atom_off).float()
        return per.sqrt()

    def fit_call():
        return conformer.fit_conformers(xd, target, plan)

    def post_call():
        return torch.stack([post_optimize_compound_coords_batched(xd, target[s], cb, LAS_edge_index=las)[0] for s in range(S)], 0)

    fit, post = fit_call(), post_call()
    it, st = fit.iters.cpu().numpy(), fit.stop.cpu().numpy()
    lines = ["conformer_fit_bench: %d ligands (%d atoms, %d torsions: %d-%d per ligand), %d poses on %s" % (
        B, N, T, tcount.min(), tcount.max(), S, torch.cuda.get_device_name(0)),
        "fit: accepted steps median %d, largest %d; stop codes converged / cap / rejections = %d / %d / %d of %d" % (
            np.median(it), it.max(), (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), it.size),
        "median RMSD to the noise-free pose: fitted %.3f A, post-optimised %.3f A, the noisy target %.3f A, rigid fit only %.3f A" % (
            rmsd_to(fit.coords, clean).median().item(), rmsd_to(post, clean).median().item(), rmsd_to(target, clean).median().item(),
            rmsd_to(conformer.fit_conformers(xd, target, None, atom_off=off).coords, clean).median().item()),
        "largest bond-length error against the start conformer: fitted %.2e A, post-optimised %.2e A" % (bond_error(fit.coords), bond_error(post))]

    lib = _lib.load()
    out = {k: torch.empty(*s, dtype=dt, device=dev) for k, s, dt in (
        ("coords", (S, N, 3), torch.float32), ("angles", (S, T), torch.float32), ("rmsd0", (S, B), torch.float32), ("rmsd", (S, B), torch.float32),
        ("iters", (S, B), torch.int32), ("stop", (S, B), torch.int32), ("status", (B,), torch.int32))}
    max_atoms, max_tor = int(np.diff(off).max()), int(tcount.max())

    def fit_k():
        rc = lib.fabind_conformer_fit(xd.data_ptr(), target.data_ptr(), plan.atom_off.data_ptr(), B, N, S, plan.off.data_ptr(), plan.quad.data_ptr(),
                                      plan.side.data_ptr(), T, max_atoms, max_tor, 50, 1e-6, out["coords"].data_ptr(), out["angles"].data_ptr(),
                                      out["rmsd0"].data_ptr(), out["rmsd"].data_ptr(), out["iters"].data_ptr(), out["stop"].data_ptr(),
                                      out["status"].data_ptr(), None, _lib.stream())
        assert rc == 0

    for fn in (fit_call, post_call, fit_k):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(out["coords"], fit.coords)
    t_fit, t_post, k_fit, k_post = [], [], [], []
    for _ in range(3):                                                      # the two sides alternate
        t_fit.append(timed(fit_call, a.reps))
        t_post.append(timed(post_call, max(a.reps // 5, 2)))
        k_fit.append(event_time(fit_k, a.reps, a.inner))
        k_post.append(event_time(post_call, max(a.reps // 5, 2), 1))
    med = lambda v: float(np.median(v))                                     # noqa: E731
    lines += ["fit_conformers               : 1 native launch, call %.3f ms (median of 3 x %d), kernel alone %.3f ms (HIP events; windows %.3f-%.3f ms)" % (
        med(t_fit), a.reps, med(k_fit), min(k_fit), max(k_fit)),
        "%d x post_optimize (1000 steps): %d native launches, calls %.3f ms, device time of the calls %.3f ms (windows %.3f-%.3f ms)" % (
            S, S, med(t_post), med(k_post), min(k_post), max(k_post)),
        "ratio post-optimisation / fit : calls %.1fx, device time %.1fx" % (med(t_post) / med(t_fit), med(k_post) / med(k_fit))]

    xh, th = x.astype(np.float64), target.cpu().numpy()
    q, sd, toff, _ = R.batch_plan(mols)
    t0, worst = time.perf_counter(), 0.0
    for c in range(a.host_cases):
        b, s = c % B, c % S
        sl = slice(off[b], off[b + 1])
        r = F.fit_one(xh[sl], th[s, sl], q[toff[b]:toff[b + 1]], sd[toff[b]:toff[b + 1]])
        worst = max(worst, abs(r["rmsd"] - float(fit.rmsd[s, b])))
    per = (time.perf_counter() - t0) / max(a.host_cases, 1)
    lines.append("numpy restatement (float64, host): %.1f ms per (ligand, pose) over %d cases = %.1f s for all %d; its RMSD differs from the "
                 "device's by at most %.2e A" % (per * 1e3, a.host_cases, per * B * S, B * S, worst))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
