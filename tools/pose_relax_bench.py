"""Sampled poses relaxed out of protein and internal clashes on the device: 64 complexes x 40 poses, about 12,000 protein heavy atoms each.

The ligands and the protein are those of tools/protein_contact_bench.py (random drug-like graphs; ONE synthetic protein moved rigidly per
complex), with a pocket carved round each ligand's reference pose (every protein heavy atom with d / (r_i + r_p) < 0.95 to it removed)
and targets perturbed as in the host experiment of DESIGN.md section 19: every torsion changed by a uniform angle in +-0.3 rad, a
rotation vector of 0.1 sigma rad, a shift of 0.5 A sigma.

Reports, for `fabind_amd.relax.relax_poses` started from `fit_conformers`' angles: the median wall time of a synchronised call (argument
checks and the read-back included), the device time of the kernel alone (HIP events around the native call, several calls per window),
iterations and stop codes, the share of PROTEIN_CLASH and CLASH poses and the mean volume overlap before and after; for scale, the
time of `fit_conformers` on the same batch and of the float64 numpy restatement of tests/relax_refs.py on the host, timed on a few
(complex, pose) against the protein atoms within 14 A of the target and scaled.  The figures are timings, not chemistry.

    python tools/pose_relax_bench.py [--complexes 64] [--poses 40] [--atoms 12000] [--reps 5] [--inner 3] [--host-cases 4]
                                     [--out profiles/pose_relax.txt]"""
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
import relax_refs as X  # noqa: E402
import validity_refs as V  # noqa: E402
from fabind_amd import conformer, kernels as K, relax, validity  # noqa: E402
from conformer_bench import random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complexes", type=int, default=64)
    ap.add_argument("--poses", type=int, default=40)
    ap.add_argument("--atoms", type=int, default=12000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-cases", type=int, default=4)
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
    quad, sd, toff, _ = R.batch_plan(mols)
    rl = V.BONDI
    r_lig = np.asarray([rl.get(int(v), 2.0) for v in z], np.float32)
    prots, Y = [], np.zeros((S, N, 3), np.float32)
    for b in range(B):
        sl = slice(off[b], off[b + 1])
        xb = x[sl].astype(np.float64)
        placed = (xb - xb.mean(0) + rng.uniform(0.25 * side, 0.75 * side, size=3) + shifts[b]).astype(np.float32)
        pxyz, pz = X.carve((p0.astype(np.float64) + shifts[b]).astype(np.float32), pz0, placed, r_lig[sl])
        prots.append((pxyz, pz))
        c = dict(mol=dict(mols[b], quad=quad[toff[b]:toff[b + 1]], side=sd[toff[b]:toff[b + 1]]), placed=placed)
        for s in range(S):
            Y[s, sl] = X.make_target(c, 1000 * b + s)
    poff = np.concatenate([[0], np.cumsum([len(p[1]) for p in prots])]).astype(np.int32)
    d = lambda t: torch.as_tensor(t).to(dev)                                # noqa: E731
    xd, yd = d(x), d(Y)
    tp = conformer.rotatable_bonds(d(bi), d(codes), off)
    vp = validity.validity_plan(d(bi), d(codes), d(z), xd, off)
    grid = validity.protein_grid(d(np.concatenate([p[0] for p in prots])), d(np.concatenate([p[1] for p in prots])), poff)

    def fit_call():
        return conformer.fit_conformers(xd, yd, tp)

    fit = fit_call()

    def relax_call():
        return relax.relax_poses(xd, yd, tp, vp, grid, angles0=fit.angles)

    out = relax_call()
    T = int(tp.quad.shape[0])
    bufs = {k: torch.empty(*s, dtype=dt, device=dev) for k, s, dt in (
        ("coords", (S, N, 3), torch.float32), ("angles", (S, T), torch.float32), ("energy0", (S, B, 3), torch.float64),
        ("energy", (S, B, 3), torch.float64), ("iters", (S, B), torch.int32), ("stop", (S, B), torch.int32), ("status", (B,), torch.int32))}
    tcount = torch.diff(tp.off).cpu().numpy()
    reach = 0.8 * (float(vp.radii.max()) + grid.max_radius)

    def relax_k():
        K.pose_relax(xd, yd, fit.angles, tp.atom_off, B, tp.off, tp.quad, tp.side, T, int(np.diff(off).max()), int(tcount.max()), vp.status, vp.cls,
                     vp.radii, grid.status, grid.origin, grid.dims, grid.cell_off, grid.atom_off, grid.cell_ptr, grid.xyz, grid.radii, grid.edge,
                     reach, (1.0, 100.0, 100.0, 0.80, 0.75), 100, 1e-6, bufs["coords"], bufs["angles"], bufs["energy0"], bufs["energy"],
                     bufs["iters"], bufs["stop"], bufs["status"], None)

    for fn in (fit_call, relax_call, relax_k):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(bufs["coords"], out.coords) and torch.equal(bufs["energy"], out.energy)
    t_fit, t_relax, k_relax = [], [], []
    for _ in range(3):
        t_fit.append(timed(fit_call, a.reps))
        t_relax.append(timed(relax_call, a.reps))
        k_relax.append(event_time(relax_k, a.reps, a.inner))
    med = lambda v: float(np.median(v))                                     # noqa: E731
    it, st = out.iters.cpu().numpy(), out.stop.cpu().numpy()

    def shares(poses):
        pc = validity.check_poses_protein(poses, vp, grid)
        own = validity.check_poses(poses, vp)
        return (float((pc.flags & validity.PROTEIN_CLASH != 0).float().mean()), float((own.flags & validity.CLASH != 0).float().mean()),
                float(pc.stats[:, :, 2].mean()))

    at_target, at_fit, at_end = shares(yd), shares(fit.coords), shares(out.coords)
    cb = torch.repeat_interleave(torch.arange(B, device=dev), torch.diff(tp.atom_off).long())
    rm = (torch.zeros(S, B, device=dev).index_add_(1, cb, ((out.coords - yd) ** 2).sum(-1)) / torch.diff(tp.atom_off).float()).sqrt()
    e0 = (out.energy0 * torch.tensor([1.0, 100.0, 100.0], dtype=torch.float64, device=dev)).sum(-1)
    e1 = (out.energy * torch.tensor([1.0, 100.0, 100.0], dtype=torch.float64, device=dev)).sum(-1)
    lines = ["pose_relax_bench: %d complexes, %d protein atoms (%d kept, %d cells), %d ligand atoms (%d torsions: %d-%d per ligand), %d poses on %s" % (
        B, int(poff[-1]), grid.xyz.shape[0], grid.cell_ptr.numel() - 1, N, T, tcount.min(), tcount.max(), S, torch.cuda.get_device_name(0)),
        "relax_poses   : 1 native launch, one read-back; call %.3f ms (median of 3 x %d); kernel alone %.3f ms (HIP events; windows %.3f-%.3f ms)" % (
            med(t_relax), a.reps, med(k_relax), min(k_relax), max(k_relax)),
        "fit_conformers on the same batch: call %.3f ms; relaxation / fit = %.1fx" % (med(t_fit), med(t_relax) / med(t_fit)),
        "accepted steps: median %d, largest %d; stop codes converged / cap / rejections / non-finite = %d / %d / %d / %d of %d" % (
            np.median(it), it.max(), (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), (st == 3).sum(), it.size),
        "weighted E: median %.3f at the start, %.3f at the end; median RMSD of the relaxed pose to its target %.3f A" % (
            e0.median().item(), e1.median().item(), rm.median().item()),
        "share of poses flagged PROTEIN_CLASH / CLASH, mean volume overlap: targets %.3f / %.3f, %.4f; fitted %.3f / %.3f, %.4f; "
        "relaxed %.3f / %.3f, %.4f" % (at_target + at_fit + at_end)]
    # ---- the host restatement on a few (complex, pose): the protein atoms within 14 A of the target, brute force
    a0 = fit.angles.cpu().numpy()
    dev_e = out.energy.cpu().numpy()
    t_host, worst = 0.0, 0.0
    for c in range(a.host_cases):
        b, s = (7 * c) % B, (11 * c) % S
        sl = slice(off[b], off[b + 1])
        kx, kr, _ = C.kept(*prots[b])
        nearby = np.sqrt(C._d2(Y[s, sl], kx)).min(0) < 14.0
        m = mols[b]
        vpl = V.plan(m, z[sl], x[sl])
        t0 = time.perf_counter()
        o = X.relax_one(x[sl], Y[s, sl], quad[toff[b]:toff[b + 1]], sd[toff[b]:toff[b + 1]], vpl["cls"], vpl["radii"], kx[nearby], kr[nearby],
                        angles0=a0[s, toff[b]:toff[b + 1]])
        t_host += time.perf_counter() - t0
        worst = max(worst, abs(X.total(o["energy"]) - X.total(dev_e[s, b])) / max(X.total(o["energy"]), 1e-12))
    per = t_host / max(a.host_cases, 1)
    lines.append("numpy restatement (float64, host): %.0f ms per (complex, pose) over %d cases = about %.0f s for all %d; its final E differs "
                 "from the device's by at most %.2e relative" % (per * 1e3, a.host_cases, per * B * S, B * S, worst))
    lines.append("note: one synthetic protein moved rigidly per complex, random-graph ligands with embedded (not minimised) conformers; the "
                 "figures are timings and counts, not chemistry")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
