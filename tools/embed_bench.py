"""Start conformers by distance geometry on the device against the float64 numpy restatement on the host: 64 ligands of 20-60 heavy
atoms x 10 conformers.  The ligands are those of the other pose benches (`conformer_bench.random_ligand`: a six-ring and a branching
tree) with the valences kept possible (`sane_ligand`: at most four neighbours, three at an atom with a DOUBLE or AROMATIC bond, one
multiple bond per atom); --raw takes the other benches' graphs as they are, most of which no conformer can satisfy (an atom with
five neighbours, a double bond at a four-neighbour atom) -- the worst case of the kernel: every try runs to the step cap.

Reports, for `fabind_amd.embed`: the median wall time of a synchronised `distance_bounds` call and `embed_conformers` call (argument
checks and read-backs included), the device time of the embedding kernel alone (HIP events around the native call), the device kernel
launches of each call (torch.profiler), the distribution of statuses, tries and steps, the largest violation left, and the time the
float64 restatement of tests/embed_refs.py takes for the bounds of every ligand and for ONE conformer of every ligand (interpreted
numpy, one ligand at a time; the figure for the whole batch is that times the number of conformers).  The bounds of the two sides are
compared bit for bit before anything is timed.  With --resources the registers, scratch, LDS and occupancy of the two kernels are read
from a compilation of csrc/embed.hip (needs hipcc).

    python tools/embed_bench.py [--ligands 64] [--confs 10] [--reps 5] [--raw] [--resources] [--out profiles/embed.txt]"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import conformer_refs as R  # noqa: E402
import embed_refs as E  # noqa: E402
from fabind_amd import build as B_, embed, kernels as K  # noqa: E402
from conformer_bench import launches, random_ligand, timed  # noqa: E402
from pose_cluster_bench import event_time  # noqa: E402


def sane_ligand(n, rng):
    """`random_ligand` with possible valences: the parent is one of the last four atoms that can take a neighbour (else any such atom)."""
    bonds, codes = [(i, (i + 1) % 6) for i in range(6)], [R.AROMATIC] * 6
    deg, cap, multi = [2] * 6, [3] * 6, [True] * 6
    for a in range(6, n):
        cand = [p for p in range(max(0, a - 4), a) if deg[p] < cap[p]] or [p for p in range(a) if deg[p] < cap[p]]
        p = cand[int(rng.randint(len(cand)))]
        dbl = bool(rng.rand() < 0.25) and not multi[p] and deg[p] < 3
        bonds.append((p, a))
        codes.append(R.DOUBLE if dbl else R.SINGLE)
        deg[p] += 1
        deg.append(1); cap.append(3 if dbl else 4); multi.append(dbl)
        if dbl:
            cap[p], multi[p] = 3, True
    return R.mol(n, bonds, codes)


def resources():
    """Per kernel of csrc/embed.hip: what the compiler reports (-Rpass-analysis=kernel-resource-usage)."""
    cmd = [B_.HIPCC] + B_.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B_.CSRC, "embed.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    out, name = [], None
    for ln in r.stdout.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = "embed_bounds_kernel" if "embed_bounds" in m.group(2) else "embed_conformers_kernel" if "embed_conformers" in m.group(2) else m.group(2)
            out.append([name])
        elif out:
            out[-1].append("%s %s" % (m.group(1).split(" [")[0], m.group(2)))
    return ["%s: %s" % (o[0], ", ".join(o[1:])) for o in out] or ["(no resource report: %s)" % r.stdout[-200:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--confs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--raw", action="store_true", help="the graphs of the other pose benches, valences not kept possible")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    mols = [(random_ligand if a.raw else sane_ligand)(int(rng.randint(20, 61)), rng) for _ in range(a.ligands)]
    _, bi, codes, off = R.pack(mols, [np.zeros((m["n"], 3), np.float32) for m in mols])
    N, B, S = int(off[-1]), a.ligands, a.confs
    z = rng.choice([6, 6, 6, 7, 8], N)
    d = lambda t: torch.as_tensor(t).to(dev)                                # noqa: E731
    dbi, dcodes, dz = d(bi), d(codes), d(z)

    def new_bounds():
        return embed.distance_bounds(dbi, dcodes, dz, off, on_overflow="skip")

    db = new_bounds()

    def new_embed():
        return embed.embed_conformers(db, n_confs=S, seed=0)

    em = new_embed()
    t0 = time.perf_counter()
    plans = [E.bounds(m, z[off[b]:off[b + 1]]) for b, m in enumerate(mols)]
    t_hb = (time.perf_counter() - t0) * 1e3
    hb, mo = db.bounds.cpu().numpy(), db.mat_off.cpu().numpy()
    assert all(np.array_equal(hb[mo[b]:mo[b + 1]].view(np.int32), p["bounds"].reshape(-1).view(np.int32)) for b, p in enumerate(plans))
    assert db.status.cpu().tolist() == [p["status"] for p in plans]
    t0 = time.perf_counter()
    href = [E.embed(p, seed=0, key=b, conf=0) for b, p in enumerate(plans)]
    t_he = (time.perf_counter() - t0) * 1e3
    st, tries, steps, viol = (t.cpu().numpy() for t in (em.status, em.tries, em.steps, em.viol))
    live = st <= 1
    lines = ["embed_bench%s: %d ligands (%d atoms, %d signed-volume terms), %d conformers each on %s"
             % (" --raw" if a.raw else "", B, N, db.quads.shape[0], S, torch.cuda.get_device_name(0)),
             "statuses of the %d (ligand, conformer) pairs: %s; plan statuses: %s" % (
                 st.size, {int(k): int((st == k).sum()) for k in np.unique(st)}, {int(k): int((db.status.cpu().numpy() == k).sum()) for k in np.unique(db.status.cpu().numpy())}),
             "tries: mean %.2f, max %d, histogram %s" % (tries[live].mean(), tries[live].max(), np.bincount(tries[live]).tolist()),
             "steps of the returned try: median %d, 90th percentile %d, max %d" % (np.median(steps[live]), np.percentile(steps[live], 90), steps[live].max()),
             "largest violation left (A): median %.3f, max %.3f" % (np.median(viol[live]), viol[live].max()),
             "host restatement, conformer 0 of every ligand: statuses %s, tries mean %.2f, steps median %d" % (
                 {int(k): sum(r["status"] == k for r in href) for k in sorted({r["status"] for r in href})},
                 np.mean([r["tries"] for r in href]), np.median([r["steps"] for r in href]))]
    coords, status = torch.empty_like(em.coords), torch.empty_like(em.status)
    tr, sp = torch.empty_like(em.tries), torch.empty_like(em.steps)
    vi, en = torch.empty_like(em.viol), torch.empty_like(em.energy)
    keys = torch.arange(B, dtype=torch.int32, device=dev)

    def embed_k():
        K.embed_conformers(db.bounds, db.mat_off, db.atom_off, B, N, S, db.status, db.quad_off, db.quads, db.quad_lo, db.quad_hi, keys, 0,
                           embed.MAX_TRIES, embed.MAX_STEPS, embed.POWER_ITERS, (embed.VIOL_TOL, embed.V_TOL, embed.W_V, embed.W_4), coords,
                           status, tr, sp, vi, en, None)

    embed_k()
    torch.cuda.synchronize()
    assert torch.equal(coords, em.coords)
    t_b, t_e, k_e = [], [], []
    for _ in range(3):
        t_b.append(timed(new_bounds, a.reps))
        t_e.append(timed(new_embed, a.reps))
        k_e.append(event_time(embed_k, a.reps, 1))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    lines += ["distance_bounds : 2 native launches (count, write) of %s kernel launches in all, two read-backs; call %.3f ms (median of 3 x %d)"
              % (launches(new_bounds), med(t_b), a.reps),
              "embed_conformers: 1 native launch of %s kernel launches in all (argument checks included), one read-back; call %.3f ms; "
              "embedding kernel alone %.3f ms (HIP events; spread of the three windows %.3f-%.3f ms) = %.1f us per conformer"
              % (launches(new_embed), med(t_e), med(k_e), min(k_e), max(k_e), 1e3 * med(k_e) / (B * S)),
              "host restatement (float64 numpy, one ligand at a time): bounds of %d ligands %.0f ms; one conformer of each %.0f ms "
              "(x %d conformers: %.1f s for the batch the device embeds in one launch)" % (B, t_hb, t_he, S, t_he * S / 1e3)]
    if a.resources:
        lines += resources()
    lines.append("note: the ligands are random graphs, not chemistry (with --raw most have impossible valences and end with status 1 after "
                 "every try has run to the step cap: the kernel's worst case); measured once on one box")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
