"""Times the ligand symmetry kernels (csrc/symmetry.hip): automorphism search (count + write launches) and scoring over
automorphisms for 64 drug-like ligands x 10 poses, and -- where networkx is installed -- the host search it replaces
(GraphMatcher per ligand, the stand-in for graph-tool's subgraph_isomorphism) on the same graphs.

usage: python tools/symmetry_bench.py [--reps R]       prints one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from fabind_amd.symmetry import ligand_automorphisms, symmetric_rmsd
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "symmetry_graphs.npz")))
    names = [str(s) for s in g["names"]]
    drug = [i for i, n in enumerate(names) if n.startswith("druglike")]
    ids = [drug[b % len(drug)] for b in range(64)]
    dev = torch.device("cuda:0")
    labs, bonds, off = [], [], [0]
    for gi in ids:
        labs.append(g["g%d_labels" % gi])
        bonds.append(g["g%d_bonds" % gi].astype(np.int64) + off[-1])
        off.append(off[-1] + len(labs[-1]))
    lab = torch.from_numpy(np.concatenate(labs)).to(dev)
    bi = torch.from_numpy(np.concatenate(bonds, 1)).to(dev)
    aoff = torch.tensor(off, dtype=torch.int32, device=dev)
    cb = torch.repeat_interleave(torch.arange(64, device=dev), torch.diff(aoff).long())
    N = int(off[-1])
    gen = torch.Generator(device="cpu").manual_seed(0)
    true = (3 * torch.randn(N, 3, generator=gen)).to(dev)
    pred = (true[None] + 0.8 * torch.randn(10, N, 3, generator=gen).to(dev)).contiguous()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3
    A = ligand_automorphisms(lab, bi, aoff, cap=4096)
    res = dict(ligands=64, poses=10, atoms=N, automorphisms=int(A.count.sum()),
               search_ms=timed(lambda: ligand_automorphisms(lab, bi, aoff, cap=4096)),
               score_ms=timed(lambda: symmetric_rmsd(pred, true, cb, A)))
    try:
        from make_golden_symmetry import automorphisms_networkx
        t0 = time.perf_counter()
        for gi in ids:
            automorphisms_networkx(g["g%d_labels" % gi], g["g%d_bonds" % gi])
        res["networkx_search_ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        res["networkx_search_ms"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
