"""LAS constraint pairs from the bond list, device against a host loop: 64 ligands of 20-60 atoms with ring systems on one device.

Reports, for `fabind_amd.topology.las_pairs`: device kernel launches of one call (torch.profiler), the median wall time of a
synchronised call (index glue and the one read-back included) and the device time of the two kernels of csrc/topology.hip alone
(HIP events around the native calls); and the wall time of the same work as a host loop -- the numpy restatement of
tests/topology_refs.py, ligand by ligand.  The host side is interpreted numpy / Python, not RDKit.

    python tools/las_bench.py [--ligands 64] [--reps 20] [--out profiles/las.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import topology_refs as T  # noqa: E402
from fabind_amd import kernels as K, topology  # noqa: E402
from conformer_bench import launches, timed  # noqa: E402


def kernel_time(bi, off, reps):
    """Median device time (ms) of the count pass and of the write pass alone."""
    dev = bi.device
    N, B = int(off[-1]), len(off) - 1
    aoff = torch.as_tensor(off, dtype=torch.int32).to(dev)
    nptr, nidx = topology._neighbour_lists(bi, N)
    rc = torch.zeros(N, dtype=torch.int32, device=dev)
    mr = torch.zeros(N, 8, dtype=torch.int32, device=dev)
    rp, st = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    K.las_pairs(nptr, nidx, aoff, B, rc, mr, rp, st)
    row_off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    row_off[1:] = torch.cumsum(rc, 0)
    El = int(row_off[-1])
    out = torch.empty(2, El, dtype=torch.int64, device=dev)
    passes = (lambda: K.las_pairs(nptr, nidx, aoff, B, rc, mr, rp, st), lambda: K.las_pairs(nptr, nidx, aoff, B, rc, mr, rp, st, row_off, El, out))
    res = []
    for fn in passes:
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        res.append(float(np.median(ts)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    mols = []
    for _ in range(a.ligands):
        n = int(rng.integers(20, 61))
        mols.append((n, T.random_ring_system(rng, n)))
    off = np.concatenate([[0], np.cumsum([n for n, _ in mols])]).astype(np.int64)
    bi = np.concatenate([np.asarray(b, np.int64).T + off[k] for k, (_, b) in enumerate(mols)], 1)
    bid = torch.from_numpy(bi).to(dev)
    do = lambda: topology.las_pairs(bid, off)
    got = do()
    lines = ["las_bench: %d ligands (%d atoms, %d bonds, %d non-tree bonds, %d pairs, %d ring pairs) on %s" % (
        a.ligands, off[-1], bi.shape[1], bi.shape[1] - off[-1] + a.ligands, got.edge_index.shape[1], int(got.ring_pairs.sum()),
        torch.cuda.get_device_name(0))]
    nl, tw = launches(do), timed(do, a.reps)
    tc, tf = kernel_time(bid, off, a.reps)
    lines.append("device las_pairs (incl. its index glue and the one read-back): %s kernel launches, %.3f ms" % (nl, tw))
    lines.append("device kernels alone (HIP events): count pass %.3f ms, write pass %.3f ms" % (tc, tf))
    t = time.perf_counter()
    ei, poff, rp, st = T.las_pairs(bi, off)
    th = (time.perf_counter() - t) * 1e3
    same = np.array_equal(got.edge_index.cpu().numpy(), ei) and np.array_equal(got.off.cpu().numpy(), poff) and \
        np.array_equal(got.ring_pairs.cpu().numpy(), rp)
    lines.append("host loop (numpy / Python restatement, ligand by ligand; not RDKit): %.1f ms; device == host: %s" % (th, same))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
