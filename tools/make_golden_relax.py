"""Writes tests/golden/relax_cases.npz: what the float64 and the float32-pose restatement of tests/relax_refs.py give on the committed
case list `relax_refs.CASES`, so that tests/test_gpu_relax.py compares the device with recorded numbers instead of running two hundred
Gauss-Newton iterations per case in numpy.  tests/test_relax_refs_cpu.py recomputes every number and compares.

Per case c: cases [C, 2] = (complex, target); angles0 (concatenated, angle_off [C + 1]): the float64 fit's angles rounded to float32, the
start of both restatements and of the device; sums64 / sums32 [C, 3]: the three unweighted sums at the end; E64 / E32 [C]: the
weighted totals; d32 [C]: RMSD between the two final poses; coords64 (concatenated, atom_off [C + 1]); prot0, prot1, clash0, clash1
[C]: the statistics of the two checks at the fitted pose and at the float64 result; iters64, stop64 [C].

usage (CPU): python tools/make_golden_relax.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relax_refs as X  # noqa: E402
from helpers import load_npz  # noqa: E402


def main(out):
    res = X.Results(load_npz("conformer_ligands"))
    rows, ang, xyz, s64, s32, it, st = [], [], [], [], [], [], []
    for k, s in X.CASES:
        rows.append(res.row(k, s))
        _, fit, o64 = res.run(k, s)
        _, _, o32 = res.run(k, s, np.float32)
        ang.append(fit["angles"].astype(np.float32))
        xyz.append(o64["coords"])
        s64.append(o64["energy"]); s32.append(o32["energy"])
        it.append(o64["iters"]); st.append(o64["stop"])
        print("case %2d %d %-18s E64 %.6f |E32 - E64| %.2e d32 %.2e prot %.3f -> %.3f clash %.3f -> %.3f" % (
            k, s, res.cx[k]["name"], rows[-1]["E64"], abs(rows[-1]["E32"] - rows[-1]["E64"]), rows[-1]["d32"], rows[-1]["prot0"],
            rows[-1]["prot1"], rows[-1]["clash0"], rows[-1]["clash1"]))
    col = lambda name: np.asarray([r[name] for r in rows], np.float64)
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    np.savez_compressed(out, cases=np.asarray(X.CASES, np.int64), angles0=np.concatenate(ang), angle_off=off(ang), coords64=np.concatenate(xyz),
                        atom_off=off(xyz), sums64=np.asarray(s64), sums32=np.asarray(s32), E64=col("E64"), E32=col("E32"), d32=col("d32"),
                        prot0=col("prot0"), prot1=col("prot1"), clash0=col("clash0"), clash1=col("clash1"), iters64=np.asarray(it, np.int64),
                        stop64=np.asarray(st, np.int64))
    print("wrote %s: %d cases, yardstick max |E32 - E64| = %.3e" % (out, len(rows), np.abs(col("E32") - col("E64")).max()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "relax_cases.npz"))
