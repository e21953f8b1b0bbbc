"""Writes tests/golden/conformer_ligands.npz: the heavy atoms of the reference's four example ligands
(FABind_plus/inference_examples/gt_mol_files/*/*_ligand.sdf, read as plain-text V2000 by tests/conformer_refs.py: atomic symbols as
numbers, coordinates, bonds, bond codes -- arrays only), and the output of the REFERENCE's own utils/utils.py::uniform_random_rotation
for seeded numpy draws, imported with name-only stand-ins for its absent third-party packages (oracle/refshim.py).  Needs the
reference tree (oracle.refshim.REFERENCE_ROOT); run it from the repository root:  python tests/make_conformer_golden.py

uniform_random_rotation draws x2, x3, x1 in that order with np.random.rand(); re-seeding and drawing three numbers recovers them, so
every recorded rotation has known uniforms."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conformer_refs as R  # noqa: E402

NAMES = ("6ckl", "6efk", "6g3c", "6n93")
Z = {"C": 6, "N": 7, "O": 8, "F": 9, "P": 15, "S": 16, "Cl": 17, "Br": 35, "I": 53, "B": 5, "Si": 14, "Se": 34}
ROT_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def main():
    from oracle import refshim
    out = {"names": np.array(NAMES)}
    for name in NAMES:
        path = os.path.join(refshim.REFERENCE_ROOT, "FABind_plus", "inference_examples", "gt_mol_files", name, name + "_ligand.sdf")
        sym, xyz, bonds, codes = R.parse_v2000(open(path).read())
        out[name + "_z"] = np.array([Z[s] for s in sym], np.int32)
        out[name + "_xyz"] = xyz.astype(np.float64)
        out[name + "_bonds"] = bonds.astype(np.int32)
        out[name + "_codes"] = codes.astype(np.int32)
        q, _, _ = R.plan(len(sym), bonds, codes)
        print("%s: %d heavy atoms, %d bonds, %d rotatable" % (name, len(sym), len(bonds), len(q)))
    try:
        urr = refshim.load_reference("FABind_plus")["utils.utils"].uniform_random_rotation
    except Exception as e:                                             # recorded in DESIGN.md section 13 if it ever happens
        print("reference uniform_random_rotation not importable (%r): the restatement stands on the formula" % (e,))
        urr = None
    if urr is not None:
        xs, us, ys = [], [], []
        for s in ROT_SEEDS:
            x = out[NAMES[s % len(NAMES)] + "_xyz"][:12] + (s * 1.5)
            np.random.seed(s)
            y = urr(x.copy())
            np.random.seed(s)
            x2, x3, x1 = np.random.rand(3)
            xs.append(x); us.append([x1, x2, x3]); ys.append(y)
            err = np.abs(R.perturb_one(x, np.zeros((0, 4), np.int32), np.zeros((0, 8), np.uint32), [], (x1, x2, x3), centre=False) - y).max()
            print("seed %d: restatement vs reference uniform_random_rotation: %.2e" % (s, err))
        out["rot_x"], out["rot_u"], out["rot_y"] = np.asarray(xs), np.asarray(us), np.asarray(ys)
    path = os.path.join(ROOT, "tests", "golden", "conformer_ligands.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
