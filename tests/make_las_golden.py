"""Writes tests/golden/las_molecules.npz (arrays only): the output of the REFERENCE's own
utils/generation_utils.py::get_LAS_distance_constraint_mask for two groups of molecules, with `Chem.GetAdjacencyMatrix` and
`Chem.GetSymmSSSR` of the name-only rdkit stub (oracle/refshim.py) given, in this process only, bodies that read from a stand-in
molecule (an adjacency matrix and a ring list).  That pins the mask arithmetic -- the 2-hop, `binarize`, the ring loop, the zero
diagonal -- to the reference's code; the ring lists themselves come from

* the hand molecules of tests/topology_refs.py: rings written out by hand there;
* the four example ligands of tests/golden/conformer_ligands.npz (6ckl, 6efk, 6g3c, 6n93): rings from the brute-force definition
  (topology_refs.brute_rings: every simple cycle, Gaussian elimination against all strictly shorter ones).  All four are within its
  reach (the script stops otherwise), so none used the restatement.

Needs the reference tree (oracle.refshim.REFERENCE_ROOT); run it from the repository root:  python tests/make_las_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import topology_refs as T  # noqa: E402
from make_distgen_golden import load_reference  # noqa: E402

LIGANDS = ("6ckl", "6efk", "6g3c", "6n93")


class StandInMol:
    def __init__(self, n, bonds, rings):
        self.adj = np.zeros((n, n), np.int32)                          # RDKit's GetAdjacencyMatrix: int32, symmetric, zero diagonal
        for a, b in bonds:
            self.adj[a, b] = self.adj[b, a] = 1
        self.rings = [tuple(int(i) for i in r) for r in rings]


def main():
    ref = load_reference()
    ref.Chem.GetAdjacencyMatrix = lambda mol: mol.adj.copy()
    ref.Chem.GetSymmSSSR = lambda mol: mol.rings
    mols = [(name, n, bonds, rings, "hand") for name, (n, bonds, rings, _) in T.hand_molecules().items()]
    lig = np.load(os.path.join(ROOT, "tests", "golden", "conformer_ligands.npz"))
    for name in LIGANDS:
        n, bonds = int(lig[name + "_z"].shape[0]), [(int(a), int(b)) for a, b in lig[name + "_bonds"]]
        rings = T.brute_rings(n, T.adjacency(n, bonds))
        if rings is None:
            raise SystemExit("%s: more simple cycles than the brute force enumerates" % name)
        mols.append((name, n, bonds, rings, "brute"))
    out = {"names": np.array([m[0] for m in mols]), "ring_source": np.array([m[4] for m in mols])}
    for name, n, bonds, rings, src in mols:
        mask = ref.get_LAS_distance_constraint_mask(StandInMol(n, bonds, rings)).numpy()
        assert mask.shape == (n, n) and set(np.unique(mask)) <= {0, 1}
        out[name + "_n"] = np.int32(n)
        out[name + "_bonds"] = np.asarray(bonds, np.int32).reshape(-1, 2)
        out[name + "_ring_flat"] = np.asarray([i for r in rings for i in r], np.int32)
        out[name + "_ring_off"] = np.cumsum([0] + [len(r) for r in rings]).astype(np.int32)
        out[name + "_mask"] = mask.astype(np.uint8)
        mine, ring_pairs, status = T.las_mask(n, bonds)
        print("%-22s %3d atoms %3d bonds %2d rings (%s): %4d pairs, %3d ring pairs, restatement == reference function: %s" % (
            name, n, len(bonds), len(rings), src, int(mask.sum()), ring_pairs, bool((mine == mask).all()) and status == 0))
    path = os.path.join(ROOT, "tests", "golden", "las_molecules.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
