"""CPU: ligand symmetry contract (fabind_amd/symmetry.py, csrc/symmetry.hip) -- the reference's atom labels without RDKit, the
golden automorphism sets (tests/golden/symmetry_graphs.npz, tools/make_golden_symmetry.py) against the definition, and the
sources free of scalar-memory store instructions."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_atom_labels_hand_worked():
    from fabind_amd.symmetry import bond_code, reference_atom_labels
    # benzene: every carbon has two aromatic bonds -> 6 * 100 + 1 + 1
    ring = [[0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 0]]
    assert reference_atom_labels([6] * 6, ring, [1] * 6).tolist() == [602] * 6
    # acetone C(C)(C)=O: carbonyl O 803, carbonyl C 600 + 3 + 4 + 4, methyls 604
    lab = reference_atom_labels([6, 6, 6, 8], [[0, 0, 0], [1, 2, 3]], ["SINGLE", "SINGLE", "DOUBLE"])
    assert lab.dtype == torch.int32 and lab.tolist() == [611, 604, 604, 803]
    # acetonitrile C-C#N, an unknown bond type (code 5) and an isolated atom
    assert reference_atom_labels([6, 6, 7], [[0, 1], [1, 2]], [4, 2]).tolist() == [604, 606, 702]
    assert reference_atom_labels([6, 6, 17], [[0], [1]], ["DATIVE"]).tolist() == [605, 605, 1700]
    assert [bond_code(t) for t in ("AROMATIC", "TRIPLE", "DOUBLE", "SINGLE", "ZERO", 3)] == [1, 2, 3, 4, 5, 3]
    with pytest.raises(ValueError):
        reference_atom_labels([6, 6], [[0], [1]], [4, 4])


def _graphs():
    g = load_npz("symmetry_graphs")
    return g, [str(s) for s in g["names"]]


def test_fixture_automorphisms_preserve_labels_and_bonds():
    g, names = _graphs()
    want = {"chain_mixed": 1, "chain_equal": 2, "benzene": 12, "neopentane": 24, "cyclohexane": 12, "nitrate_salt": 8,
            "single_atom": 1, "c60": 120}
    for gi, name in enumerate(names):
        lab, e, autos = g["g%d_labels" % gi], g["g%d_bonds" % gi], g["g%d_autos" % gi]
        n = len(lab)
        adj = np.zeros((n, n), dtype=bool)
        adj[e[0], e[1]] = adj[e[1], e[0]] = True
        assert not adj.diagonal().any()
        if name in want:
            assert len(autos) == want[name], name
        assert np.array_equal(autos[0], np.arange(n)), name                       # identity first
        assert len({tuple(a) for a in autos}) == len(autos)
        assert all(tuple(autos[k]) < tuple(autos[k + 1]) for k in range(len(autos) - 1)), name      # ascending lexicographic order
        for a in autos:
            assert np.array_equal(np.sort(a), np.arange(n))                       # a permutation
            assert np.array_equal(lab[a], lab)
            assert np.array_equal(adj[np.ix_(a, a)], adj), name
    assert any(n.startswith("druglike") and 60 <= len(g["g%d_labels" % i]) <= 150 for i, n in enumerate(names))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "symmetry_graphs.npz")) < 1 << 20


def test_fixture_minima_are_consistent():
    """The float64 expectations are the minima over the fixture sets (and the identity never beats them)."""
    g, _ = _graphs()
    off = np.concatenate([[0], np.cumsum([len(g["g%d_labels" % i]) for i in g["batch_graph"]])])
    for b, gi in enumerate(g["batch_graph"][:16]):
        autos = g["g%d_autos" % gi]
        t = g["true"][off[b]:off[b + 1]].astype(np.float64)
        for s in range(g["pred"].shape[0]):
            p = g["pred"][s, off[b]:off[b + 1]].astype(np.float64)
            r = np.sqrt(((p[autos] - t) ** 2).sum(-1).mean(-1))
            assert np.isclose(r.min(), g["exp_rmsd"][s, b], rtol=1e-12, atol=0) and int(np.argmin(r)) == g["exp_arg_rmsd"][s, b]
            assert r.min() <= r[0]


def test_symmetry_api_refuses_cpu_tensors():
    from fabind_amd import symmetry
    with pytest.raises(RuntimeError, match="HIP device"):
        symmetry.ligand_automorphisms(torch.zeros(3, dtype=torch.int32), torch.tensor([[0, 1], [1, 2]]), [0, 3])


def _scalar_store_words():
    # assembled from parts so that this file itself does not name them
    s = "s" + "_"
    return [s + w for w in ("store", "buffer" + "_store", "scratch" + "_store", "atomic", "buffer" + "_atomic", "dcache" + "_wb",
                            "dcache" + "_discard")]


def test_no_source_names_a_scalar_store_instruction():
    pat = re.compile("|".join(re.escape(w) for w in _scalar_store_words()), re.I)
    hits = []
    for d in ("fabind_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(ROOT, d)):
            for f in fs:
                if f.endswith((".hip", ".h", ".cpp", ".cc", ".s", ".S", ".py")):
                    with open(os.path.join(dp, f), errors="replace") as fh:
                        if pat.search(fh.read()):
                            hits.append(os.path.join(dp, f))
    assert not hits, hits


def test_symmetry_kernels_in_the_library():
    """The entry points are exported and bound, and the built symmetry kernels contain no scalar-memory stores."""
    import shutil
    import subprocess
    import tempfile
    from fabind_amd import _lib
    lib = _lib.load()
    for nm in ("fabind_sym_automorphisms", "fabind_sym_score"):
        assert nm in _lib.SIGNATURES and hasattr(lib, nm)
    assert lib.fabind_abi_version() == 19
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    obj = os.path.join(ROOT, "fabind_amd", "csrc", "symmetry.o")
    if not (os.path.exists(objdump) and os.path.exists(obj)):
        return
    tmp = tempfile.mkdtemp()
    try:
        loc = os.path.join(tmp, "symmetry.o")
        shutil.copy(obj, loc)
        subprocess.run([objdump, "--offloading", loc], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        dis = ""
        for f in os.listdir(tmp):
            if "amdgcn" in f:
                dis += subprocess.run([objdump, "-d", os.path.join(tmp, f)], check=True, stdout=subprocess.PIPE,
                                      universal_newlines=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if dis:
        assert "sym_search_kernel" in dis and "sym_score_kernel" in dis
        assert not re.search(r"^\s+(%s)" % "|".join(_scalar_store_words()), dis, flags=re.M)
