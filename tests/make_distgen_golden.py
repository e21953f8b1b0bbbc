"""Writes tests/golden/distgen.npz: the synthetic cases of tests/distgen_refs.py run through the REFERENCE's own
utils/generation_utils.py::distance_optimize_compound_coords on the CPU (float32), with the float64 restatement's values from
the same starts where a run is too long to repeat in a test.  Needs the reference tree (oracle.refshim.REFERENCE_ROOT); run it
from the repository root:  python tests/make_distgen_golden.py

The reference draws its start with torch.rand(coords.shape) right after the caller's torch.manual_seed(s); distgen_refs.start(...)
draws the same numbers again, so every recorded run has a known x0."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import distgen_refs as R  # noqa: E402

SHORT_SIZES = [(20, 7), (70, 30), (130, 65)]
FULL_SIZES = [(40, 12), (70, 30)]
N_START = 4


def load_reference():
    from oracle import refshim
    import torch._dynamo  # noqa: F401  (torch.optim pulls it in lazily; import it before the name-only stubs exist)
    refshim._install_stubs()
    for name in ("rdkit.Chem.Draw", "rdkit.Chem.AllChem"):
        sys.modules.setdefault(name, types.ModuleType(name))
        setattr(sys.modules["rdkit.Chem"], name.rsplit(".", 1)[1], sys.modules[name])
    path = os.path.join(refshim.REFERENCE_ROOT, "FABind", "fabind", "utils", "generation_utils.py")
    spec = importlib.util.spec_from_file_location("_ref_generation_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, c, seed, epochs, mode, masked):
    t = lambda a: torch.from_numpy(c[a])
    torch.manual_seed(seed)
    x, loss, rmsd = ref.distance_optimize_compound_coords(t("coords"), t("y"), t("pocket"), t("D"), total_epoch=epochs,
                                                          LAS_distance_constraint_mask=t("mask") if masked else None, mode=mode)
    return x.detach().numpy().astype(np.float32), np.asarray(loss, np.float64), np.asarray(rmsd, np.float64)


def main():
    ref = load_reference()
    out = {}
    names = []
    for ci, (P, n) in enumerate(SHORT_SIZES):
        c = R.synthetic(P, n, seed=100 + ci, noise=0.5)
        for k, v in c.items():
            out["s%d_%s" % (ci, k)] = v
        seed = 7 + ci
        x0 = R.start(c["pocket"], n, seed)
        out["s%d_x0" % ci] = x0
        for mode, epochs in ((0, 20), (1, 20), (2, 3)):
            for masked in (1, 0):
                name = "s%d_m%d_k%d" % (ci, mode, masked)
                x, loss, rmsd = run_reference(ref, c, seed, epochs, mode, masked)
                r64 = R.restate(x0, c["y"], c["pocket"], c["D"], c["mask"] if masked else None, epochs, mode, truth=c["coords"])
                out[name + "_x"], out[name + "_loss"], out[name + "_rmsd"] = x, loss, rmsd
                print("%s: reference fp32 vs float64 restatement: x %.2e A, loss %.2e rel, rmsd %.2e" % (
                    name, np.abs(x - r64["x"]).max(), (np.abs(loss - r64["loss"]) / np.abs(r64["loss"])).max(),
                    np.abs(rmsd - r64["rmsd"]).max()), flush=True)
                names.append(name)
    out["short_cases"] = np.array(names)
    for ci, (P, n) in enumerate(FULL_SIZES):
        c = R.synthetic(P, n, seed=200 + ci)
        for k, v in c.items():
            out["f%d_%s" % (ci, k)] = v
        rec = {k: [] for k in ("x0", "ref_loss", "ref_rmsd", "ref_rmsd499", "ref_loss0", "f64_loss", "f64_rmsd", "f64_rmsd499")}
        for s in range(N_START):
            seed = 1000 + 10 * ci + s
            x0 = R.start(c["pocket"], n, seed)
            _, loss, rmsd = run_reference(ref, c, seed, 5000, 0, 1)
            r64 = R.restate(x0, c["y"], c["pocket"], c["D"], c["mask"], 5000, 0, truth=c["coords"])
            for k, v in (("x0", x0), ("ref_loss", loss[-1]), ("ref_rmsd", rmsd[-1]), ("ref_rmsd499", rmsd[499]), ("ref_loss0", loss[0]),
                         ("f64_loss", r64["loss"][-1]), ("f64_rmsd", r64["rmsd"][-1]), ("f64_rmsd499", r64["rmsd"][499])):
                rec[k].append(v)
            print("f%d start %d: loss %.4f / %.4f  rmsd %.4f / %.4f  rmsd@499 %.4f / %.4f (reference fp32 / float64)" % (
                ci, s, loss[-1], r64["loss"][-1], rmsd[-1], r64["rmsd"][-1], rmsd[499], r64["rmsd"][499]), flush=True)
        for k, v in rec.items():
            out["f%d_%s" % (ci, k)] = np.asarray(v, np.float32 if k == "x0" else np.float64)
    path = os.path.join(ROOT, "tests", "golden", "distgen.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
