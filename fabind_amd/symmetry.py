"""Ligand symmetry on the GPU: label-preserving automorphisms and the symmetry-corrected RMSD over them.

FABind+ scores docking with symmetry-corrected RMSD (reference utils/training.py:273-286 -> utils/get_sym_rmsd.py: spyrmsd on the
host, one complex at a time under a 10 s alarm, plain RMSD on any failure) and trains its permutation-invariant loss on
`data.isomorphisms`, produced offline by tools/inject_isomorphism_to_data.py -> utils/isomorphism.py::isomorphic_core (RDKit +
graph-tool).  Here both run for a whole batch in csrc/symmetry.hip:

* `ligand_automorphisms`: the automorphism search (one wave per ligand, colour refinement + depth-first search with a step
  budget), returning every ligand's automorphisms in ascending lexicographic order, identity first.  graph-tool's order is
  unspecified, so the only visible difference is which minimiser wins an exact tie downstream.
* `symmetric_rmsd` / `best_automorphism_index`: the minimum over those automorphisms (one work-group per ligand and pose).

Contract: heavy atoms are nodes, the bond list is undirected and simple, every atom carries an int32 label
(`reference_atom_labels` reproduces the reference's `atomGetnum`); an automorphism a satisfies label[a[i]] == label[i] and
(i, j) bonded <=> (a[i], a[j]) bonded.  Bond types enter only through the labels, as in the reference.  Disconnected ligands
are supported (swapping identical components is an automorphism).  Kabsch superposition is not applied (spyrmsd's default)."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .utils.post_optim_utils import _neighbour_lists

BOND_TYPES = ("AROMATIC", "TRIPLE", "DOUBLE", "SINGLE")          # codes 1..4; anything else 5 (isomorphism.py:34-45)
STATUS = {0: "ok", 1: "more than cap automorphisms", 2: "step budget exhausted", 3: "more than 256 atoms"}


def bond_code(bond_type):
    """Code of one bond type as `safe_index_bond` of the reference gives it: a name (RDKit's str(BondType)) or an int code."""
    if isinstance(bond_type, str):
        return BOND_TYPES.index(bond_type) + 1 if bond_type in BOND_TYPES else 5
    return int(bond_type)


def reference_atom_labels(atomic_numbers, bond_index, bond_codes):
    """`isomorphism.py::atomGetnum` without RDKit: label = atomic number * 100 + sum of the codes of the atom's bonds
    (AROMATIC 1, TRIPLE 2, DOUBLE 3, SINGLE 4, anything else 5).  atomic_numbers [n]; bond_index [2, E], each bond ONCE;
    bond_codes [E] ints or bond-type names.  -> int32 tensor [n] on the device of `atomic_numbers` (CPU for lists)."""
    z = torch.as_tensor(atomic_numbers)
    dev = z.device
    z = z.to(torch.int64)
    e = torch.as_tensor(bond_index, dtype=torch.int64, device=dev).reshape(2, -1)
    if len(bond_codes) and isinstance(list(bond_codes)[0], str):
        bond_codes = [bond_code(t) for t in bond_codes]
    c = torch.as_tensor(bond_codes, dtype=torch.int64, device=dev).reshape(-1)
    if c.numel() != e.shape[1]:
        raise ValueError("reference_atom_labels: %d bonds but %d bond codes" % (e.shape[1], c.numel()))
    s = torch.zeros_like(z).index_add_(0, e[0], c).index_add_(0, e[1], c)
    return (z * 100 + s).to(torch.int32)


@dataclass
class Automorphisms:
    """Automorphisms of a batch of ligands, all on the device.  flat: int32 [sum_b count_b * n_b], ligand b's k-th automorphism at
    flat[off[b] + k * n_b : ... + n_b] (local atom ids, ascending lexicographic order, identity first); off: int32 [B + 1];
    count: int32 [B]; status: int32 [B] (0 ok, 1 more than cap, 2 step budget exhausted, 3 more than 256 atoms);
    atom_off: int32 [B + 1], the ligands' atom ranges."""
    flat: torch.Tensor
    off: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor
    atom_off: torch.Tensor


def _atom_off(atom_off, dev, n_atoms):
    """atom_off as int32 on `dev`, checked on the host (the kernels index with it): 1-D, starts at 0, non-decreasing, ends at N."""
    a = torch.as_tensor(atom_off).to(device=dev, dtype=torch.int32).contiguous()
    h = a.cpu().numpy()
    if a.dim() != 1 or a.numel() < 1 or h[0] != 0 or (np.diff(h) < 0).any() or int(h[-1]) != n_atoms:
        raise ValueError("atom_off must be a non-decreasing [B + 1] offset vector from 0 to %d" % n_atoms)
    return a


def ligand_automorphisms(labels, bond_index, atom_off, cap=1000, max_steps=1_000_000, on_overflow="raise"):
    """All label-preserving automorphisms of every ligand of a batch (csrc/symmetry.hip).

    labels: int [N] on the HIP device (e.g. `reference_atom_labels`); bond_index: [2, E] GLOBAL atom ids, either or both
    directions, never crossing ligands; atom_off: [B + 1] atom offsets of the ligands.  cap: automorphisms kept per ligand;
    max_steps: candidate assignments the search of one ligand may make (every search terminates).
    on_overflow: "raise" -> RuntimeError naming every ligand with status != 0; "truncate" -> such a ligand keeps what its search
    found (the identity plus the first cap - 1 others in search order for status 1; the identity alone for status 3) and reports its
    status.  A minimum over a truncated set (an RMSD, a permutation loss) is then only an upper bound on the symmetric one;
    `symmetric_rmsd` therefore falls back to plain RMSD for such ligands.
    -> Automorphisms (flat, off, count, status on the device).  Two launches of the search (count, then write): one host sync sizes
    the output."""
    if on_overflow not in ("raise", "truncate"):
        raise ValueError("on_overflow must be 'raise' or 'truncate'")
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise RuntimeError("fabind_amd: ligand_automorphisms runs on a HIP device only (no CPU fallback)")
    if int(cap) < 1 or int(max_steps) < 0 or int(cap) > 2 ** 30 or int(max_steps) > 2 ** 31 - 1:
        raise ValueError("cap must be >= 1, max_steps in [0, 2^31)")
    dev = labels.device
    lab = labels.to(torch.int32).contiguous()
    N = lab.numel()
    aoff = _atom_off(atom_off, dev, N)
    B = aoff.numel() - 1
    bi = torch.as_tensor(bond_index).to(device=dev, dtype=torch.int64).reshape(2, -1)
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= N):
        raise ValueError("bond_index holds atom ids outside [0, %d)" % N)
    nptr, nidx = _neighbour_lists(bi, N, dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    check(lib.fabind_sym_automorphisms(ptr(lab), ptr(nptr), ptr(nidx), ptr(aoff), B, int(cap), int(max_steps), None, None, None,
                                       ptr(count), ptr(status), stream()), "fabind_sym_automorphisms(count)")
    cnt_h, st_h, aoff_h = count.cpu().numpy(), status.cpu().numpy(), aoff.cpu().numpy().astype(np.int64)
    bad = np.nonzero(st_h)[0]
    if len(bad) and on_overflow == "raise":
        raise RuntimeError("ligand_automorphisms: " + "; ".join("ligand %d: status %d (%s)" % (b, st_h[b], STATUS[int(st_h[b])])
                                                                 for b in bad))
    n_b = np.diff(aoff_h)
    kept = np.minimum(cnt_h.astype(np.int64), int(cap))
    off_h = np.zeros(B + 1, dtype=np.int64)
    off_h[1:] = np.cumsum(kept * n_b)
    if off_h[-1] >= 2 ** 31:
        raise RuntimeError("ligand_automorphisms: %d output entries exceed the int32 offsets; lower cap or split the batch" % off_h[-1])
    off = torch.from_numpy(off_h.astype(np.int32)).to(dev)
    flat = torch.empty(int(off_h[-1]), dtype=torch.int32, device=dev)
    scratch = torch.empty_like(flat)
    check(lib.fabind_sym_automorphisms(ptr(lab), ptr(nptr), ptr(nidx), ptr(aoff), B, int(cap), int(max_steps), ptr(off),
                                       ptr(scratch), ptr(flat), ptr(count), ptr(status), stream()), "fabind_sym_automorphisms(write)")
    return Automorphisms(flat=flat, off=off, count=count, status=status, atom_off=aoff)


def to_isomorphism_lists(autos):
    """`data.isomorphisms` as FABind+'s loader and `best_isomorphism_index` read it (what tools/inject_isomorphism_to_data.py
    stores from graph-tool): per ligand a list of int64 numpy index arrays, one per automorphism."""
    flat, off, cnt, aoff = (t.cpu().numpy() for t in (autos.flat, autos.off, autos.count, autos.atom_off))
    out = []
    for b in range(len(cnt)):
        n = int(aoff[b + 1] - aoff[b])
        k = int(off[b + 1] - off[b]) // n if n else int(cnt[b])
        a = flat[off[b]:off[b + 1]].astype(np.int64).reshape(k, n)
        out.append([a[i] for i in range(k)])
    return out


def _score(pred, true, autos, use_cnt, atom_off, want_idx=False):
    if not (pred.is_cuda and true.is_cuda):
        raise RuntimeError("fabind_amd: symmetric scoring runs on a HIP device only (no CPU fallback)")
    dev = pred.device
    p = pred.detach().to(torch.float32)
    stacked = p.dim() == 3
    p = (p if stacked else p.unsqueeze(0)).contiguous()
    t = true.detach().to(device=dev, dtype=torch.float32).contiguous()
    S, N = p.shape[0], p.shape[1]
    if p.shape[2] != 3 or tuple(t.shape) != (N, 3):
        raise ValueError("pred must be [N, 3] or [S, N, 3] and true [N, 3]; got %s and %s" % (tuple(pred.shape), tuple(true.shape)))
    aoff = _atom_off(atom_off, dev, N)
    if not torch.equal(aoff, autos.atom_off.to(dev)):
        raise ValueError("atom_off does not match the ligands of `autos`")
    B = aoff.numel() - 1
    if S > 65535:
        raise ValueError("at most 65535 poses")
    max_atoms = int(torch.diff(aoff).max()) if B else 0
    r = torch.empty(S, B, dtype=torch.float32, device=dev)
    l1 = torch.empty_like(r)
    ar = torch.empty(S, B, dtype=torch.int32, device=dev)
    al = torch.empty_like(ar)
    idx = torch.empty(N, dtype=torch.int32, device=dev) if want_idx else None
    check(_lib.load().fabind_sym_score(ptr(p), S, N, ptr(t), ptr(aoff), ptr(autos.off), ptr(use_cnt), ptr(autos.flat), B, max_atoms,
                                       ptr(r), ptr(ar), ptr(l1), ptr(al), ptr(idx), stream()), "fabind_sym_score")
    return r, ar, l1, al, idx, stacked


def symmetric_rmsd(pred, true, compound_batch, autos, return_details=False):
    """Symmetry-corrected RMSD per complex -- the vector the reference's `--symmetric-rmsd` branch builds (training.py:273-286):
    min over the ligand's automorphisms a of sqrt(mean_i |pred[a[i]] - true[i]|^2), no centring, no superposition.
    pred [N, 3] -> rmsd [B]; pred [S, N, 3] (S stacked poses, FABind+ sampling) -> rmsd [S, B].  true [N, 3]; compound_batch [N]:
    ligand id per atom (must agree with autos.atom_off).  A ligand with status != 0 gets plain RMSD, as the reference's exception
    path does.  -> (rmsd, corrected: bool [B], True where the minimum ran over the ligand's complete automorphism set);
    with return_details also the argmin automorphism [B] / [S, B] and the Smooth-L1 minimum and its argmin."""
    cb = torch.as_tensor(compound_batch).to(pred.device)
    B = autos.atom_off.numel() - 1
    if cb.numel() != pred.shape[-2] or not torch.equal(torch.bincount(cb.long(), minlength=B)[:B].to(torch.int32),
                                                       torch.diff(autos.atom_off)):
        raise ValueError("compound_batch does not match the ligands of `autos`")
    corrected = autos.status == 0
    use = torch.where(corrected, autos.count, torch.zeros_like(autos.count)).contiguous()
    r, ar, l1, al, _, stacked = _score(pred, true, autos, use, autos.atom_off)
    if not stacked:
        r, ar, l1, al = r[0], ar[0], l1[0], al[0]
    if return_details:
        return r, corrected, ar, l1, al
    return r, corrected


def best_automorphism_index(pos_x, pos_y, autos, atom_off=None):
    """The `new_idx` of `plus.models.model.best_isomorphism_index` on the scoring kernel: per ligand the automorphism with the
    smallest mean Smooth-L1 (beta 1) between pos_x[a] and pos_y (the FIRST in the lexicographic order on a tie), as global
    atom indices int64 [N] -- pos_x[new_idx] is the permuted prediction.  Uses every automorphism `autos` holds (a truncated set
    included).  No gradient.  atom_off defaults to autos.atom_off."""
    aoff = autos.atom_off if atom_off is None else atom_off
    _, _, _, _, idx, _ = _score(pos_x, pos_y, autos, autos.count, aoff, want_idx=True)
    return idx.long()
