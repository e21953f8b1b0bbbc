"""Ligand poses from a predicted protein-ligand distance map on the GPU (reference FABind/fabind/utils/generation_utils.py:24-120,
the TankBind-style generation: Adam on the ligand coordinates against `y_pred`, the ligand's own geometry weighed in after epoch
500, repeated from random starts).

`compute_RMSD` and `distance_loss_function` are plain torch and differentiable, like the reference's.  `distance_optimize_compound_coords`
and `get_info_pred_distance` keep the reference's names, arguments and return values for ONE ligand with dense inputs;
`distance_optimize_compound_coords_batched` runs a whole batch and all restarts in one kernel launch (csrc/distgen.hip: one
work-group per (ligand, repeat), every epoch inside the kernel).  HIP device tensors only -- there is no CPU fallback.

Numerics: the objective is non-smooth and Adam moves a coordinate by ~lr = 0.1 A per step, so the iteration is chaotic: the
reference's own float32 run leaves a float64 run of the same formulas by ~1e-6 A within 20 epochs and by a few percent of the
loss after 5000.  The kernel follows the float64 iteration as closely as the reference's float32 run does (tests pin a short
horizon) and reaches the same loss / RMSD level at the full horizon."""
import ctypes
from collections import namedtuple

import torch

from .. import _lib
from .._lib import check, ptr, stream

_DIRECT = "donot_use_mm_for_euclid_dist"    # the matmul form of cdist loses the small distances (and the zero diagonal) to cancellation
MAX_ATOMS = 512           # per ligand (csrc/distgen.hip: DG_THREADS * DG_APT)
MAX_POCKET = 4096         # pocket residues per complex (DG_MAX_POCKET)

DistGenResult = namedtuple("DistGenResult", "x loss terms rmsd best x_best loss_trace rmsd_trace")
DistGenResult.__doc__ = """x [R, sum n, 3]; loss, rmsd [R, L]; terms [R, L, 2] = (interaction, configuration) of the last epoch; best [L] =
the repeat with the smallest final loss; x_best [sum n, 3] = x gathered by it; loss_trace / rmsd_trace [R, L, epochs] or None."""


def compute_RMSD(a, b):
    return torch.sqrt((((a - b) ** 2).sum(axis=-1)).mean())


def distance_loss_function(epoch, y_pred, x, protein_nodes_xyz, compound_pair_dis_constraint, LAS_distance_constraint_mask=None,
                           mode=0):
    """-> (loss, (interaction, configuration)) at 0-based `epoch`, with the reference's schedule (configuration enters after
    epoch 500 with weight 5e-3 (epoch - 500))."""
    dis = torch.cdist(protein_nodes_xyz, x, compute_mode=_DIRECT).clamp(max=10)
    r = (dis - y_pred).abs()
    if mode == 0:
        interaction = r.sum()
    elif mode == 1:
        interaction = (r ** 2).sum()
    elif mode == 2:
        interaction = ((r + 1e-5) ** 0.5).sum()
    else:
        raise NotImplementedError("mode %r" % (mode,))
    own = torch.cdist(x, x, compute_mode=_DIRECT)
    dev = (own - compound_pair_dis_constraint).abs()
    if LAS_distance_constraint_mask is not None:
        configuration = dev[LAS_distance_constraint_mask].sum() + 2 * (1.22 - own).relu().sum()
    else:
        configuration = dev.sum()
    loss = interaction if epoch < 500 else interaction + 5e-3 * (epoch - 500) * configuration
    return loss, (interaction.item(), configuration.item())


def _offsets(cnt, dtype):
    off = torch.zeros(cnt.shape[0] + 1, dtype=dtype, device=cnt.device)
    off[1:] = torch.cumsum(cnt, 0)
    return off


def _constraint_lists(pairs, dist, n_atoms):
    """CSR over atoms of a list of ordered pairs (k, j) with target distances: duplicates of an ordered pair count once (as in a
    boolean mask; should they carry different distances, the smallest is taken -- a fixed rule, not the order of a scatter); every distinct (k, j) puts (j, D) into k's list and (k, D) into j's list -- an entry weighs 1/2 in the loss and 1
    in its owner's gradient, which reproduces an arbitrary (also asymmetric) mask.  pairs int64 [2, E], dist [E] -> (ptr int32
    [n_atoms + 1], other int32 [2 E'], dist [2 E'])."""
    pairs = pairs.to(torch.int64)
    key, inv = torch.unique(pairs[0] * n_atoms + pairs[1], return_inverse=True)
    d = torch.zeros(key.shape[0], dtype=dist.dtype, device=dist.device).scatter_reduce_(0, inv, dist, "amin", include_self=False)
    k, j = torch.div(key, n_atoms, rounding_mode="floor"), key % n_atoms
    owner, other = torch.cat([k, j]), torch.cat([j, k])
    order = torch.argsort(owner, stable=True)
    ptr_ = _offsets(torch.bincount(owner, minlength=n_atoms), torch.int32)
    return ptr_, other[order].to(torch.int32).contiguous(), torch.cat([d, d])[order].contiguous()


def _all_pairs(cnt, off):
    """Every ordered pair (k, j), k == j included, of every ligand as GLOBAL atom ids [2, sum n^2]."""
    sq = cnt * cnt
    lig = torch.repeat_interleave(torch.arange(cnt.shape[0], device=cnt.device), sq)
    local = torch.arange(int(sq.sum().item()), device=cnt.device) - _offsets(sq, torch.int64)[:-1][lig]
    n = cnt[lig]
    return torch.stack([off[lig] + torch.div(local, n, rounding_mode="floor"), off[lig] + local % n])


def distance_optimize_compound_coords_batched(coords, y_pred, pocket_xyz, pocket_batch, compound_batch,
                                              reference_compound_coords=None, pair_dis_constraint=None, LAS_edge_index=None,
                                              total_epoch=5000, mode=0, n_repeat=1, init=None, generator=None, lr=0.1,
                                              config_start=500, config_rate=5e-3, return_trace=False):
    """All ligands of a batch and all `n_repeat` starts in one launch.
    coords [sum n, 3]: the true pose the RMSD is taken to (None: the RMSD is NaN).  y_pred: the model's flat distance map, per
    complex [residues, atoms] with the atom index fastest.  pocket_xyz [sum P, 3] / pocket_batch: the residues y_pred was paired
    against, sorted by complex; compound_batch: sorted ligand id per atom.
    Geometry: LAS_edge_index [2, E] GLOBAL atom ids lists the constrained ordered pairs (the excluded-volume term is then on); None
    constrains every ordered pair and drops the excluded volume.  Target distances: pair_dis_constraint (a tensor [E] aligned with
    LAS_edge_index, or a list of dense [n_l, n_l] matrices, or one dense matrix for a single ligand), else the distances of
    reference_compound_coords [sum n, 3].
    init: start coordinates [n_repeat, sum n, 3] ([sum n, 3] for one repeat); None draws 5 (2u - 1) + the mean of the complex's
    pocket with torch.rand on the device from `generator`.  -> DistGenResult."""
    if not pocket_xyz.is_cuda:
        raise RuntimeError("fabind_amd: distance-map generation runs on a HIP device only (no CPU fallback); got %s" % pocket_xyz.device)
    if mode not in (0, 1, 2):
        raise NotImplementedError("mode %r" % (mode,))
    dev = pocket_xyz.device
    R = int(n_repeat)
    cb = compound_batch.to(dev)
    N = cb.shape[0]
    cnt = torch.bincount(cb)
    L = cnt.shape[0]
    pcnt = torch.bincount(pocket_batch.to(dev), minlength=L)
    if pcnt.shape[0] != L:
        raise ValueError("pocket_batch names %d complexes, compound_batch %d" % (pcnt.shape[0], L))
    off, poff = _offsets(cnt, torch.int32), _offsets(pcnt, torch.int32)
    ysz = pcnt * cnt
    yoff = _offsets(ysz, torch.int64)
    pocket = pocket_xyz.detach().to(torch.float32).contiguous()
    y = y_pred.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()

    # constraint lists
    off64 = off.to(torch.int64)
    if LAS_edge_index is not None:
        pairs = LAS_edge_index.to(device=dev, dtype=torch.int64)
        if pairs.dim() != 2 or pairs.shape[0] != 2:
            raise ValueError("LAS_edge_index must be [2, E], got %s" % (tuple(pairs.shape),))
        if pairs.shape[1]:
            # the kernel indexes a ligand's LDS coordinates with (id - first atom of the ligand): refuse what would leave them
            inside = pairs.clamp(0, max(N - 1, 0))
            out_of_range, crossing = torch.stack([(inside != pairs).any(), (cb[inside[0]] != cb[inside[1]]).any()]).tolist()
            if out_of_range:
                raise ValueError("LAS_edge_index holds atom ids outside [0, %d)" % N)
            if crossing:
                raise ValueError("LAS_edge_index holds an edge between atoms of two different ligands")
    else:
        pairs = _all_pairs(cnt, off64[:-1])
    if pair_dis_constraint is not None and torch.is_tensor(pair_dis_constraint) and pair_dis_constraint.dim() == 1:
        dist = pair_dis_constraint.to(device=dev, dtype=torch.float32)
        if LAS_edge_index is None or dist.shape[0] != pairs.shape[1]:
            raise ValueError("a 1-D pair_dis_constraint holds one distance per column of LAS_edge_index")
    elif pair_dis_constraint is not None:
        mats = [pair_dis_constraint] if torch.is_tensor(pair_dis_constraint) else list(pair_dis_constraint)
        if len(mats) != L or any(tuple(m.shape) != (c, c) for m, c in zip(mats, cnt.tolist())):
            raise ValueError("pair_dis_constraint: one dense [n, n] matrix per ligand")
        flat = torch.cat([m.to(device=dev, dtype=torch.float32).reshape(-1) for m in mats])
        lig = cb[pairs[0]]
        dist = flat[_offsets(cnt.to(torch.int64) ** 2, torch.int64)[:-1][lig] + (pairs[0] - off64[lig]) * cnt[lig] + (pairs[1] - off64[lig])]
    elif reference_compound_coords is not None:
        ref = reference_compound_coords.detach().to(device=dev, dtype=torch.float32)
        dist = (ref[pairs[0]] - ref[pairs[1]]).norm(dim=-1)
    else:
        raise ValueError("give pair_dis_constraint or reference_compound_coords")
    cptr, cidx, cd = _constraint_lists(pairs, dist, N)

    sizes = torch.stack([cnt.max(), pcnt.max(), (cptr[off64[1:]] - cptr[off64[:-1]]).max().to(torch.int64), (pcnt * (cnt | 1)).max(),
                         ysz.sum()]).tolist()
    max_atoms, max_pocket, max_con, max_y, y_total = (int(s) for s in sizes)
    if y.shape[0] != y_total:
        raise ValueError("y_pred has %d entries, the batch pairs %d" % (y.shape[0], y_total))

    if init is None:
        u = torch.rand((R, N, 3), device=dev, dtype=torch.float32, generator=generator)
        centre = torch.zeros(L, 3, device=dev).index_add_(0, pocket_batch.to(dev), pocket) / pcnt.clamp(min=1).unsqueeze(1)
        x0 = 5 * (2 * u - 1) + centre[cb].unsqueeze(0)
    else:
        x0 = init.detach().to(device=dev, dtype=torch.float32)
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0)
        if tuple(x0.shape) != (R, N, 3):
            raise ValueError("init must be [n_repeat, n_atoms, 3] = %s, got %s" % ((R, N, 3), tuple(x0.shape)))
    x0 = x0.contiguous()
    truth = torch.zeros(N, 3, device=dev) if coords is None else coords.detach().to(device=dev, dtype=torch.float32).contiguous()

    x = torch.empty_like(x0)
    loss = torch.empty(R, L, dtype=torch.float32, device=dev)
    terms = torch.empty(R, L, 2, dtype=torch.float32, device=dev)
    rmsd = torch.empty(R, L, dtype=torch.float32, device=dev)
    tl = torch.empty(R, L, int(total_epoch), dtype=torch.float32, device=dev) if return_trace else None
    tr = torch.empty_like(tl) if return_trace else None
    rate_lr = (ctypes.c_double * 2)(float(config_rate), float(lr))          # host memory, read before the call returns
    check(_lib.load().fabind_distmap_generate(ptr(x0), ptr(truth), ptr(pocket), ptr(poff), ptr(y), ptr(yoff), ptr(off), ptr(cptr),
                                              ptr(cidx), ptr(cd.to(torch.float32)), L, R, N, max_atoms, max_pocket, max_con, max_y,
                                              1 if LAS_edge_index is not None else 0, int(mode), int(total_epoch), int(config_start),
                                              ctypes.addressof(rate_lr), ptr(x), ptr(loss), ptr(terms), ptr(rmsd), ptr(tl),
                                              ptr(tr), stream()), "fabind_distmap_generate")
    if coords is None:
        rmsd.fill_(float("nan"))
        if tr is not None:
            tr.fill_(float("nan"))
    best = torch.argmin(loss, dim=0)
    x_best = x[best[cb], torch.arange(N, device=dev)]
    return DistGenResult(x, loss, terms, rmsd, best, x_best, tl, tr)


def _dense_call(coords, y_pred, protein_nodes_xyz, compound_pair_dis_constraint, total_epoch, LAS_distance_constraint_mask, mode,
                n_repeat, init, generator):
    if not protein_nodes_xyz.is_cuda:
        raise RuntimeError("fabind_amd: distance-map generation runs on a HIP device only (no CPU fallback); got %s"
                           % protein_nodes_xyz.device)
    dev = protein_nodes_xyz.device
    n, P = coords.shape[0], protein_nodes_xyz.shape[0]
    if tuple(y_pred.shape) != (P, n):
        raise ValueError("y_pred must be [residues, atoms] = %s, got %s" % ((P, n), tuple(y_pred.shape)))
    D = compound_pair_dis_constraint.to(dev)
    las = dist = None
    if LAS_distance_constraint_mask is not None:
        las = torch.nonzero(LAS_distance_constraint_mask.to(dev).bool()).t().contiguous()
        dist = D[las[0], las[1]].to(torch.float32)
    return distance_optimize_compound_coords_batched(
        coords, y_pred, protein_nodes_xyz, torch.zeros(P, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
        pair_dis_constraint=dist if las is not None else D, LAS_edge_index=las, total_epoch=total_epoch, mode=mode, n_repeat=n_repeat,
        init=init, generator=generator, return_trace=True)


def distance_optimize_compound_coords(coords, y_pred, protein_nodes_xyz, compound_pair_dis_constraint, total_epoch=5000,
                                      loss_function=distance_loss_function, LAS_distance_constraint_mask=None, mode=0,
                                      show_progress=False, *, init=None, generator=None):
    """The reference's per-ligand entry point on dense inputs (y_pred [P, n], constraint [n, n], mask [n, n] bool):
    -> (x [n, 3], loss_list, rmsd_list), the lists holding every epoch's loss (before its step) and RMSD (after it)."""
    if loss_function is not distance_loss_function:
        raise NotImplementedError("the kernel evaluates this module's distance_loss_function only")
    r = _dense_call(coords, y_pred, protein_nodes_xyz, compound_pair_dis_constraint, total_epoch, LAS_distance_constraint_mask, mode,
                    1, init, generator)
    return r.x[0], r.loss_trace[0, 0].tolist(), r.rmsd_trace[0, 0].tolist()


def get_info_pred_distance(coords, y_pred, protein_nodes_xyz, compound_pair_dis_constraint, n_repeat=1,
                           LAS_distance_constraint_mask=None, mode=0, show_progress=False, *, total_epoch=5000, generator=None):
    """The reference's table of `n_repeat` restarts (all in one launch): a pandas.DataFrame with repeat, rmsd, loss, coords."""
    import pandas as pd
    r = _dense_call(coords, y_pred, protein_nodes_xyz, compound_pair_dis_constraint, total_epoch, LAS_distance_constraint_mask, mode,
                    n_repeat, None, generator)
    xs, rm, ls = r.x.cpu().numpy(), r.rmsd[:, 0].tolist(), r.loss[:, 0].tolist()
    return pd.DataFrame([[i, rm[i], float(ls[i]), xs[i]] for i in range(int(n_repeat))], columns=["repeat", "rmsd", "loss", "coords"])
