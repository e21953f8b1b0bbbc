"""Pose generation from a distance map at pocket-sized shapes -- 64 ligands (20-60 atoms, ~100 pocket residues each) x 4 restarts x
5000 epochs -- three ways in one process:
  (a) the same loop written in torch on the device: one padded batch [256, n_max, 3], autograd + torch.optim.Adam, 5000 round trips
  (b) fabind_amd.utils.generation_utils.distance_optimize_compound_coords_batched (csrc/distgen.hip: one launch)
  (c) the same call in mode 2, which the kernel iterates in double
All start from the same x0; (a) and (b) use mode 0, all use the LAS mask |i - j| <= 2 and the reference's schedule.  Timing as everywhere in the
project: device events, median of `--repeats` runs after one warm-up run (min .. max).  Kernel launches are counted with
torch.profiler: per epoch for (a) (over `--prof-epochs` epochs), per call for (b).

usage: distgen_bench.py [--ligands 64] [--restarts 4] [--epochs 5000] [--repeats 3] [--out profiles/distgen.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_batch(n_lig, dev, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    ligs = []
    for _ in range(n_lig):
        n = int(torch.randint(20, 61, (1,), generator=g))
        P = int(torch.randint(90, 111, (1,), generator=g))
        step = torch.randn(n, 3, generator=g)
        coords = torch.cumsum(1.5 * step / step.norm(dim=-1, keepdim=True), 0)
        coords = coords - coords.mean(0)
        pocket = 8.0 * torch.randn(P, 3, generator=g)
        i = torch.arange(n)
        ligs.append(dict(coords=coords, pocket=pocket, y=torch.cdist(pocket, coords).clamp(max=10), D=torch.cdist(coords, coords),
                         mask=(i[:, None] - i[None, :]).abs() <= 2))
    return [{k: v.to(dev) for k, v in lg.items()} for lg in ligs]


def kernel_args(ligs, dev):
    import torch
    cb = torch.cat([torch.full((lg["coords"].shape[0],), i, device=dev) for i, lg in enumerate(ligs)])
    pb = torch.cat([torch.full((lg["pocket"].shape[0],), i, device=dev) for i, lg in enumerate(ligs)])
    las, dist, off = [], [], 0
    for lg in ligs:
        e = torch.nonzero(lg["mask"]).t()
        las.append(e + off)
        dist.append(lg["D"][e[0], e[1]])
        off += lg["coords"].shape[0]
    return dict(coords=torch.cat([lg["coords"] for lg in ligs]), y_pred=torch.cat([lg["y"].reshape(-1) for lg in ligs]),
                pocket_xyz=torch.cat([lg["pocket"] for lg in ligs]), pocket_batch=pb, compound_batch=cb, LAS_edge_index=torch.cat(las, 1),
                pair_dis_constraint=torch.cat(dist))


def torch_loop(ligs, x0, epochs, dev):
    """x0 [R, sum n, 3] -> final loss [R, L]: every (ligand, restart) as one row of a padded batch; the rows do not interact, so one
    Adam over the padded tensor is the per-ligand Adam of the reference."""
    import torch
    R, L = x0.shape[0], len(ligs)
    nm, pm = max(lg["coords"].shape[0] for lg in ligs), max(lg["pocket"].shape[0] for lg in ligs)
    z = lambda *s: torch.zeros(*s, device=dev)
    pocket, y, pair, D, las, atoms, x = z(L, pm, 3), z(L, pm, nm), z(L, pm, nm), z(L, nm, nm), z(L, nm, nm), z(L, nm, nm), z(R, L, nm, 3)
    off = 0
    for i, lg in enumerate(ligs):
        n, P = lg["coords"].shape[0], lg["pocket"].shape[0]
        pocket[i, :P], y[i, :P, :n], pair[i, :P, :n], D[i, :n, :n], las[i, :n, :n], atoms[i, :n, :n] = lg["pocket"], lg["y"], 1, lg["D"], lg["mask"].float(), 1
        x[:, i, :n] = x0[:, off:off + n]
        off += n
    rep = lambda a: a.unsqueeze(0).expand(R, *a.shape).reshape(R * L, *a.shape[1:])
    pocket, y, pair, D, las, atoms = (rep(a) for a in (pocket, y, pair, D, las, atoms))
    x = x.reshape(R * L, nm, 3).clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=0.1)
    mode = "donot_use_mm_for_euclid_dist"
    per_row = None
    for epoch in range(epochs):
        opt.zero_grad()
        inter = ((torch.cdist(pocket, x, compute_mode=mode).clamp(max=10) - y).abs() * pair).sum((1, 2))
        own = torch.cdist(x, x, compute_mode=mode)
        config = ((own - D).abs() * las).sum((1, 2)) + 2 * ((1.22 - own).relu() * atoms).sum((1, 2))
        per_row = inter if epoch < 500 else inter + 5e-3 * (epoch - 500) * config
        per_row.sum().backward()
        opt.step()
    return per_row.detach().reshape(R, L)


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1], out


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=64)
    ap.add_argument("--restarts", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prof-epochs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distgen.txt"))
    a = ap.parse_args()
    import torch
    from fabind_amd.utils.generation_utils import distance_optimize_compound_coords_batched as generate
    dev = torch.device("cuda:0")
    ligs = make_batch(a.ligands, dev)
    kw = kernel_args(ligs, dev)
    N = kw["coords"].shape[0]
    gen = torch.Generator(device=dev).manual_seed(1)
    centre = torch.stack([lg["pocket"].mean(0) for lg in ligs])[kw["compound_batch"]]
    x0 = 5 * (2 * torch.rand((a.restarts, N, 3), device=dev, generator=gen) - 1) + centre

    run_k = lambda: generate(init=x0, n_repeat=a.restarts, total_epoch=a.epochs, **kw)
    run_t = lambda: torch_loop(ligs, x0, a.epochs, dev)
    k_med, k_lo, k_hi, res = timed(run_k, a.repeats)
    d_med, d_lo, d_hi, _ = timed(lambda: generate(init=x0, n_repeat=a.restarts, total_epoch=a.epochs, mode=2, **kw), a.repeats)
    t_med, t_lo, t_hi, t_loss = timed(run_t, max(1, min(a.repeats, 2)))
    k_launch = count_kernels(lambda: generate(init=x0, n_repeat=a.restarts, total_epoch=a.prof_epochs, **kw))
    t_launch = (count_kernels(lambda: torch_loop(ligs, x0, 2 * a.prof_epochs, dev)) - count_kernels(lambda: torch_loop(ligs, x0, a.prof_epochs, dev))) / float(a.prof_epochs)
    sizes = [lg["coords"].shape[0] for lg in ligs]
    lines = ["pose generation from a distance map: %d ligands (%d-%d atoms, %d-%d residues) x %d restarts x %d epochs; %s" % (
                 a.ligands, min(sizes), max(sizes), min(lg["pocket"].shape[0] for lg in ligs), max(lg["pocket"].shape[0] for lg in ligs),
                 a.restarts, a.epochs, torch.cuda.get_device_name(0)),
             "ms per call: median of the timed runs after one warm-up run (min .. max); kernel launches from torch.profiler",
             "%-58s %12s %25s %18s" % ("path", "ms", "(min .. max)", "kernel launches"),
             "(a) %-54s %12.1f %11.1f .. %10.1f %12.1f / epoch" % ("torch loop on the device, one padded batch", t_med, t_lo, t_hi, t_launch),
             "(b) %-54s %12.2f %11.2f .. %10.2f %12d / call (host glue included: 1 is the generation kernel)" % (
                 "distance_optimize_compound_coords_batched", k_med, k_lo, k_hi, k_launch),
             "(c) %-54s %12.2f %11.2f .. %10.2f %12s" % ("the same call in mode 2 (the kernel's double forms)", d_med, d_lo, d_hi, "as (b)"),
             "(a) / (b): %.0fx; (b) is %.2f us per epoch, %.1f us per (ligand, restart, 1000 epochs)" % (
                 t_med / k_med, k_med * 1e3 / a.epochs, k_med * 1e3 / (a.ligands * a.restarts * a.epochs / 1000.0)),
             "final loss, mean over (restart, ligand): torch loop %.2f, kernel %.2f; final RMSD of the kernel: median %.3f A, best-of-%d median %.3f A" % (
                 float(t_loss.mean()), float(res.loss.mean()), float(res.rmsd.median()), a.restarts,
                 float(res.rmsd.gather(0, res.best.unsqueeze(0)).median()))]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
