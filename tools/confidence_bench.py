"""FABind+ confidence step -- pose statistics, ranking loss (+ BCE) and its backward to the scores -- for S copies of one complex, two ways
in one process:
  (a) the reference's own formulation (FABind_plus/fabind/utils/training_confidence.py:41-80) with torch device ops: scatter-mean RMSD,
      argsort, the python double loop over the S(S-1)/2 pairs, BCEWithLogits, autograd backward.  The reference additionally reads one
      python float back per pair (`ranking_accuracy_list.append(float(...))`, :65); that read-back is left out here, in (a)'s favour.
  (b) ops.pose_stats + ops.rank_loss (csrc/ranking.hip) and the backward multiply.
Timing as everywhere in the project: device events around `--steps` steps after warm-up, median of five repeats (min .. max = the
spread).  Launch counts per step come from `rocprofv3 --kernel-trace --stats` runs of this file in a fresh process (`--child`), as the
difference between a run of 3 steps and a run of 1.

usage: confidence_bench.py [--steps 10] [--warmup 3] [--copies 8 40] [--no-prof] [--out profiles/confidence_loss.txt]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = {"a": "torch double loop (reference formulation)", "b": "ops.pose_stats + ops.rank_loss"}
ATOMS = 30                       # ligand atoms per copy


def make_inputs(S, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(S)
    truth = (torch.rand(ATOMS, 3, device=dev, generator=g) * 40 - 20).repeat(S, 1)
    spread = torch.linspace(0.3, 4.0, S, device=dev)[torch.randperm(S, device=dev, generator=g)].repeat_interleave(ATOMS)
    pred = truth + torch.randn(S * ATOMS, 3, device=dev, generator=g) * spread[:, None]
    cb = torch.arange(S, device=dev).repeat_interleave(ATOMS)
    scores = torch.randn(S, device=dev, generator=g).requires_grad_(True)
    return pred, truth, cb, scores


def make_step(path, S, dev):
    """-> (step function returning (loss, d loss / d scores), scores)."""
    import torch
    import torch.nn.functional as F
    from fabind_amd import ops
    pred, truth, cb, scores = make_inputs(S, dev)
    if path == "a":
        def step():
            scores.grad = None
            sd = ((pred.detach() - truth) ** 2).sum(dim=-1)
            cnt = torch.zeros(S, device=dev).index_add_(0, cb, torch.ones_like(sd))
            rmsd = (torch.zeros(S, device=dev).index_add_(0, cb, sd) / cnt).sqrt().detach()       # scatter_mean(...).sqrt()
            order = rmsd.argsort()
            ss = scores[order]
            ranking_loss = 0.
            for i in range(S):
                for j in range(i):
                    ranking_loss += - F.logsigmoid(ss[j] - ss[i])
            ranking_loss = ranking_loss / (S * (S - 1) / 2)
            loss = ranking_loss + F.binary_cross_entropy_with_logits(scores, (rmsd < 2).float())
            loss.backward()
            return loss.detach(), scores.grad
    else:
        def step():
            scores.grad = None
            rmsd, _ = ops.pose_stats(pred, truth, cb, S)
            loss = ops.rank_loss(scores, rmsd, mode="logsigmoid", with_ce=True)[0]
            loss.backward()
            return loss.detach(), scores.grad
    return step


def time_step(step, steps, warmup):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    ms.sort()
    return ms[2], ms[0], ms[4]


def child(path, S, steps):
    import torch
    step = make_step(path, S, torch.device("cuda:0"))
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _rows(d, suffix):
    out = []
    for f in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(f, newline="") as fh:
            out.extend(csv.DictReader(fh))
    return out


def launches_per_step(path, S, tmp):
    """Kernels per step: difference of a 3-step and a 1-step run, each a fresh process under rocprofv3."""
    counts = []
    for steps in (1, 3):
        d = os.path.join(tmp, "%s_%d_%d" % (path, S, steps))
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--child", path, "--copies", str(S), "--steps", str(steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
        kern = _rows(d, "_kernel_trace.csv")
        if not kern:
            raise RuntimeError("no kernel trace under %s: %s" % (d, os.listdir(d) if os.path.isdir(d) else "(missing)"))
        counts.append(len(kern))
    return (counts[1] - counts[0]) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, nargs="+", default=[8, 40])
    ap.add_argument("--no-prof", action="store_true", help="skip the rocprofv3 launch counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_loss.txt"))
    ap.add_argument("--child", choices=sorted(PATHS), help="(internal) run one path for --steps steps at --copies[0] and exit")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.copies[0], a.steps)
    import torch
    dev = torch.device("cuda:0")
    res, agree = {}, {}
    for S in a.copies:
        outs = {}
        for path in sorted(PATHS):
            step = make_step(path, S, dev)
            res[path, S] = time_step(step, a.steps, a.warmup)
            loss, grad = step()
            outs[path] = (float(loss), grad.double().cpu())
        agree[S] = (abs(outs["a"][0] - outs["b"][0]), float((outs["a"][1] - outs["b"][1]).abs().max()))
    counts = {}
    if not a.no_prof:
        tmp = tempfile.mkdtemp(prefix="confidence_bench_")
        try:
            for S in a.copies:
                for path in sorted(PATHS):
                    counts[path, S] = launches_per_step(path, S, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    lines = ["confidence step (pose statistics + logsigmoid ranking loss + BCE + backward to the scores), %d atoms per copy; %s"
             % (ATOMS, torch.cuda.get_device_name(0)),
             "ms per step: median of 5 repeats of %d steps after %d warm-up steps (min .. max); kernels per step from rocprofv3 kernel traces"
             % (a.steps, a.warmup),
             "%6s  %-46s %10s %21s %14s" % ("copies", "path", "ms/step", "(min .. max)", "kernels/step")]
    for S in a.copies:
        for path in sorted(PATHS):
            med, lo, hi = res[path, S]
            k = ("%14.1f" % counts[path, S]) if (path, S) in counts else ("%14s" % "-")
            lines.append("%6d  (%s) %-42s %10.3f %9.3f .. %8.3f %s" % (S, path, PATHS[path], med, lo, hi, k))
        lines.append("%6d  (b) vs (a): %.1fx; |loss difference| %.2e, max |gradient difference| %.2e"
                     % (S, res["a", S][0] / res["b", S][0], agree[S][0], agree[S][1]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
