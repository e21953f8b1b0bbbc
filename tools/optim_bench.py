"""The tail of a training step -- clip + optimizer step -- on the production IaBNet parameter set (394 tensors, 36,270,615 parameters),
three ways in one process:
  (a) the tail of `parallel.train_step` with a torch optimizer: parallel.clip_grad_norm_ + torch.optim.AdamW
  (b) torch's best: torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True)
  (c) fabind_amd.optim.FusedAdam (csrc/optim.hip: clip and non-finite guard inside the step)
Gradients are seeded synthetic values laid out as ParamPack leaves them: views of ONE flat fp32 buffer at arbitrary element offsets.
Timing as everywhere in the project: device events around `--steps` steps after warm-up, median of five repeats (min .. max = the
spread).  Launch counts per step come from `rocprofv3 --kernel-trace --memory-copy-trace --stats` runs of this file in a fresh process
(`--child`), as the difference between a run of 4 steps and a run of 2; (c) must be 2 kernels + 1 host-to-device copy (asserted).

usage: optim_bench.py [--steps 20] [--warmup 5] [--no-prof] [--out profiles/optim_step_tail.txt]"""
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

MODES = {"a": "parallel.clip_grad_norm_ + torch AdamW", "b": "torch clip (foreach) + AdamW(fused=True)", "c": "FusedAdam"}
BYTES_PER_PARAM = 32           # update: read p, g, m, v + write p, m, v (28) and the norm pass's read of g (4)


class _Log:
    def log_message(self, m):
        pass


def production_shapes():
    import bench
    import torch
    from fabind_amd.models import get_model
    torch.manual_seed(0)
    m = get_model(bench.stack_args(512, 4, 8), _Log(), None)
    shapes = [tuple(p.shape) for p in m.parameters() if p.requires_grad]
    assert len(shapes) == 394 and sum(int(torch.Size(s).numel()) for s in shapes) == 36270615
    return shapes


def make_tail(mode, shapes, dev):
    """-> (step function, params) of one tail on its own copy of the parameter set."""
    import torch
    from fabind_amd import parallel
    from fabind_amd.optim import FusedAdam
    g = torch.Generator(device=dev).manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
    n = sum(p.numel() for p in params)
    flat = torch.randn(n, device=dev, generator=g) * 1e-3          # norm ~ 6: the clip is active
    off = 0
    for p in params:                                               # ParamPack._backward's layout: back to back, no alignment padding
        p.grad = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    if mode == "a":
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01)

        def step():
            parallel.clip_grad_norm_(params, 1.0)
            opt.step()
    elif mode == "b":
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01, fused=True)

        def step():
            torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
            opt.step()
    else:
        opt = FusedAdam(params, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0)

        def step():
            opt.step()
    return step, params


def time_tail(step, steps, warmup):
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


def copy_bandwidth(dev, n_bytes):
    """Device-to-device copy rate (bytes read + written per second) over a buffer of the step's size."""
    import torch
    src = torch.empty(n_bytes // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    return 2 * src.numel() * 4 / (time_tail(lambda: dst.copy_(src), 10, 3)[0] * 1e-3)


def child(mode, steps):
    import torch
    dev = torch.device("cuda:0")
    step, _ = make_tail(mode, production_shapes(), dev)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _rows(d, suffix):
    out = []
    for f in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(f, newline="") as fh:
            out.extend(csv.DictReader(fh))
    return out


def launches_per_step(mode, tmp):
    """(kernels, host-to-device copies) per step: difference of a 4-step and a 2-step run, each a fresh process under rocprofv3."""
    counts = []
    for steps in (2, 4):
        d = os.path.join(tmp, "%s%d" % (mode, steps))
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
        kern = _rows(d, "_kernel_trace.csv")
        if not kern:
            raise RuntimeError("no kernel trace under %s: %s" % (d, os.listdir(d) if os.path.isdir(d) else "(missing)"))
        h2d = [c for c in _rows(d, "_memory_copy_trace.csv") if "HOST_TO_DEVICE" in (c.get("Direction") or "").upper()]
        counts.append((len(kern), len(h2d)))
    return (counts[1][0] - counts[0][0]) / 2.0, (counts[1][1] - counts[0][1]) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true", help="skip the rocprofv3 launch counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_tail.txt"))
    ap.add_argument("--child", choices=sorted(MODES), help="(internal) run one tail for --steps steps and exit")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps)
    import torch
    dev = torch.device("cuda:0")
    shapes = production_shapes()
    n_param = sum(int(torch.Size(s).numel()) for s in shapes)
    res = {}
    for mode in sorted(MODES):
        step, params = make_tail(mode, shapes, dev)
        res[mode] = time_tail(step, a.steps, a.warmup)
        del step, params
        torch.cuda.empty_cache()
    bw = copy_bandwidth(dev, n_param * BYTES_PER_PARAM)
    floor_ms = n_param * BYTES_PER_PARAM / bw * 1e3
    counts = {}
    if not a.no_prof:
        tmp = tempfile.mkdtemp(prefix="optim_bench_")
        try:
            for mode in sorted(MODES):
                counts[mode] = launches_per_step(mode, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    lines = ["step tail on the production IaBNet parameter set: %d tensors, %d parameters; %s" % (len(shapes), n_param, torch.cuda.get_device_name(0)),
             "ms per step: median of 5 repeats of %d steps after %d warm-up steps (min .. max); launches per step from rocprofv3 kernel / memory-copy traces"
             % (a.steps, a.warmup),
             "%-46s %10s %21s %14s %12s" % ("tail", "ms/step", "(min .. max)", "kernels/step", "H2D/step")]
    for mode in sorted(MODES):
        med, lo, hi = res[mode]
        k = ("%14.1f %12.1f" % counts[mode]) if mode in counts else ("%14s %12s" % ("-", "-"))
        lines.append("(%s) %-42s %10.3f %9.3f .. %8.3f %s" % (mode, MODES[mode], med, lo, hi, k))
    spread_a = res["a"][2] - res["a"][1]
    lines.append("(c) vs (a): %.2fx, %.3f ms saved per step; spread of (a)'s five repeats %.3f ms" % (res["a"][0] / res["c"][0], res["a"][0] - res["c"][0], spread_a))
    lines.append("(c) vs (b): %.2fx" % (res["b"][0] / res["c"][0]))
    lines.append("floor: %.2f GB per step (%d B per parameter) at the measured device copy rate %.2f TB/s = %.3f ms; (c) is at %.2fx the floor"
                 % (n_param * BYTES_PER_PARAM / 1e9, BYTES_PER_PARAM, bw / 1e12, floor_ms, res["c"][0] / floor_ms))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    assert res["a"][0] - res["c"][0] > spread_a, "FusedAdam is not faster than today's tail by more than its spread"
    if counts:
        assert counts["c"] == (2.0, 1.0), "FusedAdam issued %s kernels / H2D copies per step, expected (2, 1)" % (counts["c"],)


if __name__ == "__main__":
    main()
