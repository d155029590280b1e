"""Step time of the fused training step under the training objectives: the airfoil workload of bench.py
(5233 nodes, B = 8, fp32, eager) with the default objective and with normalized / rmse, and -- given a built checkout of the
parent commit -- the parent's step in the same call, alternating, so that the default route can be seen to be the same code path.

    python profiles/objective_rates.py [--parent DIR] [--rounds 3] [--out profiles/objective_rates.txt]

Every figure comes from a fresh child process (its own import, mesh, warm-up): `--steps` steps, each bracketed by HIP events on
the launching stream; the median per-step time and the wall-clock rate between two synchronisations are reported.  The spread
between the rounds of one variant is the same-box noise a difference has to exceed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANTS = {"default": None, "normalized/rmse": ("normalized", "rmse")}


def child(root, variant, steps, warmup, batch):
    sys.path.insert(0, root)
    import time
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload("airfoil", batch, "cuda", seed=0)
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    data = bench.data_tuple(wl)
    sim(data, True, True)
    kw = {} if VARIANTS[variant] is None else {"objective": eng.Objective(*VARIANTS[variant])}
    dp = eng.DataParallel(sim, **kw)
    for _ in range(warmup):
        loss = dp.step_loss_backward(data, True)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(steps):
        loss = dp.step_loss_backward(data, True)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    print(json.dumps({"median_ms": statistics.median(ms), "steps_per_s": steps / wall, "loss": float(loss), "package": os.path.dirname(os.path.realpath(eng.__file__))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=2, metavar=("ROOT", "VARIANT"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.steps, args.warmup, args.batch)
    runs = [("this commit", ROOT, "default"), ("this commit", ROOT, "normalized/rmse")]
    if args.parent:
        runs.insert(0, ("parent", os.path.abspath(args.parent), "default"))
    res = {r[:1] + r[2:]: [] for r in runs}
    for rnd in range(args.rounds):
        for who, root, variant in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, variant, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
            if out.returncode != 0:
                raise SystemExit(f"{who} / {variant} failed ({out.returncode}):\n{out.stderr[-3000:]}")
            r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
            res[(who, variant)].append(r)
            print(f"round {rnd} {who:12s} {variant:16s} {r['median_ms']:.3f} ms/step (median of HIP events), {r['steps_per_s']:.1f} steps/s, "
                  f"loss {r['loss']:.6f}", flush=True)
    lines = ["# Fused training step under the training objectives: profiles/objective_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, fp32, eager; {args.steps} steps per run after {args.warmup} warm-up steps, a fresh process per run,",
             f"# {args.rounds} rounds alternating the variants in one call on one MI355X.  ms/step = median of per-step HIP events.",
             "# No figure is a pass criterion of the feature.",
             "#", "# commit        objective         ms/step per round                 median    steps/s (wall, median)"]
    for (who, variant), rs in res.items():
        ms = [r["median_ms"] for r in rs]
        lines.append(f"  {who:12s}  {variant:16s}  {'  '.join(f'{m:.3f}' for m in ms):32s}  {statistics.median(ms):.3f}     "
                     f"{statistics.median(r['steps_per_s'] for r in rs):.1f}")
    if args.parent:
        a, b = [r["median_ms"] for r in res[("parent", "default")]], [r["median_ms"] for r in res[("this commit", "default")]]
        lines.append(f"# default objective, this commit against the parent: {statistics.median(b) / statistics.median(a) - 1:+.2%} "
                     f"(spread between rounds: parent {max(a) / min(a) - 1:.2%}, this commit {max(b) / min(b) - 1:.2%})")
    a, b = [r["median_ms"] for r in res[("this commit", "default")]], [r["median_ms"] for r in res[("this commit", "normalized/rmse")]]
    lines.append(f"# normalized / rmse against the default objective: {statistics.median(b) - statistics.median(a):+.3f} ms/step "
                 f"({statistics.median(b) / statistics.median(a) - 1:+.2%})")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
