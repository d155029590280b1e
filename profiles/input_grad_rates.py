"""What the input gradient costs the fused training step: the airfoil workload of bench.py (5233 nodes, B = 8,
eager) in fp32 and bf16, unroll 1 and 4, with `input_grad` off and on, and -- given a built checkout of the parent commit -- the
parent's step in the same call, alternating, so that the default step can be seen to be the same code path.

    python profiles/input_grad_rates.py [--parent DIR] [--rounds 2] [--out profiles/input_grad_rates.txt]

Every figure comes from a fresh child process (its own import, mesh, warm-up): `--steps` steps, each bracketed by HIP events on
the launching stream; the median per-step time and the wall-clock rate between two synchronisations are reported.  The spread
between the rounds of one variant is the same-box noise a difference has to exceed.  The only prior figure is the surcharge of the
position kernels on the autograd route (profiles/pos_grad_cost.txt): +0.54 ms fp32 / +0.20 ms bf16 per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONFIGS = [(prec, K) for prec in ("f32", "bf16") for K in (1, 4)]


def child(root, prec, K, flag, steps, warmup, batch):
    sys.path.insert(0, root)
    import time
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload("airfoil", batch, "cuda", seed=0)
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    sim.process.precision = prec
    data = bench.data_tuple(wl)
    sim(data, True, True)
    C = data[1].shape[-1]
    state = data[0][..., :C]
    later = torch.stack([state + (k + 1) * (data[1] - state) for k in range(1, K)]) if K > 1 else None
    kw = {"input_grad": True} if flag else {}                 # the parent's constructor does not know the keyword
    dp = eng.DataParallel(sim, unroll=K, **kw)
    for _ in range(warmup):
        loss = dp.step_loss_backward(data, True, later)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(steps):
        loss = dp.step_loss_backward(data, True, later)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    out = {"median_ms": statistics.median(ms), "steps_per_s": steps / wall, "loss": float(loss), "package": os.path.dirname(os.path.realpath(eng.__file__))}
    if flag:
        out["grad_in_absmax"] = float(dp.fused.input_grad().abs().max())
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=4, metavar=("ROOT", "PRECISION", "UNROLL", "INPUT_GRAD"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]), args.child[3] == "1", args.steps, args.warmup, args.batch)
    who = [("this commit", ROOT, 0), ("this commit + input_grad", ROOT, 1)]
    if args.parent:
        who.insert(0, ("parent", os.path.abspath(args.parent), 0))
    res = {}
    for rnd in range(args.rounds):
        for prec, K in CONFIGS:
            for name, root, flag in who:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", root, prec, str(K), str(flag), "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--batch", str(args.batch)]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
                if out.returncode != 0:
                    raise SystemExit(f"{name} / {prec} / unroll {K} failed ({out.returncode}):\n{out.stderr[-3000:]}")
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                res.setdefault((prec, K, name), []).append(r)
                print(f"round {rnd} {prec:5s} unroll {K} {name:26s} {r['median_ms']:.3f} ms/step (median of HIP events), "
                      f"{r['steps_per_s']:.1f} steps/s, loss {r['loss']:.6f}", flush=True)
    lines = ["# Fused training step with and without the input gradient: profiles/input_grad_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, eager; {args.steps} steps per run after {args.warmup} warm-up steps, a fresh process per run,",
             f"# {args.rounds} rounds alternating the variants in one call on one MI355X.  ms/step = median of per-step HIP events; a step is",
             "# `unroll` forwards and backwards.  No figure is a pass criterion of the feature.",
             "#", "# precision  unroll  variant                     ms/step per round         median    steps/s (wall, median)"]
    med = lambda prec, K, name: statistics.median(r["median_ms"] for r in res[(prec, K, name)])
    for (prec, K, name), rs in res.items():
        ms = [r["median_ms"] for r in rs]
        lines.append(f"  {prec:9s}  {K:<6d}  {name:26s}  {'  '.join(f'{m:.3f}' for m in ms):24s}  {statistics.median(ms):.3f}    "
                     f"{statistics.median(r['steps_per_s'] for r in rs):.1f}")
    base = "parent" if args.parent else "this commit"
    for prec, K in CONFIGS:
        b = med(prec, K, base)
        line = f"# {prec} unroll {K}: "
        if args.parent:
            a = [r["median_ms"] for r in res[(prec, K, "parent")]]
            c = [r["median_ms"] for r in res[(prec, K, "this commit")]]
            line += (f"default step against the parent {med(prec, K, 'this commit') / b - 1:+.2%} (spread between rounds: parent "
                     f"{max(a) / min(a) - 1:.2%}, this commit {max(c) / min(c) - 1:.2%}); ")
        g = med(prec, K, "this commit + input_grad")
        line += f"input_grad against {'the parent' if args.parent else 'the default step'} {g - b:+.3f} ms/step ({g / b - 1:+.2%}), {(g - b) / K:+.3f} ms per unrolled step"
        lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
