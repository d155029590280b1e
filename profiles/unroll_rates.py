#!/usr/bin/env python3
"""Cost of the unrolled training loss: one K = 4 `FusedStep(unroll=4)` at airfoil B = 8 against 4 x the single step
(`FusedStep()`, the code path unroll = 1 takes), fp32 and bf16, the two alternated round by round in ONE process so that clock
and thermal drift hit both alike.  Times are HIP events around groups of steps, the median over the rounds is reported.
Also prints what the K steps keep for their backward (the per-step saved buffers of step._Arena).

  python profiles/unroll_rates.py [--rounds 12] [--steps 5]        writes profiles/unroll_rates.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import bsms_gnn_amd as eng

K, B = 4, 8


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "unroll_rates.txt"))
    args = ap.parse_args()
    wl = bench.build_workload("airfoil", B, "cuda")
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    data = bench.data_tuple(wl)
    sim(data, True, True)
    node_in, tar = data[0], data[1]
    state = node_in[..., :tar.shape[-1]]
    later = torch.stack([state + (k + 1) * (tar - state) for k in range(1, K)])
    grads = eng.GradBuckets(list(sim.parameters()))
    single = eng.FusedStep(sim, grads)
    variants = {"BPTT": eng.FusedStep(sim, grads, unroll=K), "detached": eng.FusedStep(sim, grads, unroll=K, detach=True)}
    lines = [f"airfoil B = {B}, {wl['levels'][0][0]} nodes, K = {K}; median of {args.rounds} rounds of {args.steps} steps, ms per call",
             f"{'precision':10s} {'variant':9s} {'single':>8s} {'4 x single':>11s} {'unrolled':>9s} {'ratio':>7s}"]
    for prec in ("f32", "bf16"):
        sim.process.precision = prec
        fns = {"single": lambda: single(data, True), **{n: (lambda s=s: s(data, True, later)) for n, s in variants.items()}}
        for fn in fns.values():                     # buffers, plans, lazy kernel attributes
            timed(fn, 2)
        t = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                t[n].append(timed(fn, args.steps))
        med = {n: statistics.median(v) for n, v in t.items()}
        for n in variants:
            lines.append(f"{prec:10s} {n:9s} {med['single']:8.3f} {K * med['single']:11.3f} {med[n]:9.3f} {med[n] / (K * med['single']):7.3f}")
        if prec == "f32":
            ar = variants["BPTT"]._arena._t
            per_step = sum(t_.numel() for k, t_ in ar.items() if k.endswith("@1") and not k.startswith("g_pred"))
            total = sum(t_.numel() for t_ in ar.values())
            lines.append(f"memory f32: {per_step / 2**30:.2f} GiB saved per extra step, {total / 2**30:.2f} GiB in the step's arena at K = {K} "
                         f"({(total - (K - 1) * per_step) / 2**30:.2f} GiB of it step 0 + the shared work areas, i.e. what K = 1 holds)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
