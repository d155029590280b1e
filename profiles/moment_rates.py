"""Rates of the dataset statistics on one MI355X, by the protocol of profiles/edge_objective_rates.py: every figure
from a fresh child process, the variants alternating over the rounds of one call.

    python profiles/moment_rates.py [--parent DIR] [--rounds 3] [--out profiles/moment_rates.txt]

(a) `TrajectoryBank.moments()` on an airfoil-shaped bank that leaves the caches (160 trajectories x 101 frames x 5233 nodes x 3
    channels: 1.01 GB of state): device-event time over 20 calls after warm-up, the algorithmic bytes from the shapes, bytes/s and the
    share of the HBM peak.  Kernel time comes from a separate run:  rocprofv3 --kernel-trace --stats -- python profiles/moment_rates.py
    --moments ROOT  (its own child, not part of this call).
(b) the route it replaces: the wall time of accumulation_steps = 300 warm-up `Trainer.iter` calls on batches of 8 from the same bank
    (on the parent commit when --parent is given: that path is not edited here) against ONE `Trainer.fit_normalizers` call, alternated,
    a device synchronise closing each timed window.
(c) bench.py's default step on the parent and on this commit, alternated, and `--dump-outputs` of both compared byte for byte."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HBM_PEAK = 8.0e12            # bytes/s, the MI355X's HBM3E peak (spec)
TRAJS, FRAMES = 160, 101


def build_bank(root, trajs):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import bsms_gnn_amd as eng
    pts, cells = bench.mesh_points("airfoil")
    n = pts.shape[0]
    cfg = SimpleNamespace(field_names=["node_type", "cells", "mesh_pos", "density", "velocity"], output_field_names=["velocity", "density"],
                          mesh_type="tri", unet_depth=3, consist_mesh=True, noise_level=[10.0, 10.0, 0.01], noise_gamma=1.0)
    bank = eng.TrajectoryBank(cfg, dataset="airfoil", seed=0)
    rng = np.random.default_rng(0)
    node_type = np.repeat(rng.choice((0, 0, 0, 4, 5), (1, n, 1)).astype(np.float32), FRAMES, 0)
    mesh_pos, cell_frames = np.repeat(pts.astype(np.float32)[None], FRAMES, 0), np.repeat(cells[None], FRAMES, 0)
    for _ in range(trajs):
        bank.add({"cells": cell_frames, "mesh_pos": mesh_pos, "node_type": node_type,
                  "velocity": rng.standard_normal((FRAMES, n, 2), dtype=np.float32) * 30.0 + 100.0,
                  "density": rng.standard_normal((FRAMES, n, 1), dtype=np.float32) * 0.1 + 1.2})
    return eng, bank, n


def moments_child(root, trajs, calls):
    import torch
    eng, bank, n = build_bank(root, trajs)
    for _ in range(3):
        mom = bank.moments()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(calls):
        mom = bank.moments()
        evs[i + 1].record()
    torch.cuda.synchronize()
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(calls)]
    nbytes = trajs * (FRAMES * n * 3 * 4 + n * 4)          # every state frame once, the static type column once
    print(json.dumps({"ms": ms, "bytes": nbytes, "rows": float(mom.rows), "n": n}))


def trainer_of(eng, accumulation_steps):
    import torch
    mcfg = SimpleNamespace(out_dim=3, latent_dim=128, hidden_layer=2, unet_depth=3, pos_dim=2, consistent_mesh=True,
                           accumulation_steps=accumulation_steps)
    opt = SimpleNamespace(peak_lr=1e-4, weight_decay=1e-2, warmup_steps=100, decay_steps=1000, gnorm_clip=1.0)
    torch.manual_seed(0)
    return eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, opt)


def route_child(root, trajs, route, repeats):
    """`repeats` timed windows in one process (a fresh Trainer each): 300 warm-up iterations, or one fit."""
    import torch
    eng, bank, _ = build_bank(root, trajs)
    out = []
    for _ in range(repeats + 1):                            # the first window warms the process up and is dropped
        tr = trainer_of(eng, 300)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "warmup":
            for _ in range(300):
                tr.iter(bank.sample(8))
            assert not tr._warming_up()
        else:
            tr.fit_normalizers(bank)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    print(json.dumps({"seconds": out[1:]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trajs", type=int, default=TRAJS)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--moments", metavar="ROOT")
    ap.add_argument("--route", nargs=2, metavar=("ROOT", "ROUTE"))
    args = ap.parse_args()
    if args.moments:
        return moments_child(args.moments, args.trajs, args.calls)
    if args.route:
        return route_child(args.route[0], args.trajs, args.route[1], 2)
    sys.path.insert(0, HERE)
    from edge_objective_rates import bench_default, run, same_dumps
    me = [sys.executable, os.path.abspath(__file__), "--trajs", str(args.trajs), "--calls", str(args.calls)]
    parent = os.path.abspath(args.parent) if args.parent else None
    spread = lambda xs: max(xs) / min(xs) - 1
    lines = ["# Dataset statistics on the device (DESIGN.md 4.25): profiles/moment_rates.py, one call on one MI355X, a fresh process per figure.",
             "# No figure is a pass criterion of the feature."]
    # ---- (a)
    m = run([*me, "--moments", ROOT], ROOT)
    med = statistics.median(m["ms"])
    lines += ["#", f"# (a) TrajectoryBank.moments(): {args.trajs} trajectories x {FRAMES} frames x {m['n']} nodes x 3 channels, {m['rows']:.0f} rows; "
              f"{len(m['ms'])} calls after 3 warm-up calls, device events around each call (bsms_moment_sums + bsms_moment_fold)",
              f"  algorithmic bytes (every state frame once + the static type column, from the shapes): {m['bytes']} ({m['bytes'] / 1e9:.3f} GB)",
              f"  ms per call: median {med:.3f}, min {min(m['ms']):.3f}, max {max(m['ms']):.3f}",
              f"  algorithmic bytes/s at the median: {m['bytes'] / (med * 1e-3) / 1e12:.3f} TB/s = {m['bytes'] / (med * 1e-3) / HBM_PEAK:.1%} of the HBM peak "
              f"of {HBM_PEAK / 1e12:.1f} TB/s (spec; a float4 copy measures 6.29 TB/s)"]
    # ---- (b)
    routes = [("300 warm-up Trainer.iter calls, batches of 8" + (" (parent commit)" if parent else " (this commit)"), parent or ROOT, "warmup"),
              ("one Trainer.fit_normalizers call (this commit)", ROOT, "fit")]
    res = {name: [] for name, _, _ in routes}
    for rnd in range(args.rounds):
        for name, root, route in routes:
            r = run([*me, "--route", root, route], root)
            res[name] += r["seconds"]
            print(f"round {rnd} {name}: {r['seconds']}", flush=True)
    lines += ["#", f"# (b) wall seconds from an untouched Trainer to fitted normalisers on the bank of (a), device synchronise closing the window; "
              f"{args.rounds} rounds alternating the routes, 2 windows per process after one dropped"]
    for name, xs in res.items():
        lines.append(f"  {name:72s} {'  '.join(f'{x:.4f}' for x in xs)}   median {statistics.median(xs):.4f} s   spread {spread(xs):.1%}")
    a, b = (statistics.median(res[name]) for name, _, _ in routes)
    lines.append(f"# the fit takes {b / a:.2%} of the warm-up's wall time ({a / b:.0f}x); the warm-up sees 300 x 8 of the bank's {args.trajs * (FRAMES - 1)} pairs, the fit all of them")
    # ---- (c)
    whos = ([("parent", parent)] if parent else []) + [("this commit", ROOT)]
    bres = {who: [] for who, _ in whos}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            for who, root in whos:
                dump = os.path.join(tmp, who.replace(" ", "_")) if rnd == args.rounds - 1 else None
                bres[who].append(bench_default(root, args.steps, args.warmup, dump))
                print(f"bench.py round {rnd} {who:12s} {bres[who][-1]['steps_per_s']:.2f} steps/s", flush=True)
        lines += ["#", "# (c) the default step in bench.py (--gpus 1 --no-cpu-baseline --no-roofline --no-other-lines): steps/s per round (ms/step)"]
        for who, _ in whos:
            rs = bres[who]
            lines.append(f"  {who:12s}  {'  '.join('%.2f' % r['steps_per_s'] for r in rs)}   median {statistics.median(r['steps_per_s'] for r in rs):.2f}   "
                         f"({'  '.join('%.3f' % r['median_ms'] for r in rs)} ms)   loss {rs[-1]['loss']!r}")
        if parent:
            a, b = (statistics.median(r["steps_per_s"] for r in bres[w]) for w in ("parent", "this commit"))
            n, same = same_dumps(os.path.join(tmp, "parent"), os.path.join(tmp, "this_commit"))
            lines.append(f"# this commit against the parent: {b / a - 1:+.2%} (spread between rounds: parent {spread([r['steps_per_s'] for r in bres['parent']]):.2%}, "
                         f"this commit {spread([r['steps_per_s'] for r in bres['this commit']]):.2%}); --dump-outputs of the last round: {n} arrays, "
                         f"{'byte-identical' if same else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
