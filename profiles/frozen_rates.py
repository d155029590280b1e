"""What the weight gradients cost the fused step, measured by leaving them out: the airfoil workload of bench.py
(5233 nodes, B = 8, fp32, eager) at unroll 1 and 4, four variants alternated in ONE process on one set of inputs:

    (a) everything trainable                          (b) processor frozen, encoder and decoder trainable
    (c) input_grad=True, everything trainable         (d) input_grad=True, nothing trainable (a data-only backward)

    python profiles/frozen_rates.py [--parent DIR] [--rounds 3] [--stats-csv FILE] [--out profiles/frozen_rates.txt]

Every round times `--steps` steps of each variant, each step bracketed by HIP events on the launching stream; the median per-step
time is reported per round.  (a) is run TWICE per round (a, a'): the spread between the two is the run-to-run noise a difference
has to exceed.  `--parent DIR` (a checkout of the parent commit with its library built) adds the parent's step (a) from a fresh
child process per round, against which this commit's (a) is held to that spread.

Per-kernel times come from a separate run under the profiler, which this script does not start itself:

    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/frozen_rates.py --trace
    python profiles/frozen_rates.py --stats-csv DIR/.../*_kernel_stats.csv ...

`--trace` runs (c) and then (d) at unroll 1, `--steps` steps each; `--stats-csv` copies the rows of the edge backward kernels
(k_edge_bwd<NB, RB, LONE, STORE>: STORE = true is the storing build, false the no-store build a frozen edge MLP takes) and of
the weight-gradient kernels into the report.  No figure is a pass criterion of the feature."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANTS = {"a": ("everything trainable", (), False), "a'": ("everything trainable (again)", (), False),
            "b": ("processor frozen", ("process",), False), "c": ("input_grad, everything trainable", (), True),
            "d": ("input_grad, nothing trainable", ("encode", "process", "decode"), True)}


def setup(root, batch):
    sys.path.insert(0, root)
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload("airfoil", batch, "cuda", seed=0)
    data = bench.data_tuple(wl)
    torch.manual_seed(0)
    first = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    first(data, True, True)                                            # one normaliser accumulation
    return torch, bench, eng, wl, data, first


def make_engine(eng, bench, wl, first, freeze, input_grad, K):
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    sim.load_state_dict(first.state_dict())
    for name in freeze:
        getattr(sim, name).requires_grad_(False)
    kw = {"input_grad": True} if input_grad else {}                    # the parent's constructor may not know the keyword
    dp = eng.DataParallel(sim, unroll=K, **kw)
    assert dp.fused is not None, "the variant fell back to the autograd route"
    return dp


def later_targets(torch, data, K):
    C = data[1].shape[-1]
    state = data[0][..., :C]
    return torch.stack([state + (k + 1) * (data[1] - state) for k in range(1, K)]) if K > 1 else None


def timed(torch, dp, data, later, steps):
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        loss = dp.step_loss_backward(data, True, later)
        evs[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(steps)), float(loss)


def parent_child(root, K, steps, warmup, batch):
    torch, bench, eng, wl, data, first = setup(root, batch)
    dp = make_engine(eng, bench, wl, first, (), False, K)
    later = later_targets(torch, data, K)
    for _ in range(warmup):
        dp.step_loss_backward(data, True, later)
    ms, loss = timed(torch, dp, data, later, steps)
    print(json.dumps({"median_ms": ms, "loss": loss, "package": os.path.dirname(os.path.realpath(eng.__file__))}))


def trace(steps, warmup, batch):
    torch, bench, eng, wl, data, first = setup(ROOT, batch)
    for v in ("c", "d"):
        dp = make_engine(eng, bench, wl, first, VARIANTS[v][1], True, 1)
        for _ in range(warmup + steps):
            dp.step_loss_backward(data, True, None)
        torch.cuda.synchronize()


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_edge_bwd" in name or "k_wgrad" in name or "k_rowsum_pair" in name or "k_small_reduce" in name:
                short = name[name.find("k_"):].split("(")[0]
                rows.append((short, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--unroll", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--stats-csv", help="kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--trace`")
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parent-child", nargs=2, metavar=("ROOT", "UNROLL"))
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args.parent_child[0], int(args.parent_child[1]), args.steps, args.warmup, args.batch)
    if args.trace:
        return trace(args.steps, args.warmup, args.batch)
    torch, bench, eng, wl, data, first = setup(ROOT, args.batch)
    res, losses, grad_in = {}, {}, {}
    for K in args.unroll:
        later = later_targets(torch, data, K)
        engines = {v: make_engine(eng, bench, wl, first, fr, ig, K) for v, (_, fr, ig) in VARIANTS.items()}
        for dp in engines.values():
            for _ in range(args.warmup):
                dp.step_loss_backward(data, True, later)
        for rnd in range(args.rounds):
            if args.parent:
                cmd = [sys.executable, os.path.abspath(__file__), "--parent-child", os.path.abspath(args.parent), str(K), "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--batch", str(args.batch)]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=os.path.abspath(args.parent))
                if out.returncode != 0:
                    raise SystemExit(f"parent / unroll {K} failed ({out.returncode}):\n{out.stderr[-3000:]}")
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                res.setdefault((K, "parent"), []).append(r["median_ms"])
                losses[(K, "parent")] = r["loss"]
                print(f"round {rnd} unroll {K} parent (a) {r['median_ms']:.3f} ms/step, loss {r['loss']:.6f} [{r['package']}]", flush=True)
            for v, dp in engines.items():
                ms, loss = timed(torch, dp, data, later, args.steps)
                res.setdefault((K, v), []).append(ms)
                losses[(K, v)] = loss
                if VARIANTS[v][2]:
                    grad_in[(K, v)] = dp.fused.input_grad().clone()
                print(f"round {rnd} unroll {K} ({v}) {VARIANTS[v][0]:34s} {ms:.3f} ms/step, loss {loss:.6f}", flush=True)
        same = bool(torch.equal(grad_in[(K, "c")], grad_in[(K, "d")]))
        print(f"unroll {K}: input gradient of (d) bit-equal to (c): {same}; losses equal: {len({losses[(K, v)] for v in VARIANTS}) == 1}", flush=True)
        grad_in[K] = same
        del engines
    med = lambda K, v: statistics.median(res[(K, v)])
    lines = ["# Fused training step with frozen MLPs: profiles/frozen_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, fp32, eager; {args.rounds} rounds of {args.steps} steps per variant after {args.warmup} warm-up steps,",
             "# the variants alternated in one process on one MI355X.  ms/step = median of per-step HIP events; a step is `unroll` forwards",
             "# and backwards.  No figure is a pass criterion of the feature.",
             "#", "# unroll  variant                                   ms/step per round              median"]
    for (K, v), ms in res.items():
        name = "parent: everything trainable (own process)" if v == "parent" else f"({v}) {VARIANTS[v][0]}"
        lines.append(f"  {K:<6d}  {name:42s}  {'  '.join(f'{m:.3f}' for m in ms):28s}  {statistics.median(ms):.3f}")
    for K in args.unroll:
        spread = max(abs(x / y - 1) for x, y in zip(res[(K, "a")], res[(K, "a'")]))
        lines.append(f"# unroll {K}: run-to-run spread, (a) against (a') in the same round: up to {spread:.2%}")
        if args.parent:
            p = res[(K, "parent")]
            lines.append(f"# unroll {K}: (a) against the parent's step {med(K, 'a') / statistics.median(p) - 1:+.2%} (the parent's own rounds: "
                         f"{max(p) / min(p) - 1:.2%} apart)")
        lines.append(f"# unroll {K}: (b) against (a) {med(K, 'b') - med(K, 'a'):+.3f} ms/step ({med(K, 'b') / med(K, 'a') - 1:+.2%}); "
                     f"(d) against (c) {med(K, 'd') - med(K, 'c'):+.3f} ms/step ({med(K, 'd') / med(K, 'c') - 1:+.2%}); "
                     f"input gradient of (d) bit-equal to (c): {grad_in[K]}")
    if args.stats_csv:
        lines += ["#", "# Kernels of (c) and then of (d) at unroll 1 (the same number of steps each), from a separate `rocprofv3 --kernel-trace --stats` run",
                  "# of `--trace` (k_edge_bwd<NB, RB, LONE, STORE>: STORE = true in (c), false in (d); the level-0 launch is the largest: see max):",
                  "# kernel                                                  calls   total ms   average us   max us"]
        for name, calls, total, avg, mx in kernel_rows(args.stats_csv):
            lines.append(f"  {name[:54]:54s}  {calls:6d}  {total:9.2f}  {avg:11.1f}  {mx:7.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
