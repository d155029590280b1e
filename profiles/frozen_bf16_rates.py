"""What frozen MLPs save the fused step in the bf16 precisions: the airfoil workload of bench.py (5233 nodes, B = 8,
eager, unroll 1) in bf16 and bf16_nodes, five variants alternated in ONE process on one set of inputs:

    (a) everything trainable, and the same engine built again (a')   (b) processor frozen, encoder and decoder trainable
    (c) input_grad=True, everything trainable                        (d) input_grad=True, nothing trainable (a data-only backward)

    python profiles/frozen_bf16_rates.py [--parent DIR] [--rounds 3] [--stats-csv FILE] [--out profiles/frozen_bf16_rates.txt]

Every round times `--steps` steps of each variant, each step bracketed by HIP events on the launching stream; the median per-step
time is reported per round.  (a) against (a') in the same round is the run-to-run spread a difference has to exceed.  `--parent DIR`
(a checkout of the parent commit with its library built) adds the parent's step (a) in f32, bf16 and bf16_nodes from a fresh child
process per round, and this commit's f32 step (a) / (a') beside it: nothing frozen makes the parent's calls, so the two are held to
that spread.

Per-kernel times come from a separate run under the profiler, which this script does not start itself:

    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/frozen_bf16_rates.py --trace
    python profiles/frozen_bf16_rates.py --stats-csv DIR/.../*_kernel_stats.csv ...

`--trace` runs (c) and then (d) in bf16, `--steps` steps each; `--stats-csv` copies the rows of the fused edge backward
(k_edge_fused_bwd + k_ef_reduce in (c), k_edge_data_bwd in (d)), of the scatter pair and of the weight-gradient kernels into the
report.  The only condition: a frozen variant is not slower than its trainable one beyond the spread."""
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
KERNELS = ("k_edge_fused_bwd", "k_edge_data_bwd", "k_ef_reduce", "k_wgrad", "k_rowsum_pair", "k_small_reduce")


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


def make_engine(eng, bench, wl, first, prec, freeze, input_grad):
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    sim.load_state_dict(first.state_dict())
    sim.process.precision = prec
    for name in freeze:
        getattr(sim, name).requires_grad_(False)
    dp = eng.DataParallel(sim, **({"input_grad": True} if input_grad else {}))
    assert dp.fused is not None, "the variant fell back to the autograd route"
    return dp


def timed(torch, dp, data, steps):
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        loss = dp.step_loss_backward(data, True)
        evs[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(steps)), float(loss)


def parent_child(root, prec, steps, warmup, batch):
    torch, bench, eng, wl, data, first = setup(root, batch)
    dp = make_engine(eng, bench, wl, first, prec, (), False)
    for _ in range(warmup):
        dp.step_loss_backward(data, True)
    ms, loss = timed(torch, dp, data, steps)
    print(json.dumps({"median_ms": ms, "loss": loss, "package": os.path.dirname(os.path.realpath(eng.__file__))}))


def trace(steps, warmup, batch):
    torch, bench, eng, wl, data, first = setup(ROOT, batch)
    for v in ("c", "d"):
        dp = make_engine(eng, bench, wl, first, "bf16", VARIANTS[v][1], True)
        for _ in range(warmup + steps):
            dp.step_loss_backward(data, True)
        torch.cuda.synchronize()


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in KERNELS):
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
    ap.add_argument("--stats-csv", help="kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--trace`")
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parent-child", nargs=2, metavar=("ROOT", "PRECISION"))
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args.parent_child[0], args.parent_child[1], args.steps, args.warmup, args.batch)
    if args.trace:
        return trace(args.steps, args.warmup, args.batch)
    torch, bench, eng, wl, data, first = setup(ROOT, args.batch)
    res, losses, same_ig = {}, {}, {}
    for prec in ("f32", "bf16", "bf16_nodes"):
        names = ("a", "a'") if prec == "f32" else tuple(VARIANTS)      # f32 with frozen MLPs: profiles/frozen_rates.py
        if prec == "f32" and not args.parent:
            continue
        engines = {v: make_engine(eng, bench, wl, first, prec, VARIANTS[v][1], VARIANTS[v][2]) for v in names}
        for dp in engines.values():
            for _ in range(args.warmup):
                dp.step_loss_backward(data, True)
        grad_in = {}
        for rnd in range(args.rounds):
            if args.parent:
                cmd = [sys.executable, os.path.abspath(__file__), "--parent-child", os.path.abspath(args.parent), prec, "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--batch", str(args.batch)]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=os.path.abspath(args.parent))
                if out.returncode != 0:
                    raise SystemExit(f"parent / {prec} failed ({out.returncode}):\n{out.stderr[-3000:]}")
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                res.setdefault((prec, "parent"), []).append(r["median_ms"])
                losses[(prec, "parent")] = r["loss"]
                print(f"round {rnd} {prec} parent (a) {r['median_ms']:.3f} ms/step, loss {r['loss']:.6f} [{r['package']}]", flush=True)
            for v, dp in engines.items():
                ms, loss = timed(torch, dp, data, args.steps)
                res.setdefault((prec, v), []).append(ms)
                losses[(prec, v)] = loss
                if VARIANTS[v][2]:
                    grad_in[v] = dp.fused.input_grad().clone()
                print(f"round {rnd} {prec} ({v}) {VARIANTS[v][0]:34s} {ms:.3f} ms/step, loss {loss:.6f}", flush=True)
        if grad_in:
            same_ig[prec] = bool(torch.equal(grad_in["c"], grad_in["d"]))
        print(f"{prec}: losses of all variants (and the parent) equal: {len({losses[k] for k in losses if k[0] == prec}) == 1}", flush=True)
        del engines
    med = lambda p, v: statistics.median(res[(p, v)])
    lines = ["# Fused training step with frozen MLPs in the bf16 precisions: profiles/frozen_bf16_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, eager, unroll 1; {args.rounds} rounds of {args.steps} steps per variant after {args.warmup} warm-up",
             "# steps, the variants alternated in one process on one MI355X.  ms/step = median of per-step HIP events.",
             "#", "# precision   variant                                     ms/step per round              median"]
    for (p, v), ms in res.items():
        name = "parent: everything trainable (own process)" if v == "parent" else f"({v}) {VARIANTS[v][0]}"
        lines.append(f"  {p:<10s}  {name:42s}  {'  '.join(f'{m:.3f}' for m in ms):28s}  {statistics.median(ms):.3f}")
    for p in sorted({k[0] for k in res}, key=("f32", "bf16", "bf16_nodes").index):
        spread = max(abs(x / y - 1) for x, y in zip(res[(p, "a")], res[(p, "a'")]))
        lines.append(f"# {p}: run-to-run spread, (a) against (a') in the same round: up to {spread:.2%}; losses of all variants"
                     f"{' and the parent' if args.parent else ''} equal: {len({losses[k] for k in losses if k[0] == p}) == 1}")
        if args.parent:
            q = res[(p, "parent")]
            lines.append(f"# {p}: (a) against the parent's step {med(p, 'a') / statistics.median(q) - 1:+.2%} (the parent's own rounds: "
                         f"{max(q) / min(q) - 1:.2%} apart)")
        if (p, "b") in res:
            lines.append(f"# {p}: (b) against (a) {med(p, 'b') - med(p, 'a'):+.3f} ms/step ({med(p, 'b') / med(p, 'a') - 1:+.2%}); "
                         f"(d) against (c) {med(p, 'd') - med(p, 'c'):+.3f} ms/step ({med(p, 'd') / med(p, 'c') - 1:+.2%}); "
                         f"input gradient of (d) bit-equal to (c): {same_ig[p]}")
    if args.stats_csv:
        lines += ["#", "# Kernels of (c) and then of (d) in bf16 (the same number of steps each), from a separate `rocprofv3 --kernel-trace --stats` run of",
                  "# `--trace` (k_edge_fused_bwd + k_ef_reduce belong to (c), k_edge_data_bwd and k_rowsum_pair_bf16 to (d); the level-0 launch is the largest: max):",
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
