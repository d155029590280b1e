"""Cost of node-weighted objectives on the airfoil workload of bench.py (5233 nodes, B = 8, eager), by the protocol
of profiles/objective_rates.py: every figure from a fresh child process, the variants alternating over the rounds of one call.

    python profiles/node_weight_rates.py [--parent DIR] [--rounds 3] [--out profiles/node_weight_rates.txt]

Steps, fp32 and bf16: the default objective and normalized / rmse on the parent (given a built checkout of it) and on this commit,
and normalized / rmse with `node_weighted` (the lumped measure of the mesh, shared [N]) on this commit.  Kernels: the two `_w`
entries against their unweighted counterparts at R = 8 x 5233, C = 3, as the mean of a run of back-to-back launches between two HIP
events (launch-bound kernels: the figure is the rate at which the queue drains them, not a lone kernel's duration)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OBJECTIVES = {"default": None, "normalized/rmse": ("normalized", "rmse"), "normalized/rmse weighted": ("normalized", "rmse")}


def step_child(root, variant, dtype, steps, warmup, batch):
    sys.path.insert(0, root)
    import time
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload("airfoil", batch, "cuda", seed=0)
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    if dtype != "f32":
        sim.process.precision = dtype
    data = bench.data_tuple(wl)
    sim(data, True, True)
    kw, call = {}, {}
    if OBJECTIVES[variant] is not None:
        weighted = variant.endswith("weighted")
        kw["objective"] = eng.Objective(*OBJECTIVES[variant], **({"node_weighted": True} if weighted else {}))
        if weighted:
            pts, cells = bench.mesh_points("airfoil")
            call["node_weights"] = torch.from_numpy(eng.lumped_node_measure(pts, cells, "tri")).cuda()
    dp = eng.DataParallel(sim, **kw)
    for _ in range(warmup):
        loss = dp.step_loss_backward(data, True, **call)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(steps):
        loss = dp.step_loss_backward(data, True, **call)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    print(json.dumps({"median_ms": statistics.median(ms), "steps_per_s": steps / wall, "loss": float(loss)}))


def kernel_child(root, launches, batch):
    sys.path.insert(0, root)
    import torch
    import bsms_gnn_amd as eng
    L, s = eng._abi.lib(), torch.cuda.current_stream().cuda_stream
    R, C = batch * 5233, 3
    gen = torch.Generator().manual_seed(0)
    pred, tar = torch.randn(R, C, generator=gen).cuda(), torch.randn(R, C, generator=gen).cuda()
    mask, w = (torch.rand(R, generator=gen) < 0.8).float().cuda(), torch.rand(R, generator=gen).cuda() + 0.1
    stats = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in ([0.1] * C, [1.2] * C, 1e-8)]
    sums = torch.empty(1 + 3 * C, dtype=torch.float64, device="cuda")
    work = torch.empty(L.bsms_error_sums_work_bytes(1, R), dtype=torch.uint8, device="cuda")
    loss, gnp = torch.empty(1, device="cuda"), torch.empty(R, C, device="cuda")
    p = lambda t: t.data_ptr()
    tail = (R, C, *map(p, stats), None, None, None, p(sums), None, 1, 0, 1.0, None, None, p(loss), None, None, p(gnp), s)
    calls = {
        "bsms_error_sums": lambda: L.bsms_error_sums(p(pred), p(tar), p(mask), 1, R, C, R, R, R, p(sums), p(work), s),
        "bsms_error_sums_w": lambda: L.bsms_error_sums_w(p(pred), p(tar), p(mask), p(w), 1, R, C, R, R, R, R, p(sums), p(work), s),
        "bsms_sim_objective_bwd": lambda: L.bsms_sim_objective_bwd(p(pred), p(tar), p(mask), *tail),
        "bsms_sim_objective_bwd_w (period R)": lambda: L.bsms_sim_objective_bwd_w(p(pred), p(tar), p(mask), p(w), R, *tail),
        "bsms_sim_objective_bwd_w (period N)": lambda: L.bsms_sim_objective_bwd_w(p(pred), p(tar), p(mask), p(w), R // batch, *tail),
    }
    out = {}
    for name, f in calls.items():
        for _ in range(20):
            eng._abi.check(f(), name)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            f()
        b.record()
        torch.cuda.synchronize()
        out[name] = 1e3 * a.elapsed_time(b) / launches
    print(json.dumps(out))


def run(cmd, cwd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if out.returncode != 0:
        raise SystemExit(f"{' '.join(cmd[2:])} failed ({out.returncode}):\n{out.stderr[-3000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "VARIANT", "DTYPE"))
    ap.add_argument("--kernels", metavar="ROOT")
    args = ap.parse_args()
    if args.child:
        return step_child(*args.child, args.steps, args.warmup, args.batch)
    if args.kernels:
        return kernel_child(args.kernels, args.launches, args.batch)
    me = [sys.executable, os.path.abspath(__file__)]
    sizes = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch)]
    runs = [("this commit", ROOT, v) for v in OBJECTIVES]
    if args.parent:
        runs = [("parent", os.path.abspath(args.parent), "default"), runs[0], ("parent", os.path.abspath(args.parent), "normalized/rmse"), *runs[1:]]
    lines = ["# Node-weighted objectives (DESIGN.md 4.19): profiles/node_weight_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, eager; {args.steps} steps per run after {args.warmup} warm-up steps, a fresh process per run,",
             f"# {args.rounds} rounds alternating the variants in one call on one MI355X.  ms/step = median of per-step HIP events.",
             "# No figure is a pass criterion of the feature."]
    for dtype in ("f32", "bf16"):
        res = {(who, v): [] for who, _, v in runs}
        for rnd in range(args.rounds):
            for who, root, variant in runs:
                r = run([*me, "--child", root, variant, dtype, *sizes], root)
                res[(who, variant)].append(r)
                print(f"{dtype} round {rnd} {who:12s} {variant:26s} {r['median_ms']:.3f} ms/step, {r['steps_per_s']:.1f} steps/s, loss {r['loss']:.6f}", flush=True)
        lines += ["#", f"# {dtype}", "# commit        objective                   ms/step per round                 median    steps/s (wall, median)"]
        med = {}
        for (who, variant), rs in res.items():
            ms = [r["median_ms"] for r in rs]
            med[(who, variant)] = statistics.median(ms)
            lines.append(f"  {who:12s}  {variant:26s}  {'  '.join(f'{m:.3f}' for m in ms):32s}  {med[(who, variant)]:.3f}     "
                         f"{statistics.median(r['steps_per_s'] for r in rs):.1f}")
        spread = lambda k: max(r["median_ms"] for r in res[k]) / min(r["median_ms"] for r in res[k]) - 1
        if args.parent:
            for v in ("default", "normalized/rmse"):
                lines.append(f"# {v}, this commit against the parent: {med[('this commit', v)] / med[('parent', v)] - 1:+.2%} "
                             f"(spread between rounds: parent {spread(('parent', v)):.2%}, this commit {spread(('this commit', v)):.2%})")
        b = med[("this commit", "normalized/rmse weighted")]
        for who in (("parent",) if args.parent else ()) + ("this commit",):       # the baseline: the unweighted objective on the parent
            a = med[(who, "normalized/rmse")]
            lines.append(f"# the flag: normalized / rmse weighted on this commit against unweighted on {'the parent' if who == 'parent' else who}: "
                         f"{b - a:+.3f} ms/step ({b / a - 1:+.2%})")
    ks = [run([*me, "--kernels", ROOT, "--launches", str(args.launches), "--batch", str(args.batch)], ROOT) for _ in range(args.rounds)]
    lines += ["#", f"# the entries alone at R = {args.batch} x 5233, C = 3: us per call, mean over {args.launches} back-to-back launches, per round"]
    for name in ks[0]:
        us = [k[name] for k in ks]
        lines.append(f"  {name:38s}  {'  '.join(f'{u:.2f}' for u in us):24s}  median {statistics.median(us):.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
