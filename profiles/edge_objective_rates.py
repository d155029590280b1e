"""Cost of the objective with an edge-difference term on the airfoil workload of bench.py (5233 nodes, B = 8, eager), by
the protocol of profiles/robust_rates.py: every figure from a fresh child process, the variants alternating over the rounds of one call.

    python profiles/edge_objective_rates.py [--parent DIR] [--rounds 3] [--out profiles/edge_objective_rates.txt]

(a) bench.py's default step on the parent (given a built checkout of it) and on this commit, and `--dump-outputs` of both compared
    byte for byte.
(b) fp32 and bf16: normalized / mse with the edge term (lambda = 0.1, "difference" and "quotient") on this commit against normalized /
    mse on the parent (and on this commit).
(c) bsms_sim_edge_objective_bwd alone against bsms_sim_objective_bwd + bsms_edge_diff_bwd(accumulate) as two launches -- the same
    gradient without the fusion -- and bsms_edge_diff_sums + bsms_edge_diff_fold, on the level-0 graphs of the airfoil (5233 rows,
    p = 2) and the surface mesh (16384 rows, p = 3), S = 8, C = 4: the mean of a run of back-to-back launches between two HIP events
    (launch-bound kernels: the figure is the rate at which the queue drains them, not a lone kernel's duration)."""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OBJECTIVES = {"normalized/mse": dict(space="normalized", kind="mse"),
              "normalized/mse + 0.1 difference": dict(space="normalized", kind="mse", edge_weight=0.1, edge_weighting="difference"),
              "normalized/mse + 0.1 quotient": dict(space="normalized", kind="mse", edge_weight=0.1, edge_weighting="quotient")}


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
    dp = eng.DataParallel(sim, objective=eng.Objective(**OBJECTIVES[variant]))
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
    print(json.dumps({"median_ms": statistics.median(ms), "steps_per_s": steps / wall, "loss": float(loss)}))


def kernel_child(root, launches, S):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bench
    import bsms_gnn_amd as eng
    from bsms_gnn_amd.hierarchy import to_flat_edge
    L, X, s = eng._abi.lib(), eng._abi.ext(), torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()
    out = {}
    for mesh in ("airfoil", "surface"):
        pts, cells = bench.mesh_points(mesh, None)
        g, pos = torch.tensor(np.asarray(to_flat_edge(cells, "tri")), dtype=torch.int64), torch.tensor(pts, dtype=torch.float32)
        N, p, C = pos.shape[0], pos.shape[1], 4
        R = S * N
        plan = eng.graph.plan_for(g.cuda(), N)
        h = plan.handle
        gen = torch.Generator().manual_seed(0)
        pred, tar = torch.randn(R, C, generator=gen).cuda(), torch.randn(R, C, generator=gen).cuda()
        mask = (torch.rand(R, generator=gen) < 0.9).float().cuda()
        dpos = pos.repeat(S, 1).contiguous().cuda()
        stats = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in ([0.1] * C, [1.2] * C, 1e-8)]
        st = tuple(map(p_, stats))
        sums = torch.ones(2 + 4 * C, dtype=torch.float64, device="cuda")
        esums = torch.empty(S, 1 + 2 * C, dtype=torch.float64, device="cuda")
        work = torch.empty(L.bsms_edge_diff_work_bytes(S, N), dtype=torch.uint8, device="cuda")
        coef = torch.full((S, C), 0.01, dtype=torch.float64, device="cuda")
        loss, gp, gnp = torch.empty(1, device="cuda"), torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda")
        for wname, wid in (("difference", 0), ("quotient", 1)):
            def two():
                L.bsms_sim_objective_bwd(p_(pred), p_(tar), p_(mask), R, C, *st, None, None, None, p_(sums), None, 1, 1, 1.0, None, None, p_(loss), None,
                                         p_(gp), p_(gnp), s)
                return L.bsms_edge_diff_bwd(h, 0, N, p_(pred), p_(tar), p_(mask), p_(dpos), S, C, p, wid, N, N, N, N, p_(coef), 1, p_(gp), N, s)

            def sums_fold():
                L.bsms_edge_diff_sums(h, 0, N, p_(pred), p_(tar), p_(mask), p_(dpos), S, C, p, wid, N, N, N, N, p_(esums), p_(work), s)
                return X.bsms_edge_diff_fold(p_(esums), S, C, p_(sums[1 + 3 * C:]), s)

            calls = {
                "bsms_sim_objective_bwd alone": lambda: L.bsms_sim_objective_bwd(p_(pred), p_(tar), p_(mask), R, C, *st, None, None, None, p_(sums), None,
                                                                                 1, 1, 1.0, None, None, p_(loss), None, p_(gp), p_(gnp), s),
                "bsms_sim_objective_bwd + bsms_edge_diff_bwd (two launches)": two,
                "bsms_sim_edge_objective_bwd (one launch)": lambda: X.bsms_sim_edge_objective_bwd(
                    h, N, S, p_(pred), p_(tar), p_(mask), p_(dpos), C, p, wid, *st, None, None, None, p_(sums), p_(sums[1 + 3 * C:]), None, 1, 1, 0.1, 1.0,
                    None, None, p_(loss), None, None, p_(gp), p_(gnp), s),
                "bsms_edge_diff_sums + bsms_edge_diff_fold": sums_fold,
            }
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
                out[f"{mesh} ({N} rows, p = {p}) {wname}: {name}"] = 1e3 * a.elapsed_time(b) / launches
    print(json.dumps(out))


def run(cmd, cwd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if out.returncode != 0:
        raise SystemExit(f"{' '.join(cmd[1:])} failed ({out.returncode}):\n{out.stderr[-3000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def bench_default(root, steps, warmup, dump=None):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-roofline",
           "--no-other-lines"] + (["--dump-outputs", dump] if dump else [])
    r = run(cmd, root)
    return {"steps_per_s": r["value"], "median_ms": r["step_ms_hipevent"]["median"], "loss": r["config"]["loss"]}


def same_dumps(a, b):
    names = sorted(os.listdir(a))
    return len(names), names == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)


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
    parent = os.path.abspath(args.parent) if args.parent else None
    lines = ["# The objective with an edge-difference term (DESIGN.md 4.22): profiles/edge_objective_rates.py",
             f"# airfoil mesh (5233 nodes), B = {args.batch}, eager; {args.steps} steps per run after {args.warmup} warm-up steps, a fresh process per run,",
             f"# {args.rounds} rounds alternating the variants in one call on one MI355X.  ms/step = median of per-step HIP events.",
             "# No figure is a pass criterion of the feature."]
    spread = lambda rs, key: max(r[key] for r in rs) / min(r[key] for r in rs) - 1
    # ---- (a) the default step in bench.py, the parent and this commit alternated; --dump-outputs of the last round compared
    whos = ([("parent", parent)] if parent else []) + [("this commit", ROOT)]
    res = {who: [] for who, _ in whos}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            for who, root in whos:
                dump = os.path.join(tmp, who.replace(" ", "_")) if rnd == args.rounds - 1 else None
                res[who].append(bench_default(root, args.steps, args.warmup, dump))
                print(f"bench.py round {rnd} {who:12s} {res[who][-1]['steps_per_s']:.2f} steps/s", flush=True)
        lines += ["#", "# (a) the default step in bench.py (--gpus 1 --no-cpu-baseline --no-roofline --no-other-lines): steps/s per round (ms/step)"]
        for who, _ in whos:
            rs = res[who]
            lines.append(f"  {who:12s}  {'  '.join('%.2f' % r['steps_per_s'] for r in rs)}   median {statistics.median(r['steps_per_s'] for r in rs):.2f}   "
                         f"({'  '.join('%.3f' % r['median_ms'] for r in rs)} ms)   loss {rs[-1]['loss']!r}")
        if parent:
            a, b = (statistics.median(r["steps_per_s"] for r in res[w]) for w in ("parent", "this commit"))
            n, same = same_dumps(os.path.join(tmp, "parent"), os.path.join(tmp, "this_commit"))
            lines.append(f"# this commit against the parent: {b / a - 1:+.2%} (spread between rounds: parent {spread(res['parent'], 'steps_per_s'):.2%}, "
                         f"this commit {spread(res['this commit'], 'steps_per_s'):.2%}); --dump-outputs of the last round: {n} arrays, "
                         f"{'byte-identical' if same else 'DIFFERENT'}")
    # ---- (b) the new path
    runs = ([("parent", parent, "normalized/mse")] if parent else []) + [("this commit", ROOT, v) for v in OBJECTIVES]
    base = "normalized/mse"
    for dtype in ("f32", "bf16"):
        res = {(who, v): [] for who, _, v in runs}
        for rnd in range(args.rounds):
            for who, root, variant in runs:
                r = run([*me, "--child", root, variant, dtype, *sizes], root if who == "parent" else ROOT)
                res[(who, variant)].append(r)
                print(f"{dtype} round {rnd} {who:12s} {variant:32s} {r['median_ms']:.3f} ms/step, {r['steps_per_s']:.1f} steps/s, loss {r['loss']:.6f}", flush=True)
        lines += ["#", f"# (b) {dtype}", "# commit        objective                         ms/step per round                 median    steps/s (wall, median)"]
        med = {}
        for key, rs in res.items():
            ms = [r["median_ms"] for r in rs]
            med[key] = statistics.median(ms)
            lines.append(f"  {key[0]:12s}  {key[1]:32s}  {'  '.join(f'{m:.3f}' for m in ms):32s}  {med[key]:.3f}     "
                         f"{statistics.median(r['steps_per_s'] for r in rs):.1f}")
        for who in (("parent",) if parent else ()) + ("this commit",):
            a = med[(who, base)]
            for v in list(OBJECTIVES)[1:]:
                b = med[("this commit", v)]
                lines.append(f"# {v} on this commit against {base} on {'the parent' if who == 'parent' else who}: {b - a:+.3f} ms/step ({b / a - 1:+.2%}); "
                             f"spread between rounds {spread(res[('this commit', v)], 'median_ms'):.2%} / {spread(res[(who, base)], 'median_ms'):.2%}")
    # ---- (c) the entries alone
    ks = [run([*me, "--kernels", ROOT, "--launches", str(args.launches), "--batch", str(args.batch)], ROOT) for _ in range(args.rounds)]
    lines += ["#", f"# (c) the entries alone, S = {args.batch}, C = 4: us per call, mean over {args.launches} back-to-back launches, per round"]
    for name in ks[0]:
        us = [k[name] for k in ks]
        lines.append(f"  {name:100s}  {'  '.join(f'{u:.2f}' for u in us):24s}  median {statistics.median(us):.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
