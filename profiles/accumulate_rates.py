"""What gradient accumulation costs and saves on the airfoil workload of bench.py (5233 nodes, eager):

  step    the plain step (accumulate = 1) at B = 8, fp32 and bf16 -- and, given a built checkout of the parent commit, the parent's
          step in the same call, alternating, so that accumulate = 1 can be seen to be the same code path;
  fold    bsms_grad_fold against bsms_grad_accumulate at the airfoil parameter count, in one process (same traffic: one
          read-modify-write stream and one read stream over the flat buffer);
  cycle   one cycle of 2 x B = 4 and of 4 x B = 2 against the one-shot B = 8 step: ms per 8 samples, and the bytes the step holds
          (its arena of activations and workspaces, plus the scratch flat buffer) -- the trade of time for memory.

    python profiles/accumulate_rates.py [--parent DIR] [--rounds 3] [--out profiles/accumulate_rates.txt]

Every figure comes from a fresh child process (its own import, mesh, warm-up); steps and cycles are bracketed by HIP events on
the launching stream and the median is reported.  The spread between the rounds of one variant is the same-box noise a
difference has to exceed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _setup(root, batch, precision="f32"):
    sys.path.insert(0, root)
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload("airfoil", batch, "cuda", seed=0)
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(bench.make_cfg(wl["cfg"])).cuda()
    data = bench.data_tuple(wl)
    sim(data, True, True)
    sim.process.precision = precision
    return torch, eng, sim, data


def _timed(torch, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def child_step(root, precision, steps, warmup, batch):
    torch, eng, sim, data = _setup(root, batch, precision)
    dp = eng.DataParallel(sim)
    out = {}
    ms = _timed(torch, lambda: out.__setitem__("loss", dp.step_loss_backward(data, True)), warmup, steps)
    print(json.dumps({"median_ms": statistics.median(ms), "loss": float(out["loss"]), "package": os.path.dirname(os.path.realpath(eng.__file__))}))


def child_fold(root, steps, warmup, batch):
    torch, eng, sim, _ = _setup(root, 1)
    n = eng.GradBuckets(list(sim.parameters())).flat.numel()
    L, s = eng._abi.lib(), torch.cuda.current_stream().cuda_stream
    acc, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    coef = torch.tensor([0.6, 0.4], device="cuda")
    fold = lambda: eng._abi.check(L.bsms_grad_fold(acc.data_ptr(), g.data_ptr(), n, coef.data_ptr(), s), "bsms_grad_fold")
    accumulate = lambda: eng._abi.check(L.bsms_grad_accumulate(acc.data_ptr(), g.data_ptr(), n, 0, s), "bsms_grad_accumulate")
    res = {"fold": [], "accumulate": []}
    for _ in range(5):                                  # alternating blocks in one process
        acc.normal_()
        res["fold"].append(statistics.median(_timed(torch, fold, warmup, steps)))
        acc.normal_()
        res["accumulate"].append(statistics.median(_timed(torch, accumulate, warmup, steps)))
    print(json.dumps({"n": n, "fold_us": [1e3 * v for v in res["fold"]], "accumulate_us": [1e3 * v for v in res["accumulate"]]}))


def child_cycle(root, M, steps, warmup, batch):
    torch, eng, sim, data = _setup(root, batch)
    grads = eng.GradBuckets(list(sim.parameters()))
    b = batch // M
    node_in, tar, mask, m_gs, m_ids = data
    parts = [(node_in[i * b:(i + 1) * b], tar[i * b:(i + 1) * b], mask[i * b:(i + 1) * b], [g[:b] for g in m_gs], [i_[:b] for i_ in m_ids])
             for i in range(M)]
    step = eng.FusedStep(sim, grads, accumulate=M)

    def cycle():
        for d in parts:
            step(d, True)

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = _timed(torch, cycle, warmup, steps)
    arena = sum(t.numel() * t.element_size() for t in step._arena._t.values() if t is not None)
    scratch = sum(t.numel() * t.element_size() for t in (step._gscratch, step._gsum) if t is not None)
    loss = float(step.accumulated_loss()) if M > 1 else float("nan")
    print(json.dumps({"median_ms": statistics.median(ms), "arena_bytes": arena, "scratch_bytes": scratch,
                      "peak_over_base_bytes": torch.cuda.max_memory_allocated() - base, "accumulated_loss": loss}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "ROOT", "ARG"))
    args = ap.parse_args()
    if args.child:
        mode, root, arg = args.child
        if mode == "step":
            return child_step(root, arg, args.steps, args.warmup, args.batch)
        if mode == "fold":
            return child_fold(root, args.steps, args.warmup, args.batch)
        return child_cycle(root, int(arg), args.steps, args.warmup, args.batch)

    def run(mode, root, arg):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, root, str(arg), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--batch", str(args.batch)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        if out.returncode != 0:
            raise SystemExit(f"{mode} {root} {arg} failed ({out.returncode}):\n{out.stderr[-3000:]}")
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])

    roots = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this commit", ROOT)]
    steps = {(who, prec): [] for prec in ("f32", "bf16") for who, _ in roots}
    cycles = {M: [] for M in (1, 2, 4)}
    for rnd in range(args.rounds):
        for prec in ("f32", "bf16"):
            for who, root in roots:
                r = run("step", root, prec)
                steps[(who, prec)].append(r["median_ms"])
                print(f"round {rnd} step  {who:12s} {prec:5s} {r['median_ms']:.3f} ms/step  loss {r['loss']:.6f}", flush=True)
        for M in cycles:
            r = run("cycle", ROOT, M)
            cycles[M].append(r)
            print(f"round {rnd} cycle {M} x B = {args.batch // M}: {r['median_ms']:.3f} ms per {args.batch} samples, arena {r['arena_bytes'] / 2 ** 20:.1f} MiB", flush=True)
    fold = run("fold", ROOT, 0)
    med = statistics.median
    lines = ["# Gradient accumulation: profiles/accumulate_rates.py",
             f"# airfoil mesh (5233 nodes), eager; {args.steps} timed steps (cycles) per run after {args.warmup} warm-up, a fresh process per run,",
             f"# {args.rounds} rounds alternating the variants in one call on one MI355X.  Times are medians of per-step (per-cycle) HIP events.",
             "# No figure is a pass criterion of the feature.",
             "#", f"# 1. the plain step (accumulate = 1), B = {args.batch}",
             "# commit        precision  ms/step per round                 median"]
    for (who, prec), ms in steps.items():
        lines.append(f"  {who:12s}  {prec:9s}  {'  '.join(f'{m:.3f}' for m in ms):32s}  {med(ms):.3f}")
    if args.parent:
        for prec in ("f32", "bf16"):
            a, b = steps[("parent", prec)], steps[("this commit", prec)]
            lines.append(f"# {prec}: this commit against the parent {med(b) / med(a) - 1:+.2%} "
                         f"(spread between rounds: parent {max(a) / min(a) - 1:.2%}, this commit {max(b) / min(b) - 1:.2%})")
    else:
        lines.append("# parent: not measured (no --parent checkout given)")
    f_us, a_us = med(fold["fold_us"]), med(fold["accumulate_us"])
    lines += ["#", f"# 2. bsms_grad_fold against bsms_grad_accumulate, n = {fold['n']} floats ({4 * fold['n'] / 2 ** 20:.2f} MiB), one process, five alternating blocks",
              f"  bsms_grad_fold        {f_us:.2f} us per launch (blocks: {'  '.join(f'{v:.2f}' for v in fold['fold_us'])})",
              f"  bsms_grad_accumulate  {a_us:.2f} us per launch (blocks: {'  '.join(f'{v:.2f}' for v in fold['accumulate_us'])})",
              f"# ratio fold / accumulate: {f_us / a_us:.3f}",
              "#", f"# 3. one cycle against the one-shot step, fp32, {args.batch} samples",
              "# micro-batches   ms per 8 samples per round        median    arena MiB  scratch MiB  peak allocated over the model MiB"]
    one = med(r["median_ms"] for r in cycles[1])
    for M, rs in cycles.items():
        ms = [r["median_ms"] for r in rs]
        lines.append(f"  {M} x B = {args.batch // M:<9d} {'  '.join(f'{m:.3f}' for m in ms):32s}  {med(ms):.3f}    {rs[-1]['arena_bytes'] / 2 ** 20:8.1f}  {rs[-1]['scratch_bytes'] / 2 ** 20:8.1f}"
                     f"     {rs[-1]['peak_over_base_bytes'] / 2 ** 20:8.1f}")
    for M in (2, 4):
        t, a = med(r["median_ms"] for r in cycles[M]), cycles[M][-1]
        held, held1 = a["arena_bytes"] + a["scratch_bytes"], cycles[1][-1]["arena_bytes"] + cycles[1][-1]["scratch_bytes"]
        lines.append(f"# {M} x B = {args.batch // M}: {t / one - 1:+.1%} time for {1 - held / held1:.1%} fewer bytes held by the step")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
