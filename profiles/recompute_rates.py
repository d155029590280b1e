"""What activation recomputation in the U-Net backward costs and saves:

  a  flag off against the parent commit: bench.py (default workload, --dump-outputs) in a built checkout of the parent and in this one,
     alternating in one call -- the dumped loss / prediction / gradients compared byte for byte, the rates next to the spread between
     two runs of the same commit;
  b  flag on against flag off in ONE process: the fused step on the airfoil workload of bench.py at B = 8, fp32 and bf16, unroll = 1 and
     unroll = 4, in alternating blocks; and the stand-alone training forward of the U-Net, which is what a backward re-runs;
  c  the bytes the step holds (FusedStep.held_bytes: capacities of its buffers, no allocator statistics) at the airfoil B = 8 and the
     surface B = 2 shapes, flag off and on.  K = 1 and K = 2 are allocated and read; K = 4 and K = 16 follow from
     shared + first step + (K - 1) x per_step, which tests/test_hip_recompute.py::test_held_bytes pins.

    python profiles/recompute_rates.py [--parent DIR] [--rounds 3] [--out profiles/recompute_rates.txt]

Every part runs in fresh child processes; steps are bracketed by HIP events on the launching stream and the median is reported."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MIB = float(1 << 20)


def _setup(workload, batch, precision="f32"):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import bsms_gnn_amd as eng
    wl = bench.build_workload(workload, batch, "cuda", seed=0)
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
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))


def _later(torch, data, K):
    state, tar = data[0][..., :data[1].shape[-1]], data[1]
    return torch.stack([state + (k + 1) * (tar - state) for k in range(1, K)]) if K > 1 else None


def child_cost(precision, steps, warmup, batch):
    torch, eng, sim, data = _setup("airfoil", batch, precision)
    grads = eng.GradBuckets(list(sim.parameters()))
    out = {"precision": precision}
    for K in (1, 4):
        later = _later(torch, data, K)
        pair = {flag: eng.FusedStep(sim, grads, unroll=K, recompute=flag) for flag in (False, True)}
        ms = {False: [], True: []}
        for _ in range(3):                                    # alternating blocks in one process
            for flag, step in pair.items():
                ms[flag].append(_timed(torch, lambda: step(data, True, later), warmup, steps // K))
        out[f"unroll{K}"] = {"off_ms": ms[False], "on_ms": ms[True]}
        del pair
        torch.cuda.empty_cache()
    # the U-Net's training forward alone: what every backward runs once more, block by block
    node_in = data[0]
    C, p = sim.cfg.out_dim, sim.pos_dim
    h = torch.randn(batch, node_in.shape[1], sim.cfg.latent_dim, device="cuda").requires_grad_(True)
    pos = node_in[..., C:C + p].contiguous()
    m_gs, m_ids = [g[0] for g in data[3]], [i[0] for i in data[4]]
    for name, flag in (("full", False), ("lean", True)):
        sim.process.recompute = flag
        out[f"unet_forward_{name}_ms"] = _timed(torch, lambda: sim.process(h, m_ids, m_gs, pos), warmup, steps)
    sim.process.recompute = False
    out["blocks"] = 2 * sim.cfg.unet_depth + 1
    print(json.dumps(out))


def child_memory(workload, batch):
    torch, eng, sim, data = _setup(workload, batch)
    grads = eng.GradBuckets(list(sim.parameters()))
    out = {"workload": workload, "batch": batch}
    for flag in (False, True):
        for K in (1, 2):
            step = eng.FusedStep(sim, grads, unroll=K, recompute=flag)
            step(data, True, _later(torch, data, K))
            torch.cuda.synchronize()
            held = step.held_bytes()
            held["total"] = sum(t.numel() * t.element_size() for t in step._arena._t.values() if t is not None)
            out[f"{'on' if flag else 'off'}{K}"] = held
            del step
            torch.cuda.empty_cache()
    print(json.dumps(out))


def run_child(mode, *rest, steps, warmup, batch):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, *map(str, rest), "--steps", str(steps), "--warmup", str(warmup), "--batch", str(batch)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"{mode} {rest} failed ({out.returncode}):\n{out.stderr[-3000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def run_bench(root, steps, warmup, dump):
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    if out.returncode != 0:
        raise SystemExit(f"bench.py in {root} failed ({out.returncode}):\n{out.stderr[-3000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def same_dumps(a, b):
    names = sorted(os.listdir(a))
    if names != sorted(os.listdir(b)) or not names:
        return False, len(names)
    return all(open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read() for n in names), len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+")
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "cost":
            return child_cost(args.child[1], args.steps, args.warmup, args.batch)
        return child_memory(args.child[1], int(args.child[2]))
    kw = dict(steps=args.steps, warmup=args.warmup, batch=args.batch)
    med = statistics.median
    lines = ["# Activation recomputation in the U-Net backward: profiles/recompute_rates.py",
             f"# one MI355X, eager; medians of per-step HIP events, {args.steps} timed steps after {args.warmup} warm-up unless stated.",
             "# No figure is a pass criterion of the feature."]

    if "a" in args.parts:
        lines += ["#", "# a. flag off against the parent: bench.py --gpus 1 (airfoil, B = 8, fp32), alternating, a fresh process per run"]
        if not args.parent:
            lines.append("# parent: not measured (no --parent checkout given)")
        else:
            roots = [("parent", os.path.abspath(args.parent)), ("this commit", ROOT)]
            rate = {who: [] for who, _ in roots}
            equal = []
            with tempfile.TemporaryDirectory() as tmp:
                for rnd in range(args.rounds):
                    for who, root in roots:
                        r = run_bench(root, args.steps, args.warmup, os.path.join(tmp, f"{who[:4]}{rnd}"))
                        rate[who].append(r["value"])
                        print(f"round {rnd} {who:12s} {r['value']:.2f} steps/s", flush=True)
                    equal.append(same_dumps(os.path.join(tmp, f"pare{rnd}"), os.path.join(tmp, f"this{rnd}")))
            lines.append("# commit        steps/s per round                 median")
            for who, v in rate.items():
                lines.append(f"  {who:12s}  {'  '.join(f'{x:.2f}' for x in v):32s}  {med(v):.2f}")
            a, b = rate["parent"], rate["this commit"]
            lines.append(f"# this commit against the parent {med(b) / med(a) - 1:+.2%} (spread between rounds: parent {max(a) / min(a) - 1:.2%}, "
                         f"this commit {max(b) / min(b) - 1:.2%})")
            lines.append(f"# --dump-outputs, {equal[0][1]} arrays (loss, prediction, every parameter gradient): "
                         + ("byte-identical to the parent's in every round" if all(e for e, _ in equal) else f"DIFFER from the parent's: {equal}"))

    if "b" in args.parts:
        lines += ["#", f"# b. flag on against flag off, one process per precision, airfoil B = {args.batch}: three alternating blocks per variant,",
                  "#    ms per CALL (unroll = 4: one call is four forwards and four backwards, timed over a quarter of the steps)",
                  "# precision  unroll  off: blocks            median    on: blocks             median    extra ms  extra"]
        for prec in ("f32", "bf16"):
            r = run_child("cost", prec, **kw)
            for K in (1, 4):
                off, on = r[f"unroll{K}"]["off_ms"], r[f"unroll{K}"]["on_ms"]
                lines.append(f"  {prec:9s}  {K:<6d}  {'  '.join(f'{x:.3f}' for x in off):22s} {med(off):7.3f}    {'  '.join(f'{x:.3f}' for x in on):22s} {med(on):7.3f}"
                             f"    {med(on) - med(off):7.3f}  {med(on) / med(off) - 1:+.1%}")
            full, lean = r["unet_forward_full_ms"], r["unet_forward_lean_ms"]
            extra1 = med(r["unroll1"]["on_ms"]) - med(r["unroll1"]["off_ms"])
            lines.append(f"# {prec}: the U-Net's training forward alone (one-call autograd node, its own prepacks): full {full:.3f} ms, lean {lean:.3f} ms; "
                         f"the flag's extra time per step at unroll = 1 is {extra1 / full:.2f} of the full one ({r['blocks']} blocks, each re-run with its prepack)")

    if "c" in args.parts:
        lines += ["#", "# c. bytes held by the step (FusedStep.held_bytes), MiB; K = 1, 2 allocated, K = 4, 16 = shared + first step + (K - 1) x per_step",
                  "# shape          flag  per_step     shared     K = 1       K = 4      K = 16"]
        for workload, batch in (("airfoil", 8), ("surface", 2)):
            r = run_child("memory", workload, batch, **kw)
            tot = {}
            for flag in ("off", "on"):
                h1, h2 = r[f"{flag}1"], r[f"{flag}2"]
                first = h2["total"] - h2["shared"] - h2["per_step"]
                tot[flag] = {K: h2["shared"] + first + (K - 1) * h2["per_step"] for K in (1, 4, 16)}
                assert tot[flag][1] == h1["total"] or h1["shared"] != h2["shared"], (h1, h2)
                lines.append(f"  {workload + ' B = ' + str(batch):13s}  {flag:4s}  {h2['per_step'] / MIB:9.1f}  {h2['shared'] / MIB:9.1f}  {h1['total'] / MIB:9.1f}  "
                             f"{tot[flag][4] / MIB:10.1f}  {tot[flag][16] / MIB:10.1f}")
            lines.append(f"# {workload}: per unrolled step {r['off2']['per_step'] / r['on2']['per_step']:.1f}x fewer bytes; K = 16 holds "
                         f"{tot['on'][16] / 2 ** 30:.1f} GiB instead of {tot['off'][16] / 2 ** 30:.1f} GiB")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
