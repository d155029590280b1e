"""Time of one optimizer call at the two production sizes: the airfoil model (n = 1 917 827) and the surface model
(the 35.8 MB gradient), parameter layout and per-tensor groups taken from the real models.

Variants, alternated round by round in ONE process, each timed with HIP events around CALLS in-order launches on one stream:
  adamw        bsms_adamw_step as Trainer calls it (clip 1.0, norm out): k_sumsq_partials + k_adamw
  degenerate   bsms_optim_step with groups = ema = counters = NULL: k_sumsq_partials + k_optim
  groups       + one group per parameter tensor, weight_decay 0 on the 1-D ones (no_decay_bias), lr_scale 0.1 on the processor
  groups+ema   + the moving average (9 streams instead of 7)
  all          + the non-finite guard (k_optim_commit behind the update, step number from the device counter)

Usage (on an MI355X):  python profiles/optim_rates.py [--calls 300] [--rounds 5] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (WORKLOADS, make_cfg: the model shapes of the benchmark lines)
import bsms_gnn_amd as eng  # noqa: E402

HP = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, max_norm=1.0)


def layout(kind):
    """(n, per-tensor rows) of a workload's model: GradBuckets order, no_decay_bias, the processor at a tenth of the rate."""
    model = eng.BSMS_Simulator(bench.make_cfg(bench.WORKLOADS[kind]))
    buckets = eng.GradBuckets(model.parameters())
    name_of = {p: k for k, p in model.named_parameters()}
    rows = []
    for p in sorted(buckets.params, key=lambda q: buckets._slot[q][0]):
        off, cnt = buckets._slot[p]
        rows.append((off, cnt, 0.1 if name_of[p].startswith("process.") else 1.0, 0.0 if p.dim() == 1 else HP["wd"]))
    merged = eng.segment_table(buckets, eng.param_groups(model, no_decay_bias=True, lr_scales={"process": 0.1}), HP["wd"])
    return buckets.flat.numel(), rows, len(merged)


class Problem:
    def __init__(self, n, rows):
        L = self.L = eng._abi.lib()
        gen = torch.Generator(device="cuda").manual_seed(0)
        self.n = n
        self.p = torch.randn(n, device="cuda", generator=gen)
        self.g = torch.randn(n, device="cuda", generator=gen) * 1e-3
        self.m, self.v, self.ema = torch.zeros_like(self.p), torch.zeros_like(self.p), self.p.clone()
        self.norm = torch.zeros(1, device="cuda")
        self.counters = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.work = torch.empty(int(L.bsms_optim_work_bytes()), dtype=torch.uint8, device="cuda")
        G = eng._abi.OptimGroup
        arr = (G * len(rows))(*[G(*r) for r in rows])
        self.handle = C.c_void_p()
        eng._abi.check(L.bsms_optim_groups_create(C.cast(arr, C.c_void_p), len(rows), n, C.cast(C.byref(self.handle), eng._abi.PP)), "groups_create")
        self.steps = 0

    def call(self, variant):
        L, s = self.L, torch.cuda.current_stream().cuda_stream
        ptrs = (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n)
        self.steps += 1
        if variant == "adamw":
            rc = L.bsms_adamw_step(*ptrs, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], self.steps, HP["max_norm"],
                                   self.norm.data_ptr(), self.work.data_ptr(), s)
        else:
            groups = self.handle if variant != "degenerate" else None
            ema = self.ema.data_ptr() if variant in ("groups+ema", "all") else None
            guard = variant == "all"
            rc = L.bsms_optim_step(*ptrs, groups, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], 0 if guard else self.steps,
                                   HP["max_norm"], ema, 0.999, self.counters.data_ptr() if guard else None, self.norm.data_ptr(),
                                   self.work.data_ptr(), s)
        eng._abi.check(rc, variant)

    def close(self):
        self.L.bsms_optim_groups_destroy(self.handle)


VARIANTS = ["adamw", "degenerate", "groups", "groups+ema", "all"]
STREAMS = {"adamw": 7, "degenerate": 7, "groups": 7, "groups+ema": 9, "all": 9}     # 4-byte streams per element, the norm's read of g not counted


def measure(kind, calls, rounds, say):
    n, rows, nmerged = layout(kind)
    prob = Problem(n, rows)
    say(f"\n## {kind}: n = {n} ({4 * n / 1e6:.1f} MB per stream), {len(rows)} parameter tensors = groups ({nmerged} segments once equal neighbours are merged)")
    for v in VARIANTS:                       # warm-up: code objects, the group table in cache
        for _ in range(20):
            prob.call(v)
    torch.cuda.synchronize()
    times = {v: [] for v in VARIANTS}
    for _ in range(rounds):
        for v in VARIANTS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                prob.call(v)
            t1.record()
            t1.synchronize()
            times[v].append(t0.elapsed_time(t1) * 1e3 / calls)
    assert bool(torch.isfinite(prob.p).all()) and int(prob.counters[1]) == 0
    say(f"  {'variant':<12} us per call, {rounds} rounds of {calls} calls" + " " * 22 + "median   min      GB/s at the median (streams x 4n bytes)")
    base = statistics.median(times["adamw"])
    for v in VARIANTS:
        med = statistics.median(times[v])
        say(f"  {v:<12} " + "  ".join(f"{t:7.2f}" for t in times[v]) + f"   {med:7.2f}  {min(times[v]):7.2f}   {STREAMS[v] * 4 * n / med / 1e3:7.0f}"
            + ("" if v == "adamw" else f"   ({(med / base - 1) * 100:+.1f} % against adamw)"))
    prob.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/optim_rates.py measures on the GPU; none found")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}; HIP events around {args.calls} in-order calls, variants alternated, {args.rounds} rounds, one process")
    for kind in ("airfoil", "surface"):
        measure(kind, args.calls, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
