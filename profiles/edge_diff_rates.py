#!/usr/bin/env python3
"""Edge-difference sums: what the two entries cost next to bsms_error_sums on the same rows, and what
`rollout_bank(edge_errors=)` adds to a rollout evaluation.

  (1) bsms_edge_diff_sums ("difference" and "quotient"), bsms_edge_diff_bwd and bsms_error_sums alone, alternated in one process,
      on the level-0 graph of the bench workload's airfoil mesh (5233 rows, C = 4, p = 2) with S = 8 (a batch) and S = 600 (the time
      steps of a trajectory), and of its surface mesh (16384 rows, p = 3) with S = 8.  A window is `--calls` calls between two device
      events; the figure is microseconds per call (median [min .. max] over the repeats).
  (2) For S = 600 the bytes the sums kernel has to move at least -- pred, target, mask and positions once, the index arrays once
      (they are shared by the segments) -- over the time, against the HBM peak of 8.0 TB/s.
  (3) rollout_bank(batch=8) over 8 trajectories on the airfoil mesh with and without `edge_errors`, alternated, trajectory-steps/s.

  python profiles/edge_diff_rates.py --out profiles/edge_diff_rates.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bsms_gnn_amd as eng

HBM_PEAK = 8.0e12      # bytes/s, specification


def level0(kind):
    """(edge list [2, E] int64, positions [N, p] float32) of the bench workload's mesh."""
    import bench
    from bsms_gnn_amd.hierarchy import to_flat_edge
    pts, cells = bench.mesh_points(kind, None)
    return torch.tensor(np.asarray(to_flat_edge(cells, "tri")), dtype=torch.int64), torch.tensor(pts, dtype=torch.float32)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def entries(kind, S, C, args, lines):
    g, pos = level0(kind)
    N, E, p = pos.shape[0], g.shape[1], pos.shape[1]
    plan = eng.graph.plan_for(g.cuda(), N)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pred, tar = torch.randn(S, N, C, device="cuda", generator=gen), torch.randn(S, N, C, device="cuda", generator=gen)
    mask, dpos = (torch.rand(N, device="cuda", generator=gen) < 0.9).float(), pos.cuda()
    coef = torch.rand(S, C, device="cuda", dtype=torch.float64)
    grad = torch.empty(S, N, C, device="cuda")
    runs = {"error_sums": lambda: eng.error_sums(pred, tar, mask, N, mask_stride=0),
            "edge_diff_sums difference": lambda: eng.edge_diff_sums(pred, tar, mask, plan, mask_stride=0),
            "edge_diff_sums quotient": lambda: eng.edge_diff_sums(pred, tar, mask, plan, pos=dpos, weighting="quotient", mask_stride=0, pos_stride=0),
            "edge_diff_bwd difference": lambda: eng.edge_diff_bwd(pred, tar, mask, plan, coef, mask_stride=0),
            "edge_diff_bwd quotient": lambda: eng.edge_diff_bwd(pred, tar, mask, plan, coef, pos=dpos, weighting="quotient", mask_stride=0, pos_stride=0)}
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    got = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            got[k].append(timed(run, args.calls))
    lines.append(f"  {kind}: N = {N}, E = {E}, C = {C}, p = {p}, S = {S}   (us per call, host wrapper included)")
    for k, v in got.items():
        lines.append(f"    {k:28s} {statistics.median(v):9.1f}  [{min(v):9.1f} .. {max(v):9.1f}]")
    if S >= 100:
        for k, extra in (("edge_diff_sums difference", 0), ("edge_diff_sums quotient", N * p * 4)):
            least = S * N * (2 * C) * 4 + N * 4 + extra + (N + 1 + E) * 4        # pred + target, one mask, positions, rowptr + src
            t = statistics.median(got[k]) * 1e-6
            lines.append(f"    {k}: at least {least / 1e6:.1f} MB in {t * 1e6:.1f} us = {least / t / 1e12:.3f} TB/s = {least / t / HBM_PEAK:.3f} of the HBM peak; the "
                         f"neighbour rows ({S * E * 2 * C * 4 / 1e6:.1f} MB of gathers, served by the caches) and E / N = {E / N:.1f} dependent index -> row loads per "
                         "row come on top")


def rollouts(args, lines):
    from databank_rates import data_cfg, make_trainer, trajectory
    n_traj = 8
    tr = make_trainer("airfoil", True)
    bank = eng.TrajectoryBank(data_cfg("airfoil", True), dataset="airfoil", seed=0)
    for s in range(n_traj):
        bank.add(trajectory("airfoil", args.frames, s))
    tr.iter(bank.sample(n_traj, train=False))
    steps = n_traj * (args.frames - 1)
    runs = {"without edge_errors": lambda: eng.rollout_bank(tr, bank, batch=n_traj),
            "with edge_errors": lambda: eng.rollout_bank(tr, bank, batch=n_traj, edge_errors=eng.RolloutErrors(bank.device)),
            "with edge_errors, quotient": lambda: eng.rollout_bank(tr, bank, batch=n_traj, edge_errors=eng.RolloutErrors(bank.device), edge_weighting="quotient")}
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    got = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            got[k].append(steps / (time.perf_counter() - t0))
    lines.append(f"  rollout_bank(batch=8): {n_traj} trajectories of {args.frames - 1} steps on the 5233-node airfoil mesh, fp32, eager (trajectory-steps/s)")
    for k, v in got.items():
        lines.append(f"    {k:28s} {statistics.median(v):9.1f}  [{min(v):9.1f} .. {max(v):9.1f}]")


def main(args):
    lines = [f"# python profiles/edge_diff_rates.py --calls {args.calls} --repeats {args.repeats} --frames {args.frames}   ({torch.cuda.get_device_name(0)})",
             "# median [min .. max] over the repeats; the runs of a block alternate in one process"]
    entries("airfoil", 8, 4, args, lines)
    entries("airfoil", 600, 4, args, lines)
    entries("surface", 8, 4, args, lines)
    if not args.no_rollout:
        rollouts(args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edge_diff_rates.py measures on the GPU; none found")
    torch.set_num_threads(max(1, min(8, eng.trainer.usable_cpus())))
    main(args)
