#!/usr/bin/env python3
"""Rollout evaluation from the device-resident trajectory bank: trajectory-steps per second (one step of ONE trajectory counts one,
so a batched step of 8 counts 8) of
  (D)  rollout_dataset(trainer, bank.rollouts())   -- one trajectory at a time, [T-1,...] copies materialised per trajectory,
                                                      statistics as ~15 torch reductions per trajectory
  (B1) rollout_bank(trainer, bank, batch=1)        -- one at a time, targets read in place, statistics from bsms_error_sums
  (B8) rollout_bank(trainer, bank, batch=8)        -- eight trajectories advanced together
on an airfoil-size bank (8 synthetic trajectories on the bench workload's 5233-node mesh; the generator of
tests/test_hip_databank.py: airfoil_traj), fp32, eager steps.  The three alternate in one process; every window is a full pass over the
bank and ends in a device synchronise.

  python profiles/eval_rates.py --out profiles/eval_rates.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bsms_gnn_amd as eng
from databank_rates import data_cfg, make_trainer, trajectory

N_TRAJ = 8


def main(args):
    tr = make_trainer("airfoil", True)
    bank = eng.TrajectoryBank(data_cfg("airfoil", True), dataset="airfoil", seed=0)
    for s in range(N_TRAJ):
        bank.add(trajectory("airfoil", args.frames, s))
    tr.iter(bank.sample(N_TRAJ, train=False))          # warm-up step: normaliser statistics
    steps = N_TRAJ * (args.frames - 1)
    runs = {"D": lambda: eng.rollout_dataset(tr, bank.rollouts()),
            "B1": lambda: eng.rollout_bank(tr, bank, batch=1),
            "B8": lambda: eng.rollout_bank(tr, bank, batch=N_TRAJ)}
    summaries = {}
    for k, run in runs.items():                        # warm every shape the timed windows use
        summaries[k] = run().summary()
    torch.cuda.synchronize()
    got = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            got[k].append(steps / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in got.items()}
    worst = max(float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) for k in ("B1", "B8") for name in ("all", "channel", "time")
                for a, b in zip(summaries[k][name], summaries["D"][name]))
    lines = [f"# python profiles/eval_rates.py --frames {args.frames} --repeats {args.repeats}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.get_num_threads()} host threads)",
             f"# trajectory-steps/s over {N_TRAJ} trajectories of {args.frames - 1} steps on the 5233-node airfoil mesh, fp32, eager; median [min .. max] over "
             "the repeats; windows alternate D B1 B8"]
    for k in runs:
        lines.append(f"  {k:2s} {med[k]:8.1f} steps/s  [{min(got[k]):8.1f} .. {max(got[k]):8.1f}]" + ("" if k == "D" else f"   {k}/D = {med[k] / med['D']:.2f}"))
    lines.append(f"  spread of D (max - min over median): {100 * (max(got['D']) - min(got['D'])) / med['D']:.1f} %")
    lines.append(f"  worst relative difference of the B1 / B8 summaries from D's: {worst:.1e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_rates.py measures on the GPU; none found")
    torch.set_num_threads(max(1, min(8, eng.trainer.usable_cpus())))
    main(args)
