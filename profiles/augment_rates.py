#!/usr/bin/env python3
"""Frame augmentation in the data path: airfoil (5233 nodes, consistent mesh), B = 8, training noise on, three routes alternated
in one process:
  (P) `bsms_batch_assemble`      -- TrajectoryBank without augmentation: what the parent commit runs, call for call
  (X) `bsms_batch_assemble_xf`   -- TrajectoryBank(augment=Augment(reflect=True)): matrices drawn on the host, one launch
  (T) (P) + torch ops            -- what a user would do without the feature: the same matrices uploaded, then einsum on the
                                    velocity columns of node_in and node_tar and on the position columns, written back
  (E) the entry of (X) alone      -- assembly figure only: fixed matrices handed in as `transforms=`, so the difference X - E is
                                    the host's `Augment.sample` (a NumPy generator seeded per batch) and E - P the entry itself
Two figures per route: the assembly alone (microseconds per batch, host clock around a window that ends in a synchronise) and
the training step fed by it (steps/s of `trainer.iter`, optimizer on).  The step of (P) IS the parent's step: without an
`augment` the bank makes exactly the calls it made before the feature.

  python profiles/augment_rates.py --out profiles/augment_rates.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bsms_gnn_amd as eng
from databank_rates import B, data_cfg, make_trainer, trajectory

AUG = eng.Augment(reflect=True)


class Routes:
    def __init__(self, frames):
        dcfg = data_cfg("airfoil", True)
        self.tr = make_trainer("airfoil", True)
        self.plain = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=0)
        self.aug = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=0, augment=AUG)
        for s in range(4):
            traj = trajectory("airfoil", frames, s)
            self.plain.add(traj), self.aug.add(traj)
        self.tr.iter(self.plain.sample(B))                 # warm-up step: normaliser statistics
        self.draw = 0
        self.fixed = AUG.sample(2, B, 0, 0)

    def picks(self, bank):
        picks = bank.next_picks(B)
        return picks if len(picks) == B else bank.next_picks(B)

    def P(self):
        return self.plain.batch(self.picks(self.plain))

    def X(self):
        return self.aug.batch(self.picks(self.aug))

    def E(self):
        return self.plain.batch(self.picks(self.plain), transforms=self.fixed)

    def T(self):
        self.draw += 1
        batch = self.plain.batch(self.picks(self.plain), draw=self.draw)
        q = torch.from_numpy(AUG.sample(2, B, self.plain.seed, self.draw)).to(batch[0].device, non_blocking=True)
        node_in, node_tar = batch[0], batch[1]
        node_in[..., 0:2] = torch.einsum("bij,bnj->bni", q, node_in[..., 0:2])
        node_in[..., 3:5] = torch.einsum("bij,bnj->bni", q, node_in[..., 3:5])
        node_tar[..., 0:2] = torch.einsum("bij,bnj->bni", q, node_tar[..., 0:2])
        return batch

    def assembly_us(self, route, calls):
        fn = getattr(self, route)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    def steps_per_s(self, route, steps):
        fn = getattr(self, route)
        for _ in range(10):
            self.tr.iter(fn())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.tr.iter(fn())
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)


def main(args):
    r = Routes(args.frames)
    kinds = ["P", "X", "T"]
    asm, step = {k: [] for k in ["P", "X", "E", "T"]}, {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k in asm:
            asm[k].append(r.assembly_us(k, args.calls))
    for _ in range(args.repeats):
        for k in kinds:
            step[k].append(r.steps_per_s(k, args.steps))
    n, c, p = r.plain._trajs[0].N, 3, 2
    row = 4 * ((2 * c + p + 1) + (c + p + 1) + c + 1)      # read state_t, state_t+1, pos, type; write node_in, node_tar, mask
    lines = [f"# python profiles/augment_rates.py --calls {args.calls} --steps {args.steps} --repeats {args.repeats}   "
             f"({torch.cuda.get_device_name(0)}, {torch.get_num_threads()} host threads)",
             f"# airfoil, B = {B}, {n} nodes, noise on; median [min .. max] over the repeats; windows alternate P X (E) T",
             f"# bytes per batch from shapes: {B} x {n} rows x {row} B = {B * n * row / 1e6:.2f} MB for P and for X alike (the matrices are kernel arguments)",
             "assembly alone, microseconds per batch (host clock, window ends in a synchronise):"]
    med = {k: statistics.median(v) for k, v in asm.items()}
    for k in asm:
        lines.append(f"  {k}  {med[k]:8.1f} us  [{min(asm[k]):8.1f} .. {max(asm[k]):8.1f}]" + ("" if k == "P" else f"   {k}/P = {med[k] / med['P']:.2f}"))
    lines.append("training step fed by each route, steps/s of trainer.iter (optimizer on); P is the parent commit's step:")
    med = {k: statistics.median(v) for k, v in step.items()}
    for k in kinds:
        lines.append(f"  {k}  {med[k]:8.1f} steps/s  [{min(step[k]):8.1f} .. {max(step[k]):8.1f}]" + ("" if k == "P" else f"   {k}/P = {med[k] / med['P']:.3f}"))
    lines.append(f"  spread of P (max - min over median): {100 * (max(step['P']) - min(step['P'])) / med['P']:.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_rates.py measures on the GPU; none found")
    torch.set_num_threads(max(1, min(8, eng.trainer.usable_cpus())))
    main(args)
