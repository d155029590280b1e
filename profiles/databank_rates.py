#!/usr/bin/env python3
"""Feeding the trainer: steps/s of `trainer.iter` (optimizer on, B = 8) with three sources of batches, alternated in one process:
  (A) one cached device batch replayed                       -- the ceiling
  (B) `TrajectoryBank.sample(8)` (training noise on)         -- batches assembled on the GPU from resident trajectories
  (C) the host route: datapipe.TrajectoryDataset -> make_loader -> trainer.DevicePrefetcher (training noise on)
  (C2, variable meshes only) TrajectoryDataset samples -> Trainer.collate
for airfoil fp32, airfoil bf16 (consistent mesh, 5233 nodes) and cylinder (8 different meshes of 1885 nodes, variable-mesh path).
Trajectories are synthetic fields on the bench workloads' meshes.  The consistent-mesh dataset reads in-memory dicts with a cached
hierarchy; the variable-mesh dataset reads .npz files from a temporary directory (page cache), because datapipe names the
hierarchy cache of a variable-mesh trajectory after its file.

  python profiles/databank_rates.py                      rates (the table of profiles/databank_rates.txt)
  python profiles/databank_rates.py --mode kernels       a few training batches + one 601-frame rollout trajectory: run under
                                                         `rocprofv3 --kernel-trace --stats` for the time of k_batch_assemble
  python profiles/databank_rates.py --mode copies --steps N   N steady-state `sample(8)` calls after the set-up: run under
                                                         `rocprofv3 --memory-copy-trace` with N = 0 and N = 200; equal host-to-device
                                                         copy counts mean the steady state issues none
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import bsms_gnn_amd as eng
import bsms_gnn_amd.datapipe as dp

B = 8
OPT = SimpleNamespace(peak_lr=1e-4, weight_decay=1e-2, warmup_steps=10, decay_steps=100000, gnorm_clip=1.0)


def trajectory(kind, T, seed, mesh_seed=None):
    w = bench.WORKLOADS[kind]
    pts, cells = bench.mesh_points(kind, mesh_seed)
    n, rng = w["nodes"], np.random.default_rng(seed)
    out = {"cells": np.repeat(cells[None], T, 0), "mesh_pos": np.repeat(pts.astype(np.float32)[None], T, 0),
           "node_type": np.repeat(rng.choice((0, 0, 0, 4, 5), (1, n, 1)).astype(np.float32), T, 0),
           "velocity": rng.standard_normal((T, n, 2)).astype(np.float32)}
    if w["out_dim"] == 3:
        out["density"] = rng.standard_normal((T, n, 1)).astype(np.float32)
    return out


def data_cfg(kind, consistent):
    w = bench.WORKLOADS[kind]
    outs = ["velocity", "density"] if w["out_dim"] == 3 else ["velocity"]
    return SimpleNamespace(field_names=["node_type", "cells", "mesh_pos", *outs], output_field_names=outs, mesh_type="tri",
                           unet_depth=w["levels"], consist_mesh=consistent, noise_level=[10, 10, 0.01] if w["out_dim"] == 3 else [0.02, 0.02],
                           noise_gamma=0.8)


def make_trainer(kind, consistent):
    mcfg = bench.make_cfg(bench.WORKLOADS[kind])
    mcfg.consistent_mesh, mcfg.accumulation_steps = consistent, 1
    torch.manual_seed(0)
    return eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)


class Variant:
    def __init__(self, name, kind, consistent, precision, frames, tmp):
        self.name, self.consistent = name, consistent
        self.dcfg = data_cfg(kind, consistent)
        self.dataset = "airfoil" if kind == "airfoil" else "cylinder_flow"
        if consistent:
            self.sources = [trajectory(kind, frames, s) for s in range(4)]
            self.cache_dir = os.path.join(tmp, name)
            os.makedirs(self.cache_dir)
        else:
            self.sources, self.cache_dir = [], None
            os.makedirs(os.path.join(tmp, name))
            for s in range(B):
                path = os.path.join(tmp, name, f"traj{s}.npz")
                np.savez(path, **trajectory(kind, frames, s, mesh_seed=s))
                self.sources.append(path)
        self.tr = make_trainer(kind, consistent)
        # same seed and the default order on both routes: B and C train on the same sequence of picks
        self.bank = eng.TrajectoryBank(self.dcfg, dataset=self.dataset, seed=0, process=self.tr.model.process, cache_dir=self.cache_dir)
        for s in self.sources:
            self.bank.add(s)
        self.cached = self.bank.sample(B)
        self.tr.iter(self.cached)                      # warm-up step: normaliser statistics
        self.tr.model.process.precision = precision
        self._host = self._host2 = None

    def host_batches(self):
        while True:
            ds = dp.TrajectoryDataset(self.dcfg, self.sources, dataset=self.dataset, mode="train", seed=0, cache_dir=self.cache_dir)
            for batch in eng.DevicePrefetcher(dp.make_loader(ds, B), self.tr):
                if not self.consistent or batch[0].shape[0] == B:      # (the epoch length is a multiple of B here anyway)
                    yield batch

    def host_collated(self):
        while True:
            ds = dp.TrajectoryDataset(self.dcfg, self.sources, dataset=self.dataset, mode="train", seed=0, cache_dir=self.cache_dir)
            group = []
            for sample in ds:
                group.append(sample)
                if len(group) == B:
                    yield self.tr.collate(group)
                    group = []

    def bank_batch(self):
        picks = self.bank.next_picks(B)
        if len(picks) < B:                             # tail of an epoch: take the head of the next one instead
            picks = self.bank.next_picks(B)
        return self.bank.batch(picks)

    def close(self):
        for g in (self._host, self._host2):
            if g is not None:
                g.close()

    def window(self, which, steps):
        if which == "A":
            nxt = lambda: self.cached
        elif which == "B":
            nxt = self.bank_batch
        elif which == "C":
            self._host = self._host or self.host_batches()
            nxt = lambda: next(self._host)
        else:
            self._host2 = self._host2 or self.host_collated()
            nxt = lambda: next(self._host2)
        for _ in range(10):
            self.tr.iter(nxt())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.tr.iter(nxt())
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)


def rates(args):
    lines = [f"# python profiles/databank_rates.py --steps {args.steps} --repeats {args.repeats}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.get_num_threads()} host threads)", "# steps/s of trainer.iter (optimizer on), B = 8; median [min .. max] over the repeats; windows alternate A B C (C2)"]
    with tempfile.TemporaryDirectory() as tmp:
        for name, kind, consistent, precision in (("airfoil_f32", "airfoil", True, "f32"), ("airfoil_bf16", "airfoil", True, "bf16"),
                                                  ("cylinder_variable", "cylinder", False, "f32")):
            v = Variant(name, kind, consistent, precision, args.frames, tmp)
            kinds = ["A", "B", "C"] + ([] if consistent else ["C2"])
            got = {k: [] for k in kinds}
            for _ in range(args.repeats):
                for k in kinds:
                    got[k].append(v.window(k, args.steps))
            med = {k: statistics.median(r) for k, r in got.items()}
            spread = (max(got["A"]) - min(got["A"])) / med["A"]
            lines.append(f"{name}: resident {v.bank.bytes_resident / 1e6:.1f} MB in {len(v.bank)} trajectories")
            for k in kinds:
                lines.append(f"  {k:2s} {med[k]:8.1f} steps/s  [{min(got[k]):8.1f} .. {max(got[k]):8.1f}]" + ("" if k == "A" else f"   {k}/A = {med[k] / med['A']:.3f}"))
            lines.append(f"  spread of A (max - min over median): {100 * spread:.1f} %")
            v.close()
            del v
            torch.cuda.synchronize()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


def kernels(args):
    """Under rocprofv3 --kernel-trace --stats: 50 training batches (B = 8, noise on) and 3 full 601-frame trajectories."""
    dcfg = data_cfg("airfoil", True)
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=0)
    bank.add(trajectory("airfoil", 601, 0))
    n, c, p = bench.WORKLOADS["airfoil"]["nodes"], 3, 2
    row_train = 4 * ((2 * c + p + 1) + (c + p + 1) + c + 1)          # read state_t, state_t+1, pos, type; write node_in, node_tar, mask
    for _ in range(50):
        bank.sample(B)
    torch.cuda.synchronize()
    for _ in range(3):
        bank.trajectory(0)
        torch.cuda.synchronize()
    print(f"bytes moved per launch (from shapes): training batch {B * n * row_train / 1e6:.2f} MB in 1 launch; "
          f"trajectory {600 * n * row_train / 1e6:.1f} MB in {-(-600 // 64)} launches (64 samples each, the last {600 % 64})")


def copies(args):
    dcfg = data_cfg("airfoil", True)
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=0)
    for s in range(2):
        bank.add(trajectory("airfoil", 129, s))
    bank.sample(B)
    torch.cuda.synchronize()
    for _ in range(args.steps):
        bank.sample(B)
    torch.cuda.synchronize()
    print(f"set-up + {args.steps} steady-state sample({B}) calls done")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("rates", "kernels", "copies"), default="rates")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("databank_rates.py measures on the GPU; none found")
    torch.set_num_threads(max(1, min(8, eng.trainer.usable_cpus())))
    {"rates": rates, "kernels": kernels, "copies": copies}[args.mode](args)
