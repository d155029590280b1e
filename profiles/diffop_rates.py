#!/usr/bin/env python3
"""Cell gradients on the device: what the four entries of libbsms_hip_diffop.so cost on the bench workload's airfoil
mesh (5233 nodes, 10 445 triangles) for a 100-frame rollout of 3 channels, next to the same jobs composed from torch ops
(`index_select` of the corner rows, elementwise fp64 ops, `index_add_`), alternated in one process.

  (1) bsms_cell_gradient, bsms_node_gradient, bsms_cell_gradient_sums (with a velocity pair) and bsms_cell_gradient_bwd through
      `MeshGradient`, S = 100, C = 3.  A window is `--calls` calls between two device events; the figure is microseconds per call
      (median [min .. max] over the repeats), host wrapper included.
  (2) The bytes each entry has to move at least -- the fields once, the output once, the index arrays once -- over the time, against
      the HBM peak of 8.0 TB/s.
  (3) bsms_node_gradient on the same mesh with a hub appended (one node joined to 512 others), `long_list` = 1 << 40 (every node walked
      by its own thread), the default, and 8.

  python profiles/diffop_rates.py --out profiles/diffop_rates.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bsms_gnn_amd as eng

HBM_PEAK = 8.0e12      # bytes/s, specification


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


class TorchOps:
    """The same jobs from torch ops, fp64 after the gather as the entries compute: index_select, elementwise, index_add_."""

    def __init__(self, pos, tris):
        self.tris = tris.long()
        p = pos.double()
        a, b, c = (p[self.tris[:, k]] for k in range(3))
        self.A2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        self.kx = torch.stack([b[:, 1] - c[:, 1], c[:, 1] - a[:, 1], a[:, 1] - b[:, 1]], -1)          # [T, 3]
        self.ky = torch.stack([c[:, 0] - b[:, 0], a[:, 0] - c[:, 0], b[:, 0] - a[:, 0]], -1)
        self.N = pos.shape[0]
        self.den = torch.zeros(self.N, dtype=torch.float64, device=pos.device).index_add_(0, self.tris.reshape(-1), self.A2.abs().repeat_interleave(3))

    def normals(self, f):
        v = [f.index_select(1, self.tris[:, k]).double() for k in range(3)]                          # three [S, T, C]
        nx = v[0] * self.kx[:, 0, None] + v[1] * self.kx[:, 1, None] + v[2] * self.kx[:, 2, None]
        ny = v[0] * self.ky[:, 0, None] + v[1] * self.ky[:, 1, None] + v[2] * self.ky[:, 2, None]
        return nx, ny

    def cell_gradient(self, f):
        nx, ny = self.normals(f)
        return torch.stack([nx / self.A2[:, None], ny / self.A2[:, None]], -1).float()

    def node_gradient(self, f):
        nx, ny = self.normals(f)
        n = torch.stack([nx, ny], -1) * torch.sign(self.A2)[:, None, None]
        num = torch.zeros(f.shape[0], self.N, f.shape[2], 2, dtype=torch.float64, device=f.device)
        for k in range(3):
            num.index_add_(1, self.tris[:, k], n)                                                     # float atomics: not reproducible
        return (num / self.den[:, None, None]).float()

    def sums(self, pred, tar, mask, cu, cv):
        w = (mask[self.tris].double().prod(-1) * self.A2.abs() * 0.5)[None, :, None]
        G = lambda f: [n / self.A2[:, None] for n in self.normals(f)]
        (dx, dy), (tx, ty), (px, py) = G(pred - tar), G(tar), G(pred)
        cols = [w.sum(1).expand(pred.shape[0], 1), (w * (dx * dx + dy * dy)).sum(1), (w * (tx * tx + ty * ty)).sum(1)]
        for x in (px[..., cu] + py[..., cv], tx[..., cu] + ty[..., cv], dx[..., cv] - dy[..., cu], tx[..., cv] - ty[..., cu]):
            cols.append((w[..., 0] * x * x).sum(1, keepdim=True))
        return torch.cat(cols, 1)

    def backward(self, pred, tar, mask, coef, cu, cv):
        p = pred.detach().clone().requires_grad_(True)
        s = self.sums(p, tar, mask, cu, cv)
        C = pred.shape[2]
        J = (coef[:, :C] * s[:, 1:1 + C]).sum() + (coef[:, C] * s[:, 1 + 2 * C]).sum() + (coef[:, C + 1] * s[:, 3 + 2 * C]).sum()
        return torch.autograd.grad(J, p)[0]


def block(title, runs, args, lines, least=None):
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    got = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            got[k].append(timed(run, args.calls))
    lines.append(title)
    for k, v in got.items():
        med = statistics.median(v)
        tail = ""
        if least and k in least:
            tail = f"   at least {least[k] / 1e6:.2f} MB: {least[k] / (med * 1e-6) / 1e12:.3f} TB/s = {least[k] / (med * 1e-6) / HBM_PEAK:.3f} of the HBM peak"
        lines.append(f"    {k:34s} {med:9.1f}  [{min(v):9.1f} .. {max(v):9.1f}]{tail}")
    return {k: statistics.median(v) for k, v in got.items()}


def main(args):
    import bench
    pts, cells = bench.mesh_points("airfoil", None)
    pos = torch.tensor(np.asarray(pts)[:, :2], dtype=torch.float32)
    cells = np.asarray(cells, dtype=np.int64)
    S, C, cu, cv = args.frames, 3, 0, 1
    ops = eng.MeshGradient(pos, cells, "tri")
    N, T = ops.N, ops.T
    gen = torch.Generator(device="cuda").manual_seed(0)
    roll = torch.randn(S + 1, N, C, device="cuda", generator=gen)
    pred, tar = roll[1:], roll[:-1]                                     # two strided views of one resident array, read in place
    mask = (torch.rand(N, device="cuda", generator=gen) < 0.9).float()
    coef = torch.rand(S, C + 2, device="cuda", dtype=torch.float64)
    grad = torch.empty(S, N, C, device="cuda")
    ref = TorchOps(ops.pos, ops.tris)
    lines = [f"# python profiles/diffop_rates.py --calls {args.calls} --repeats {args.repeats} --frames {args.frames}   ({torch.cuda.get_device_name(0)})",
             "# us per call, median [min .. max] over the repeats; the runs of a block alternate in one process"]
    idx = (3 * T + N + 1 + ops.nnz) * 4 + N * 8
    least = {"bsms_cell_gradient": S * N * C * 4 + S * T * C * 8 + idx, "bsms_node_gradient": S * N * C * 4 + S * N * C * 8 + idx,
             "bsms_cell_gradient_sums": 2 * S * N * C * 4 + N * 4 + idx, "bsms_cell_gradient_bwd": 3 * S * N * C * 4 + N * 4 + idx}
    runs = {"bsms_cell_gradient": lambda: ops.cell_gradient(pred), "torch cell gradient": lambda: ref.cell_gradient(pred),
            "bsms_node_gradient": lambda: ops.node_gradient(pred), "torch node gradient (index_add_)": lambda: ref.node_gradient(pred),
            "bsms_cell_gradient_sums": lambda: ops.sums(pred, tar, mask, (cu, cv)), "torch sums": lambda: ref.sums(pred, tar, mask, cu, cv),
            "bsms_cell_gradient_bwd": lambda: ops.backward(pred, tar, mask, coef, (cu, cv), out=grad),
            "torch backward (autograd)": lambda: ref.backward(pred, tar, mask, coef, cu, cv)}
    block(f"  airfoil: N = {N}, T = {T}, nnz = {ops.nnz}, longest list {int((ops.inc_ptr[1:] - ops.inc_ptr[:-1]).max())}, S = {S}, C = {C}", runs, args, lines, least)
    err = float((ops.node_gradient(pred) - ref.node_gradient(pred)).abs().max())
    lines.append(f"    (largest |entry - torch composition| of the node gradient: {err:.3g})")

    hub = np.concatenate([cells, [[N, k, k + 1] for k in range(0, 1024, 2)]])
    hpos = torch.cat([pos, torch.tensor([[3.0, 3.0]])])
    hops = eng.MeshGradient(hpos, hub, "tri")
    hf = torch.randn(S, N + 1, C, device="cuda", generator=gen)
    walks = {f"bsms_node_gradient long_list={name}": (lambda k=k: hops.node_gradient(hf, long_list=k)) for name, k in (("none", 1 << 40), ("default", 0), ("8", 8))}
    block(f"  airfoil + a hub of {int((hops.inc_ptr[1:] - hops.inc_ptr[:-1]).max())} triangles, S = {S}, C = {C}", walks, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diffop_rates.py measures on the GPU; none found")
    main(args)
