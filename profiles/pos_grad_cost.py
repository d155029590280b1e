#!/usr/bin/env python3
"""Cost of position gradients on the airfoil B=8 training step (bench.build_workload: 5233 nodes, 5 levels, D=128).

One step = BSMS_Simulator forward + masked RMSE + backward through autograd, with and without node_in.requires_grad, in fp32
and bf16; the two variants alternate round by round in ONE process (same box, same clocks).  Then a kernel trace of its own
(rocprofv3 --kernel-trace --stats, a child process running only the position-gradient steps) gives the time of the new kernels
per step against their traffic formula (posgrad.hip):
    k_narrow_t  per block:  B E_l (D s + 2 f 4)          s = 4 (fp32 gE[0]) or 2 (bf16), f = fiber pitch (4 floats for p <= 3)
    k_pos_node  per block:  2 B E_l f 4 + 4 (2 (N_l + 1) + E_l) + B N_l p 4 (x2 when it accumulates)
    (every level has an up and a down block, the bottom level one)

    python profiles/pos_grad_cost.py [--rounds 6] [--steps 20] [--out FILE]
"""
import argparse
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def setup(batch=8):
    import torch
    import bsms_gnn_amd as eng
    from bench import build_workload, data_tuple, make_cfg
    wl = build_workload("airfoil", batch, "cuda")
    data = data_tuple(wl)
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(make_cfg(wl["cfg"])).cuda()
    sim(data, True, True)                                   # one normaliser accumulation
    return eng, sim, data, wl


def step(eng, sim, data, pos_grad):
    sim.zero_grad(set_to_none=True)
    ni = data[0].detach().requires_grad_(pos_grad)
    pred = sim((ni, *data[1:]), True, False)
    eng.masked_rmse(pred, data[1], data[2]).backward()


def timed(args):
    import torch
    eng, sim, data, wl = setup()
    lines = [f"airfoil B=8 levels (N, E): {wl['levels']}"]
    for prec in ("f32", "bf16"):
        sim.process.precision = prec
        for v in (False, True):
            for _ in range(5):
                step(eng, sim, data, v)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for r in range(args.rounds):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    step(eng, sim, data, v)
                b.record()
                b.synchronize()
                ms[v].append(a.elapsed_time(b) / args.steps)
        med = {v: sorted(x)[len(x) // 2] for v, x in ms.items()}
        lines.append(f"{prec:5s} step (autograd): without position gradient {med[False]:.3f} ms, with {med[True]:.3f} ms, "
                     f"overhead {med[True] - med[False]:+.3f} ms ({100 * (med[True] / med[False] - 1):+.1f} %)   "
                     f"[per-round ms off {' '.join(f'{x:.3f}' for x in ms[False])} | on {' '.join(f'{x:.3f}' for x in ms[True])}]")
    return lines, wl


def trace_child(args):
    import torch
    eng, sim, data, _ = setup()
    for prec in ("f32", "bf16"):
        sim.process.precision = prec
        for _ in range(args.steps):
            step(eng, sim, data, True)
        torch.cuda.synchronize()


def formula(wl, bf16):
    B, D, p = 8, wl["cfg"]["latent"], wl["cfg"]["pos_dim"]
    f = 4 if p <= 3 else 8
    s = 2 if bf16 else 4
    lv = wl["levels"]
    narrow = node = 0
    for l, (N, E) in enumerate(lv):
        blocks = 1 if l == len(lv) - 1 else 2
        narrow += blocks * B * E * (D * s + 2 * f * 4)
        node += blocks * (2 * B * E * f * 4 + 4 * (2 * (N + 1) + E)) + B * N * p * 4 * (3 if blocks == 2 else 1)
    return narrow, node, B * lv[0][1] * (D * s + 2 * f * 4)


def traced(args, wl):
    tmp = tempfile.mkdtemp(prefix="posgrad_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "r", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", "--steps", str(args.steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    files = glob.glob(os.path.join(tmp, "**", "r_kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return [f"trace run failed (rc {r.returncode}): {r.stderr[-400:]}"]
    rows = list(csv.DictReader(open(files[0])))
    out = []
    for bf16, tag in ((False, "f32"), (True, "bf16")):
        flag = "true" if bf16 else "false"
        pick = lambda r, k: k in r["Kernel_Name"] and (k != "k_narrow_t" or re.search(rf"k_narrow_t<[^>]*, {flag}, true>", r["Kernel_Name"]))
        dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        nar = [dur(r) for r in rows if pick(r, "k_narrow_t")]
        nodes_all = [r for r in rows if "k_pos_node" in r["Kernel_Name"]]
        half = len(nodes_all) // 2                                  # the fp32 steps ran first, then the bf16 ones
        nod = [dur(r) for r in (nodes_all[:half] if not bf16 else nodes_all[half:])]
        n_nar, n_nod, b_l0 = formula(wl, bf16)
        per_step = lambda xs: sum(xs) / args.steps
        t_nar, t_nod = per_step(nar), per_step(nod)
        l0 = sorted(nar)[-2 * args.steps:]                          # the largest launches: the two level-0 blocks of every step
        t_l0 = sum(l0) / len(l0)
        out.append(f"{tag:5s} k_narrow_t: {t_nar * 1e6:7.1f} us/step over {len(nar) // args.steps} launches, {n_nar / 1e6:6.1f} MB/step -> "
                   f"{n_nar / t_nar / 1e9:6.0f} GB/s ({n_nar / t_nar / HBM_PEAK:.2f} of HBM peak); level-0 launch {t_l0 * 1e6:.1f} us, "
                   f"{b_l0 / 1e6:.1f} MB -> {b_l0 / t_l0 / 1e9:.0f} GB/s ({b_l0 / t_l0 / HBM_PEAK:.2f})")
        out.append(f"{tag:5s} k_pos_node: {t_nod * 1e6:7.1f} us/step over {len(nod) // args.steps} launches, {n_nod / 1e6:6.1f} MB/step -> "
                   f"{n_nod / t_nod / 1e9:6.0f} GB/s ({n_nod / t_nod / HBM_PEAK:.2f} of HBM peak)")
    enc = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if re.search(r"k_narrow_t<[^>]*, false>", r["Kernel_Name"])]
    if enc:
        out.append(f"encoder input gradient (k_narrow_t, narrow MLP input): {sum(enc) / (2 * args.steps) * 1e6:.1f} us/step")
    stats = glob.glob(os.path.join(tmp, "**", "r_kernel_stats.csv"), recursive=True)
    if stats:
        for r in csv.DictReader(open(stats[0])):
            if "k_narrow_t" in r["Name"] or "k_pos_node" in r["Name"]:
                out.append(f"  stats: {int(r['Calls']):5d} calls  avg {float(r['AverageNs']) / 1e3:8.2f} us  {r['Name'][:110]}")
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    lines, wl = timed(args)
    lines += traced(args, wl)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
