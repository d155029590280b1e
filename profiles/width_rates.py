"""fp32 training-step rate of the airfoil-like workload (bench.py: 5233 nodes, 5 levels, B = 8) at every latent width
D = 64 .. 256, and the level-0 edge aggregation at D = 192 (and 128) against its algorithmic bytes.  One box, one process:
    python profiles/width_rates.py [--steps 60] [--warmup 15] [--out profiles/width_rates.txt]
Prints one line per width (steps/s, ms/step) and the aggregation's fraction of the 8 TB/s HBM peak."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import WORKLOADS, build_workload, data_tuple, make_cfg, roofline_objects, timed_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--widths", default="64,96,128,160,192,224,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bsms_gnn_amd as eng
    lines = [f"airfoil-like fp32 step, B = 8, depth 5, {args.steps} timed steps after {args.warmup} (bench.timed_steps), "
             f"{torch.cuda.get_device_name(0)}"]
    for D in (int(d) for d in args.widths.split(",")):
        wl = build_workload("airfoil", 8, "cuda", cfg=dict(WORKLOADS["airfoil"], latent=D))
        torch.manual_seed(0)
        sim = eng.BSMS_Simulator(make_cfg(wl["cfg"])).cuda()
        data = data_tuple(wl)
        sim(data, True, True)
        dp = eng.DataParallel(sim)
        rate, ms, loss = timed_steps(lambda: dp.step_loss_backward(data, True), args.warmup, args.steps)
        lines.append(f"D = {D:3d}: {rate:7.1f} steps/s  {ms:6.3f} ms/step  loss {loss:.6f}")
        print(lines[-1], flush=True)
        if D in (128, 192):
            roof, _ = roofline_objects(wl, 8)
            agg = (f"  level-0 aggregation at D = {D}: {roof['avg_us']:.1f} us, {roof['achieved']:.0f} GB/s of algorithmic bytes "
                   f"({roof['algorithmic_bytes'] / 1e6:.1f} MB) = {roof['frac']:.3f} of the HBM peak (cold buffers); "
                   f"warm {roof['frac_warm']:.3f}; a plain device copy under the same rotation: "
                   f"{roof['cold_device_copy']['GBps']:.0f} GB/s")
            lines.append(agg)
            print(agg, flush=True)
        del dp, sim, data, wl
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
