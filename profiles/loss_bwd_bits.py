"""The bits of the six loss-gradient entries, for comparing two builds of the libraries:

    python profiles/loss_bwd_bits.py DIR > bits.txt

DIR holds libbsms_hip.so and libbsms_hip_ext.so.  Every entry runs on fixed seeded inputs -- R in {1, 255, 257, 1025}, C in {1, 3, 8},
with and without a carried pair, every space and kind, with and without node weights, both edge weightings -- and the script prints one
line per output buffer (loss_out, chan_out, parts_out, g_pred, grad_norm_pred) with its SHA-256, then a last line with the number of
those lines and the SHA-256 of all of them.  Two builds compute the same thing iff their outputs are identical line for line
(profiles/loss_bwd_bits.txt: the last line of this commit's output, which is also that of its parent's)."""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(lib_dir):
    sys.path.insert(0, ROOT)
    import bsms_gnn_amd as eng
    from bsms_gnn_amd import _abi
    from bsms_gnn_amd.graph import LevelPlan
    _abi.LIB_PATH = os.path.join(os.path.abspath(lib_dir), "libbsms_hip.so")          # before the first lib()
    _abi.EXT_LIB_PATH = os.path.join(os.path.abspath(lib_dir), "libbsms_hip_ext.so")
    L, X = _abi.lib(), _abi.ext()
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    total, count = hashlib.sha256(), [0]

    def report(tag, outs):
        torch.cuda.synchronize()
        for name, t in outs.items():
            line = f"{tag} {name} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}"
            print(line)
            total.update((line + "\n").encode())
            count[0] += 1

    for R, C in itertools.product((1, 255, 257, 1025), (1, 3, 8)):
        rng = np.random.default_rng(1000 * R + C)
        pred, tar = rng.standard_normal((R, C)).astype(np.float32), rng.standard_normal((R, C)).astype(np.float32)
        mask = (rng.random(R) < 0.8).astype(np.float32)
        mask[0], mask[R - 1] = 0.0, 1.0
        pos = rng.random((R, 2)).astype(np.float32)
        stats = lambda n: (lambda mean: [dev(mean), dev(mean * mean + 0.5 + rng.random(n)), dev(np.array(1e-8))])(rng.standard_normal(n))
        o_stats, i_stats = stats(C), stats(C + 1)
        g_next, g_nin = rng.standard_normal((R, C)).astype(np.float32), rng.standard_normal((R, C + 1)).astype(np.float32)
        g_next[mask == 0], g_nin[mask == 0] = np.inf, np.nan
        se = ((pred.astype(np.float64) - tar) ** 2 * mask[:, None]).sum(0)
        pair = dev(np.array([se.sum(), mask.sum()], np.float32))
        row = dev(np.concatenate([[float(mask.sum())], se]))
        erow = dev(np.concatenate([[1.5 * R], 0.5 + rng.random(C)]))
        cw, delta, nw = dev(0.5 + 1.5 * rng.random(C)), dev(0.25 + rng.random(C)), dev((0.5 + rng.random(R)).astype(np.float32))
        ring = np.arange(R)
        plan = LevelPlan(torch.from_numpy(np.stack([np.concatenate([ring, (ring + 1) % R]), np.concatenate([(ring + 1) % R, ring])])), R,
                         device="cuda")
        dp, dt, dm, dpos, dgn, dgi = dev(pred), dev(tar), dev(mask), dev(pos), dev(g_next), dev(g_nin)
        rows, both = (p(dp), p(dt), p(dm)), (*map(p, o_stats), *map(p, i_stats))
        fresh = lambda *names: {n: torch.full({"loss_out": (1,), "chan_out": (C,), "parts_out": (2,)}.get(n, (R, C)), 7.0, device="cuda") for n in names}

        o = fresh("loss_out", "grad_norm_pred")
        _abi.check(L.bsms_sim_loss_bwd(*rows, R, C, *map(p, o_stats), p(pair), p(o["loss_out"]), p(o["grad_norm_pred"]), s), "bsms_sim_loss_bwd")
        report(f"bsms_sim_loss_bwd R={R} C={C}", o)
        for carry in (0, 1):
            w, gn, gi = (0.375, p(dgn), p(dgi)) if carry else (1.0, None, None)
            tag = f"R={R} C={C} carry={carry}"
            o = fresh("loss_out", "g_pred", "grad_norm_pred")
            _abi.check(L.bsms_sim_unroll_bwd(*rows, R, C, *both, p(pair), w, gn, gi, p(o["loss_out"]), p(o["g_pred"]), p(o["grad_norm_pred"]), s),
                       "bsms_sim_unroll_bwd")
            report(f"bsms_sim_unroll_bwd {tag}", o)
            for space, kind in itertools.product((0, 1), (0, 1)):
                tail = lambda o: (w, gn, gi, p(o["loss_out"]), p(o["chan_out"]), p(o["g_pred"]), p(o["grad_norm_pred"]), s)
                o = fresh("loss_out", "chan_out", "g_pred", "grad_norm_pred")
                _abi.check(L.bsms_sim_objective_bwd(*rows, R, C, *both, p(row), p(cw), space, kind, *tail(o)), "bsms_sim_objective_bwd")
                report(f"bsms_sim_objective_bwd {tag} space={space} kind={kind}", o)
                o = fresh("loss_out", "chan_out", "g_pred", "grad_norm_pred")
                _abi.check(L.bsms_sim_objective_bwd_w(*rows, p(nw), R, R, C, *both, p(row), p(cw), space, kind, *tail(o)), "bsms_sim_objective_bwd_w")
                report(f"bsms_sim_objective_bwd_w {tag} space={space} kind={kind}", o)
                for weighted in (0, 1):                               # `kind` is the robust kind here: 0 = mae, 1 = huber
                    o = fresh("loss_out", "chan_out", "g_pred", "grad_norm_pred")
                    _abi.check(L.bsms_sim_robust_bwd(*rows, p(nw) if weighted else None, R, R, C, *both, p(row), p(cw), p(delta), space, kind,
                                                     *tail(o)), "bsms_sim_robust_bwd")
                    report(f"bsms_sim_robust_bwd {tag} space={space} rkind={kind} weights={weighted}", o)
                for weighting in (0, 1):
                    o = fresh("loss_out", "parts_out", "chan_out", "g_pred", "grad_norm_pred")
                    _abi.check(X.bsms_sim_edge_objective_bwd(plan.handle, R, 1, *rows, p(dpos), C, 2, weighting, *both, p(row), p(erow), p(cw), space,
                                                             kind, 0.25, w, gn, gi, p(o["loss_out"]), p(o["parts_out"]), p(o["chan_out"]),
                                                             p(o["g_pred"]), p(o["grad_norm_pred"]), s), "bsms_sim_edge_objective_bwd")
                    report(f"bsms_sim_edge_objective_bwd {tag} space={space} kind={kind} weighting={weighting}", o)
    print(f"all {count[0]} lines {total.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1])
