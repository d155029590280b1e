"""The bits of every entry behind the shared piece sum (csrc/piece_sum.h), for comparing two builds of the libraries:

    python profiles/piece_sum_bits.py DIR > bits.txt

DIR holds libbsms_hip.so and its three companions.  Every entry runs on fixed seeded inputs and the script prints one line per output
buffer with its SHA-256, then a last line with the number of those lines and the SHA-256 of all of them.  Two builds compute the same
thing iff their outputs are identical line for line (profiles/piece_sum_bits.txt: the last line of this commit's output, which is
also that of its parent's).

  bsms_error_sums, _w, bsms_robust_sums (both spaces and kinds, with and without weights, rows of `sums` 3 doubles wider than a row),
  bsms_edge_diff_sums (both weightings), bsms_edge_diff_bwd (with and without accumulate):
      segments of 0, 1, 255, 1023, 1024, 1025, 2049 rows (no piece, one short, one full, a ragged second and third piece);
      S in {1, 3, 70}; C in {1, 3, 8}; target / mask / weights / pos shared by the segments (stride 0), dense, or 5 rows apart;
      edges: a ring on those rows, as the whole plan and as the window [7, 7 + rows) of a ring on rows + 20
  bsms_moment_sums: tables of 1, 64 and 65 entries with n in {1, 85, 342}, frames in {1, 31, 32, 33}, type_stride 0 and n
  bsms_edge_diff_fold, bsms_moment_fold: S in {0, 1, 2, 70}
Outputs are pre-filled with 7.0, so what an entry must not write is part of the hash."""
import ctypes
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, SEGS, CHANS, PAD, SMAX = (0, 1, 255, 1023, 1024, 1025, 2049), (1, 3, 70), (1, 3, 8), 5, 70


def main(lib_dir):
    sys.path.insert(0, ROOT)
    import bsms_gnn_amd  # noqa: F401
    from bsms_gnn_amd import _abi
    from bsms_gnn_amd.graph import LevelPlan
    lib_dir = os.path.abspath(lib_dir)
    _abi.LIB_PATH = os.path.join(lib_dir, "libbsms_hip.so")            # before the first lib()
    _abi.EXT_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_ext.so")
    _abi.STATS_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_stats.so")
    _abi.SAMPLE_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_sample.so")
    L, X, T = _abi.lib(), _abi.ext(), _abi.stats()
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fresh = lambda *shape, dtype=torch.float64: torch.full(shape, 7.0, device="cuda", dtype=dtype)
    work = lambda nbytes: torch.empty(max(int(nbytes), 8), device="cuda", dtype=torch.uint8)

    total, count = hashlib.sha256(), [0]

    def report(tag, t):
        line = f"{tag} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}"       # .cpu() waits for the stream
        print(line)
        total.update((line + "\n").encode())
        count[0] += 1

    def ring(n):
        n = max(n, 1)
        i = np.arange(n)
        return LevelPlan(torch.from_numpy(np.stack([np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i])])), n, device="cuda")

    for n, C in itertools.product(ROWS, CHANS):
        rng = np.random.default_rng(1000 * n + C)
        pitch = n + PAD
        pred = rng.standard_normal((SMAX, pitch, C)).astype(np.float32)
        tar = (3 * rng.standard_normal((SMAX, pitch, C))).astype(np.float32)
        mask = (rng.random((SMAX, pitch)) < 0.8).astype(np.float32)
        wts = (0.5 + rng.random((SMAX, pitch))).astype(np.float32)
        pos = rng.random((SMAX, pitch, 2)).astype(np.float32)
        padded = [dev(a) for a in (pred, tar, mask, wts, pos)]
        dense = [dev(a[:, :n]) for a in (pred, tar, mask, wts, pos)]
        mean = rng.standard_normal(C)
        stats = [dev(mean), dev(mean * mean + 0.5 + rng.random(C)), dev(np.array(1e-8)), dev(0.25 + rng.random(C))]
        coef = dev(rng.standard_normal((SMAX, C)))
        plans = {"whole": (ring(n), 0), "window": (ring(n + 20), 7)}
        for S, mode in itertools.product(SEGS, ("shared", "dense", "padded")):
            dp, dt, dm, dw, dx = dense if mode == "dense" else padded
            ps = n if mode == "dense" else pitch
            ts = 0 if mode == "shared" else ps                           # target, mask, weights and pos share one stride
            tag = f"n={n} C={C} S={S} {mode}"
            ncol = 1 + 3 * C
            out = fresh(S, ncol)
            wk = work(L.bsms_error_sums_work_bytes(S, n))
            _abi.check(L.bsms_error_sums(p(dp), p(dt), p(dm), S, n, C, ps, ts, ts, p(out), p(wk), s), "bsms_error_sums")
            report(f"bsms_error_sums {tag}", out)
            out = fresh(S, ncol)
            _abi.check(L.bsms_error_sums_w(p(dp), p(dt), p(dm), p(dw), S, n, C, ps, ts, ts, ts, p(out), p(wk), s), "bsms_error_sums_w")
            report(f"bsms_error_sums_w {tag}", out)
            for space, rkind, weighted in itertools.product((0, 1), (0, 1), (0, 1)):
                out = fresh(S, 1 + C + 3)
                _abi.check(L.bsms_robust_sums(p(dp), p(dt), p(dm), p(dw) if weighted else None, S, n, C, ps, ts, ts, ts, *map(p, stats), space,
                                              rkind, p(out), 1 + C + 3, p(wk), s), "bsms_robust_sums")
                report(f"bsms_robust_sums {tag} space={space} rkind={rkind} weights={weighted}", out)
            wk = work(L.bsms_edge_diff_work_bytes(S, n))
            for (where, (plan, row0)), weighting in itertools.product(plans.items(), (0, 1)):
                args = (plan.handle, row0, n, p(dp), p(dt), p(dm), p(dx), S, C, 2, weighting, ps, ts, ts, ts)
                out = fresh(S, 1 + 2 * C)
                _abi.check(L.bsms_edge_diff_sums(*args, p(out), p(wk), s), "bsms_edge_diff_sums")
                report(f"bsms_edge_diff_sums {tag} {where} weighting={weighting}", out)
                for accumulate in (0, 1):
                    grad = fresh(S, pitch, C, dtype=torch.float32)
                    _abi.check(L.bsms_edge_diff_bwd(*args, p(coef), accumulate, p(grad), pitch, s), "bsms_edge_diff_bwd")
                    report(f"bsms_edge_diff_bwd {tag} {where} weighting={weighting} accumulate={accumulate}", grad)

    for S, C in itertools.product((0, 1, 2, 70), CHANS):
        rng = np.random.default_rng(77 * S + C)
        rows, out = dev(rng.standard_normal((S, 1 + 2 * C))), fresh(1 + 2 * C)
        _abi.check(X.bsms_edge_diff_fold(p(rows) if S else None, S, C, p(out), s), "bsms_edge_diff_fold")
        report(f"bsms_edge_diff_fold S={S} C={C}", out)
    for S, W in itertools.product((0, 1, 2, 70), (8, 16, 36, 64, 65, 200)):
        rng = np.random.default_rng(91 * S + W)
        rows, out = dev(rng.standard_normal((S, W))), fresh(W + 3)
        _abi.check(T.bsms_moment_fold(p(rows) if S else None, S, W, p(out), s), "bsms_moment_fold")
        report(f"bsms_moment_fold S={S} W={W}", out)

    valid = (ctypes.c_float * 2)(0.0, 5.0)
    for C in CHANS:
        rng = np.random.default_rng(500 + C)
        entries, keep = [], []
        for k, (n, frames, per_frame) in enumerate(itertools.islice(itertools.cycle(itertools.product((1, 85, 342), (1, 31, 32, 33), (0, 1))), 65)):
            frame0 = 2 * (k % 2)
            state = dev(rng.standard_normal((frame0 + frames + 1, n, C)).astype(np.float32))
            typ = dev(rng.choice(np.array([0.0, 1.0, 5.0], np.float32), size=(frame0 + frames + 1, n) if per_frame else (n,)))
            keep += [state, typ]
            entries.append(_abi.MomentTraj(p(state), p(typ), n, frame0, frames, n if per_frame else 0))
        wk = work(T.bsms_moment_work_bytes(342 * 33))
        tables = [entries[k:k + 1] for k in range(24)] + [entries[:64], entries]
        for table in tables:
            S = len(table)
            arr, out = (_abi.MomentTraj * S)(*table), fresh(S, 4 * C + 4)
            _abi.check(T.bsms_moment_sums(ctypes.addressof(arr), S, C, ctypes.addressof(valid), 2, p(out), p(wk), s), "bsms_moment_sums")
            tag = f"entries={S}" if S > 1 else f"n={table[0].n} frames={table[0].frames} type_stride={table[0].type_stride}"
            report(f"bsms_moment_sums C={C} {tag}", out)
    print(f"all {count[0]} lines {total.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1])
