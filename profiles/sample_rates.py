"""Rates of the mesh sampler on one MI355X.

    python profiles/sample_rates.py [--parent DIR] [--rounds 3] [--out profiles/sample_rates.txt]

On the airfoil stand-in mesh of bench.py (5233 nodes, its Delaunay triangles), device events around batches of back-to-back calls
after warm-up, the median batch divided by its calls:
(a) bsms_raster_owner at 256 x 256 and 1024 x 1024, and the sweep of the lane / wave threshold (`small_box`) at 1024 x 1024;
(b) bsms_field_gather at S * C = 4 * 3 and at a 100-frame rollout (S = 100, C = 3): the bytes the algorithm must move (the output
    once, the owner image once, the nodal values once) over the time, as a share of the HBM peak;
(c) bsms_point_owner at P = 1024;
(d) the same three operations written with torch ops on the device (fp64 brute-force containment over pixel chunks + gather);
(e) the device-to-host copy that Trainer.eval_panels and rollout_frames make unnecessary, alone;
(f) bench.py's default step on the parent (--parent) and on this commit, alternated, and `--dump-outputs` of both byte for byte.
(a)-(e) run in one child process, every bench.py run in its own."""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HBM_PEAK = 8.0e12            # bytes/s, the MI355X's HBM3E peak (spec)
SWEEP = (1, 16, 64, 128, 256, 512, 1024, 2048, 4096, 16384)


def timed(fn, calls=20, batches=7, warm=3):
    """Median microseconds per call: device events around `calls` back-to-back calls, `batches` times."""
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(out)


def torch_owner(pos, tris, q, chunk=4096):
    """The alternative a user has today: brute-force containment by the same contract in torch fp64, `chunk` points at a time."""
    import torch
    p = pos.double()
    a, b, c = (p[tris[:, k].long()][None] for k in range(3))
    orient = lambda u, v, w: (v[..., 0] - u[..., 0]) * (w[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (w[..., 0] - u[..., 0])
    A = orient(a, b, c)
    ok, sg = (A != 0) & torch.isfinite(A), torch.where(A > 0, 1.0, -1.0).double()
    T = tris.shape[0]
    ids = torch.arange(T, device=pos.device, dtype=torch.int32)[None]
    out = []
    for lo in range(0, q.shape[0], chunk):
        w = q[lo:lo + chunk, None, :]
        inside = ok & (orient(b, c, w) * sg >= 0) & (orient(c, a, w) * sg >= 0) & (orient(a, b, w) * sg >= 0)
        first = torch.where(inside, ids, T).amin(1)
        out.append(torch.where(first < T, first, -1))
    return torch.cat(out).int()


def torch_gather(pos, tris, owner, q, fields, fill):
    """fields [S, N, C] -> [S, P, C]: weights by the contract in torch fp64, three gathers."""
    import torch
    p = pos.double()
    t = owner.clamp_min(0).long()
    a, b, c = (p[tris[t, k].long()] for k in range(3))
    orient = lambda u, v, w: (v[..., 0] - u[..., 0]) * (w[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (w[..., 0] - u[..., 0])
    e0, e1, e2 = orient(b, c, q), orient(c, a, q), orient(a, b, q)
    s = (e0 + e1) + e2
    f = fields.double()
    val = ((e0 / s)[None, :, None] * f[:, tris[t, 0].long()] + (e1 / s)[None, :, None] * f[:, tris[t, 1].long()]) + (e2 / s)[None, :, None] * f[:, tris[t, 2].long()]
    return torch.where((owner >= 0)[None, :, None], val.float(), torch.full((), fill, device=pos.device))


def child(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bench
    import bsms_gnn_amd as eng
    pts, cells = bench.mesh_points("airfoil")
    s = eng.MeshSampler(pts.astype(np.float32), cells, "tri")
    N, T = s.N, s.T
    rng = np.random.default_rng(0)
    res = {"N": N, "T": T, "raster": {}, "sweep": {}, "gather": {}, "torch": {}, "d2h": {}}
    for side in (256, 1024):
        res["raster"][side] = timed(lambda: s._tri_owners(side, side, small_box=-1))      # -1: not the cached image, the entry's default threshold
    for small in SWEEP:
        res["sweep"][small] = timed(lambda: s._tri_owners(1024, 1024, small_box=small))
    owners = {side: s._tri_owners(side, side) for side in (256, 1024)}
    # the list walk: the airfoil has no box above 16384 pixels, so four triangles over the whole image are put behind its own
    far = np.array([[-5.0, -5.0], [9.0, -5.0], [-5.0, 9.0]])
    listed = eng.MeshSampler(np.concatenate([pts, far]).astype(np.float32), np.concatenate([cells, [[N, N + 1, N + 2]] * 4]), "tri")
    res["listed"] = {side: timed(lambda: listed._tri_owners(side, side, bounds=s.bounds, small_box=-1)) for side in (256, 1024)}
    same = all(torch.equal(torch.where(owners[side] >= 0, owners[side], T), listed._tri_owners(side, side, bounds=s.bounds)) for side in (256, 1024))
    res["listed"]["same_owners"] = bool(same)
    # the largest boxes of the mesh at 1024 x 1024, from the host: what the thresholds sort
    p64 = pts.astype(np.float32).astype(np.float64)[cells]
    W, H, x0, y0, dx, dy = s.grid(1024, 1024)
    box = ((p64[..., 0].max(1) - p64[..., 0].min(1)) / dx + 3) * ((p64[..., 1].max(1) - p64[..., 1].min(1)) / dy + 3)
    res["boxes"] = {"median": float(np.median(box)), "p99": float(np.quantile(box, 0.99)), "max": float(box.max()),
                    "over_64": int((box > 64).sum()), "over_16384": int((box > 16384).sum())}
    for S, Cn in ((4, 3), (100, 3)):
        f = torch.from_numpy(rng.standard_normal((S, N, Cn)).astype(np.float32)).cuda()
        for side in (256, 1024):
            us = timed(lambda: s.rasterize(f, side, side), calls=10)
            nbytes = S * Cn * side * side * 4 + side * side * 4 + S * N * Cn * 4
            res["gather"][f"{S}x{Cn}@{side}"] = {"us": us, "bytes": nbytes}
    q = torch.from_numpy(rng.random((1024, 2))).cuda()
    res["point_owner_us"] = timed(lambda: s._locate(q))
    f43 = torch.from_numpy(rng.standard_normal((4, N, 3)).astype(np.float32)).cuda()
    res["probe_4x3_us"] = timed(lambda: s.probe(f43, q))
    # ---- torch ops
    centres = torch.from_numpy(s.pixel_centres(256, 256).reshape(-1, 2)).cuda()
    res["torch"]["owner@256"] = timed(lambda: torch_owner(s.pos, s.tris, centres), calls=2, batches=3, warm=1)
    res["torch"]["owner_P1024"] = timed(lambda: torch_owner(s.pos, s.tris, q), calls=5, batches=5, warm=1)
    own256 = owners[256].reshape(-1)
    res["torch"]["owners_equal"] = bool(torch.equal(torch_owner(s.pos, s.tris, centres), own256) and torch.equal(torch_owner(s.pos, s.tris, q), s._locate(q)))
    res["torch"]["gather_4x3@256"] = timed(lambda: torch_gather(s.pos, s.tris, own256, centres, f43, float("nan")), calls=5, batches=5, warm=1)
    mine = s.rasterize(f43, 256, 256).reshape(4, 3, -1).permute(0, 2, 1)
    theirs = torch_gather(s.pos, s.tris, own256, centres, f43, float("nan"))
    res["torch"]["values_equal"] = bool(torch.equal(torch.nan_to_num(mine), torch.nan_to_num(theirs)))
    # ---- the copies to the host that a CPU route starts with
    for name, shape in (("eval_panels: input, label, prediction [3, 8, N, 3]", (3, 8, N, 3)), ("rollout: 100 frames [100, N, 3]", (100, N, 3))):
        t = torch.randn(*shape, device="cuda")
        host = torch.empty(shape, pin_memory=True)
        res["d2h"][name] = {"us": timed(lambda: host.copy_(t, non_blocking=True), calls=10), "bytes": t.numel() * 4}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--child", metavar="ROOT")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    sys.path.insert(0, HERE)
    from edge_objective_rates import bench_default, run, same_dumps
    r = run([sys.executable, os.path.abspath(__file__), "--child", ROOT], ROOT)
    lines = ["# Mesh sampler (DESIGN.md 4.26): profiles/sample_rates.py, one call on one MI355X.  No figure is a pass criterion of the feature.",
             f"# Airfoil stand-in mesh of bench.py: {r['N']} nodes, {r['T']} triangles.  us per call: device events around 20 back-to-back calls (10 for",
             "# the gathers), the median of 7 such batches after 3 warm-up calls.", "#",
             "# (a) bsms_raster_owner (memset of the image, memset of the list counter, k_raster_tris, k_raster_listed)"]
    for side, us in r["raster"].items():
        lines.append(f"  {side} x {side}: {us:8.1f} us")
    b = r["boxes"]
    lines += [f"#     boxes at 1024 x 1024 (pixels, with the one-pixel margin): median {b['median']:.0f}, 99th percentile {b['p99']:.0f}, largest {b['max']:.0f}; "
              f"{b['over_64']} of {r['T']} above 64, {b['over_16384']} above 16384",
              "#     sweep of small_box (the triangle's eight lanes walk boxes up to it, the wave those above) at 1024 x 1024:"]
    lines.append("  " + "   ".join(f"{k}: {us:.1f}" for k, us in r["sweep"].items()) + "   us")
    best = min(r["sweep"], key=lambda k: r["sweep"][k])
    lines += [f"#     fastest: small_box = {best}; the default is 64 (kSmallBox in csrc/sample/raster.hip)",
              "#     the list walk (k_raster_listed), which the airfoil never takes: the same mesh with four triangles over the whole image appended",
              f"  256 x 256: {r['listed']['256']:8.1f} us     1024 x 1024: {r['listed']['1024']:8.1f} us     (the airfoil's own owners unchanged, the rest "
              f"owned by the first of the four: {r['listed']['same_owners']})",
              "#     NOT swept: the wave / list threshold kWaveBox = 16384, the list walk's grid kListBlocks = 256 and the list's size kListCap = 1023",
              "#     are set by reasoning (256 pixels per lane of a wave; one pixel per thread of the smallest listed box of 256 x 256; 4 KB), not by measurement", "#",
              "# (b) bsms_field_gather through MeshSampler.rasterize (owner image cached): us, algorithmic bytes (output + owner image + nodal values, once each), share of the 8.0 TB/s HBM peak"]
    for name, g in r["gather"].items():
        S, rest = name.split("x")
        Cn, side = rest.split("@")
        lines.append(f"  S = {S:>3s}, C = {Cn}, {side:>4s} x {side:<4s}: {g['us']:9.1f} us   {g['bytes'] / 1e6:9.2f} MB   {g['bytes'] / (g['us'] * 1e-6) / 1e12:.3f} TB/s = "
                     f"{g['bytes'] / (g['us'] * 1e-6) / HBM_PEAK:.1%}")
    lines += ["#", f"# (c) bsms_point_owner, P = 1024 random points in the unit square ({1024 * r['T']} containment tests at most): {r['point_owner_us']:.1f} us; "
              f"MeshSampler.probe of S * C = 4 * 3 at them (locate + gather): {r['probe_4x3_us']:.1f} us", "#",
              "# (d) the same with torch ops on the device (fp64 brute force by the same contract over chunks of 4096 points, then three gathers);",
              f"#     owners equal to the entries': {r['torch']['owners_equal']}, values bit-equal: {r['torch']['values_equal']}",
              f"  owners of 256 x 256 centres: {r['torch']['owner@256']:.0f} us   (bsms_raster_owner: {r['raster']['256']:.1f} us, {r['torch']['owner@256'] / r['raster']['256']:.0f}x)",
              f"  owners of 1024 points:       {r['torch']['owner_P1024']:.0f} us   (bsms_point_owner: {r['point_owner_us']:.1f} us, {r['torch']['owner_P1024'] / r['point_owner_us']:.0f}x)",
              f"  gather S * C = 4 * 3 at 256 x 256: {r['torch']['gather_4x3@256']:.0f} us   (bsms_field_gather: {r['gather']['4x3@256']['us']:.1f} us, "
              f"{r['torch']['gather_4x3@256'] / r['gather']['4x3@256']['us']:.0f}x)",
              "#     torch owners at 1024 x 1024: not measured (16 times the chunks of 256 x 256)", "#",
              "# (e) the device-to-host copy a CPU triangulation route starts with (pinned destination, the copy alone; no CPU interpolation is timed)"]
    for name, d in r["d2h"].items():
        lines.append(f"  {name}: {d['bytes'] / 1e6:.2f} MB, {d['us']:.1f} us")
    # ---- (f)
    parent = os.path.abspath(args.parent) if args.parent else None
    whos = ([("parent", parent)] if parent else []) + [("this commit", ROOT)]
    spread = lambda xs: max(xs) / min(xs) - 1
    bres = {who: [] for who, _ in whos}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            for who, root in whos:
                dump = os.path.join(tmp, who.replace(" ", "_")) if rnd == args.rounds - 1 else None
                bres[who].append(bench_default(root, args.steps, args.warmup, dump))
                print(f"bench.py round {rnd} {who:12s} {bres[who][-1]['steps_per_s']:.2f} steps/s", flush=True)
        lines += ["#", "# (f) the default step in bench.py (--gpus 1 --no-cpu-baseline --no-roofline --no-other-lines): steps/s per round (ms/step)"]
        for who, _ in whos:
            rs = bres[who]
            lines.append(f"  {who:12s}  {'  '.join('%.2f' % x['steps_per_s'] for x in rs)}   median {statistics.median(x['steps_per_s'] for x in rs):.2f}   "
                         f"({'  '.join('%.3f' % x['median_ms'] for x in rs)} ms)   loss {rs[-1]['loss']!r}")
        if parent:
            a, c = (statistics.median(x["steps_per_s"] for x in bres[w]) for w in ("parent", "this commit"))
            n, same = same_dumps(os.path.join(tmp, "parent"), os.path.join(tmp, "this_commit"))
            lines.append(f"# this commit against the parent: {c / a - 1:+.2%} (spread between rounds: parent {spread([x['steps_per_s'] for x in bres['parent']]):.2%}, "
                         f"this commit {spread([x['steps_per_s'] for x in bres['this commit']]):.2%}); --dump-outputs of the last round: {n} arrays, "
                         f"{'byte-identical' if same else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
