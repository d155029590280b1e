"""Every chain launch shape of ROWS below (the row counts of tests/test_chain_launch_host.py) on the device, for comparing two builds of the libraries:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python profiles/chain_launch_trace.py DIR > OUT/hashes.txt
    python profiles/chain_launch_trace.py --kernels OUT_A OUT_B        # afterwards: the two kernel lists, compared

DIR holds libbsms_hip.so and its companions (as profiles/piece_sum_bits.py).  For every latent width and every row count of ROWS
the script runs, on seeded inputs,
  the MLP in its three forms (encoder 3 -> D, D -> D, decoder D -> 3; bsms_mlp_fwd / bsms_mlp_bwd): inference forward, training
      forward, backward, and the backward of the frozen MLP (input gradient only);
  one GMP block in fp32 (eng.GMP: bsms_gmp_fwd / bsms_gmp_bwd) and, at D = 128 / 256, in bf16 and bf16_nodes (the precisions exist
      behind the U-Net entries only: eng.BSGMP at depth 0, bsms_bsgmp_fwd_p / bsms_bsgmp_bwd_p on one level), once with the row count
      as its EDGE rows (a random graph on rows / 6 nodes) and once as its NODE rows (a ring): the same four calls;
and prints one line per output buffer with its SHA-256, then the number of lines and the SHA-256 of all of them.  Two builds launch
the same things iff their kernel traces agree line for line in name, grid, workgroup size and LDS, and compute the same things iff
these outputs agree (profiles/chain_launch_refactor.txt).  `--widths 128,256` restricts the widths."""
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (32, 64, 96, 128, 160, 192, 224, 256)
# rows on both sides of every launch threshold at 256 CUs, by resident workgroups per CU (4 at D <= 64, 2 at D = 128, else 1); what each
# row count is for: tests/test_chain_launch_host.py
ROWS = {
    4: (1, 1000, 16384, 16385, 65536, 65537, 250832),
    2: (1, 17, 1000, 3072, 3073, 6144, 6145, 16384, 16385, 28671, 28672, 28673, 32768, 32769, 40960, 40961, 49152, 49153, 57344, 57345,
        65536, 90112, 250832),
    1: (1, 1000, 16384, 16385, 20480, 20481, 24576, 24577, 28671, 28672, 28673, 32768, 32769, 57344, 57345, 90112, 250832),
}
resident = lambda D: 4 if D <= 64 else 2 if D == 128 else 1


def compare_kernels(dir_a, dir_b):
    def kernels(d):
        (path,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
        xyz = lambda r, col: "x".join(r[f"{col}_{c}"] for c in "XYZ")        # kernel-trace CSV: Grid_Size_X/_Y/_Z, Workgroup_Size_X/_Y/_Z
        return [(r["Kernel_Name"], xyz(r, "Grid_Size"), xyz(r, "Workgroup_Size"), r["LDS_Block_Size"]) for r in rows]
    a, b = kernels(dir_a), kernels(dir_b)
    chain = lambda ks: [k for k in ks if any(s in k[0] for s in ("k_chain_", "k_edge_", "k_fs_"))]
    digest = lambda ks: hashlib.sha256("\n".join(" ".join(k) for k in ks).encode()).hexdigest()
    print(f"A: {len(a)} kernels ({len(chain(a))} chain launches, {len(set(chain(a)))} distinct) {digest(a)}")
    print(f"B: {len(b)} kernels ({len(chain(b))} chain launches, {len(set(chain(b)))} distinct) {digest(b)}")
    same = a == b
    print("in dispatch order, line for line (name, grid, workgroup size, LDS):", "EQUAL" if same else "DIFFERENT")
    if not same:
        print("as sorted lists:", "EQUAL" if sorted(a) == sorted(b) else "DIFFERENT", "; the chain launches in order:",
              "EQUAL" if chain(a) == chain(b) else "DIFFERENT")
        for i, (x, y) in enumerate(zip(chain(a), chain(b))):
            if x != y:
                print(f"first difference among the chain launches, #{i}:\n  A {x}\n  B {y}")
                break
    return 0 if same or chain(a) == chain(b) and sorted(a) == sorted(b) else 1


def main(lib_dir, widths):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bsms_gnn_amd as eng
    from bsms_gnn_amd import _abi
    lib_dir = os.path.abspath(lib_dir)
    _abi.LIB_PATH = os.path.join(lib_dir, "libbsms_hip.so")            # before the first lib()
    _abi.EXT_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_ext.so")
    _abi.STATS_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_stats.so")
    _abi.SAMPLE_LIB_PATH = os.path.join(lib_dir, "libbsms_hip_sample.so")
    _abi.lib()
    total, count = hashlib.sha256(), [0]

    def report(tag, t):
        line = f"{tag} {hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()}"       # .cpu() waits for the stream
        print(line, flush=True)
        total.update((line + "\n").encode())
        count[0] += 1

    def four_calls(tag, net, call, x):
        """Inference forward, training forward, backward, backward of the frozen net: every output and gradient."""
        with torch.no_grad():
            report(f"{tag} inference y", call(x))
        for frozen in (False, True):
            for q in net.parameters():
                q.requires_grad_(not frozen)
                q.grad = None
            xx = x.clone().requires_grad_(True)
            y = call(xx)
            if not frozen:
                report(f"{tag} training y", y)
            torch.manual_seed(7)
            (y * torch.randn_like(y)).sum().backward()
            report(f"{tag} {'frozen ' if frozen else ''}grad_x", xx.grad)
            for k, q in net.named_parameters():
                if q.grad is not None:
                    report(f"{tag} grad {k}", q.grad)

    for D in widths or WIDTHS:
        for R in ROWS[resident(D)]:
            for in_dim, out_dim, ln in ((3, D, True), (D, D, True), (D, 3, False)):
                torch.manual_seed(1000 + D)
                mlp = eng.MLP(in_dim, D, out_dim, 3, ln).cuda()
                torch.manual_seed(R)
                four_calls(f"mlp {in_dim}->{out_dim} D={D} R={R}", mlp, mlp, torch.randn(R, in_dim, device="cuda"))
            for rows_are, n, e in (("edges", max(R // 6, 2), R), ("nodes", max(R, 2), max(R, 2))):
                rng = np.random.default_rng(R)
                src = rng.integers(0, n, e) if rows_are == "edges" else np.arange(n)
                dst = (src + 1 + (rng.integers(0, n - 1, e) if rows_are == "edges" else 0)) % n
                g = torch.from_numpy(np.stack([src, dst])).cuda()
                for precision in ("f32", "bf16", "bf16_nodes") if D in (128, 256) else ("f32",):
                    torch.manual_seed(2000 + D)
                    net = eng.GMP(D, 3, 2).cuda() if precision == "f32" else eng.BSGMP(0, D, 3, 2).cuda()
                    torch.manual_seed(R + 1)
                    x, pos = torch.randn(1, n, D, device="cuda"), torch.rand(1, n, 2, device="cuda")
                    if precision == "f32":
                        call = lambda h: net(h, g, pos)
                    else:
                        net.precision = precision
                        call = lambda h: net(h, [], [g], pos)
                    four_calls(f"gmp {precision} D={D} {rows_are}={R}", net, call, x)
    print(f"all {count[0]} lines {total.hexdigest()}")


if __name__ == "__main__":
    if sys.argv[1] == "--kernels":
        sys.exit(compare_kernels(sys.argv[2], sys.argv[3]))
    w = [int(v) for v in sys.argv[sys.argv.index("--widths") + 1].split(",")] if "--widths" in sys.argv else None
    main(sys.argv[1], w)
