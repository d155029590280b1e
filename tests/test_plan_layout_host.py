"""The layout of a plan's two index blocks (csrc/common.h: main_layout / pool_layout / main_ptrs / pool_ptrs), the one statement that
bsms_plan_create, bsms_plan_set_pool, the plan's own pointers, bsms_plan_concat and k_plan_concat take their offsets from, against a
plain restatement of the layout:

    every array padded to 64 int32 words;
    main block   rowptr[N+1] | t_rowptr[N+1] | src[E] | dst[E] | perm[E] | t_dst[E] | t_eid[E] | t_pos[E]
    pool block   ids[Nk] | inv[N] | k_rowptr[Nk+1] | k_src[Ek] | k_eid[Ek] | p_rowptr[N+1] | p_src[Ep] | p_eid[Ep] | k_w[Ek] | p_w[Ep]

A drifted offset is silently wrong indices in HBM, not a failed build; this pins the statement without a device.  CPU only: a small
stand-alone program (its own main, common.h included, no call into the HIP runtime, no library loaded) is compiled with g++ as plain
C++, the way the host-sanitizer library compiles plan.hip, and prints the offsets and word counts for the sizes below -- through the
layout structs AND through the pointer templates, for int32_t* and const int32_t*."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bsms-gnn_amd", "csrc")
ALIGN = 64

MAIN = ("rowptr", "t_rowptr", "src", "dst", "perm", "t_dst", "t_eid", "t_pos")
POOL = ("ids", "inv", "k_rowptr", "k_src", "k_eid", "p_rowptr", "p_src", "p_eid", "k_w", "p_w")

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include "common.h"
using namespace bsms;
int main() {
  long long N, E, Nk, Ek, Ep;
  static int32_t word;   // a base to take pointer differences from; never dereferenced
  while (std::scanf("%lld %lld %lld %lld %lld", &N, &E, &Nk, &Ek, &Ep) == 5) {
    const MainLayout m = main_layout(N, E);
    const PoolLayout k = pool_layout(N, Nk, Ek, Ep);
    std::printf("L %zu %zu %zu %zu %zu %zu %zu %zu %zu | %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", m.rowptr, m.t_rowptr, m.src, m.dst,
                m.perm, m.t_dst, m.t_eid, m.t_pos, m.words, k.ids, k.inv, k.k_rowptr, k.k_src, k.k_eid, k.p_rowptr, k.p_src, k.p_eid, k.k_w,
                k.p_w, k.words);
    const MainPtrs<int32_t> mp = main_ptrs(&word, N, E);
    const PoolPtrs<int32_t> kp = pool_ptrs(&word, N, Nk, Ek, Ep);
    const MainPtrs<const int32_t> mc = main_ptrs<const int32_t>(&word, N, E);
    const PoolPtrs<const int32_t> kc = pool_ptrs<const int32_t>(&word, N, Nk, Ek, Ep);
#define D(p) (long long)((p) - &word)
    std::printf("P %lld %lld %lld %lld %lld %lld %lld %lld | %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", D(mp.rowptr), D(mp.t_rowptr),
                D(mp.src), D(mp.dst), D(mp.perm), D(mp.t_dst), D(mp.t_eid), D(mp.t_pos), D(kp.ids), D(kp.inv), D(kp.k_rowptr), D(kp.k_src),
                D(kp.k_eid), D(kp.p_rowptr), D(kp.p_src), D(kp.p_eid), D(kp.k_w), D(kp.p_w));
    std::printf("C %lld %lld %lld %lld %lld %lld %lld %lld | %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", D(mc.rowptr), D(mc.t_rowptr),
                D(mc.src), D(mc.dst), D(mc.perm), D(mc.t_dst), D(mc.t_eid), D(mc.t_pos), D(kc.ids), D(kc.inv), D(kc.k_rowptr), D(kc.k_src),
                D(kc.k_eid), D(kc.p_rowptr), D(kc.p_src), D(kc.p_eid), D(kc.k_w), D(kc.p_w));
  }
  return 0;
}
"""


def pad(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def offsets(lengths):
    """Padded start of every array laid one behind the other, and the total."""
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += pad(n)
    return out, at


def expected(N, E, Nk, Ek, Ep):
    main, words = offsets([N + 1, N + 1, E, E, E, E, E, E])
    pool, pool_words = offsets([Nk, N, Nk + 1, Ek, Ek, N + 1, Ep, Ep, Ek, Ep])
    return main, words, pool, pool_words


# every padding edge: N + 1 and Nk + 1 at 64 and 65; E, Ek, Ep and Nk at 0, 1, 64 and 65; Nk = 0 with a pool; and one real level
EDGE = (0, 1, 64, 65)
SIZES = [(N, E, Nk, Ek, Ep) for N, E, Nk, Ek, Ep in itertools.product((63, 64, 200), EDGE, (0, 1, 63, 64, 65), EDGE, EDGE) if Nk <= N]
SIZES += [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 1, 1, 1), (250832, 1503344, 62708, 376212, 375800)]


def test_the_cases_sit_on_every_padding_edge():
    for col in (1, 2, 3, 4):                                    # E, Nk, Ek, Ep
        assert {0, 1, 64, 65} <= {s[col] for s in SIZES}
    assert {64, 65} <= {s[0] + 1 for s in SIZES} and {64, 65} <= {s[2] + 1 for s in SIZES}
    assert any(s[2] == 0 and s[0] > 0 for s in SIZES)
    # the restatement itself, on a case worked by hand: N = 64, E = 65, Nk = 1, Ek = 64, Ep = 0
    main, words, pool, pool_words = expected(64, 65, 1, 64, 0)
    assert main == [0, 128, 256, 384, 512, 640, 768, 896] and words == 1024
    assert pool == [0, 64, 128, 192, 256, 320, 448, 448, 448, 512] and pool_words == 512


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_layout_statement_matches_the_written_out_formulas(tmp_path):
    src, exe = tmp_path / "layout.cc", tmp_path / "layout"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % s for s in SIZES), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * len(SIZES)
    for i, s in enumerate(SIZES):
        main, words, pool, pool_words = expected(*s)
        kind, got = zip(*(ln.split(" ", 1) for ln in lines[3 * i:3 * i + 3]))
        assert kind == ("L", "P", "C")
        got = [[[int(v) for v in half.split()] for half in g.split("|")] for g in got]
        assert got[0] == [main + [words], pool + [pool_words]], (s, dict(zip(MAIN + ("words",), got[0][0])), dict(zip(POOL + ("words",), got[0][1])))
        assert got[1] == [main, pool], ("int32_t*", s, got[1])
        assert got[2] == [main, pool], ("const int32_t*", s, got[2])
