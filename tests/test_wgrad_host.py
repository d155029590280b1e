"""CPU: argument validation of the weight-gradient primitives bsms_wgrad / bsms_small_wgrad (include/bsms_hip.h).  Every rejected
call returns its error code with a message BEFORE anything is launched: without a GPU a launch would come back as BSMS_E_HIP (-4),
so the specific codes asserted here also show that no launch was attempted.  The pointers are made-up addresses that no accepted
path may dereference; cases that test an early check carry a second, later defect (a null dW), so that a broken early check
still ends in an error code and never in a launch."""
import ctypes as C

import pytest

INVALID, SHAPE, UNSUPPORTED = -1, -2, -3
P = 0x10000                      # a 16-byte aligned, never dereferenced "device" address


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from bsms_gnn_amd import _abi
    return _abi.lib()


def job(**kw):
    from bsms_gnn_amd._abi import WgradJob
    f = dict(G=P, A=P, dW=P, db=P, R=100, ldg=128, lda=128, ldw=128, col0=0, bf16=0, g_bound=None, a_bound=None, g_mul=1.0, a_mul=1.0)
    f.update(kw)
    return WgradJob(**f)


def table(*jobs):
    from bsms_gnn_amd._abi import WgradJob
    return (WgradJob * len(jobs))(*jobs)


def err(L):
    return L.bsms_last_error().decode()


def test_struct_layout_matches_the_header():
    """bsms_wgrad_job: four pointers, R, five ints (+ 4 bytes of padding), two pointers, two floats -- 88 bytes with natural alignment."""
    from bsms_gnn_amd._abi import WgradJob
    assert C.sizeof(WgradJob) == 88
    assert [getattr(WgradJob, n).offset for n in ("G", "A", "dW", "db", "R", "ldg", "col0", "bf16", "g_bound", "a_bound", "g_mul", "a_mul")] == \
        [0, 8, 16, 24, 32, 40, 52, 56, 64, 72, 80, 84]


def test_size_queries(L):
    assert L.bsms_wgrad_bound_width() == 8192
    sizes = {D: L.bsms_wgrad_work_bytes(D, 20) for D in range(32, 257, 32)}
    assert all(v >= 1024 * 128 * 128 * 4 for v in sizes.values())            # 1024 partial tiles of 128 x 128 floats at least
    for D in (0, 16, 48, 288, -32):
        assert L.bsms_wgrad_work_bytes(D, 1) == 0 and L.bsms_small_wgrad_work_bytes(D) == 0
    assert L.bsms_wgrad_work_bytes(128, 21) == 0 and L.bsms_wgrad_work_bytes(128, -1) == 0
    for D in range(32, 257, 32):
        assert L.bsms_small_wgrad_work_bytes(D) >= 512 * 10 * D * 4            # 512 partial blocks of (8 + 2) x D floats


def test_wgrad_rejects_before_any_launch(L):
    D, wb = 128, L.bsms_wgrad_work_bytes(128, 20)
    ok = job()
    # empty call: nothing to do, nothing launched
    assert L.bsms_wgrad(None, 0, D, 0, None, 0, None) == 0
    # null jobs with njobs > 0
    assert L.bsms_wgrad(None, 1, D, 0, P, wb, None) == INVALID and "jobs is null" in err(L)
    # more than 20 jobs, negative count
    many = table(*[job(dW=None) for _ in range(21)])
    assert L.bsms_wgrad(many, 21, D, 0, P, wb, None) == INVALID and "21 jobs" in err(L)
    assert L.bsms_wgrad(many, -1, D, 0, P, wb, None) == INVALID
    # D outside the envelope
    for bad in (0, 16, 48, 130, 288, -128):
        assert L.bsms_wgrad(table(job(dW=None)), 1, bad, 0, P, wb, None) == UNSUPPORTED, bad
        assert "not supported" in err(L)
    # work: null, misaligned, too small
    assert L.bsms_wgrad(table(job(dW=None)), 1, D, 0, None, wb, None) == INVALID and "work" in err(L)
    assert L.bsms_wgrad(table(job(dW=None)), 1, D, 0, P + 4, wb, None) == INVALID and "work" in err(L)
    assert L.bsms_wgrad(table(job(dW=None)), 1, D, 0, P, wb - 1, None) == INVALID and "bytes" in err(L)
    assert L.bsms_wgrad(table(job(dW=None)), 1, D, 0, P, 0, None) == INVALID
    # R out of range -- also on a job that is skipped (its row count shapes the launch of the others)
    for R in (-1, 2 ** 31, 2 ** 40):
        assert L.bsms_wgrad(table(job(R=R, dW=None)), 1, D, 0, P, wb, None) == SHAPE and "R=" in err(L)
        assert L.bsms_wgrad(table(job(dW=None), job(R=R, dW=None)), 2, D, 0b10, P, wb, None) == SHAPE and "job 1" in err(L)
    # row pitches: below D, not a multiple of the 16-byte load, out of range; bf16 rows count 8 elements per load
    for kw in (dict(ldg=127), dict(ldg=124), dict(ldg=130), dict(lda=64), dict(lda=133), dict(ldg=-128), dict(lda=1 << 24),
               dict(bf16=1, ldg=132), dict(bf16=1, lda=140)):
        assert L.bsms_wgrad(table(job(dW=None, **kw)), 1, D, 0, P, wb, None) == SHAPE, kw
        assert "ldg=" in err(L) or "lda=" in err(L)
    # the dW block must fit into its matrix
    for kw in (dict(ldw=127), dict(ldw=200, col0=73), dict(col0=-1, ldw=256), dict(ldw=1 << 24)):
        assert L.bsms_wgrad(table(job(dW=None, **kw)), 1, D, 0, P, wb, None) == SHAPE, kw
        assert "ldw=" in err(L)
    # null G / A / dW on a job that runs (db is nullable and is not among them)
    for name in ("G", "A", "dW"):
        assert L.bsms_wgrad(table(ok, job(**{name: None})), 2, D, 0, P, wb, None) == INVALID, name
        assert "job 1" in err(L) and "null" in err(L)
    # misaligned pointers: 16-byte row loads, the float4 stores of db and of an aligned dW block, the bound slots
    for kw in (dict(G=P + 4), dict(A=P + 8), dict(db=P + 4), dict(dW=P + 4), dict(dW=P + 2, ldw=259, col0=3),
               dict(g_bound=P + 4, a_bound=P), dict(g_bound=P, a_bound=P + 12)):
        assert L.bsms_wgrad(table(job(**kw)), 1, D, 0, P, wb, None) == INVALID, kw
        assert "aligned" in err(L)
    # a bounded (fp16 x 2) job needs usable multipliers
    for kw in (dict(g_mul=0.0), dict(a_mul=-1.0), dict(g_mul=float("inf")), dict(a_mul=float("nan"))):
        assert L.bsms_wgrad(table(job(g_bound=P, a_bound=P, **kw)), 1, D, 0, P, wb, None) == INVALID, kw
        assert "g_mul" in err(L)
    # a call whose jobs are all skipped is accepted with null pointers and launches nothing
    null = job(G=None, A=None, dW=None, db=None)
    assert L.bsms_wgrad(table(null, null), 2, D, 0b11, P, wb, None) == 0


def test_small_wgrad_rejects_before_any_launch(L):
    D, wb = 96, L.bsms_small_wgrad_work_bytes(96)

    def call(G=P, S=P, R=100, D=D, S_cols=3, S_ld=0, out=P, os=1, of=3, colsum=None, colsum_S=None, work=P, work_bytes=wb):
        return L.bsms_small_wgrad(G, S, R, D, S_cols, S_ld, out, os, of, colsum, colsum_S, work, work_bytes, None)

    for bad in (0, 16, 100, 288):
        assert call(D=bad, out=None) == UNSUPPORTED and "not supported" in err(L)
    for bad in (0, 9, -1):
        assert call(S_cols=bad, out=None) == UNSUPPORTED and "narrow width" in err(L)
    for bad in (-1, 2 ** 31):
        assert call(R=bad, out=None) == SHAPE and "R=" in err(L)
    for bad in (2, -4):
        assert call(S_ld=bad, out=None) == SHAPE and "S_ld=" in err(L)
    for kw in (dict(os=0), dict(of=0), dict(os=-1)):
        assert call(out=None, **kw) == SHAPE and "strides" in err(L)
    for kw in (dict(G=None), dict(S=None), dict(out=None), dict(work=None)):
        assert call(**kw) == INVALID and "null" in err(L), kw
    # 16-byte loads of G always, of S when its row pitch is a multiple of 4 (S_ld = 4 here; S_cols = 3 rows are read by element)
    assert call(G=P + 4) == INVALID and "aligned" in err(L)
    assert call(S=P + 4, S_ld=4) == INVALID and "aligned" in err(L)
    assert call(S=P + 4, S_cols=8, of=8) == INVALID and "aligned" in err(L)
    assert call(work=P + 8) == INVALID and "aligned" in err(L)
    assert call(work_bytes=wb - 1) == INVALID and "bytes" in err(L)
    assert call(work_bytes=L.bsms_small_wgrad_work_bytes(64), D=128) == INVALID
