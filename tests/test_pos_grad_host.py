"""CPU: the position-gradient entries of the C ABI (bsms_gmp_bwd_pos, bsms_bsgmp_bwd_pos and their size queries) are
exported and bound, the size queries answer without a GPU, and the argument checks return their documented codes and
messages before anything touches a device."""
import ctypes as C

import pytest

NEW = ("bsms_gmp_pos_work_bytes", "bsms_gmp_bwd_pos", "bsms_bsgmp_pos_work_bytes", "bsms_bsgmp_bwd_pos")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_new_symbols_exported_and_bound(lib):
    from bsms_gnn_amd import _abi
    raw = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in _abi.SIGNATURES, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1], name
    assert lib.bsms_abi_version() == 4


def test_size_queries(lib):
    B, E = 8, 31354                       # airfoil level 0 (bench workload)
    for p in range(1, 8):
        n = lib.bsms_gmp_pos_work_bytes(B, E, p)
        assert n >= B * E * (4 if p <= 3 else 8) * 4, (p, n)    # one fiber-pitch row of d r_e per edge
    assert lib.bsms_gmp_pos_work_bytes(1, 0, 2) > 0             # an edgeless graph is a valid shape
    assert lib.bsms_gmp_pos_work_bytes(B, E, 0) == 0 and lib.bsms_gmp_pos_work_bytes(B, E, 8) == 0
    assert lib.bsms_gmp_pos_work_bytes(-1, E, 2) == 0 and lib.bsms_gmp_pos_work_bytes(B, -1, 2) == 0
    assert lib.bsms_bsgmp_pos_work_bytes(None, 0, 1, 2) == 0    # no plans
    assert lib.bsms_bsgmp_pos_work_bytes(None, 3, 1, 9) == 0


def _gmp_bwd_pos(lib, p, grad_pos, pos_work):
    return lib.bsms_gmp_bwd_pos(None, None, None, None, 1, 128, p, 0, 3, None, None, None, None, None, grad_pos, pos_work,
                                None)


def _bsgmp_bwd_pos(lib, p, grad_pos, pos_work):
    return lib.bsms_bsgmp_bwd_pos(None, None, 2, None, None, None, 1, 128, p, 0, 3, None, None, None, None, None, 0,
                                  grad_pos, pos_work, None)


def test_argument_validation(lib):
    host = C.create_string_buffer(64)     # a non-null address; the checks return before it could be used
    addr = C.addressof(host)
    for call, who in ((_gmp_bwd_pos, b"gmp_bwd_pos"), (_bsgmp_bwd_pos, b"bsgmp_bwd_pos")):
        assert call(lib, 2, addr, None) == -1                    # BSMS_E_INVALID_ARG
        msg = lib.bsms_last_error()
        assert who in msg and b"pos_work" in msg, msg
        for p in (0, 8, -3):
            assert call(lib, p, None, None) == -1
            msg = lib.bsms_last_error()
            assert who in msg and b"pos_dim" in msg, msg
        # with the position arguments in order, the checks of the entry it extends follow (here: no plans)
        assert call(lib, 2, None, None) == -1
        assert b"pos_work" not in lib.bsms_last_error() and b"pos_dim" not in lib.bsms_last_error()
