"""CPU: the host side of the pack group (bsms_pack_group_*) -- every refusal returns its error code from host
code, before any device call: this file runs where there is no GPU, with addresses that must never be dereferenced.  What the
group's launch writes is pinned on the GPU (tests/test_hip_pack_group.py)."""
import ctypes as C

import pytest

OK, E_INVALID_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3
ONE = 0x1000                                                           # a non-null address nobody may dereference
H, D = 3, 128


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from bsms_gnn_amd import _abi
    return _abi.lib()


@pytest.fixture
def group(L):
    h = C.c_void_p()
    assert L.bsms_pack_group_create(C.cast(C.byref(h), C.POINTER(C.c_void_p))) == OK and h.value
    yield h
    L.bsms_pack_group_destroy(h)                                       # never launched: host memory only


def arr(vals):
    return C.cast((C.c_void_p * len(vals))(*vals), C.POINTER(C.c_void_p))


def mlp(L, g, params="all", saved=ONE, work=None, R=100, in_dim=3, width=D, out_dim=D, hidden=H, ln=1):
    n = 2 * (max(hidden, 0) + 1)
    pp = arr([ONE] * n) if params == "all" else params
    return L.bsms_pack_group_add_mlp(g, R, in_dim, width, out_dim, hidden, ln, pp, saved, work)


def test_create_and_destroy_take_null(L):
    assert L.bsms_pack_group_create(None) == E_INVALID_ARG
    L.bsms_pack_group_destroy(None)


def test_null_group_is_refused_everywhere(L):
    assert mlp(L, None) == E_INVALID_ARG and b"group is null" in L.bsms_last_error()
    assert L.bsms_pack_group_add_bsgmp(None, arr([ONE]), 0, 2, D, 2, H, arr([ONE] * 16), ONE, None, 0) == E_INVALID_ARG
    assert L.bsms_pack_group_launch(None, None) == E_INVALID_ARG


def test_an_empty_group_launches_nothing(L, group):
    assert L.bsms_pack_group_launch(group, None) == OK                 # no pack, no bound array: no device call
    assert mlp(L, group) == OK                                         # ... and the group is not sealed by it


def test_add_mlp_refusals(L, group):
    assert mlp(L, group, params=None) == E_INVALID_ARG
    assert mlp(L, group, saved=None, work=None) == E_INVALID_ARG       # neither the training nor the inference layout
    holes = [ONE] * (2 * (H + 1))
    holes[4] = None
    assert mlp(L, group, params=arr(holes)) == E_INVALID_ARG and b"parameter 4" in L.bsms_last_error()
    for width in (0, 16, 48, 288, 512):                                # a multiple of 32, 32..256
        assert mlp(L, group, width=width, out_dim=width) == E_UNSUPPORTED, width
    for hidden in (0, -1, 8):
        assert mlp(L, group, hidden=hidden) == E_UNSUPPORTED, hidden
    assert mlp(L, group, R=-1) == E_SHAPE
    assert mlp(L, group, in_dim=9) == E_UNSUPPORTED                    # neither narrow (<= 8) nor D
    assert mlp(L, group, in_dim=D, out_dim=3, ln=1) == E_UNSUPPORTED   # a narrow output has no LayerNorm
    assert mlp(L, group, in_dim=D, out_dim=9, ln=0) == E_UNSUPPORTED
    # nothing above was added: the group is still empty, and an empty group launches nothing
    assert L.bsms_pack_group_launch(group, None) == OK
    # the three supported shapes, training and inference layout
    assert mlp(L, group) == OK and mlp(L, group, in_dim=D) == OK and mlp(L, group, in_dim=D, out_dim=3, ln=0) == OK
    assert mlp(L, group, saved=None, work=ONE) == OK


def test_add_bsgmp_refusals(L, group):
    n = 4 * (H + 1)
    call = lambda plans=arr([None]), depth=0, B=2, width=D, p=2, hidden=H, params=arr([ONE] * n), saved=ONE, work=None, prec=0: \
        L.bsms_pack_group_add_bsgmp(group, plans, depth, B, width, p, hidden, params, saved, work, prec)
    assert call(plans=None) == E_INVALID_ARG
    assert call(depth=-1) == E_INVALID_ARG and call(depth=17) == E_INVALID_ARG
    assert call() == E_INVALID_ARG and b"plan of level 0 is null" in L.bsms_last_error()
    assert L.bsms_pack_group_launch(group, None) == OK                 # still empty
    # (the checks behind the plan table -- width, hidden, pos_dim, precision, parameters -- need a plan, which lives on the device:
    # tests/test_hip_pack_group.py::test_add_bsgmp_refusals_with_a_plan)


def test_abi_version_is_unchanged(L):
    assert L.bsms_abi_version() == 4                                   # entries were added, no signature changed
