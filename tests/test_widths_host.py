"""Latent widths at the C ABI, without a GPU: every multiple of 32 from 32 to 256 is accepted (include/bsms_hip.h), others
are refused before any argument is looked at."""
import pytest

NEW_WIDTHS = [96, 160, 192, 224]


@pytest.fixture(scope="module")
def L():
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_abi_version_unchanged(L):
    assert L.bsms_abi_version() == 4


def test_size_queries_cover_the_new_widths(L):
    # (128 and 256 are left out of the ordering: their work areas also hold the bf16 precisions' fused-backward partials)
    widths = [32, 64, 96, 160, 192, 224]
    mlp_saved = [L.bsms_mlp_saved_bytes(1000, 3, D, D, 3) for D in widths]
    mlp_work = [L.bsms_mlp_work_bytes(1000, 3, D, D, 3) for D in widths]
    gmp_saved = [L.bsms_gmp_saved_bytes(2, 500, 3000, D, 3) for D in widths]
    gmp_work = [L.bsms_gmp_work_bytes(2, 500, 3000, D, 3) for D in widths]
    for sizes in (mlp_saved, mlp_work, gmp_saved, gmp_work):
        assert all(s > 0 for s in sizes), sizes
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes


@pytest.mark.parametrize("D", NEW_WIDTHS)
def test_new_width_passes_the_width_check(L, D):
    # the width is accepted: the call gets as far as the null input and reports that instead
    assert L.bsms_mlp_fwd(None, 10, D, D, D, 3, 1, None, None, None, None, None) == -1
    err = L.bsms_last_error()
    assert b"null argument" in err and b"not supported" not in err


@pytest.mark.parametrize("D", [48, 80, 288, 512])
def test_other_widths_still_refused(L, D):
    assert L.bsms_mlp_fwd(None, 10, D, D, D, 3, 1, None, None, None, None, None) == -3
    assert b"not supported" in L.bsms_last_error()
