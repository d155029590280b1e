"""CPU: the host side of frozen MLPs in the bf16 precisions -- the flag bit BSMS_BWD_FROZEN_BF16 in the header and
at the entries that take `flags`, FusedStep.supports over precision x width x freeze pattern, and FusedStep on a CPU model.  No
kernel is launched (tests/test_hip_frozen_bf16.py runs them)."""
import os
import re

import pytest
import torch

from conftest import ROOT

OK, E_INVALID_ARG = 0, -1
FROZEN_BF16 = 32


def _sim(width, depth=2):
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    return eng, eng.BSMS_Simulator(ro.make_cfg(2, width, 2, depth, 2))


def test_header_constant_and_python_mirror():
    text = open(os.path.join(ROOT, "include", "bsms_hip.h")).read()
    enums = dict((k, int(v)) for k, v in re.findall(r"enum \{ (BSMS_(?:BWD|FWD)_[A-Z0-9_]+) = (\d+) \};", text))
    assert enums == {"BSMS_BWD_DEFER_JOIN": 1, "BSMS_BWD_RECOMPUTE": 2, "BSMS_FWD_LEAN": 4, "BSMS_BWD_FROZEN_BF16": 32}
    from bsms_gnn_amd import _abi, ops
    assert ops.BWD_FROZEN_BF16 == FROZEN_BF16 and (ops.FWD_LEAN, ops.BWD_RECOMPUTE) == (4, 2)
    assert _abi.lib().bsms_abi_version() == 4 and len(_abi.SIGNATURES) == 99          # no new entry, no signature changed


def test_flag_bit_at_the_entries_without_a_device():
    from bsms_gnn_amd import _abi
    L = _abi.lib()
    one = 0x1000                                                       # a non-null address that must never be dereferenced
    err = lambda: L.bsms_last_error()
    # size queries: the bit is known (a null plan table gives 0 with and without it: the sizes themselves are compared on the GPU), 64 is not
    none_pl, _keep = _abi.ptr_array([None])
    for query in (L.bsms_bsgmp_saved_bytes_ex, L.bsms_bsgmp_work_bytes_ex):
        for flags in (0, 2):
            assert query(none_pl, 0, 2, 128, 2, 3, 1, flags | FROZEN_BF16) == query(none_pl, 0, 2, 128, 2, 3, 1, flags)
        assert query(none_pl, 0, 2, 128, 2, 3, 1, 64) == 0 and query(none_pl, 0, 2, 128, 2, 3, 1, FROZEN_BF16 | 64) == 0
    a = (None, None, 0, one, one, one, 2, 128, 2, 0, 3, None)
    calls = {
        "ex": lambda flags, prec: L.bsms_bsgmp_bwd_ex(*a, one, one, one, None, prec, flags, None),
        "ev": lambda flags, prec: L.bsms_bsgmp_bwd_ev(*a, one, one, one, None, prec, flags, None, None),
        "pos_ev": lambda flags, prec: L.bsms_bsgmp_bwd_pos_ev(*a, one, one, one, None, prec, flags, None, None, None, None),
    }
    for name, call in calls.items():
        for prec in (0, 1, 2):
            for flags in (FROZEN_BF16, FROZEN_BF16 | 1, FROZEN_BF16 | 2 | 1):
                assert call(flags, prec) == E_INVALID_ARG and b"unknown bits" not in err(), (name, prec, flags)      # null plans
            for flags in (64, FROZEN_BF16 | 64, 4, 8, 16, FROZEN_BF16 | 4, FROZEN_BF16 | 8, FROZEN_BF16 | 16):
                assert call(flags, prec) == E_INVALID_ARG and b"unknown bits" in err(), (name, prec, flags)
    # the forward's `reuse` does not know the bit
    fwd = lambda reuse: L.bsms_bsgmp_fwd_p(None, None, 0, one, one, 2, 128, 2, 0, 3, None, one, one, one, reuse, 1, None)
    assert fwd(FROZEN_BF16) == E_INVALID_ARG and b"unknown bits" in err()
    assert fwd(64) == E_INVALID_ARG and b"unknown bits" in err()


PATTERNS = {
    "nothing": lambda m: None,
    "processor": lambda m: m.process.requires_grad_(False),
    "encoder": lambda m: m.encode.requires_grad_(False),
    "all_but_decoder": lambda m: (m.encode.requires_grad_(False), m.process.requires_grad_(False)),
    "everything": lambda m: m.requires_grad_(False),
    "one_edge_mlp": lambda m: m.process.down_gmps[1].mlp_edge.requires_grad_(False),
    "mixed_mlp": lambda m: m.encode.seq[0].bias.requires_grad_(False),
}


@pytest.mark.parametrize("width", [32, 128, 256])
@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16_nodes"])
def test_supports_matrix(prec, width):
    for name, freeze in PATTERNS.items():
        eng, sim = _sim(width)
        sim.process.precision = prec
        freeze(sim)
        if name == "mixed_mlp":
            want = False                                               # an MLP is frozen as a whole, in every precision
        elif name == "nothing" or prec == "f32":
            want = True
        else:
            want = width in (128, 256)                                 # a bf16 precision with frozen MLPs: the widths the bf16 kernels are built for
        assert eng.FusedStep.supports(sim) is want, (prec, width, name)
    eng, sim = _sim(width)
    sim.process.precision, sim.process.per_block = prec, True
    sim.process.requires_grad_(False)
    assert not eng.FusedStep.supports(sim)


@pytest.mark.parametrize("prec", ["bf16", "bf16_nodes"])
def test_fused_step_on_a_cpu_model_still_refuses(prec):
    """Building the step launches nothing and looks at no precision; a CPU batch is refused like every CPU batch, frozen or not."""
    eng, sim = _sim(128)
    sim.process.precision = prec
    sim.process.requires_grad_(False)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads, input_grad=True)
    assert step._frozen_bit == 0                                       # decided with the pointer tables, at the first call
    z = torch.zeros(1, 10, 5)
    data = (z, z[..., :2], z[..., :1], [torch.zeros(1, 2, 4, dtype=torch.int64)] * 3, [torch.zeros(1, 3, dtype=torch.int64)] * 2)
    with pytest.raises(eng._abi.BsmsError, match="GPU only"):
        step(data, True, None)
    with pytest.raises(eng._abi.BsmsError, match="GPU only"):
        eng.input_gradient(sim, data, param_grad=False)
    sim.requires_grad_(False)
    with pytest.raises(ValueError, match="nothing is trainable"):
        eng.FusedStep(sim, eng.GradBuckets(list(sim.parameters())))
    sim.process.down_gmps[0].mlp_node.seq[0].bias.requires_grad_(True)
    with pytest.raises(ValueError, match="frozen as a whole"):
        eng.FusedStep(sim, eng.GradBuckets(list(sim.parameters())), input_grad=True)._pointer_tables()
