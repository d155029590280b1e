"""CPU: the host side of frozen parameters -- FusedStep.supports at MLP granularity, GradBuckets over a partly
frozen model, the cache key of input_gradient, the argument checks of FusedStep, the bucket schedule when blocks run no side
lane, and the host checks of bsms_mlp_bwd_ex's `grads` table.  No kernel is launched (tests/test_hip_frozen.py runs them)."""
import ctypes as C

import pytest
import torch

OK, E_INVALID_ARG = 0, -1


def _sim(depth=2):
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    return eng, eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, depth, 2))


def test_supports_is_decided_per_mlp():
    eng, sim = _sim()
    assert eng.FusedStep.supports(sim)
    sim.process.requires_grad_(False)                                  # every block's two MLPs frozen, encoder and decoder trainable
    assert eng.FusedStep.supports(sim)
    sim.process.requires_grad_(True)
    sim.process.down_gmps[1].mlp_edge.requires_grad_(False)            # one MLP of one block
    sim.decode.requires_grad_(False)
    assert eng.FusedStep.supports(sim)
    sim.process.precision = "bf16"                                     # frozen + a bf16 precision: the autograd route
    assert not eng.FusedStep.supports(sim)
    sim.process.precision = "f32"
    sim.encode.seq[0].bias.requires_grad_(False)                       # mixed within an MLP
    assert not eng.FusedStep.supports(sim)
    sim.requires_grad_(False)                                          # nothing trainable: legal (a data-only step)
    assert eng.FusedStep.supports(sim)
    _, sim = _sim()
    sim.process.precision = "bf16_nodes"                               # nothing frozen: any precision, as before
    assert eng.FusedStep.supports(sim)
    sim.process.per_block = True
    assert not eng.FusedStep.supports(sim)


def test_grad_buckets_lay_out_the_trainable_slots_only():
    eng, sim = _sim()
    sim.process.requires_grad_(False)
    grads = eng.GradBuckets(list(sim.parameters()), bucket_bytes=4 << 10)
    live = [*sim.encode.parameters(), *sim.decode.parameters()]
    assert grads.params == live and grads.flat.numel() == sum(q.numel() for q in live)
    off = 0
    for q in reversed(live):                                           # reversed parameter order, no holes for the frozen ones
        assert grads._slot[q] == (off, q.numel()) and q._bsms_grad_slot[1:] == (off, q.numel())
        off += q.numel()
    assert all(q not in grads._slot and not hasattr(q, "_bsms_grad_slot") for q in sim.process.parameters())
    assert sum(len(b["params"]) for b in grads.buckets) == len(live) and sum(b["view"].numel() for b in grads.buckets) == grads.flat.numel()
    sim.requires_grad_(False)
    empty = eng.GradBuckets(list(sim.parameters()))                    # nothing trainable: an empty buffer, no bucket
    assert empty.params == [] and empty.flat.numel() == 0 and empty.buckets == [] and empty.flat.dtype == torch.float32
    empty.zero()
    empty.finish()


def test_input_gradient_cache_key_separates_param_grad():
    import inspect
    eng, sim = _sim()
    from bsms_gnn_amd.step import _input_gradient_key
    obj = eng.Objective()
    a, b = _input_gradient_key(2, None, False, obj, True), _input_gradient_key(2, None, False, obj, False)
    assert a != b and a[:-1] == b[:-1]
    assert _input_gradient_key(2, [0.5, 0.5], 0, obj, 1) == _input_gradient_key(2, (0.5, 0.5), False, obj, True)
    sig = inspect.signature(eng.input_gradient)
    assert sig.parameters["param_grad"].default is True                # today's behaviour unless asked
    z = torch.zeros(1, 10, 5)
    data = (z, z[..., :2], z[..., :1], [torch.zeros(1, 2, 4, dtype=torch.int64)] * 3, [torch.zeros(1, 3, dtype=torch.int64)] * 2)
    with pytest.raises(eng._abi.BsmsError, match="GPU only"):           # refused like every CPU batch, and nothing was attached to the model
        eng.input_gradient(sim, data, param_grad=False)
    assert "grads" not in sim._bsms_input_grad_steps and all(q.grad is None for q in sim.parameters())
    assert all(not hasattr(q, "_bsms_grad_slot") for q in sim.parameters())


def test_fused_step_validates_param_grad():
    eng, sim = _sim()
    grads = eng.GradBuckets(list(sim.parameters()))
    with pytest.raises(ValueError, match="compute nothing"):
        eng.FusedStep(sim, grads, param_grad=False)
    with pytest.raises(ValueError, match="GradBuckets"):
        eng.FusedStep(sim, None, input_grad=True)
    step = eng.FusedStep(sim, None, input_grad=True, param_grad=False)
    assert step.grads is None and all(q.grad is None for q in sim.parameters())
    sim.requires_grad_(False)                                          # nothing trainable and no input gradient: refused when built
    empty = eng.GradBuckets(list(sim.parameters()))
    with pytest.raises(ValueError, match="nothing is trainable"):
        eng.FusedStep(sim, empty)
    assert eng.FusedStep(sim, empty, input_grad=True)._any_live is False


def test_bucket_schedule_skips_blocks_without_side_lanes():
    """Execution order of the backward: up_gmps[L-1] .. up_gmps[0], bottom, down_gmps[L-1] .. down_gmps[0].  The decoder's deferred
    weight gradients are covered by the event of the first block that runs side lanes -- a block with both MLPs frozen records
    its event on the caller's stream -- or, with the whole processor frozen, only by the final join."""
    eng, sim = _sim(depth=2)
    decoder_stage = lambda step, grads: {st for bk, st in zip(grads.buckets, step._bucket_schedule(2)) if any(q in set(sim.decode.parameters()) for q in bk["params"])}
    grads = eng.GradBuckets(list(sim.parameters()), bucket_bytes=1 << 10)
    assert 0 in decoder_stage(eng.FusedStep(sim, grads), grads)        # nothing frozen: the first block, as before
    sim.process.up_gmps[1].requires_grad_(False)                       # execution index 0 runs no lane
    sim.process.up_gmps[0].mlp_node.requires_grad_(False)              # execution index 1 still does (its edge MLP)
    grads = eng.GradBuckets(list(sim.parameters()), bucket_bytes=1 << 10)
    sched = eng.FusedStep(sim, grads)._bucket_schedule(2)
    assert all(st is None or st >= 1 for st in sched) and 0 not in sched
    sim.process.requires_grad_(False)
    grads = eng.GradBuckets(list(sim.parameters()), bucket_bytes=1 << 10)
    assert decoder_stage(eng.FusedStep(sim, grads), grads) == {None}


def test_mlp_bwd_checks_the_grads_table_on_the_host():
    from bsms_gnn_amd import _abi
    L = _abi.lib()
    one = 0x1000                                                       # a non-null address that must never be dereferenced
    H, D = 3, 128
    n = 2 * (H + 1)
    arr = lambda vals: C.cast((C.c_void_p * n)(*vals), C.POINTER(C.c_void_p))
    call = lambda grads, gx, kind=(4, D, D, 1): L.bsms_mlp_bwd_ex(one, one, 100, kind[0], kind[1], kind[2], H, kind[3], arr([one] * n), one, one,
                                                                  gx, grads, 0, None)
    holes = [one] * n
    holes[5] = None
    assert call(arr(holes), one) == E_INVALID_ARG and b"partly null" in L.bsms_last_error()
    assert call(arr([None] * (n - 1) + [one]), None) == E_INVALID_ARG
    assert call(None, None) == OK and call(arr([None] * n), None) == OK          # frozen and no grad_x: nothing to do
    assert call(None, None, (D, D, 3, 0)) == OK
    assert L.bsms_abi_version() == 4                                   # no signature changed
