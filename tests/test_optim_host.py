"""CPU: the host side of the general optimizer step -- the refusals of bsms_optim_groups_create, which all come
from host code before any device call (this file runs where there is no GPU), and the Python layer above it: param_groups, the
segment table, the EMA warm-up schedule.  What the kernel writes is pinned on the GPU (tests/test_hip_optim.py)."""
import ctypes as C
import math

import pytest
import torch

from oracle import bsms_oracle as ro

OK, E_INVALID_ARG, E_SHAPE = 0, -1, -2
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__
    __graft_entry__.build()
    import bsms_gnn_amd as eng
    return eng


def create(eng, rows, n, ngroups=None, table="rows"):
    """(return code, handle value, message) of bsms_optim_groups_create for rows of (offset, count, lr_scale, weight_decay)."""
    L, G = eng._abi.lib(), eng._abi.OptimGroup
    arr = (G * max(len(rows), 1))(*[G(*r) for r in rows])
    h = C.c_void_p()
    rc = L.bsms_optim_groups_create(C.cast(arr, C.c_void_p) if table == "rows" else None, len(rows) if ngroups is None else ngroups,
                                    n, C.cast(C.byref(h), eng._abi.PP))
    return rc, h.value, L.bsms_last_error()


REFUSALS = [
    ("gap", [(0, 10, 1, 0), (12, 8, 1, 0)], 20, E_SHAPE, b"gap"),
    ("overlap", [(0, 10, 1, 0), (8, 12, 1, 0)], 20, E_SHAPE, b"overlap"),
    ("unsorted", [(10, 10, 1, 0), (0, 10, 1, 0)], 20, E_SHAPE, b"not sorted"),
    ("first group off zero", [(2, 18, 1, 0)], 20, E_SHAPE, b"gap"),
    ("short of n", [(0, 10, 1, 0), (10, 5, 1, 0)], 20, E_SHAPE, b"short of n"),
    ("past n", [(0, 10, 1, 0), (10, 11, 1, 0)], 20, E_SHAPE, b"past n"),
    ("count 0", [(0, 10, 1, 0), (10, 0, 1, 0), (10, 10, 1, 0)], 20, E_SHAPE, b"count=0"),
    ("negative lr_scale", [(0, 20, -0.5, 0)], 20, E_INVALID_ARG, b"lr_scale"),
    ("nan lr_scale", [(0, 20, NAN, 0)], 20, E_INVALID_ARG, b"lr_scale"),
    ("inf lr_scale", [(0, 20, INF, 0)], 20, E_INVALID_ARG, b"lr_scale"),
    ("negative weight_decay", [(0, 20, 1, -1e-3)], 20, E_INVALID_ARG, b"weight_decay"),
    ("nan weight_decay", [(0, 20, 1, NAN)], 20, E_INVALID_ARG, b"weight_decay"),
    ("inf weight_decay", [(0, 20, 1, INF)], 20, E_INVALID_ARG, b"weight_decay"),
]


@pytest.mark.parametrize("what,rows,n,code,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_groups_create_refusals(eng, what, rows, n, code, word):
    rc, handle, msg = create(eng, rows, n)
    assert rc == code and handle is None and word in msg, (what, rc, handle, msg)


def test_groups_create_refuses_table_and_count(eng):
    L = eng._abi.lib()
    rc, handle, msg = create(eng, [(0, 20, 1, 0)], 20, table=None)
    assert rc == E_INVALID_ARG and handle is None and b"table is null" in msg
    for ngroups in (0, 4097, -1):
        rc, handle, msg = create(eng, [(0, 20, 1, 0)], 20, ngroups=ngroups)
        assert rc == E_INVALID_ARG and handle is None and b"outside 1..4096" in msg, ngroups
    assert L.bsms_optim_groups_create(None, 1, 20, None) == E_INVALID_ARG and b"out is null" in L.bsms_last_error()
    assert L.bsms_optim_groups_destroy(None) == OK
    assert L.bsms_optim_work_bytes() >= L.bsms_adamw_work_bytes() + 4          # the partial sums and the norm of the call


def test_new_entries_are_bound(eng):
    for name in ("bsms_optim_groups_create", "bsms_optim_groups_destroy", "bsms_optim_work_bytes", "bsms_optim_step"):
        assert name in eng._abi.SIGNATURES and getattr(eng._abi.lib(), name).argtypes == eng._abi.SIGNATURES[name][1]
    assert len(eng._abi.SIGNATURES["bsms_optim_step"][1]) == 19
    assert C.sizeof(eng._abi.OptimGroup) == 24
    assert eng._abi.lib().bsms_abi_version() == 4                               # entries were added, no signature changed


# ---------------------------------------------------------------------------------------------------- the Python layer
@pytest.fixture()
def model(eng):
    torch.manual_seed(0)
    return eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 2, 2))


def trainable(model):
    return [(k, p) for k, p in model.named_parameters() if p.requires_grad]


def test_param_groups_no_decay_bias_is_exactly_the_1d_tensors(eng, model):
    groups = eng.param_groups(model, no_decay_bias=True)
    assert len(groups) == 1 and groups[0]["weight_decay"] == 0.0 and "lr_scale" not in groups[0]
    listed = {id(p) for p in groups[0]["params"]}
    want = {id(p) for _, p in trainable(model) if p.dim() == 1}
    assert listed == want and 0 < len(want) < len(trainable(model))
    assert eng.param_groups(model) == []                                        # no rule: everything is the default group


def test_param_groups_longest_prefix_wins(eng, model):
    groups = eng.param_groups(model, lr_scales={"process": 0.1, "process.bottom_gmp": 0.5, "process.bottom_gmp.mlp_edge": 2.0})
    scale_of = {id(p): g["lr_scale"] for g in groups for p in g["params"]}
    assert all("weight_decay" not in g for g in groups)
    seen = set()
    for name, p in trainable(model):
        want = (2.0 if name.startswith("process.bottom_gmp.mlp_edge.") else 0.5 if name.startswith("process.bottom_gmp.") else
                0.1 if name.startswith("process.") else None)
        assert scale_of.get(id(p)) == want, name
        seen.add(want)
    assert seen == {2.0, 0.5, 0.1, None}
    # a prefix ends at a dot: "proc" is not a prefix of "process.*"
    with pytest.raises(ValueError, match="matches no trainable parameter"):
        eng.param_groups(model, lr_scales={"proc": 0.1})
    with pytest.raises(ValueError, match="matches no trainable parameter"):
        eng.param_groups(model, lr_scales={"encode": 1.0, "nonsense": 0.1})
    with pytest.raises(ValueError):
        eng.param_groups(model, lr_scales={"encode": -1.0})
    # both rules at once: the 1-D tensors of the processor carry both
    both = eng.param_groups(model, no_decay_bias=True, lr_scales={"process": 0.1})
    assert {(g.get("lr_scale"), g.get("weight_decay")) for g in both} == {(0.1, None), (0.1, 0.0), (None, 0.0)} and len(both) == 3


def test_frozen_parameters_are_not_listed(eng, model):
    for p in model.process.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="matches no trainable parameter"):
        eng.param_groups(model, lr_scales={"process": 0.1})
    groups = eng.param_groups(model, no_decay_bias=True)
    frozen = {id(p) for p in model.process.parameters()}
    assert not frozen & {id(p) for p in groups[0]["params"]}


def test_segment_table_tiles_and_merges(eng, model):
    buckets = eng.GradBuckets(model.parameters())
    n = buckets.flat.numel()
    wd = 0.01
    segs = eng.segment_table(buckets, eng.param_groups(model, no_decay_bias=True, lr_scales={"process": 0.1}), wd)
    assert segs[0][0] == 0 and segs[-1][0] + segs[-1][1] == n
    for a, b in zip(segs, segs[1:]):
        assert a[0] + a[1] == b[0] and a[1] >= 1                                # sorted, no gap, no overlap
        assert a[2:] != b[2:]                                                   # equal neighbours were merged
    # every parameter lies in a segment with its own hyper-parameters
    for name, p in trainable(model):
        off, cnt = buckets._slot[p]
        seg = next(s for s in segs if s[0] <= off and off + cnt <= s[0] + s[1])
        assert seg[2] == (0.1 if name.startswith("process.") else 1.0), name
        assert seg[3] == (0.0 if p.dim() == 1 else wd), name
    # no group at all: one segment; a group equal to the default merges away too
    assert eng.segment_table(buckets, [], wd) == [(0, n, 1.0, wd)]
    assert eng.segment_table(buckets, [{"params": [p for _, p in trainable(model)][:5], "lr_scale": 1.0, "weight_decay": wd}], wd) == [(0, n, 1.0, wd)]
    # the C side accepts the table as it stands (a host check: it stops at the device allocation where there is no device)
    rc, _, msg = create(eng, [(0, n + 1, 1.0, wd)], n)
    assert rc == E_SHAPE and b"past n" in msg


def test_segment_table_refusals(eng, model):
    enc = list(model.encode.parameters())
    for p in model.decode.parameters():
        p.requires_grad_(False)
    buckets = eng.GradBuckets(model.parameters())
    with pytest.raises(ValueError, match="lists already"):
        eng.segment_table(buckets, [{"params": enc[:2]}, {"params": enc[1:3], "lr_scale": 0.5}], 0.01)
    with pytest.raises(ValueError, match="lists already"):
        eng.segment_table(buckets, [{"params": [enc[0], enc[0]]}], 0.01)
    with pytest.raises(ValueError, match="without a gradient slot"):
        eng.segment_table(buckets, [{"params": list(model.decode.parameters())[:1], "weight_decay": 0.0}], 0.01)
    with pytest.raises(ValueError, match="unknown key"):
        eng.segment_table(buckets, [{"params": enc[:1], "betas": (0.9, 0.99)}], 0.01)
    with pytest.raises(ValueError, match="finite"):
        eng.segment_table(buckets, [{"params": enc[:1], "lr_scale": NAN}], 0.01)


def test_ema_decay_at(eng):
    opt = eng.FusedAdamW.__new__(eng.FusedAdamW)
    opt.ema_decay, opt.ema_warmup = 0.999, True
    assert opt.ema_decay_at(0) == 0.1 and opt.ema_decay_at(1) == 2.0 / 11.0
    assert all(opt.ema_decay_at(t) <= opt.ema_decay_at(t + 1) for t in range(20000))
    t_star = math.ceil((10 * 0.999 - 1) / (1 - 0.999))                         # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d)
    assert opt.ema_decay_at(t_star - 2) < 0.999 and opt.ema_decay_at(t_star) == 0.999 and opt.ema_decay_at(10 ** 9) == 0.999
    opt.ema_warmup = False
    assert opt.ema_decay_at(0) == 0.999 and opt.ema_decay_at(5) == 0.999


def test_fused_adamw_without_options_holds_no_new_state(eng, model):
    """On the CPU the flat buffers are host tensors; nothing is launched by the constructor."""
    opt = eng.FusedAdamW(eng.GradBuckets(model.parameters()), lr=1e-3)
    assert opt._groups is None and opt.ema is None and opt.counters is None and opt.segments is None and not opt.extended
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "step"}
    assert opt._work.numel() == max(int(eng._abi.lib().bsms_adamw_work_bytes()), 4)
    with pytest.raises(ValueError, match="no EMA"):
        opt.ema_model(model)
    with pytest.raises(ValueError, match="ema_decay"):
        eng.FusedAdamW(eng.GradBuckets(model.parameters()), ema_decay=1.5)


def test_ema_and_guard_state_on_the_host(eng, model):
    """EMA and counters need no handle: the object is built, saved and loaded without a device."""
    opt = eng.FusedAdamW(eng.GradBuckets(model.parameters()), lr=1e-3, ema_decay=0.99, skip_nonfinite=True)
    assert opt.extended and opt._groups is None
    assert torch.equal(opt.ema, opt.flat_p) and opt.ema.data_ptr() != opt.flat_p.data_ptr()
    assert opt.counters.tolist() == [0, 0] and opt.counters.dtype == torch.int64
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "step", "ema", "counters"}
    # the aliasing copy: trainable parameters are views into `ema`, the normalisers' statistics are the live model's objects
    twin = opt.ema_model(model)
    live, avg = dict(model.named_parameters()), dict(twin.named_parameters())
    assert list(live) == list(avg)
    lo, hi = opt.ema.data_ptr(), opt.ema.data_ptr() + 4 * opt.ema.numel()
    for k, p in live.items():
        if p.requires_grad:
            assert lo <= avg[k].data_ptr() < hi and not avg[k].requires_grad and avg[k].shape == p.shape, k
            off, _ = opt.grads._slot[p]
            assert avg[k].data_ptr() == lo + 4 * off, k
        else:
            assert avg[k] is p, k
    opt.ema.mul_(2.0)
    assert torch.equal(avg["encode.seq.0.weight"], 2.0 * live["encode.seq.0.weight"])
    # a state from an optimizer without the options: ema starts from the parameters, the counters from (step, 0)
    opt.load_state_dict({"exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(), "step": 7})
    assert torch.equal(opt.ema, opt.flat_p) and opt.counters.tolist() == [7, 0] and opt.step_count == 7
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    sd["ema"] += 1.0
    sd["counters"] = torch.tensor([5, 2])
    opt.load_state_dict(sd)
    assert torch.equal(opt.ema, opt.flat_p + 1.0) and opt.counters.tolist() == [5, 2]
