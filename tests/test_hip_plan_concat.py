"""bsms_plan_concat (csrc/plan.hip, kernel k_plan_concat in csrc/rowsum.hip) against a plain NumPy statement of the plan arrays.

Every kernel of the engine reads its indices from a LevelPlan; for variable-mesh batches the plan is assembled on the device and
no host code looks at an index before a gather uses it.  This file pins that path where it had never run:

  * more than kCatParts = 16 parts (the launch is repeated per 16 parts and five running offsets are carried across launches),
  * parts whose longest array exceeds the 64 x 256 threads of a launch's x-grid (the grid-stride loop repeats),
  * all eighteen arrays against `plan_reference`, which is written from the documented definitions (argsort / bincount), not from
    the library's loops -- with the create-built plan kept as a second, independent witness at one large count,
  * blocks taken from the recycling pool, a second set_pool (device readback), set_pool on a concat-made plan, and a readback
    that is NOT preceded by a synchronize of the stream the union was queued on,
  * the union in use (segment sum, the four edge-conv variants, one fused training step through MeshBank at 17 samples),
  * the refusals.

All comparisons are exact (integers, or fp32 results whose per-row summation order the project pins as sequential).

The part with N = 0, E = 0 IS accepted by LevelPlan and by bsms_plan_concat, pooled (ids = []) and un-pooled, and is part of the
mixes below.  A part without edges cannot be bound to an EMPTY weight tensor (its data pointer is null, which the C ABI reads as
"unbind"): such parts are bound to a one-element tensor of which the batch takes the first zero elements."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

ARRAYS = ("rowptr", "src", "dst", "perm", "t_rowptr", "t_dst", "t_eid", "t_pos", "ids", "inv", "k_rowptr", "k_src", "k_eid",
          "p_rowptr", "p_src", "p_eid", "k_w", "p_w")
POOLED_ARRAYS = ARRAYS[8:]
GRID_THREADS = 64 * 256          # x-grid of one k_plan_concat launch: a longer array makes the grid-stride loop repeat
MODES = ("bound", "unbound", "unpooled")


# ------------------------------------------------------------------------------------------------ the reference (NumPy only)
def _rowptr(keys, N):
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=N))]).astype(np.int64)


def plan_reference(coo, N, ids=None, ew=None):
    """{name: int32 array} for every name in LevelPlan.ARRAYS, from the definitions bsms_plan_create / bsms_plan_set_pool document:
    the stable destination sort, the stable source sort, and the two compact transition lists."""
    gi, gj = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
    E = gi.shape[0]
    order = np.argsort(gj, kind="stable")
    slot_of_edge = np.empty(E, np.int64)
    slot_of_edge[order] = np.arange(E)
    torder = np.argsort(gi, kind="stable")
    out = dict(rowptr=_rowptr(gj, N), src=gi[order], dst=gj[order], perm=order,
               t_rowptr=_rowptr(gi, N), t_dst=gj[torder], t_eid=torder, t_pos=slot_of_edge[torder])
    for name in POOLED_ARRAYS:
        out[name] = np.empty(0, np.int64)
    if ids is not None:
        ids = np.asarray(ids, np.int64)
        Nk = ids.shape[0]
        inv = np.full(N, -1, np.int64)
        inv[ids] = np.arange(Nk)
        assert np.count_nonzero(inv >= 0) == Nk, "duplicate ids"
        lens = out["rowptr"][ids + 1] - out["rowptr"][ids]
        k_rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        slots = np.repeat(out["rowptr"][ids] - k_rowptr[:-1], lens) + np.arange(k_rowptr[-1])   # kept rows' slots, row by row
        coarse = inv[out["t_dst"]]                                                               # per transpose slot
        keep = coarse >= 0
        out.update(ids=ids, inv=inv, k_rowptr=k_rowptr, k_src=out["src"][slots], k_eid=order[slots],
                   p_rowptr=_rowptr(gi[torder][keep], N), p_src=coarse[keep], p_eid=torder[keep])
        if ew is not None:
            bits = np.ascontiguousarray(ew, np.float32).view(np.int32)
            out.update(k_w=bits[out["k_eid"]], p_w=bits[out["p_eid"]])
    return {k: np.asarray(v).astype(np.int32) for k, v in out.items()}


def union_reference(parts):
    """Offset concatenation of the per-part references (common.h: CatPart): node ids move by the nodes before the part, edge ids
    and CSR slots by the edges before it, coarse rows by the kept rows before it, the compact lists' slots by the compact
    entries before it.  Each rowptr array drops the parts' end entries (they coincide with the next part's entry 0) and gets ONE
    end entry."""
    pooled = parts[0]["ids"] is not None
    acc = {k: [] for k in ARRAYS}
    n_off = e_off = k_off = ek_off = ep_off = 0
    for p in parts:
        r = {k: v.astype(np.int64) for k, v in plan_reference(p["coo"], p["N"], p["ids"], p["ew"]).items()}
        for k in ("src", "dst", "t_dst", "ids", "k_src"):
            acc[k].append(r[k] + n_off)
        for k in ("perm", "t_eid", "t_pos", "k_eid", "p_eid"):
            acc[k].append(r[k] + e_off)
        acc["rowptr"].append(r["rowptr"][:-1] + e_off)
        acc["t_rowptr"].append(r["t_rowptr"][:-1] + e_off)
        acc["inv"].append(np.where(r["inv"] >= 0, r["inv"] + k_off, -1))
        acc["p_src"].append(r["p_src"] + k_off)
        acc["k_rowptr"].append(r["k_rowptr"][:-1] + ek_off)
        acc["p_rowptr"].append(r["p_rowptr"][:-1] + ep_off)
        acc["k_w"].append(r["k_w"])
        acc["p_w"].append(r["p_w"])
        n_off, e_off = n_off + p["N"], e_off + p["coo"].shape[1]
        k_off, ek_off, ep_off = k_off + r["ids"].shape[0], ek_off + r["k_src"].shape[0], ep_off + r["p_src"].shape[0]
    acc["rowptr"].append([e_off])
    acc["t_rowptr"].append([e_off])
    if pooled:
        acc["k_rowptr"].append([ek_off])
        acc["p_rowptr"].append([ep_off])
    return {k: np.concatenate([np.asarray(a, np.int64) for a in v]).astype(np.int32) for k, v in acc.items()}


def concat_problem(parts):
    """The host collate of `parts` (PyG Batch semantics): (coo [2, E], N, ids or None, ew or None)."""
    offs = np.concatenate([[0], np.cumsum([p["N"] for p in parts])]).astype(np.int64)
    coo = np.concatenate([p["coo"] + o for p, o in zip(parts, offs)], axis=1)
    ids = None if parts[0]["ids"] is None else np.concatenate([p["ids"] + o for p, o in zip(parts, offs)])
    ew = None if parts[0]["ew"] is None else np.concatenate([p["ew"] for p in parts])
    return coo, int(offs[-1]), ids, ew


# ------------------------------------------------------------------------------------------------ the part pool and the mixes
def _multigraph(n, e, seed, keep):
    """Directed multigraph like test_hip_widths.random_graph (degree-0 targets: the last n/8 nodes; one hub target), plus explicit
    self-loops; duplicates come with the hub.  `keep` ids in shuffled order."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n - n // 8, e)
    dst[: e // 4] = n // 3
    src[e // 4: e // 4 + 64] = dst[e // 4: e // 4 + 64]
    return dict(coo=np.stack([src, dst]).astype(np.int64), N=n, ids=rng.permutation(n)[:keep].astype(np.int64),
                ew=(rng.random(e) + 0.1).astype(np.float32))


MULTI, HEAVY, NOEDGE, SINGLE, EMPTY = 6, 7, 8, 9, 10     # positions in the pool


@pytest.fixture(scope="module")
def pool(graphs):
    out = []
    for lvl in (0, 1):
        for nm in ("del64", "del300", "surf200"):
            es, ids = graphs.levels(nm)
            n = graphs.np(f"{nm}/pos").shape[0] if lvl == 0 else int(ids[lvl - 1].numel())
            rng = np.random.default_rng(100 + len(out))
            out.append(dict(coo=es[lvl].numpy().astype(np.int64), N=n, ids=ids[lvl].numpy().astype(np.int64),
                            ew=(rng.random(es[lvl].shape[1]) + 0.1).astype(np.float32)))
    out.append(_multigraph(3000, 20000, 7, 1500))
    rng = np.random.default_rng(8)
    out.append(dict(coo=rng.integers(0, 17000, (2, 50)).astype(np.int64), N=17000, ids=np.array([16999, 0, 16384, 8191, 5], np.int64),
                    ew=(rng.random(50) + 0.1).astype(np.float32)))
    none = np.empty((2, 0), np.int64)
    out.append(dict(coo=none, N=5, ids=np.array([3, 0], np.int64), ew=np.empty(0, np.float32)))
    out.append(dict(coo=np.zeros((2, 1), np.int64), N=1, ids=np.array([0], np.int64), ew=np.array([0.75], np.float32)))
    out.append(dict(coo=none, N=0, ids=np.empty(0, np.int64), ew=np.empty(0, np.float32)))
    assert len(out) == 11
    m, h = out[MULTI], out[HEAVY]
    assert m["coo"].shape[1] > GRID_THREADS and h["N"] + 1 > GRID_THREADS > h["coo"].shape[1]       # the premise of the two large parts
    pairs = m["coo"][0] * m["N"] + m["coo"][1]
    assert np.any(m["coo"][0] == m["coo"][1]) and np.unique(pairs).size < pairs.size                # self-loops, duplicate edges
    assert np.bincount(m["coo"][1], minlength=m["N"]).min() == 0 and not np.all(np.diff(m["ids"]) > 0)   # degree-0 targets, unsorted ids
    return out


def _cyc(count, start, **at):
    mix = [(start + i) % 11 for i in range(count)]
    for k, v in at.items():
        mix[int(k[1:])] = v
    return mix


# label -> pool positions.  The two large parts (MULTI: 20 000 edges, HEAVY: 17 000 nodes) and the degenerate parts fall first, last,
# at 15 / 16 (the last part of launch 1, the first of launch 2) and at 31 / 32 (the same for launch 3).
MIXES = {
    "1": [MULTI],
    "2": [HEAVY, EMPTY],
    "16": _cyc(16, 0, _0=EMPTY, _15=MULTI),
    "17-degenerate": _cyc(17, 3, _0=MULTI, _15=HEAVY, _16=EMPTY),
    "17-large": _cyc(17, 5, _0=SINGLE, _15=NOEDGE, _16=MULTI),
    "32": _cyc(32, 1, _15=EMPTY, _16=MULTI, _31=HEAVY),
    "33": _cyc(33, 2, _0=HEAVY, _16=NOEDGE, _31=MULTI, _32=SINGLE),
    "40": _cyc(40, 4, _15=MULTI, _16=HEAVY, _31=NOEDGE, _32=MULTI, _39=EMPTY),
}
assert [len(v) for v in MIXES.values()] == [1, 2, 16, 17, 17, 32, 33, 40]


def _as_mode(part, mode):
    return dict(coo=part["coo"], N=part["N"], ids=None if mode == "unpooled" else part["ids"], ew=part["ew"] if mode == "bound" else None)


_REF = {}


def reference_of(pool, label, mode):
    """(coo, N, ids, ew, arrays) of the concatenated problem of one mix -- computed once, shared by the tests, never modified."""
    key = (label, mode)
    if key not in _REF:
        coo, N, ids, ew = concat_problem([_as_mode(pool[i], mode) for i in MIXES[label]])
        arrays = plan_reference(coo, N, ids, ew)
        for a in (coo, ids, ew, *arrays.values()):
            if a is not None:
                a.setflags(write=False)
        _REF[key] = (coo, N, ids, ew, arrays)
    return _REF[key]


def assert_arrays(got, want, tag):
    for k in ARRAYS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (*tag, k, got[k].shape, want[k].shape)
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k])
            raise AssertionError((*tag, k, f"{bad.size} of {want[k].size} entries differ, first at {int(bad[0])}: "
                                            f"{int(got[k][bad[0]])} != {int(want[k][bad[0]])}"))


# ------------------------------------------------------------------------------------------------ CPU: the reference against itself
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", list(MIXES))
def test_reference_of_the_concatenation_is_the_union_of_the_references(pool, label, mode):
    """The block-diagonal claim of bsms_plan_concat (plan.hip): the plan arrays of an offset-concatenated mesh ARE the offset
    concatenations of the parts' arrays.  Checked on the NumPy reference alone, for every mix and mode the GPU tests use."""
    import bsms_gnn_amd as eng
    assert eng.LevelPlan.ARRAYS == ARRAYS
    parts = [_as_mode(pool[i], mode) for i in MIXES[label]]
    want = reference_of(pool, label, mode)[4]
    assert_arrays(union_reference(parts), want, (mode, label))
    E, N = sum(p["coo"].shape[1] for p in parts), sum(p["N"] for p in parts)
    assert want["rowptr"].shape == (N + 1,) and want["t_pos"].shape == (E,) and want["rowptr"][-1] == E
    if mode == "unpooled":
        assert all(want[k].size == 0 for k in POOLED_ARRAYS)
    else:
        assert want["inv"].shape == (N,) and want["k_rowptr"].shape == (want["ids"].size + 1,) and want["p_rowptr"].shape == (N + 1,)
        assert (want["k_w"].size, want["p_w"].size) == ((want["k_src"].size, want["p_src"].size) if mode == "bound" else (0, 0))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _t(a):
    return torch.tensor(np.ascontiguousarray(a))          # a copy: the shared reference arrays are read-only


def _bind(plan, w):
    from bsms_gnn_amd import _abi
    from bsms_gnn_amd.ops import _stream
    _abi.check(_abi.lib().bsms_plan_bind_edge_weights(plan.handle, w.data_ptr(), _stream()), "bsms_plan_bind_edge_weights")
    plan._ew_bound = w


def _weights(ew):
    """Device weights of one part.  No edges: a one-element tensor (an empty one has a null address: "unbind")."""
    return _t(ew).cuda() if ew.size else torch.zeros(1, device="cuda")


def _make_plan(eng, coo, N, ids=None, ew=None):
    plan = eng.LevelPlan(_t(coo), N, ids=None if ids is None else _t(ids), device="cuda")
    w = None
    if ew is not None:
        w = _weights(ew)
        _bind(plan, w)
    return plan, w


@pytest.fixture(scope="module")
def dev(eng, pool):
    """Per pool entry and mode: (LevelPlan, bound weight tensor or None).  Built once; the unions only read them."""
    out = [{m: _make_plan(eng, **_as_mode(p, m)) for m in MODES} for p in pool]
    torch.cuda.synchronize()
    return out


def _union(eng, dev, label, mode, want_index=True):
    parts = [dev[i][mode][0] for i in MIXES[label]]
    ew_cat = None
    if mode == "bound":
        ew_cat = torch.cat([dev[i][mode][1][:dev[i][mode][0].E] for i in MIXES[label]])
    return eng.concat_plans(parts, ew_cat, want_index), ew_cat


def _facts(plan):
    from bsms_gnn_amd import _abi
    L = _abi.lib()
    return (plan.N, plan.E, plan.Nk, plan.max_source, plan.min_out_degree, int(L.bsms_plan_num_nodes(plan.handle)),
            int(L.bsms_plan_num_edges(plan.handle)), int(L.bsms_plan_num_pooled(plan.handle)), L.bsms_plan_bound_edge_weights(plan.handle) or 0)


CASES = [(label, mode, True) for label in MIXES for mode in MODES] + [("17-large", mode, False) for mode in MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("label,mode,want_index", CASES, ids=[f"{l}-{m}" + ("" if w else "-noindex") for l, m, w in CASES])
def test_union_equals_the_reference(eng, pool, dev, label, mode, want_index):
    """All eighteen arrays of the device-built union == plan_reference of the concatenated problem; the edge list and kept ids it
    writes == the host collate; its scalar facts == those of the plan bsms_plan_create builds from the host collate.  At 33 parts
    the create-built plan's arrays are compared too, so that an error of the reference and one of the code cannot cancel."""
    coo, N, ids, ew, want = reference_of(pool, label, mode)
    (got, coo_d, ids_d), ew_cat = _union(eng, dev, label, mode, want_index)
    torch.cuda.synchronize()
    tag = (mode, label)
    assert_arrays(got.export_ex(), want, tag)
    if want_index:
        assert np.array_equal(coo_d.cpu().numpy(), coo), (*tag, "coo")
        assert (ids_d is None) == (ids is None), (*tag, "ids")
        if ids is not None:
            assert np.array_equal(ids_d.cpu().numpy(), ids), (*tag, "ids")
    else:
        assert coo_d is None and ids_d is None
    made, _ = _make_plan(eng, coo, N, ids)
    if mode == "bound":
        assert np.array_equal(ew_cat.cpu().numpy(), ew)
        _bind(made, ew_cat)
    torch.cuda.synchronize()
    assert _facts(got) == _facts(made), (*tag, _facts(got), _facts(made))
    assert _facts(got)[-1] == (ew_cat.data_ptr() if mode == "bound" else 0)
    if label == "33":
        assert_arrays(got.export_ex(), made.export_ex(), (*tag, "create-built"))


@pytest.mark.gpu
def test_union_in_recycled_blocks_writes_every_word(eng, pool, dev):
    """The union's two blocks come from the library's recycling pool and are written by the kernel alone.  A plan with LARGE
    indices everywhere (a 20 000-edge multigraph with every node kept: no -1 in `inv`) is built, dropped and reaped, its two
    blocks being the only ones in the pool; a smaller union of other content, sized to take exactly those blocks (between half
    and all of their capacity: 415 KB and ~420 KB into 576 KB and 640 KB), must show none of the old words -- in particular -1
    wherever a node is not kept."""
    from bsms_gnn_amd import _abi, graph
    L = _abi.lib()
    torch.cuda.synchronize()
    gc.collect()
    graph._reap()
    _abi.check(L.bsms_plan_pool_trim(), "bsms_plan_pool_trim")
    fresh = [_multigraph(2600, 16000, 22, 2500), pool[NOEDGE], pool[0], pool[EMPTY]]
    made = [_make_plan(eng, **p) for p in fresh]             # before anything is in the pool: the parts take new blocks
    ew_cat = torch.cat([w[:q.E] for q, w in made])
    big = _multigraph(3000, 20000, 21, 3000)
    old, w_old = _make_plan(eng, big["coo"][::-1], big["N"], big["ids"][::-1], big["ew"])
    torch.cuda.synchronize()
    stale = old.export_ex()
    assert stale["inv"].min() >= 0 and stale["k_rowptr"][-1] == stale["p_rowptr"][-1] == 20000
    del old
    torch.cuda.synchronize()
    gc.collect()
    graph._reap()
    got, _, _ = eng.concat_plans([q for q, _ in made], ew_cat)
    torch.cuda.synchronize()
    want = plan_reference(*concat_problem(fresh))
    assert np.count_nonzero(want["inv"] < 0) > 100
    assert_arrays(got.export_ex(), want, ("recycled",))
    del w_old


# ------------------------------------------------------------------------------------------------ re-pooling and readback
@pytest.mark.gpu
def test_set_pool_twice_reads_the_block_back(eng, pool):
    """The first bsms_plan_set_pool uses (and then drops) the host copy of the CSR; the second reads the index block back from
    the device.  Both give the reference's pool arrays; the CSR arrays are untouched; binding weights fills k_w / p_w."""
    m = pool[MULTI]
    plan, _ = _make_plan(eng, m["coo"], m["N"])
    rng = np.random.default_rng(31)
    for ids in (m["ids"], rng.permutation(m["N"])[:777].astype(np.int64), np.empty(0, np.int64)):
        plan.set_pool(_t(ids))
        assert_arrays(plan.export_ex(), plan_reference(m["coo"], m["N"], ids), ("set_pool", ids.size))
    ids = np.sort(m["ids"])
    plan.set_pool(_t(ids))
    _bind(plan, _weights(m["ew"]))
    torch.cuda.synchronize()
    assert_arrays(plan.export_ex(), plan_reference(m["coo"], m["N"], ids, m["ew"]), ("set_pool", "bound"))
    rowptr, src, perm, t_rowptr = plan.export()
    want = plan_reference(m["coo"], m["N"])
    assert all(np.array_equal(a, want[k]) for a, k in ((rowptr, "rowptr"), (src, "src"), (perm, "perm"), (t_rowptr, "t_rowptr")))


def _ids_across_parts(N, seed):
    return np.random.default_rng(seed).permutation(N)[: N // 3].astype(np.int64)


@pytest.mark.gpu
def test_set_pool_on_a_concat_made_plan(eng, pool, dev):
    """A union has no host copy at all: bsms_plan_set_pool on it reads back the block the KERNEL wrote.  33 un-pooled parts, ids
    chosen across the parts (unsorted); then the weights are bound and k_w / p_w checked; then it is pooled once more."""
    coo, N, _, _, _ = reference_of(pool, "33", "unpooled")
    ew = reference_of(pool, "33", "bound")[3]
    (got, _, _), _ = _union(eng, dev, "33", "unpooled")
    torch.cuda.synchronize()
    ids = _ids_across_parts(N, 41)
    got.set_pool(_t(ids))
    assert_arrays(got.export_ex(), plan_reference(coo, N, ids), ("concat-made", "set_pool"))
    _bind(got, _weights(ew))
    torch.cuda.synchronize()
    assert_arrays(got.export_ex(), plan_reference(coo, N, ids, ew), ("concat-made", "bound"))
    ids = _ids_across_parts(N, 42)[::2]
    got.set_pool(_t(ids))
    assert_arrays(got.export_ex(), plan_reference(coo, N, ids), ("concat-made", "set_pool again"))


@pytest.mark.gpu
@pytest.mark.parametrize("reader", ["export_ex", "export", "set_pool"])
def test_readback_is_ordered_behind_a_concat_on_a_busy_side_stream(eng, pool, dev, reader):
    """bsms_plan_concat is stream-ordered; torch.cuda.Stream() is a non-blocking stream, which a plain hipMemcpy on the NULL stream
    does not wait for.  The union is queued behind tens of milliseconds of matrix products on such a stream and read back with NO
    synchronize in between: bsms_plan_export_ex, bsms_plan_export and the readback of bsms_plan_set_pool must wait for it."""
    mode = "unpooled" if reader == "set_pool" else "bound"
    coo, N, ids, ew, want = reference_of(pool, "33", mode)
    parts = [dev[i][mode][0] for i in MIXES["33"]]
    ew_cat = _t(ew).cuda() if mode == "bound" else None
    a = torch.randn(8192, 8192, device="cuda")
    c = torch.empty_like(a)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.mm(a[:256, :256], a[:256, :256])          # BLAS start-up happens here, not in the timed queue
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):                               # 6 x 1.1 TFLOP of fp32: well over 10 ms on any MI355X
            torch.mm(a, a, out=c)
        got, _, _ = eng.concat_plans(parts, ew_cat)
        busy = not side.query()
        if reader == "set_pool":
            ids = _ids_across_parts(N, 43)
            got.set_pool(_t(ids))
            want = plan_reference(coo, N, ids)
            arrays = got.export_ex()
        elif reader == "export":
            arrays = dict(zip(("rowptr", "src", "perm", "t_rowptr"), got.export()))
        else:
            arrays = got.export_ex()
    side.synchronize()
    torch.cuda.synchronize()
    assert busy, "premise: the side stream was still busy when the union was queued"
    for k, v in arrays.items():
        assert np.array_equal(v, want[k]), (reader, k)
    assert_arrays(got.export_ex(), want, (reader, "after synchronize"))


# ------------------------------------------------------------------------------------------------ the union in use
@pytest.mark.gpu
def test_kernels_on_the_union_equal_the_parts_bit_for_bit(eng, pool, dev):
    """Segment sum and the four (aggregating, pooled) edge-conv variants on a 33-part pooled and bound union == the concatenation
    along the node axis of the same call on each part's own plan, bit for bit: the parts' rows are independent and the per-row
    summation order is sequential in every launch regime (test_segment_sum_fwd_both_regimes,
    test_bound_edge_weights_transitions_bit_identical).  Width 32, B = 2.  Parts without output rows contribute nothing and are
    not called (the C ABI refuses a null output)."""
    from bsms_gnn_amd import ops
    B, D = 2, 32
    (got, _, _), ew_cat = _union(eng, dev, "33", "bound")
    mix = [dev[i]["bound"] for i in MIXES["33"]]
    gen = torch.Generator().manual_seed(5)
    src = torch.randn(B, got.E, D, generator=gen).cuda()
    xN = torch.randn(B, got.N, D, generator=gen).cuda()
    xK = torch.randn(B, got.Nk, D, generator=gen).cuda()

    def pieces(t, sizes):
        return [t[:, o - s:o].contiguous() for s, o in zip(sizes, np.cumsum(sizes))]

    def per_part(call, xs, rows):
        outs = [call(q, w, x) if r else torch.empty(B, 0, D, device="cuda") for (q, w), x, r in zip(mix, xs, rows)]
        return torch.cat(outs, dim=1)

    Ns, Es, Nks = [q.N for q, _ in mix], [q.E for q, _ in mix], [q.Nk for q, _ in mix]
    assert (sum(Ns), sum(Es), sum(Nks)) == (got.N, got.E, got.Nk) and 0 in Es and 0 in Ns and max(Es) > GRID_THREADS
    out = ops._SegmentSum.apply(src, got)
    want = per_part(lambda q, w, x: ops._SegmentSum.apply(x, q), pieces(src, Es), Ns)
    assert out.shape == want.shape and torch.equal(out, want), "segment_sum"
    for aggregating in (True, False):
        for pooled in (False, True):
            x, x_sizes = (xK, Nks) if (pooled and not aggregating) else (xN, Ns)
            rows = Nks if (pooled and aggregating) else Ns
            out = ops._edge_conv(x, ew_cat, got, aggregating, pooled)
            want = per_part(lambda q, w, xp: ops._edge_conv(xp, w, q, aggregating, pooled), pieces(x, x_sizes), rows)
            assert out.shape == want.shape and torch.equal(out, want), ("edge_conv", aggregating, pooled)
            if pooled:      # another address with the same content: the unbound path through rowptr / ids / inv of the union
                assert torch.equal(ops._edge_conv(x, ew_cat.clone(), got, aggregating, pooled), want), ("edge_conv unbound", aggregating)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_mesh_bank_batch_of_17_samples_equals_host_collate(eng, graphs):
    """test_mesh_bank_batch_equals_host_collate's assertion at a part count that crosses the 16-part launch boundary: 17 samples,
    del64 and del300 alternating, collated by MeshBank (bsms_plan_concat per level) and by collate_variable_meshes + upload -- the
    same LevelData tensors, and one fused training step gives loss, prediction and flat gradients bit for bit."""
    from oracle import bsms_oracle as ro
    cfg = ro.make_cfg(2, 32, 3, 2, 2)
    torch.manual_seed(11)
    meshes = {}
    for nm in ("del64", "del300"):
        es, ids = graphs.levels(nm)
        n = graphs.np(f"{nm}/pos").shape[0]
        sizes = [n] + [int(i.numel()) for i in ids[:2]]
        pos = torch.tensor(graphs.np(f"{nm}/pos")[:, :2], dtype=torch.float32)
        state, ntype = torch.randn(n, 2), (torch.rand(n, 1) < 0.1).float()
        x, y, mask = torch.cat([state, pos, ntype], -1), state + 0.1 * torch.randn(n, 2), (ntype == 0).float()
        meshes[nm] = [eng.LevelData(es[l], sizes[l], face=ids[l] if l < 2 else None, x=x if l == 0 else None, y=y if l == 0 else None,
                                    mask=mask if l == 0 else None) for l in range(3)]
    samples = [meshes["del64" if i % 2 == 0 else "del300"] for i in range(17)]
    sim = eng.BSMS_Simulator(cfg).cuda()
    host = [d.to("cuda") for d in eng.collate_variable_meshes(samples)]
    sim(host, False, True)                                              # normaliser statistics
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads)
    grads.flat.zero_()
    loss_h = step(host, False).clone()
    pred_h, flat_h = step.prediction().clone(), grads.flat.clone()
    bank = eng.MeshBank(sim.process, "cuda")
    devb = bank.collate(samples)
    for a, b in zip(devb, host):
        assert a.num_nodes == b.num_nodes and torch.equal(a.edge_index, b.edge_index)
        assert (a.face is None) == (b.face is None) and (a.face is None or torch.equal(a.face, b.face))
    assert torch.equal(devb[0].x, host[0].x) and torch.equal(devb[0].y, host[0].y) and torch.equal(devb[0].mask, host[0].mask)
    grads.flat.zero_()
    loss_d = step(devb, False).clone()
    assert torch.isfinite(loss_h) and flat_h.abs().max() > 0
    assert torch.equal(loss_d, loss_h) and torch.equal(step.prediction(), pred_h) and torch.equal(grads.flat, flat_h)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_leave_the_output_handle_null(eng, pool, dev):
    from bsms_gnn_amd import _abi
    from bsms_gnn_amd.ops import _stream
    L = _abi.lib()

    def refused(plans, ew_cat=None, nparts=None):
        arr, keep = _abi.ptr_array([q.handle.value for q in plans] or [None])
        out = C.c_void_p(1)                                   # not null before the call: the library has to clear it
        rc = L.bsms_plan_concat(arr, len(plans) if nparts is None else nparts, None if ew_cat is None else ew_cat.data_ptr(), None, None,
                                _stream(), C.byref(out))
        assert rc != 0 and out.value is None, (rc, out.value)
        with pytest.raises(_abi.BsmsError):
            _abi.check(rc, "bsms_plan_concat")
        return L.bsms_last_error().decode()

    plans = lambda mode, n=17: [dev[i % 6][mode][0] for i in range(n)]
    ew17 = torch.cat([dev[i % 6]["bound"][1] for i in range(17)])
    assert "no parts" in refused([], nparts=0)
    for at in (0, 16):
        for inner, outer in (("unpooled", "bound"), ("bound", "unpooled")):
            mixed = plans(outer)
            mixed[at] = dev[1][inner][0]
            assert "pool" in refused(mixed)
    for at in (0, 16):
        some = plans("bound")
        some[at] = dev[2]["unbound"][0]
        assert "no bound edge weights" in refused(some, ew17)
    assert "ew_cat given" in refused(plans("unpooled"), ew17)
    with pytest.raises(_abi.BsmsError):
        eng.concat_plans(plans("unpooled"), ew17)
    (ok, _, _), _ = _union(eng, dev, "2", "bound")          # ... and the library still works afterwards
    torch.cuda.synchronize()
    assert_arrays(ok.export_ex(), reference_of(pool, "2", "bound")[4], ("after refusals",))
