"""The buffer layouts and the argument checks of the GMP / MLP / U-Net entries, pinned as LITERALS.

Every number and every (return code, message prefix) pair below was printed by the library of commit 6487b57 (the parent of the
block-descriptor refactor of csrc/gmp.hip, csrc/bsgmp.hip and csrc/mlp.hip); nothing here is derived from the code under test.  A size
query that moves means that a carve changed the order, the alignment or the condition of one of its takes: the caller's buffers
and the library's walk over them would then disagree silently, on the device.

CPU: bsms_gmp_saved_bytes / _work_bytes and bsms_mlp_saved_bytes / _work_bytes (host arithmetic, no device needed).
GPU (about a second; plans live in device memory): the U-Net queries in all three precisions, and the refusals of the block entries
-- which entry reports a bad argument, with which code, under which name.  Every refused call returns before any launch."""
import pytest
import torch

from conftest import load_golden

OK, E_INVALID_ARG, E_UNSUPPORTED = 0, -1, -3

# (B, N, E, D, hidden): (gmp_saved, gmp_work, mlp_saved, mlp_work) with R = B * N rows for the MLP queries
BLOCK_BYTES = {
    (1, 7, 12, 32, 1): (1226240, 136776704, 1127680, 68386816),
    (1, 7, 12, 32, 3): (1488384, 136973312, 1258752, 68485120),
    (1, 7, 12, 32, 7): (2012672, 137366528, 1520896, 68681728),
    (1, 7, 12, 96, 1): (1849344, 139796736, 1371136, 69894144),
    (1, 7, 12, 96, 3): (2783232, 140386560, 1838080, 70189056),
    (1, 7, 12, 96, 7): (4651008, 141566208, 2771968, 70778880),
    (1, 7, 12, 128, 1): (2308096, 141306368, 1541888, 70647808),
    (1, 7, 12, 128, 3): (3676160, 142295552, 2225920, 71041024),
    (1, 7, 12, 128, 7): (6412288, 143665664, 3593984, 71827456),
    (1, 7, 12, 256, 1): (5139456, 147346432, 2559232, 73662464),
    (1, 7, 12, 256, 3): (8924160, 148919296, 4451584, 74448896),
    (1, 7, 12, 256, 7): (16493568, 152065024, 8236288, 76021760),
    (2, 300, 1700, 32, 1): (2488576, 137987072, 1279488, 68517888),
    (2, 300, 1700, 32, 3): (3856640, 139166720, 1558016, 68747264),
    (2, 300, 1700, 32, 7): (6592768, 141526016, 2115072, 69206016),
    (2, 300, 1700, 96, 1): (5265664, 143428608, 1805824, 70287360),
    (2, 300, 1700, 96, 3): (9271552, 146967552, 2682368, 70975488),
    (2, 300, 1700, 96, 7): (17283328, 154045440, 4435456, 72351744),
    (2, 300, 1700, 128, 1): (6801664, 146149376, 2118144, 71172096),
    (2, 300, 1700, 128, 3): (12224768, 161816576, 3342848, 72089600),
    (2, 300, 1700, 128, 7): (23070976, 160305152, 5792256, 73924608),
    (2, 300, 1700, 256, 1): (14002432, 157032448, 3709440, 74711040),
    (2, 300, 1700, 256, 3): (25897216, 166469632, 6683136, 76546048),
    (2, 300, 1700, 256, 7): (49686784, 185344000, 12630528, 80216064),
    (8, 5233, 31354, 32, 1): (95378688, 227757056, 12679936, 79101952),
    (8, 5233, 31354, 32, 3): (179911936, 302861312, 24865536, 89915392),
    (8, 5233, 31354, 32, 7): (348978432, 453069824, 49236736, 111542272),
    (8, 5233, 31354, 96, 1): (256550144, 412738560, 34353920, 102039552),
    (8, 5233, 31354, 96, 3): (491570432, 638051328, 68305664, 134479872),
    (8, 5233, 31354, 96, 7): (961611008, 1088676864, 136209152, 199360512),
    (8, 5233, 31354, 128, 1): (337283328, 505229312, 45240064, 113508352),
    (8, 5233, 31354, 128, 3): (647645440, 857550848, 90124032, 156762112),
    (8, 5233, 31354, 128, 7): (1268369664, 1406480384, 179891968, 243269632),
    (8, 5233, 31354, 256, 1): (665893120, 875192320, 89788160, 159383552),
    (8, 5233, 31354, 256, 3): (1287665920, 1476026368, 180080384, 245891072),
    (8, 5233, 31354, 256, 7): (2531211520, 2677694464, 360664832, 418906112),
}


def _lib():
    import bsms_gnn_amd as eng
    return eng._abi.lib()


def test_block_and_mlp_size_queries():
    L = _lib()
    for (B, N, E, D, H), want in BLOCK_BYTES.items():
        got = (L.bsms_gmp_saved_bytes(B, N, E, D, H), L.bsms_gmp_work_bytes(B, N, E, D, H),
               L.bsms_mlp_saved_bytes(B * N, 3, D, D, H), L.bsms_mlp_work_bytes(B * N, 3, D, D, H))
        assert got == want, (B, N, E, D, H)


@pytest.mark.parametrize("hidden", [0, 8])
def test_size_queries_return_zero_outside_the_hidden_range(hidden):
    L = _lib()
    for (B, N, E) in ((1, 7, 12), (2, 300, 1700), (8, 5233, 31354)):
        for D in (32, 96, 128, 256):
            assert L.bsms_gmp_saved_bytes(B, N, E, D, hidden) == 0 and L.bsms_gmp_work_bytes(B, N, E, D, hidden) == 0
            assert L.bsms_mlp_saved_bytes(B * N, 3, D, D, hidden) == 0 and L.bsms_mlp_work_bytes(B * N, 3, D, D, hidden) == 0


def increasing_over_the_depths(sizes, D, work):
    """`sizes`: a size query at hidden = 1 .. 7.  Non-zero and strictly increasing -- every layer adds activations, gradients and packs.
    One exception, by design: at D = 128 a `work` size also holds the per-workgroup partials of the fused edge backward, which exists at
    hidden = 3 alone (csrc/gmp.hip: edge_fused_possible; the query has no precision argument), so hidden = 3 may exceed hidden = 4 there.
    It is then held against its neighbours separately: above hidden = 2, and the other six depths increasing among themselves."""
    if sizes[0] <= 0:
        return False
    if work and D == 128:
        rest = sizes[:2] + sizes[3:]
        return sizes[2] > sizes[1] and all(b > a for a, b in zip(rest, rest[1:]))
    return all(b > a for a, b in zip(sizes, sizes[1:]))


def test_size_queries_grow_with_every_hidden_layer():
    L = _lib()
    for (B, N, E) in ((1, 7, 12), (1, 37, 150), (2, 300, 1700), (8, 5233, 31354)):
        for D in (32, 64, 96, 128, 160, 192, 224, 256):
            for name, q, work in (("gmp_saved", lambda H: L.bsms_gmp_saved_bytes(B, N, E, D, H), False),
                                  ("gmp_work", lambda H: L.bsms_gmp_work_bytes(B, N, E, D, H), True),
                                  ("mlp_saved", lambda H: L.bsms_mlp_saved_bytes(B * N, 3, D, D, H), False),
                                  ("mlp_work", lambda H: L.bsms_mlp_work_bytes(B * N, 3, D, D, H), False)):
                sizes = [q(H) for H in range(1, 8)]
                assert increasing_over_the_depths(sizes, D, work), (name, B, N, E, D, sizes)
                assert q(0) == 0 and q(8) == 0 and q(-1) == 0, (name, D)


# ------------------------------------------------------------------------------------------------ GPU: the U-Net
B_UNET, D_UNET = 2, 128
# (mesh, hidden): saved bytes in BSMS_F32 / BSMS_BF16 / BSMS_BF16_NODES, work, inference work, position work.  hidden = 3: the bf16
# precisions keep the fused layout (two projections, row images, no edge activations); hidden = 2: the unfused bf16 layout
UNET_BYTES = {
    ("line11", 3): (18468608, 14975744, 13501184, 715101952, 145897728, 1280),
    ("line11", 2): (15048448, 14035712, 13052672, 711423232, 144602880, 1280),
    ("del64_d128", 3): (23646720, 16437760, 14963200, 729372416, 149900800, 12288),
    ("del64_d128", 2): (19077632, 16349696, 15366656, 715932928, 146048000, 12288),
}


class Unet:
    """Plans and pointer tables of a golden mesh's two-level U-Net; buffers sized for (D_UNET, hidden 3) in fp32."""

    def __init__(self, tag):
        import bsms_gnn_amd as eng
        from bsms_gnn_amd.ops import _param_ptrs
        from conftest import Golden
        z = load_golden(f"bsgmp_{tag}")
        self.eng, self.L, self.depth = eng, eng._abi.lib(), int(z.np("depth"))
        es, ids = Golden("graphs").levels(str(z.np("graph")))
        self.n, self.p = z.np("pos").shape[-2], z.np("pos").shape[-1]
        self.net = eng.BSGMP(self.depth, D_UNET, 3, self.p).cuda()
        plans, self.ews, bottom = self.net.prepare([i.cuda() for i in ids[:self.depth]], [e.cuda() for e in es[:self.depth + 1]], self.n,
                                                   torch.device("cuda"))
        self.plans = [*plans, bottom]
        self.handles = [q.handle.value if hasattr(q.handle, "value") else q.handle for q in self.plans]
        self.pl, self._k1 = eng._abi.ptr_array(self.handles)
        self.ewp, self._k2 = eng._abi.ptr_array([e.data_ptr() for e in self.ews])
        self.params = self.net.block_params()
        self.pp, self._k3 = _param_ptrs(self.params)

    def sizes(self, H):
        L, a = self.L, (self.pl, self.depth, B_UNET, D_UNET, self.p)
        return (*(L.bsms_bsgmp_saved_bytes_p(*a, H, prec) for prec in (0, 1, 2)), L.bsms_bsgmp_work_bytes(*a, H),
                L.bsms_bsgmp_infer_work_bytes(*a, H), L.bsms_bsgmp_pos_work_bytes(self.pl, self.depth, B_UNET, self.p))


@pytest.fixture(scope="module")
def unets():
    return {tag: Unet(tag) for tag in ("line11", "del64_d128")}


@pytest.mark.gpu
@pytest.mark.parametrize("tag,hidden", list(UNET_BYTES))
def test_unet_size_queries(unets, tag, hidden):
    got = unets[tag].sizes(hidden)
    assert got == UNET_BYTES[(tag, hidden)]


# entry -> [(what is wrong, {overrides}, return code, prefix of bsms_last_error())].  The U-Net entries hand a bad block shape on to
# the block call, which reports it under its own name; the precision and the gradient tables are theirs.
_SHAPE = [("D = 48", dict(D=48)), ("pos_dim = 8", dict(p=8)), ("hidden = 0", dict(H=0)), ("hidden = 8", dict(H=8))]
_BF16 = [("bf16, D = 64", dict(D=64, prec=1)), ("bf16, pos_dim = 4", dict(p=4, prec=1))]
REFUSALS = {
    "bsms_gmp_fwd": [(w, o, E_UNSUPPORTED, b"gmp_fwd:") for w, o in _SHAPE],
    "bsms_gmp_bwd": [(w, o, E_UNSUPPORTED, b"gmp_bwd:") for w, o in _SHAPE] + [("partly null gradients", dict(hole=5), E_INVALID_ARG, b"gmp_bwd:")],
    "bsms_bsgmp_fwd_p": [(w, o, E_UNSUPPORTED, b"gmp_fwd:") for w, o in _SHAPE + _BF16] + [("precision = 7", dict(prec=7), E_UNSUPPORTED, b"bsgmp_fwd:")],
    "bsms_bsgmp_bwd_ev": [(w, o, E_UNSUPPORTED, b"gmp_bwd:") for w, o in _SHAPE + _BF16] + [
        ("precision = 7", dict(prec=7), E_UNSUPPORTED, b"bsgmp_bwd:"),
        ("partly null gradients", dict(hole=5), E_INVALID_ARG, b"bsgmp_bwd:"),
        ("null gradients under bf16", dict(prec=1, null_block=1), E_UNSUPPORTED, b"bsgmp_bwd:")],
    "bsms_pack_group_add_bsgmp": [(w, o, E_UNSUPPORTED, b"pack_group_add_bsgmp:") for w, o in _SHAPE + _BF16] + [
        ("precision = 7", dict(prec=7), E_UNSUPPORTED, b"pack_group_add_bsgmp:")],
}


def _refusal(u, entry, D=D_UNET, p=None, H=3, prec=0, hole=None, null_block=None):
    """One call of `entry` on the U-Net `u` (or on its level 0) with real buffers of the VALID shape; (return code, message)."""
    import ctypes as C
    L, eng, B = u.L, u.eng, B_UNET
    p = u.p if p is None else p
    s = torch.cuda.current_stream().cuda_stream
    u8 = lambda nbytes: torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    valid = (u.pl, u.depth, B, D_UNET, u.p, 3)
    saved, work = u8(L.bsms_bsgmp_saved_bytes_p(*valid, 0)), u8(L.bsms_bsgmp_work_bytes(*valid))
    h = torch.zeros(B, u.n, D_UNET, device="cuda")
    pos = torch.zeros(B, u.n, 8, device="cuda")
    out, cot, gh = torch.empty_like(h), torch.zeros_like(h), torch.full_like(h, 7.0)
    # tables long enough for hidden = 8 (4 * 9 entries per block): a refused call may look at entries before it refuses
    per, nblk = 4 * (H + 1), 2 * u.depth + 1
    filler = torch.zeros(D_UNET * (2 * D_UNET + 8), device="cuda")
    params, _k1 = eng._abi.ptr_array([filler.data_ptr()] * (per * nblk))
    g = [filler.data_ptr()] * (per * nblk)
    if hole is not None:
        g[hole] = None
    if null_block is not None:
        g[per * null_block:per * (null_block + 1)] = [None] * per
    grads, _k2 = eng._abi.ptr_array(g)
    if entry == "bsms_gmp_fwd":
        rc = L.bsms_gmp_fwd(u.handles[0], h.data_ptr(), pos.data_ptr(), B, D, p, u.n * p, H, params, out.data_ptr(), saved.data_ptr(), work.data_ptr(), s)
    elif entry == "bsms_gmp_bwd":
        rc = L.bsms_gmp_bwd(u.handles[0], h.data_ptr(), pos.data_ptr(), cot.data_ptr(), B, D, p, u.n * p, H, params, saved.data_ptr(),
                            work.data_ptr(), gh.data_ptr(), grads, s)
    elif entry == "bsms_bsgmp_fwd_p":
        rc = L.bsms_bsgmp_fwd_p(u.pl, u.ewp, u.depth, h.data_ptr(), pos.data_ptr(), B, D, p, u.n * p, H, params, out.data_ptr(), saved.data_ptr(),
                                work.data_ptr(), 0, prec, s)
    elif entry == "bsms_bsgmp_bwd_ev":
        rc = L.bsms_bsgmp_bwd_ev(u.pl, u.ewp, u.depth, h.data_ptr(), pos.data_ptr(), cot.data_ptr(), B, D, p, u.n * p, H, params, saved.data_ptr(),
                                 work.data_ptr(), gh.data_ptr(), grads, prec, 0, None, s)
    else:
        handle = C.c_void_p()
        eng._abi.check(L.bsms_pack_group_create(C.cast(C.byref(handle), C.POINTER(C.c_void_p))), "bsms_pack_group_create")
        rc = L.bsms_pack_group_add_bsgmp(handle, u.pl, u.depth, B, D, p, H, params, saved.data_ptr(), None, prec)
        L.bsms_pack_group_destroy(handle)
    msg = L.bsms_last_error()
    torch.cuda.synchronize()
    assert bool((gh == 7.0).all())                                     # refused before any launch
    return rc, msg


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(REFUSALS))
def test_refusals_keep_their_code_and_their_name(unets, entry):
    u = unets["del64_d128"]
    for what, overrides, want_rc, want_who in REFUSALS[entry]:
        rc, msg = _refusal(u, entry, **overrides)
        assert rc == want_rc and msg.startswith(want_who), (entry, what, rc, msg)
