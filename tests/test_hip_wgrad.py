"""GPU: the weight-gradient kernels of csrc/wgrad.hip addressed directly, through the C ABI (bsms_wgrad, bsms_small_wgrad), with
operands the test chooses.  dW = G^T A and db = colsum(G) are linear, so

A. INDEXING is pinned bit for bit: integer operands in [-3, 3] (about a third zeros) make every piece of every split, every
   product and every partial sum an integer below 2^24 -- whatever the kind of arithmetic, the bound, the slab partition or the
   order of the sums, the result must `torch.equal` the exact one (formed in fp64, where integers below 2^53 are exact).  Row counts
   cross every edge of the slab bookkeeping (1 .. 30 slabs, a one-row last slab, slabs shorter than the six-chunk schedule, the
   four-slab rounds of k_wgrad_reduce), at every width of the envelope, through aligned and unaligned dW sub-blocks.
B. JOB TABLES: several jobs per call, 20 jobs, an empty job, the three kinds mixed in one call, `skip_mask`, run-to-run identity.
C. The 128 x 256 tiles (D = 256, >= 262 144 rows in the call), both branches of the XCD-grouped tile map.
D. ARITHMETIC against fp64 with real-valued operands.  Per element of dW: |dW - dW64| / sum_r |G_rn| |A_rk| (the normalisation of
   profiles/r03_f16split.md), worst element and worst column (column sums of numerator and denominator).  The yardstick is a CPU fp32
   `G.T @ A` of the same operands under the same measure; criterion: engine <= 2 x fp32 + 2^-22 (the factor 2 of
   test_split_products_are_fp32_accurate; 2^-22 = the piece precision of the fp16 x 2 split).  Neither number is tuned.
E. The narrow side (k_small_wgrad / k_small_reduce) in its three production layouts.

Operands are slices of larger allocations whose rows before and after (and whose columns past D, when the pitch is wider) are NaN:
a row or column staged from outside the operand shows in dW.  Outputs live in sentinel-filled buffers that must be unchanged
outside the block the call owns.  `slab_plan` / `small_blocks` restate the launchers' partitions; they only pick row counts and
annotate failures -- nothing is asserted against the library through them.  Measured figures: profiles/wgrad_parity.txt."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -777.25                  # sentinel of the output buffers (not a value any case produces)
GUARD_ROWS = 70                 # NaN rows before and after an operand: more than one 64-row chunk
GUARD_OUT = 8                   # sentinel floats before and after an output (keeps 16-byte alignment)
KINDS = ("h2", "bf3", "bf16")   # fp16 x 2 pieces with bounds; range-free bf16 x 3; bf16 tensors
WIDTHS = (32, 64, 96, 128, 160, 192, 224, 256)
BOUND_AT = (0, 4097, -1)        # entry of the bound slot that carries the bound: first, second 16-byte read of thread 0, last
EPS_PIECE = 2.0 ** -22


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- partition mirrors
def slab_plan(Rs, D, kind):
    """launch_wgrad_same restated: (rows per slab, slabs per job, 128 x 256 tiles?) for the jobs of ONE kind in a call."""
    nblk = -(-D // 128)
    total = sum(Rs)
    wide = kind != "bf3" and D == 256 and total >= 262144
    blocks = nblk if wide else nblk * nblk
    unit = 6 * (64 if kind == "bf16" else 32)
    rows = max(128, -(-total * blocks // 128))
    rows = -(-rows // unit) * unit
    while sum(max(1, -(-R // rows)) * blocks for R in Rs) * (2 if wide else 1) > 1024:
        rows *= 2
    return rows, [max(1, -(-R // rows)) for R in Rs], wide


def small_blocks(R, D):
    """launch_small_wgrad restated: (row lanes in flight, partial blocks)."""
    nrl = 256 // (D // 4)
    rows = max(4 * nrl, -(-R // 512))
    rows = -(-rows // nrl) * nrl
    return nrl, max(1, -(-R // rows))


# ---------------------------------------------------------------------------------------------------- operands and jobs
def ints(shape, gen):
    """Integers in [-3, 3], about a third of them zero."""
    v = torch.randint(-3, 4, shape, generator=gen, device=DEV).float()
    v[torch.rand(shape, generator=gen, device=DEV) < 2.0 / 9.0] = 0.0
    return v


def normal(shape, gen):
    return torch.randn(shape, generator=gen, device=DEV)


class Operand:
    """[R, D] values inside a NaN-filled [GUARD_ROWS + R + GUARD_ROWS, ld] allocation."""

    def __init__(self, values, ld, dtype=torch.float32):
        R, D = values.shape
        self.ld = ld
        self.store = torch.full((R + 2 * GUARD_ROWS, ld), NAN, dtype=dtype, device=DEV)
        self.store[GUARD_ROWS:GUARD_ROWS + R, :D] = values.to(dtype)
        self.ptr = self.store.data_ptr() + GUARD_ROWS * ld * self.store.element_size()


class Out:
    """`n` floats between two sentinel guards; `idx` = the flat positions the call owns."""

    def __init__(self, n, idx):
        self.buf = torch.full((n + 2 * GUARD_OUT,), SENT, device=DEV)
        self.idx = idx.reshape(-1) + GUARD_OUT
        self.ptr = self.buf.data_ptr() + 4 * GUARD_OUT

    def reset(self):
        self.buf.fill_(SENT)

    def values(self):
        return self.buf[self.idx]

    def expected(self, values):
        e = torch.full_like(self.buf, SENT)
        e[self.idx] = values.reshape(-1).to(e.dtype)
        return e

    def explain(self, want):
        bad = self.buf != want
        bad |= self.buf.isnan()
        own = torch.zeros_like(bad)
        own[self.idx] = True
        first = int(bad.nonzero()[0]) - GUARD_OUT if bad.any() else None
        return (f"{int((bad & own).sum())} of {int(own.sum())} owned elements wrong, {int((bad & ~own).sum())} elements outside the "
                f"block touched, first at flat offset {first}")


class Job:
    """One bsms_wgrad_job with guarded operands, sentinel-guarded outputs and (kind h2) its two bound slots."""

    def __init__(self, eng, kind, G, A, ldw=None, col0=0, with_db=True, pad_g=0, pad_a=0, bound_at=0, g_mul=1.0, a_mul=1.0):
        self.eng, self.kind, self.G, self.A = eng, kind, G, A
        self.R, self.D = G.shape
        D = self.D
        dt = torch.bfloat16 if kind == "bf16" else torch.float32
        self.g, self.a = Operand(G, D + pad_g, dt), Operand(A, D + pad_a, dt)
        self.ldw, self.col0 = ldw or D, col0
        n, k = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(D, device=DEV), indexing="ij")
        self.w = Out(D * self.ldw, n * self.ldw + col0 + k)
        self.b = Out(D, torch.arange(D, device=DEV)) if with_db else None
        self.g_mul, self.a_mul, self.gb, self.ab = g_mul, a_mul, None, None
        if kind == "h2":   # bound = max(slot) * mul >= max |value|: the slot holds max |value| / 1, the multiplier loosens it
            width = int(eng._abi.lib().bsms_wgrad_bound_width())
            self.gb, self.ab = torch.zeros(width, device=DEV), torch.zeros(width, device=DEV)
            self.gb[bound_at] = G.abs().max() if self.R else 1.0
            self.ab[bound_at] = A.abs().max() if self.R else 1.0

    def struct(self, null_out=False):
        p = lambda t: None if t is None else t.data_ptr()
        return self.eng._abi.WgradJob(
            G=self.g.ptr, A=self.a.ptr, dW=None if null_out else self.w.ptr, db=None if null_out or self.b is None else self.b.ptr,
            R=self.R, ldg=self.g.ld, lda=self.a.ld, ldw=self.ldw, col0=self.col0, bf16=int(self.kind == "bf16"),
            g_bound=p(self.gb), a_bound=p(self.ab), g_mul=self.g_mul, a_mul=self.a_mul)

    def outs(self):
        return [o for o in (self.w, self.b) if o is not None]

    def dW(self):
        return self.w.values().view(self.D, self.D)

    def db(self):
        return self.b.values()

    def check_exact(self, note):
        """Integer operands: outputs equal the exact result, everything around them is untouched."""
        G64, A64 = self.G.double(), self.A.double()
        dW, db = G64.T @ A64, G64.sum(0)
        assert float(dW.abs().max()) < 2 ** 24
        rows, ns, wide = slab_plan([self.R], self.D, self.kind)
        note = (f"{note}: kind {self.kind} D {self.D} R {self.R} ldw {self.ldw} col0 {self.col0} -- alone in a call: {ns[0]} slabs of "
                f"{rows} rows{', 128 x 256 tiles' if wide else ''}")
        want = self.w.expected(dW)
        assert torch.equal(self.w.buf, want), f"dW {note}: {self.w.explain(want)}"
        if self.b is not None:
            want = self.b.expected(db)
            assert torch.equal(self.b.buf, want), f"db {note}: {self.b.explain(want)}"

    def check_guards(self, note):
        """Real-valued operands: finite outputs, sentinels intact."""
        for o, val in ((self.w, self.dW()), (self.b, None if self.b is None else self.db())):
            if o is None:
                continue
            assert bool(val.isfinite().all()), f"{note}: non-finite output (a row or column from outside the operand?)"
            want = o.expected(val)
            assert torch.equal(o.buf, want), f"{note}: {o.explain(want)}"


_WORK = {}


def _work(nbytes):
    if _WORK.get("n", 0) < nbytes:
        _WORK["buf"], _WORK["n"] = torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes
    return _WORK["buf"]


def launch(eng, jobs, D, skip=0, null_out=()):
    """One bsms_wgrad call on the current stream, synchronised."""
    L = eng._abi.lib()
    tab = (eng._abi.WgradJob * len(jobs))(*[j.struct(null_out=i in null_out) for i, j in enumerate(jobs)])
    nbytes = int(L.bsms_wgrad_work_bytes(D, len(jobs)))
    eng._abi.check(L.bsms_wgrad(tab, len(jobs), D, skip, _work(nbytes).data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
                   "bsms_wgrad")
    torch.cuda.synchronize()


def out_layouts(D):
    """(ldw, col0): the whole matrix; the right half of [D, 2D]; sub-blocks of the first edge Linear's [D, 2D + p + 1] weight at
    p + 1 = 3 (both only 4-byte aligned: the scalar store path) and at p + 1 = 4 (16-byte aligned)."""
    return [(D, 0), (2 * D, D), (2 * D + 3, 3), (2 * D + 3, 3 + D), (2 * D + 4, 4)]


def varied_job(eng, kind, G, A, i):
    """Job number i of a sweep: cycles the output layout (5), the bound entry (3), exact / 64 x loose bounds (2), wider operand
    pitches (2 x 2) and a null db (every 4th)."""
    D = G.shape[1]
    ldw, col0 = out_layouts(D)[i % 5]
    return Job(eng, kind, G, A, ldw, col0, with_db=i % 4 != 3, pad_g=8 * (i % 2), pad_a=16 * ((i // 2) % 2), bound_at=BOUND_AT[i % 3],
               g_mul=64.0 if i % 2 else 1.0, a_mul=64.0 if i % 4 == 2 else 1.0)


# ==================================================================================================== A: indexing, bit for bit
ROWS_F32 = [1, 31, 32, 33, 191, 192, 193, 385, 769, 2305, 2497, 3073, 5569]    # 1, 2, 3, 5, 13, 14, 17, 30 slabs of 192 rows
ROWS_BF16 = [1, 63, 64, 65, 383, 384, 385, 12 * 384 + 1, 16 * 384 + 1]        # the same edges on 64-row chunks, 384-row slabs


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_indexing_bit_for_bit(eng, kind, D):
    gen = _gen(1000 + D)
    for i, R in enumerate(ROWS_BF16 if kind == "bf16" else ROWS_F32):
        job = varied_job(eng, kind, ints((R, D), gen), ints((R, D), gen), i)
        launch(eng, [job], D)
        job.check_exact(f"sweep entry {i}")


# ==================================================================================================== B: job tables
TABLES = {"7/4000/193/1": [7, 4000, 193, 1], "2400/900/61": [2400, 900, 61], "twenty jobs": list(range(1, 21)),
          "empty job in the middle": [500, 0, 300]}


@pytest.mark.parametrize("D", (128, 160, 256))
@pytest.mark.parametrize("kind", KINDS)
def test_job_tables(eng, kind, D):
    gen = _gen(2000 + D)
    for name, Rs in TABLES.items():
        jobs = [varied_job(eng, kind, ints((R, D), gen), ints((R, D), gen), j) for j, R in enumerate(Rs)]
        launch(eng, jobs, D)
        rows, ns, _ = slab_plan(Rs, D, kind)
        for j, job in enumerate(jobs):     # an empty job (R = 0) must come back as zeros: the exact result of an empty sum
            job.check_exact(f"table {name} job {j} ({ns[j]} slabs of {rows} rows in this call)")


MIXED_KINDS = ["h2", "bf3", "bf16", "h2", "bf3", "bf16"]
MIXED_ROWS = [20000, 7000, 40000, 9000, 21000, 30000]    # per kind the pair shares slabs longer than either job would get alone:
MIXED_MASKS = [1 << j for j in range(6)] + [0b101010]   # a skipped job that stopped counting would change its partner's bits


@pytest.mark.parametrize("D", (96, 256))
@pytest.mark.parametrize("values", ("ints", "normal"))
def test_mixed_kinds_skip_mask_and_determinism(eng, values, D):
    for k in set(MIXED_KINDS):     # the premise of the masked comparison, from the mirror
        both = [R for R, kk in zip(MIXED_ROWS, MIXED_KINDS) if kk == k]
        assert slab_plan(both, D, k)[0] not in (slab_plan(both[:1], D, k)[0], slab_plan(both[1:], D, k)[0])
    gen = _gen(3000 + D)
    make = ints if values == "ints" else normal
    jobs = []
    for j, (kind, R) in enumerate(zip(MIXED_KINDS, MIXED_ROWS)):
        G, A = make((R, D), gen), make((R, D), gen)
        if kind == "bf16":
            G, A = G.bfloat16().float(), A.bfloat16().float()
        jobs.append(varied_job(eng, kind, G, A, j + 1))
    launch(eng, jobs, D)
    for j, job in enumerate(jobs):
        job.check_exact(f"mixed call job {j}") if values == "ints" else job.check_guards(f"mixed call job {j}")
    full = [[o.buf.clone() for o in job.outs()] for job in jobs]
    for job in jobs:
        for o in job.outs():
            o.reset()
    launch(eng, jobs, D)
    for j, job in enumerate(jobs):
        for o, want in zip(job.outs(), full[j]):
            assert torch.equal(o.buf, want), f"job {j}: the same call twice differs: {o.explain(want)}"
    for mask in MIXED_MASKS:
        skipped = [j for j in range(6) if mask >> j & 1]
        null_out = skipped[:1] if len(skipped) > 1 else [j for j in skipped if j % 2 == 0]   # null or untouched, both are legal
        for job in jobs:
            for o in job.outs():
                o.reset()
        launch(eng, jobs, D, skip=mask, null_out=null_out)
        for j, job in enumerate(jobs):
            for o, want in zip(job.outs(), full[j]):
                if j in skipped:
                    assert bool((o.buf == SENT).all()), f"mask {mask:#b}: skipped job {j} was written"
                else:
                    assert torch.equal(o.buf, want), f"mask {mask:#b}: job {j} differs from the unmasked call: {o.explain(want)}"


# ==================================================================================================== C: 128 x 256 tiles
WIDE_ROWS = [131073, 98304, 40000]    # >= 262 144 rows in the call; 32 / 24 / 10 slabs: whole groups of 8 slabs and a tail


@pytest.mark.parametrize("kind", ("h2", "bf16"))
def test_wide_tiles_bit_for_bit(eng, kind):
    D = 256
    rows, ns, wide = slab_plan(WIDE_ROWS, D, kind)
    assert wide and ns == [32, 24, 10], (rows, ns, wide)      # the row counts do what they were chosen for (mirror only)
    gen = _gen(4000)
    jobs = [varied_job(eng, kind, ints((R, D), gen), ints((R, D), gen), j) for j, R in enumerate(WIDE_ROWS)]
    launch(eng, jobs, D)
    for j, job in enumerate(jobs):
        job.check_exact(f"128 x 256 tiles job {j} ({ns[j]} slabs of {rows} rows in this call)")


# ==================================================================================================== D: arithmetic against fp64
def ratio(err, scale):
    """err / scale per element; 0 / 0 counts as 0 and x / 0 as inf."""
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))


class Figures:
    """Error figures of one job against fp64, for the engine and for the CPU fp32 product of the same operands."""

    def __init__(self, job):
        G64, A64 = job.G.double(), job.A.double()
        ref, self.scale = G64.T @ A64, G64.abs().T @ A64.abs()
        cpu = (job.G.cpu().T @ job.A.cpu()).to(DEV)
        self.err = {"engine": (job.dW().double() - ref).abs(), "fp32": (cpu.double() - ref).abs()}
        self.db = None
        if job.b is not None:
            bref, bscale = G64.sum(0), G64.abs().sum(0)
            bcpu = job.G.cpu().sum(0).to(DEV)
            self.db = {"engine": float(ratio((job.db().double() - bref).abs(), bscale).max()),
                       "fp32": float(ratio((bcpu.double() - bref).abs(), bscale).max())}

    def element(self, who, cols=None):
        e, s = (self.err[who], self.scale) if cols is None else (self.err[who][:, cols], self.scale[:, cols])
        return float(ratio(e, s).max())

    def column(self, who, cols=None):
        e, s = (self.err[who], self.scale) if cols is None else (self.err[who][:, cols], self.scale[:, cols])
        return float(ratio(e.sum(0), s.sum(0)).max())


def hold(fig, label, cols=None, with_db=True):
    """Print the figures, then hold the engine to 2 x fp32 + 2^-22: worst element, worst column (of `cols`), db."""
    el, co = (fig.element("engine", cols), fig.element("fp32", cols)), (fig.column("engine", cols), fig.column("fp32", cols))
    db = (fig.db["engine"], fig.db["fp32"]) if fig.db and with_db else None
    print(f"PARITY {label}: element engine {el[0]:.3e} fp32 {el[1]:.3e} | column engine {co[0]:.3e} fp32 {co[1]:.3e}"
          + (f" | db engine {db[0]:.3e} fp32 {db[1]:.3e}" if db else ""))
    assert el[0] <= 2.0 * el[1] + EPS_PIECE, f"{label}: worst element {el[0]:.3e} against fp32 {el[1]:.3e}"
    assert co[0] <= 2.0 * co[1] + EPS_PIECE, f"{label}: worst column {co[0]:.3e} against fp32 {co[1]:.3e}"
    if db:
        assert db[0] <= 2.0 * db[1] + EPS_PIECE, f"{label}: db {db[0]:.3e} against fp32 {db[1]:.3e}"


def octave(R, level, gen):
    """A column whose entries all lie within one octave below `level`, random signs."""
    return level * (0.5 + 0.5 * torch.rand(R, generator=gen, device=DEV)) * (torch.randint(0, 2, (R,), generator=gen, device=DEV) * 2 - 1)


def arithmetic_cases(kind, R, D, gen):
    """(name, G, A, {name: columns held on their own}, columns under the 2^-16 envelope)."""
    G, A = normal((R, D), gen), normal((R, D), gen)
    yield "normal", G, A, {}, []
    span_a = torch.logspace(-4, 3, R, device=DEV).unsqueeze(1)
    span_g = torch.logspace(-8, 0, R, device=DEV)[torch.randperm(R, generator=gen, device=DEV)].unsqueeze(1)
    yield "rows 1e-4..1e3 x 1e-8..1", normal((R, D), gen) * span_g, normal((R, D), gen) * span_a, {}, []
    yield "1e-30 x 1e30", normal((R, D), gen) * 1e-30, normal((R, D), gen) * 1e30, {}, []
    yield "1e-12 x 1e-12", normal((R, D), gen) * 1e-12, normal((R, D), gen) * 1e-12, {}, []
    small = [1, D // 2 + 3, D - 1]
    if kind == "bf3":      # three columns of A at 1e-7 of the tensor maximum, held per column
        A2 = normal((R, D), gen)
        top = float(A2.abs().max())
        for c in small:
            A2[:, c] = normal((R,), gen) * (1e-7 * top)
        yield "columns at 1e-7", normal((R, D), gen), A2, {f"column {c}": [c] for c in small}, []
    if kind == "h2":       # columns of A 2^-10 and 2^-18 below the bound keep the criterion; 2^-24: one bit per octave below 2^-18
        A2 = normal((R, D), gen)
        top = float(A2.abs().max())
        for c, k in zip(small, (10, 18, 24)):
            A2[:, c] = octave(R, top * 2.0 ** -k, gen)
        yield "columns below the bound", normal((R, D), gen), A2, {"column at 2^-10": [small[0]], "column at 2^-18": [small[1]]}, [small[2]]


ARITH_ROWS = (5569, 20000)


@pytest.mark.parametrize("D", (96, 128, 160, 256))
@pytest.mark.parametrize("kind", KINDS)
def test_arithmetic_against_fp64(eng, kind, D):
    gen = _gen(5000 + D)
    for i, R in enumerate(ARITH_ROWS):
        for name, G, A, own, envelope in arithmetic_cases(kind, R, D, gen):
            if kind == "bf16":      # the operands ARE bf16 tensors: every party multiplies the rounded values
                G, A = G.bfloat16().float(), A.bfloat16().float()
            job = Job(eng, kind, G, A, *out_layouts(D)[(i + 3) % 5], pad_g=8 * i)
            launch(eng, [job], D)
            label = f"D {kind} D={D} R={R} {name}"
            job.check_guards(label)
            fig = Figures(job)
            keep = [c for c in range(D) if c not in envelope]
            hold(fig, label, None if not envelope else keep)
            for cname, cols in own.items():
                hold(fig, f"{label}, {cname}", cols, with_db=False)
            for c in envelope:     # include/bsms_hip.h: 22 bits down to 2^-18 of the bound, one bit less per octave: 2^-16 at 2^-24
                e = fig.element("engine", [c])
                print(f"PARITY {label}, column at 2^-24: element engine {e:.3e} fp32 {fig.element('fp32', [c]):.3e} (envelope 2^-16 = {2.0 ** -16:.3e})")
                assert e <= 2.0 ** -16, f"{label}: column at 2^-24 of the bound: {e:.3e}"


def test_wide_tiles_arithmetic(eng):
    """One real-valued call on the 128 x 256 tiles under the criterion of D (fp16 x 2 pieces, exact bounds)."""
    D = 256
    gen = _gen(4500)
    jobs = [varied_job(eng, "h2", normal((R, D), gen), normal((R, D), gen), 2 * j) for j, R in enumerate(WIDE_ROWS)]
    launch(eng, jobs, D)
    for j, job in enumerate(jobs):
        job.check_guards(f"128 x 256 tiles job {j}")
        hold(Figures(job), f"C h2 D=256 R={job.R} normal, 128 x 256 tiles")


# ==================================================================================================== E: the narrow side
SMALL_LAYOUTS = ("encoder", "decoder", "edge")


def small_rows(D):
    """R = 1, rows in flight +- 1, one unrolled pass +- 1, and the row counts that give 32 .. 512 partial blocks (k_small_reduce sums
    four blocks per lane and round while w + 96 < nwg)."""
    nrl = 256 // (D // 4)
    rows = [1, nrl - 1, nrl + 1, 4 * nrl - 1, 4 * nrl + 1] + [(k - 1) * 4 * nrl + 1 for k in (32, 33, 97, 128, 129, 512)]
    assert [small_blocks(R, D)[1] for R in rows[5:]] == [32, 33, 97, 128, 129, 512]      # mirror only
    return rows


class SmallCase:
    def __init__(self, eng, layout, G, S, S_ld, want_colsum):
        self.eng, self.layout, self.G, self.S = eng, layout, G, S
        self.R, self.D = G.shape
        D, self.S_cols, self.S_ld = self.D, S.shape[1], S_ld
        self.g = Operand(G, D)
        self.s = Operand(S, S_ld or self.S_cols)      # columns past S_cols are NaN: read by the 16-byte path, never used
        if layout == "encoder":      # weight [D, S_cols] of the encoder's first Linear
            self.os, self.of, n = 1, self.S_cols, D * self.S_cols
        elif layout == "decoder":    # weight [S_cols, D] of the decoder's last Linear
            self.os, self.of, n = D, 1, self.S_cols * D
        else:                        # the fiber columns of the first edge Linear's weight [D, 2D + p + 1], p + 1 = S_cols
            self.os, self.of = 1, 2 * D + self.S_cols
            n = D * self.of
        s, f = torch.meshgrid(torch.arange(self.S_cols, device=DEV), torch.arange(D, device=DEV), indexing="ij")
        self.out = Out(n, s * self.os + f * self.of)
        self.colsum = Out(D, torch.arange(D, device=DEV)) if want_colsum else None
        self.colsum_S = Out(8, torch.arange(self.S_cols, device=DEV)) if layout == "decoder" else None

    def launch(self):
        L = self.eng._abi.lib()
        nbytes = int(L.bsms_small_wgrad_work_bytes(self.D))
        p = lambda o: None if o is None else o.ptr
        self.eng._abi.check(L.bsms_small_wgrad(self.g.ptr, self.s.ptr, self.R, self.D, self.S_cols, self.S_ld, self.out.ptr, self.os, self.of,
                                               p(self.colsum), p(self.colsum_S), _work(nbytes).data_ptr(), nbytes,
                                               torch.cuda.current_stream().cuda_stream), "bsms_small_wgrad")
        torch.cuda.synchronize()

    def note(self):
        nrl, nwg = small_blocks(self.R, self.D)
        return f"{self.layout} D {self.D} R {self.R} S_cols {self.S_cols} S_ld {self.S_ld}: {nwg} partial blocks, {nrl} rows in flight"

    def parts(self):
        G64, S64 = self.G.double(), self.S.double()
        return [(self.out, S64.T @ G64, S64.abs().T @ G64.abs(), lambda: self.S.cpu().T @ self.G.cpu()),
                (self.colsum, G64.sum(0), G64.abs().sum(0), lambda: self.G.cpu().sum(0)),
                (self.colsum_S, S64.sum(0), S64.abs().sum(0), lambda: self.S.cpu().sum(0))]

    def check_exact(self):
        for o, ref, _, _ in self.parts():
            if o is not None:
                want = o.expected(ref)
                assert torch.equal(o.buf, want), f"{self.note()}: {o.explain(want)}"

    def check_criterion(self):
        for name, (o, ref, scale, cpu) in zip(("out", "colsum", "colsum_S"), self.parts()):
            if o is None:
                continue
            got = o.values().view(ref.shape)
            want = o.expected(got)
            assert bool(got.isfinite().all()) and torch.equal(o.buf, want), f"{self.note()} {name}: {o.explain(want)}"
            e = float(ratio((got.double() - ref).abs(), scale).max())
            e32 = float(ratio((cpu().to(DEV).double() - ref).abs(), scale).max())
            print(f"PARITY E {self.note()} {name}: element engine {e:.3e} fp32 {e32:.3e}")
            assert e <= 2.0 * e32 + EPS_PIECE, f"{self.note()} {name}: {e:.3e} against fp32 {e32:.3e}"


def small_shapes(i):
    """(layout, S_cols, S_ld) of sweep entry i, one per layout: S_cols runs 1..8 for the encoder and the decoder (4 and 8: 16-byte
    row loads, the rest by element; 5..7 also on a padded pitch of 8), the edge layout is p = 2 on the saved fiber's pitch of 4 or
    p = 5 on a pitch of 8."""
    enc, dec = 1 + i % 8, 1 + (i + 3) % 8
    return [("encoder", enc, 8 if enc in (5, 6, 7) and i % 2 == 0 else 0), ("decoder", dec, 8 if dec in (5, 6, 7) and i < 4 else 0),
            ("edge", *((3, 4) if i % 2 == 0 else (6, 8)))]


@pytest.mark.parametrize("D", WIDTHS)
def test_narrow_side(eng, D):
    gen = _gen(6000 + D)
    rows = small_rows(D)
    for i, R in enumerate(rows):
        for layout, S_cols, S_ld in small_shapes(i):
            case = SmallCase(eng, layout, ints((R, D), gen), ints((R, S_cols), gen), S_ld, want_colsum=layout == "encoder" or i % 2 == 1)
            case.launch()
            case.check_exact()
    for i, R in ((3, rows[-2]), (10, rows[-1])):      # 129 and 512 partial blocks
        for layout, S_cols, S_ld in small_shapes(i):
            case = SmallCase(eng, layout, normal((R, D), gen), normal((R, S_cols), gen), S_ld, want_colsum=True)
            case.launch()
            case.check_criterion()
