// The generic chain kernels: k_chain_fwd / k_chain_bwd (LDS weight ring, one wave per 16 rows) and their feature-split
// forms for small launches, k_fs_fwd / k_fs_bwd.  Templates over the width (NB = D / 16): every chain_d*.hip instantiates
// them for its own width through chain_launch.h.  Like chain_dev.h: internal linkage, and the including translation unit
// sets `#pragma clang fp contract(off)` before its first include.
#pragma once
#include "chain_dev.h"

namespace {

// -------------------------------------------------------------------------------- forward chain
// Register budget of the generic chain kernels (waves per EU the compiler allocates for).  D = 32 / 64 / 128, multi-round
// launches: BSMS_CHAIN_WPE (chain_dev.h).  Single-round variants and D = 256: 2 (256 VGPRs).  D = 96 / 160 / 192 / 224
// take 2 as well: at 4 the D = 96 forward kernels spill (20-72 bytes of scratch per lane), and the wider ones need 140-230
// VGPRs (profiles/width_rates.txt) -- one workgroup per CU either way (resident_per_cu).
template <int NB, bool LONE>
constexpr int chain_wpe() { return (NB == 2 || NB == 4 || NB == 8) && !LONE ? BSMS_CHAIN_WPE : 2; }

// TIMING (experiments, profiles/tile_timeline.py): phase stamps of wave 0; a separate instantiation so that the
// production kernel carries none of it.
template <int NB, int IN, int OUT, bool TIMING = false, bool BF = false, bool LONE = false>
__global__ __launch_bounds__(kChainMaxThreads) __attribute__((amdgpu_waves_per_eu(chain_wpe<NB, LONE>()))) void k_chain_fwd(ChainFwdArgs a) {
  constexpr int D = NB * 16;
  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
  const int cw = int(blockDim.x >> 6) - a.nload;   // compute waves of this launch (4..7, chosen by the launcher); the last wave(s) load
  if (wave >= cw) {  // loader wave (uniform branch)
    loader_dispatch<NB, BF ? 1 : kPL>(a.nload, wave - cw, a.wseq, a.nseq, lds, lane, a.ntiles, a.nring, IN == IN_EDGE ? a.w0t : nullptr);
    return;
  }
  // IN_EDGE: the fiber weights are read from the LDS side table (read from HBM/L2 they cost one dependent round
  // trip per 16 bytes: 24 of them per tile, the largest part of the input stage)
  const float* w0t = a.w0t;
  if (IN == IN_EDGE) {
    lds_barrier();
    w0t = reinterpret_cast<const float*>(lds);
  }
  Slot slot{0, a.nring};  // ring slot of the next chunk; runs on across this workgroup's tiles exactly like the loader's
  float4* const ring = lds + Ring<NB>::PRE4;
  unsigned* brow = bound_row<NB>(lds, wave, lane, any_slot(a.amax));   // this wave's running magnitude bounds
  // Persistent workgroups: the grid is sized to what the chip holds at once and strides over the tiles, so a CU
  // never waits for the dispatcher to refill a slot (measured: 20-35 % of slot time was empty with one
  // workgroup per tile) and the loader is already fetching the next tile's first chunk during this epilogue.
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
  const int64_t row = int64_t(tile) * (16 * cw) + wave * 16 + (lane & 15);
  const bool live = row < a.R;
  const int64_t rowc = live ? row : 0;   // what a lane past the end reads (its results are never stored)
  const int64_t roff = live ? row * D : -1;  // row offset for stores; negative = no store
  int stamp_i = 0;
  unsigned long long waited = 0;
  auto stamp = [&]() {  // experiments: wave 0 / lane 0 records the shader clock at phase boundaries
    if (TIMING && a.timing && tid == 0 && stamp_i < 16) a.timing[int64_t(tile) * 16 + stamp_i++] = __builtin_amdgcn_s_memtime();
  };
  stamp();
  if (TIMING && a.timing && tid == 0) {
    a.timing[int64_t(tile) * 16 + 14] = __builtin_amdgcn_s_memrealtime();
    a.timing[int64_t(tile) * 16 + 13] = (uint64_t(__builtin_amdgcn_s_getreg(63508)) << 32) |  // XCC_ID
                                        uint32_t(__builtin_amdgcn_s_getreg(63492));             // HW_ID
  }

  f32x4 act[NB], acc[NB];
  // single-round launches (256-register budget, nothing to overlap a memory round trip with): the second source of a Linear
  // over [x, x2] is requested together with the first and stays in registers (the multi-round variants re-read it twice)
  constexpr bool KEEP2 = LONE && IN == IN_ROWS2 && NB == 8;
  f32x4 x2t[KEEP2 ? NB : 1];

  // ---- input stage
  if (IN == IN_ROWS || IN == IN_ROWS2) {
    load_rows<NB>(act, a.x + rowc * D, lg);
    if constexpr (KEEP2) load_rows<NB>(x2t, a.x2 + rowc * D, lg);
  } else if (IN == IN_SMALL) {
    load_features<NB>(act, a.bias_in, lg);
    for (int k = 0; k < a.K0; ++k) axpy_features<NB>(act, w0t + k * D, a.x[rowc * a.K0 + k], lg);
    relu_into<NB>(act, act);
  } else {  // IN_EDGE: relu(Ps[src] + Pd[dst] + Wf . [pos_i - pos_j, |pos_i - pos_j|])   (ops/basic.py:70-92)
    {
      const int b = int(rowc / a.E), q = int(rowc - int64_t(b) * a.E);
      const int i = a.src[q], j = a.dst[q];
      load_rows<NB>(act, a.Ps + (int64_t(b) * a.N + i) * D, lg);
      load_rows<NB>(acc, a.Pd + (int64_t(b) * a.N + j) * D, lg);
      const float* pb = a.pos + b * a.pos_bstride;
      float pi[7], pj[7];  // check_gmp: p <= 7
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const int cc = c < a.p ? c : 0;   // uniform clamp: the loads stay unconditional
        pi[c] = pb[int64_t(i) * a.p + cc];
        pj[c] = pb[int64_t(j) * a.p + cc];
      }
      // all gathers of the tile are in flight before the first use
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NB; ++t) act[t] += acc[t];
      float n2 = 0.f;
#pragma unroll
      for (int c = 0; c < 7; ++c)
        if (c < a.p) {
          const float rel = pi[c] - pj[c];
          n2 = fmaf(rel, rel, n2);
          axpy_features<NB>(act, w0t + c * D, rel, lg);
        }
      const float nrm = sqrtf(n2);
      axpy_features<NB>(act, w0t + a.p * D, nrm, lg);
      relu_into<NB>(act, act);
      if (a.fiber_out && live && lg == 0) {   // one lane per row keeps the fiber for the backward (16 or 32 bytes per edge)
        float f[8];
#pragma unroll
        for (int c = 0; c < 7; ++c) f[c] = c < a.p ? pi[c] - pj[c] : (c == a.p ? nrm : 0.f);
        f[7] = a.p == 7 ? nrm : 0.f;
        const int ld = fiber_ld(a.p);
        float4* dst = reinterpret_cast<float4*>(a.fiber_out + row * ld);
        dst[0] = make_float4(f[0], f[1], f[2], f[3]);
        if (ld == 8) dst[1] = make_float4(f[4], f[5], f[6], f[7]);
      }
    }
  }

  // ---- MFMA stages.  The activation entering a stage is stored to HBM from inside that stage (mfma_stage).
  stamp();            // input stage done
  stamp();
  float* pending = (IN == IN_SMALL || IN == IN_EDGE) ? a.store_in : nullptr;   // uniform
  if (a.nstage == 0) {
    store_rows<NB, false>(act, pending, roff, lg);
    store_mask_bits<NB>(act, pending, a.R, roff, lg);
  }
  if (OUT == OUT_PLAIN2) {  // two Linears of the SAME rows (the edge MLP's two node projections): one launch, one read of x
    const float m = row_amax<NB>(act);
    note_amax(brow, 0, m, lane);
    const RowScale rs = scale_of(m);
    mfma_stage<NB, true, 2, LONE>(acc, act, rs, ring, slot, lane);
    store_rows<NB, false>(acc, a.y, roff, lg);
    mfma_stage<NB, true, 2, LONE>(acc, act, rs, ring, slot, lane);
    store_rows<NB, false>(acc, a.y2, roff, lg);
    continue;
  }
  for (int l = 0; l < a.nstage; ++l) {
    if constexpr (BF) {
      if (IN == IN_ROWS2 && l == 0) {   // BSMS_BF16_NODES: Linear over [x, x2], both rounded to bf16 as they enter; the bias rides in the FIRST pack
        float m = row_amax<NB>(act);
        load_rows<NB>(acc, a.x2 + rowc * D, lg);
        m = fmaxf(m, row_amax<NB>(acc));
        note_amax(brow, 0, m, lane);      // bound of the fp32 rows [x, x2]: operands of the first Linear's fp32 weight-gradient job
        mfma_stage_bf<NB>(acc, act, ring, slot, lane, true, nullptr, roff, 0);
        load_rows<NB>(act, a.x2 + rowc * D, lg);
        mfma_stage_bf<NB>(acc, act, ring, slot, lane, false, nullptr, roff, 0);
      } else {
        mfma_stage_bf<NB>(acc, act, ring, slot, lane, true, pending, roff, (a.store_mode & 4) ? 0 : a.R);   // acc = bias + W act
      }
    } else if (IN == IN_ROWS2 && l == 0) {
      // Linear over the concatenation [x, x2]: ONE row scale (the larger of the two rows' maxima; the second source is
      // read once more for it -- node-level rows, L2-resident) and one weight scale (PackDesc::mate), so the second half
      // continues the raw sums of the first; the bias rides in the second pack
      float m = row_amax<NB>(act);
      stamp();          // (timing builds) x has arrived
      if constexpr (KEEP2) {
        m = fmaxf(m, row_amax<NB>(x2t));
      } else {
        load_rows<NB>(acc, a.x2 + rowc * D, lg);
        m = fmaxf(m, row_amax<NB>(acc));
      }
      stamp();          // x2 has arrived
      note_amax(brow, 0, m, lane);
      const RowScale rs = scale_of(m);
      mfma_stage<NB, true, 0, LONE>(acc, act, rs, ring, slot, lane);
      stamp();          // first half of stage 0
      if constexpr (KEEP2) {
        mfma_stage<NB, false, 2, LONE>(acc, x2t, rs, ring, slot, lane);
      } else {
        load_rows<NB>(act, a.x2 + rowc * D, lg);
        mfma_stage<NB, false, 2, LONE>(acc, act, rs, ring, slot, lane);
      }
    } else {
      const float m = row_amax<NB>(act);
      note_amax(brow, l, m, lane);
      mfma_stage<NB, true, 2, LONE, TIMING>(acc, act, scale_of(m), ring, slot, lane, pending, roff, a.store_mode & 3,
                                      (a.store_mode & 4) ? 0 : a.R, &waited, row, (a.store_mode & 8) ? 0 : a.R);  // acc = bias + W act
    }
    stamp();          // stage l done
    pending = nullptr;
    const bool last = (l == a.nstage - 1);
    if (!last || OUT == OUT_SMALL) {
      relu_into<NB>(act, acc);
      if (!last) pending = a.store[l];
      else store_rows<NB, false>(act, a.store[l], roff, lg);
    }
  }
  stamp();
  if (TIMING && a.timing && tid == 0) {
    a.timing[int64_t(tile) * 16 + 15] = __builtin_amdgcn_s_memrealtime();
    a.timing[int64_t(tile) * 16 + 11] = waited;
  }
  if (!live) continue;

  // ---- output
  if (OUT == OUT_LN) {  // LayerNorm(elementwise_affine=False), eps 1e-5  (ops/basic.py:18)
    // single-round launches: the residual rows are requested BEFORE the LayerNorm arithmetic (`act` and `x2t` are dead by
    // now) instead of one exposed round trip each after it; the additions below are the same, in the same order
    constexpr bool EARLY = LONE && !BF && NB == 8;
    if constexpr (EARLY) {
      if (a.resid) load_rows<NB>(act, a.resid + row * D, lg);
      if constexpr (KEEP2) { if (a.resid2) load_rows<NB>(x2t, a.resid2 + row * D, lg); }
    }
    const float mean = row_sum<NB>(acc) * (1.f / D);
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[t][r] -= mean;
        ss = fmaf(acc[t][r], acc[t][r], ss);
      }
    ss = group_sum(ss);
    const float rstd = 1.f / sqrtf(ss * (1.f / D) + 1e-5f);
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] *= rstd;
    if constexpr (BF && IN == IN_EDGE) {   // edge messages of the bf16 precision: stored (and consumed by the aggregation) as bf16
      store_rows_bf16<NB>(acc, a.y, roff, lg);
      if (a.rstd && lg == 0) a.rstd[row] = rstd;
      continue;
    }
    store_rows<NB, false>(acc, a.yln, roff, lg);
    if (a.rstd && lg == 0) a.rstd[row] = rstd;
    if (a.resid) {
      if constexpr (!EARLY) load_rows<NB>(act, a.resid + row * D, lg);
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[t] += act[t];
    }
    if (a.resid2) {   // (LN + x) + skip: the same two additions, in the same order, as GMP's `+ x` then BSGMP's `h + down_outs`
      if constexpr (EARLY && KEEP2) {
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[t] += x2t[t];
      } else {
        load_rows<NB>(act, a.resid2 + row * D, lg);
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[t] += act[t];
      }
    }
    store_rows<NB, false>(acc, a.y, roff, lg, a.out_mode);
    if (TIMING && a.timing && tid == 0) {
      __builtin_amdgcn_s_waitcnt(0);  // experiments: all of this wave's stores acknowledged
      a.timing[int64_t(tile) * 16 + 12] = __builtin_amdgcn_s_memrealtime();
    }
  } else if (OUT == OUT_PLAIN) {
    if (a.accumulate) store_rows<NB, true>(acc, a.y, roff, lg);
    else store_rows<NB, false>(acc, a.y, roff, lg);
  } else {  // OUT_SMALL: the narrow last Linear (decoder, models/model.py:22) on the VALU
    for (int c = 0; c < a.C; ++c) {
      const float v = dot_features<NB>(act, a.wout + c * D, lg);
      if (lg == 0) a.y[row * a.C + c] = v + a.bout[c];
    }
  }
  }  // tile loop
  flush_bounds(a.amax, kMaxStages + 1, brow, wave, lane);
}

// ------------------------------------------------------------------- small launches: feature-split forward chain ----
// A launch of a few thousand rows at most (every node-level MLP of a batch-1 step / rollout, the coarse levels of any
// step) is LATENCY, not throughput: in k_chain_fwd one wave per SIMD owns 16 rows x all 128 features and works through
// ~750-900 cycles per 32-feature chunk (profiles/census/stage_lone.hip: 24 MFMAs 427, its 16 ds_read_b128 of shared
// weight fragments 513 at the rate a lone wave gets, the two-way split 187, barrier-serialised), 4.5k cycles per Linear,
// 12 us for the node MLP whatever the row count -- and no loader / ring variation moves it (profiles/lone_timeline.py).
// Here the FEATURES of a 16-row tile are split over the four waves of a 256-thread workgroup: wave w owns output feature
// blocks 2w, 2w+1 of every Linear = a quarter of the MFMAs, of the split, of the epilogue arithmetic.  Its accumulator
// layout is exactly K block w of the next Linear's B operand (chain.h), so what the waves exchange through LDS per
// Linear is 2 KB of fp16 pieces each plus the row maximum -- two LDS barriers.  Each wave needs only ITS quarter of every
// weight chunk, and all four together read each weight byte once per tile: the fragments come straight from L2 into
// registers (one 1 KB global_load_dwordx4 per fragment), a whole Linear ahead -- no LDS ring, no loader wave, no chunk
// barriers.  Per-element arithmetic and its order are those of k_chain_fwd (same split, same three products per
// accumulator in the same order, same row scale, LayerNorm on the full row gathered through LDS): BIT-IDENTICAL results
// (tests/test_hip_parity.py::test_feature_split_kernels_equal_the_ring_kernels).  Weight traffic per row is 4-14x that
// of the persistent ring kernels, so the launcher takes this path only below kFsMaxRows rows.
// Same-box sweeps of the threshold (profiles/r04 fs_rows): airfoil B = 8 step 187.1 (never) / 188.0 (5000) / 187.3 (12288) /
// 185.2 (24000) steps/s; B = 1 rollout 1613 (never) / 1750 (3000) / 1783 (12288): the level-0 launches of a batch-1 step
// (5233 rows) gain, the 10 104 rows of level 2 at batch 8 do not.
constexpr int kFsMaxRows = 6144;    // 384 tiles of 16 rows: one and a half per CU
// The backward form re-reads the full dy / y rows in every wave and runs at 256 VGPRs: per level of the batch-1 / batch-8
// traces it wins up to ~2600 rows (14.3-16.6 us against ~19.6 for the single-round ring kernel) and loses at 4728-5233 rows
// (24.7-29.4 against 20-23 us).
constexpr int kFsMaxRowsBwd = 3072;

struct FsPack {           // one weight pack of the chain as wave `w` sees it
  float4 f[16];           // [chunk c][block i = 0, 1][plane h, l]  -> f[c * 4 + i * 2 + plane]
  float4 bias[2];         // bias of the own feature blocks (header of the last chunk), this lane's features
  float scale;            // 2^-k_w (header float kScaleSlot of chunk 0)
};
__device__ __forceinline__ void fs_request(FsPack& p, const float4* wp, int w, int lane) {
  using R = Ring<8>;
  const float4* body = wp + kChunkHdrFloats / 4 + lane;
#pragma unroll
  for (int c = 0; c < R::NCH; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) p.f[c * 4 + i * 2 + pl] = body[size_t(c) * R::CH4 + ((2 * w + i) * 2 + pl) * 64];
  const float* hdr_last = reinterpret_cast<const float*>(wp + size_t(R::NCH - 1) * R::CH4);
#pragma unroll
  for (int i = 0; i < 2; ++i) p.bias[i] = *reinterpret_cast<const float4*>(hdr_last + 16 * (2 * w + i) + 4 * (lane >> 4));
  p.scale = reinterpret_cast<const float*>(wp)[kScaleSlot];
}

// the four K blocks of the activation entering a Linear, as B operands
struct FsPieces { u32x4 h[4], l[4]; };

// One Linear on the own feature blocks.  ZERO / FIN as in mfma_stage.  `next` / `wnext` (nullable, uniform): the NEXT pack of
// the chain is requested chunk by chunk between this pack's MFMAs -- a lone wave issues a 1 KB global load per ~75 cycles
// (profiles/fs_timeline.py: 1.4k cycles for the 19 loads of a pack, against 430 for its 24 MFMAs), so the matrix
// instructions execute under the load issue instead of after it.
template <bool ZERO, int FIN>
__device__ __forceinline__ void fs_stage(f32x4 (&acc)[2], const FsPack& p, const FsPieces& x, int E, int lane,
                                         FsPack* next = nullptr, const float4* wnext = nullptr, int w = 0) {
  using R = Ring<8>;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const float4* nbody = wnext ? wnext + kChunkHdrFloats / 4 + lane : nullptr;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i] = mma(p.f[c * 4 + i * 2], x.l[c], (ZERO && c == 0) ? zero : acc[i]);
    if (wnext) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) next->f[c * 4 + i * 2 + pl] = nbody[size_t(c) * R::CH4 + ((2 * w + i) * 2 + pl) * 64];
      if (c == 3) {
        const float* hdr_last = reinterpret_cast<const float*>(wnext + size_t(R::NCH - 1) * R::CH4);
#pragma unroll
        for (int i = 0; i < 2; ++i) next->bias[i] = *reinterpret_cast<const float4*>(hdr_last + 16 * (2 * w + i) + 4 * (lane >> 4));
        next->scale = reinterpret_cast<const float*>(wnext)[kScaleSlot];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i] = mma(p.f[c * 4 + i * 2], x.h[c], acc[i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i] = mma(p.f[c * 4 + i * 2 + 1], x.h[c], acc[i]);
  }
  if (FIN != 0) {   // finish_stage on the own blocks: same fast / slow path decision (wave-uniform over the same 16 rows)
    const int fw = int(__float_as_uint(p.scale) >> 23);
    const int f = E + fw - 139;
    if (__builtin_amdgcn_ballot_w64(unsigned(f - 1) >= 254u) == 0) {
      const float inv = __uint_as_float(unsigned(f) << 23);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (FIN == 2) acc[i] = f32x4{fmaf(acc[i][0], inv, p.bias[i].x), fmaf(acc[i][1], inv, p.bias[i].y), fmaf(acc[i][2], inv, p.bias[i].z), fmaf(acc[i][3], inv, p.bias[i].w)};
        else acc[i] *= inv;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float4 b = FIN == 2 ? p.bias[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[i] = f32x4{ldexpf(acc[i][0], f - 127) + b.x, ldexpf(acc[i][1], f - 127) + b.y, ldexpf(acc[i][2], f - 127) + b.z, ldexpf(acc[i][3], f - 127) + b.w};
      }
    }
  }
}

struct FsLds {
  float pmax[16][16];       // [row][4 w + g]: largest |value| of the row among the features held by (wave w, lane group g)
  u32x4 piece[4][2][64];    // [K block][plane][lane]
  float zrow[16][132];      // full rows for the LayerNorm / the narrow output layer (pitch 132: 16-byte aligned, spread over banks)
};

__device__ __forceinline__ float fs_amax2(const f32x4 (&v)[2]) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    m = fmaxf(fmaxf(m, fabsf(v[i][0])), fabsf(v[i][1]));
    m = fmaxf(fmaxf(m, fabsf(v[i][2])), fabsf(v[i][3]));
  }
  return m;
}
// row maximum over all 128 features: every (wave, lane group) publishes its part, everybody reads the 16 parts of its row
__device__ __forceinline__ float fs_row_max(FsLds& L, float mloc, int w, int lane) {
  L.pmax[lane & 15][4 * w + (lane >> 4)] = mloc;
  lds_barrier();
  const float4* p = reinterpret_cast<const float4*>(L.pmax[lane & 15]);
  const float4 a = p[0], b = p[1], c = p[2], d = p[3];
  return fmaxf(fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w))),
               fmaxf(fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)), fmaxf(fmaxf(d.x, d.y), fmaxf(d.z, d.w))));
}
// own K block -> fp16 pieces, published; the other three are read back
__device__ __forceinline__ void fs_publish(FsLds& L, FsPieces& x, const f32x4 (&own)[2], float s, int w, int lane) {
  u32x4 h, l;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    unsigned hh, ll;
    split_h2(own[v >> 1][2 * (v & 1)], own[v >> 1][2 * (v & 1) + 1], s, hh, ll);
    h[v] = hh;
    l[v] = ll;
  }
  L.piece[w][0][lane] = h;
  L.piece[w][1][lane] = l;
  lds_barrier();
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    x.h[kb] = L.piece[kb][0][lane];
    x.l[kb] = L.piece[kb][1][lane];
  }
}
// largest |value| over the tile's rows -> this workgroup's entry of a bound slot (chain.h; wave 0 only: m is per row)
__device__ __forceinline__ void fs_note(float* slot, float m, int w, int lane) {
  if (!slot || w != 0) return;   // uniform
  int v = __float_as_int(m);
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true));
  if (lane == 15) slot[int(blockIdx.x) * 8] = __int_as_float(v);
}
// saved activation (values + ReLU sign bits) of the own feature blocks, act_floats layout (chain.h)
__device__ __forceinline__ void fs_save(float* base, const f32x4 (&own)[2], int64_t R, int64_t row, bool live, int w, int lane, bool bits) {
  if (!base || !live) return;
  constexpr int D = 128;
  const int lg = lane >> 4;
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    __builtin_nontemporal_store(own[i], reinterpret_cast<f32x4*>(base + row * D + 16 * (2 * w + i) + 4 * lg));
#pragma unroll
    for (int r = 0; r < 4; ++r) m |= (__float_as_uint(own[i][r]) != 0u ? 1u : 0u) << (4 * i + r);   // post-ReLU value: positive iff non-zero bits
  }
  if (bits) reinterpret_cast<unsigned char*>(base + pad_rows(R) * D)[(row * 4 + lg) * 4 + w] = (unsigned char)m;   // bits 8w .. 8w+7 of the word of (row, group)
}

template <int IN, int OUT>
__global__ __launch_bounds__(256) void k_fs_fwd(ChainFwdArgs a) {
  constexpr int NB = 8, D = 128;
  __shared__ FsLds L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lg = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * 16 + (lane & 15);
  const bool live = row < a.R;
  const int64_t rowc = live ? row : 0;   // what a lane past the end reads (its results are never stored)
#ifdef BSMS_EXPERIMENTS
  int stamp_i = 0;
  auto stamp = [&]() { if (a.timing && tid == 0 && stamp_i < 16) a.timing[int64_t(blockIdx.x) * 16 + stamp_i++] = __builtin_amdgcn_s_memtime(); };
#else
  auto stamp = [] {};
#endif
  stamp();
  FsPack pa, pb;                         // packs alternate between the two register sets, one Linear ahead
  fs_request(pa, a.wseq[0], w, lane);
  f32x4 own[2], acc[2];
  FsPieces x;
  float m;
  // ---- input stage (own feature blocks 2w, 2w+1 = K block w of the first Linear)
  f32x4 own2[2];
  if (IN == IN_ROWS || IN == IN_ROWS2) {
#pragma unroll
    for (int i = 0; i < 2; ++i) own[i] = *reinterpret_cast<const f32x4*>(a.x + rowc * D + 16 * (2 * w + i) + 4 * lg);
    if (IN == IN_ROWS2) {
#pragma unroll
      for (int i = 0; i < 2; ++i) own2[i] = *reinterpret_cast<const f32x4*>(a.x2 + rowc * D + 16 * (2 * w + i) + 4 * lg);
    }
  } else {  // IN_SMALL: the narrow first layer on the VALU, relu(b0 + sum_k x[k] W0[:, k])
#pragma unroll
    for (int i = 0; i < 2; ++i) own[i] = *reinterpret_cast<const f32x4*>(a.bias_in + 16 * (2 * w + i) + 4 * lg);
    for (int k = 0; k < a.K0; ++k) {
      const float xv = a.x[rowc * a.K0 + k];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float4 wv = *reinterpret_cast<const float4*>(a.w0t + k * D + 16 * (2 * w + i) + 4 * lg);
        own[i][0] = fmaf(xv, wv.x, own[i][0]);
        own[i][1] = fmaf(xv, wv.y, own[i][1]);
        own[i][2] = fmaf(xv, wv.z, own[i][2]);
        own[i][3] = fmaf(xv, wv.w, own[i][3]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) own[i][r] = __int_as_float(max(__float_as_int(own[i][r]), 0));
    fs_save(a.store_in, own, a.R, row, live, w, lane, !(a.store_mode & 4));
    if (a.nstage == 0) return;
  }
  float mloc = fs_amax2(own);
  if (IN == IN_ROWS2) mloc = fmaxf(mloc, fs_amax2(own2));
  stamp();   // loads issued
  m = fs_row_max(L, mloc, w, lane);
  stamp();   // input rows arrived, row maximum exchanged
  fs_note(a.amax[0], m, w, lane);
  RowScale rs = scale_of(m);
  fs_publish(L, x, own, rs.s, w, lane);
  stamp();   // pieces exchanged

  // ---- Linears.  `q` walks the pack sequence (a.wseq: IN_ROWS2 has two packs for its first Linear, OUT_PLAIN2 one per head)
  auto run = [&](FsPack& cur, FsPack& nxt, int q, int l) -> bool {   // returns false when the chain is finished
    const float4* wn = q + 1 < a.nseq ? a.wseq[q + 1] : nullptr;     // the next pack is requested between this pack's MFMAs
    if (OUT == OUT_PLAIN2) {   // two Linears of the SAME rows: stage q -> y (q = 0) / y2 (q = 1)
      fs_stage<true, 2>(acc, cur, x, rs.E, lane, &nxt, wn, w);
      float* y = q == 0 ? a.y : a.y2;
      if (live)
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(y + row * D + 16 * (2 * w + i) + 4 * lg) = acc[i];
      return q + 1 < a.nseq;
    }
    if (IN == IN_ROWS2 && q == 0) {   // first half of the Linear over [x, x2]: raw sums, continued by the second pack
      fs_stage<true, 0>(acc, cur, x, rs.E, lane, &nxt, wn, w);
      stamp();
      lds_barrier();                  // everybody has read the pieces of x
      fs_publish(L, x, own2, rs.s, w, lane);
      stamp();
      return true;
    }
    if (IN == IN_ROWS2 && q == 1) fs_stage<false, 2>(acc, cur, x, rs.E, lane, &nxt, wn, w);
    else fs_stage<true, 2>(acc, cur, x, rs.E, lane, &nxt, wn, w);
    stamp();   // MFMAs of the pack issued (the wave has its weights)
    const bool last = l == a.nstage - 1;
    if (!last || OUT == OUT_SMALL) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) own[i][r] = __int_as_float(max(__float_as_int(acc[i][r]), 0));
    }
    if (last) return false;
    fs_save(a.store[l], own, a.R, row, live, w, lane, !(a.store_mode & 4));
    lds_barrier();                    // the pieces of the previous activation have been read by everybody
    m = fs_row_max(L, fs_amax2(own), w, lane);
    fs_note(a.amax[l + 1], m, w, lane);
    rs = scale_of(m);
    fs_publish(L, x, own, rs.s, w, lane);
    stamp();   // next activation exchanged
    return true;
  };
  {
    int q = 0, l = 0;
    for (;;) {
      if (!run(pa, pb, q, l)) break;
      if (!(IN == IN_ROWS2 && q == 0) && OUT != OUT_PLAIN2) ++l;
      ++q;
      if (!run(pb, pa, q, l)) break;
      if (!(IN == IN_ROWS2 && q == 0) && OUT != OUT_PLAIN2) ++l;
      ++q;
    }
  }
  if (OUT == OUT_PLAIN2) return;

  // ---- output
  if (OUT == OUT_PLAIN) {
    if (!live) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4* p = reinterpret_cast<f32x4*>(a.y + row * D + 16 * (2 * w + i) + 4 * lg);
      f32x4 v = acc[i];
      if (a.accumulate) v += *p;
      *p = v;
    }
    return;
  }
  // OUT_LN / OUT_SMALL work on FULL rows: gather them through LDS in the chain layout, then exactly the arithmetic of k_chain_fwd
  lds_barrier();
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&L.zrow[lane & 15][16 * (2 * w + i) + 4 * lg]) = (OUT == OUT_SMALL) ? own[i] : acc[i];
  if (OUT == OUT_SMALL && a.store[a.nstage - 1] && live) {   // last hidden activation (plain rows, no sign bits: the backward masks by value)
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(a.store[a.nstage - 1] + row * D + 16 * (2 * w + i) + 4 * lg) = own[i];
  }
  lds_barrier();
  f32x4 z[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) z[t] = *reinterpret_cast<const f32x4*>(&L.zrow[lane & 15][16 * t + 4 * lg]);
  if (!live) return;
  if (OUT == OUT_LN) {  // LayerNorm(elementwise_affine=False), eps 1e-5  (ops/basic.py:18): every wave normalises the row, stores its quarter
    const float mean = row_sum<NB>(z) * (1.f / D);
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        z[t][r] -= mean;
        ss = fmaf(z[t][r], z[t][r], ss);
      }
    ss = group_sum(ss);
    const float rstd = 1.f / sqrtf(ss * (1.f / D) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = 2 * w + i;
      f32x4 v = z[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= rstd;
      const int64_t o = row * D + 16 * t + 4 * lg;
      if (a.yln) *reinterpret_cast<f32x4*>(a.yln + o) = v;
      if (a.resid) v += *reinterpret_cast<const f32x4*>(a.resid + o);
      if (a.resid2) v += *reinterpret_cast<const f32x4*>(a.resid2 + o);   // (LN + x) + skip, in this order
      *reinterpret_cast<f32x4*>(a.y + o) = v;
    }
    if (a.rstd && w == 0 && lg == 0) a.rstd[row] = rstd;
  } else {  // OUT_SMALL: the narrow last Linear (decoder, models/model.py:22) on the VALU; output channel c belongs to wave c % 4
    for (int c = w; c < a.C; c += 4) {
      const float v = dot_features<NB>(z, a.wout + c * D, lg);
      if (lg == 0) a.y[row * a.C + c] = v + a.bout[c];
    }
  }
}

// ------------------------------------------------------------------------------- backward chain
template <int NB>
__device__ __forceinline__ void mask_by(f32x4 (&gr)[NB], const float* act_row, int lg) {
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    const float4 m = *reinterpret_cast<const float4*>(act_row + 16 * t + 4 * lg);
    gr[t][0] = m.x > 0.f ? gr[t][0] : 0.f;
    gr[t][1] = m.y > 0.f ? gr[t][1] : 0.f;
    gr[t][2] = m.z > 0.f ? gr[t][2] : 0.f;
    gr[t][3] = m.w > 0.f ? gr[t][3] : 0.f;
  }
}

template <int NB, int GIN, int FIRST, bool BF = false, bool LONE = false>
__global__ __launch_bounds__(kChainMaxThreads) __attribute__((amdgpu_waves_per_eu(chain_wpe<NB, LONE>()))) void k_chain_bwd(ChainBwdArgs a) {
  constexpr int D = NB * 16;
  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
  const int cw = int(blockDim.x >> 6) - a.nload;   // compute waves of this launch (4..7, chosen by the launcher); the last wave(s) load
  if (wave >= cw) {  // loader wave (uniform branch)
    loader_dispatch<NB, BF ? 1 : kPL>(a.nload, wave - cw, a.wseq, a.nseq, lds, lane, a.ntiles, a.nring);
    return;
  }
  Slot slot{0, a.nring};  // ring slot of the next chunk, across this workgroup's tiles
  float4* const ring = lds + Ring<NB>::PRE4;
  unsigned* brow = bound_row<NB>(lds, wave, lane, any_slot(a.gmax));   // this wave's running magnitude bounds
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {  // persistent workgroups (see k_chain_fwd)
  const int64_t row = int64_t(tile) * (16 * cw) + wave * 16 + (lane & 15);
  const bool live = row < a.R;
  const int64_t rowc = live ? row : 0;   // what a lane past the end reads (its results are never stored)
  const int64_t roff = live ? row * D : -1;  // row offset for stores; negative = no store

  f32x4 g[NB], acc[NB];
  if (GIN == G_SMALL) {  // g = (dy . W_out) masked by the last hidden activation
    zero_tile<NB>(g);
    for (int c = 0; c < a.C; ++c) axpy_features<NB>(g, a.wout + c * D, a.dy[rowc * a.C + c], lg);
    mask_by<NB>(g, a.mask_in + rowc * D, lg);
  } else {
    const float* dyrow;
    if (GIN == G_EDGE_LN) {  // autograd of scatter_sum: gather the node gradient by target
      const int b = int(rowc / a.E), q = int(rowc - int64_t(b) * a.E);
      dyrow = a.dy + (int64_t(b) * a.N + a.dst[q]) * D;
    } else {
      dyrow = a.dy + rowc * D;
    }
    load_rows<NB>(g, dyrow, lg);
    if constexpr (BF && GIN == G_EDGE_LN) load_rows_bf16<NB>(acc, a.yln, rowc, lg);   // the bf16 messages the forward handed to the aggregation
    else load_rows<NB>(acc, a.yln + rowc * D, lg);  // acc = normalised output y
    const float rs = a.rstd[rowc];
    __builtin_amdgcn_sched_barrier(0);         // all 17 loads in flight before the first use (see k_chain_fwd)
    // LayerNorm backward (no affine): dz = rstd * (dy - mean(dy) - y * mean(dy * y))
    const float m1 = row_sum<NB>(g) * (1.f / D);
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) s2 = fmaf(g[t][r], acc[t][r], s2);
    s2 = group_sum(s2);
    const float m2 = s2 * (1.f / D);
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) g[t][r] = rs * (g[t][r] - m1 - acc[t][r] * m2);
  }
  // The gradient entering a stage is stored to HBM from inside that stage (mfma_stage), so the store has a whole
  // stage to drain before the next vmcnt wait (the ReLU-mask rows at the end of the stage).
  float* pending = a.gstore[0];   // uniform

  for (int k = 0; k < a.nstage; ++k) {
    // ReLU sign bits of the activation that masks this stage's output: one small load, issued before the stage
    unsigned mbits[mask_words<NB>()];
#pragma unroll
    for (int w = 0; w < mask_words<NB>(); ++w)
      mbits[w] = a.mask[k] ? reinterpret_cast<const unsigned*>(a.mask[k] + (BF ? pad_rows(a.R) * D / 2 : pad_rows(a.R) * D))[rowc * (4 * mask_words<NB>()) + lg * mask_words<NB>() + w]
                           : 0xffffffffu;
    if constexpr (BF) {
      zero_tile<NB>(acc);
      mfma_stage_bf<NB>(acc, g, ring, slot, lane, false, pending, roff, 0);
    } else {
      const float m = row_amax<NB>(g);
      note_amax(brow, k, m, lane);
      mfma_stage<NB, true, 1, LONE>(acc, g, scale_of(m), ring, slot, lane, pending, roff, a.store_mode & 3, 0, nullptr, row,
                              (a.store_mode & 8) ? 0 : a.R);
    }
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // bit -> all-ones / zero mask (one v_bfe_i32), then one and
        const int keep = __builtin_amdgcn_sbfe((int)mbits[(4 * t + r) >> 5], (4 * t + r) & 31, 1);
        g[t][r] = __uint_as_float(__float_as_uint(acc[t][r]) & (unsigned)keep);
      }
    pending = a.gstore[k + 1];
  }

  if constexpr (FIRST != F_NONE && BF) {   // BSMS_BF16_NODES: gN[0] stays fp32 (its weight-gradient job multiplies the fp32 rows x / aggr)
    note_amax(brow, a.nstage, row_amax<NB>(g), lane);
    store_rows<NB, false>(g, pending, roff, lg);
    pending = nullptr;
    zero_tile<NB>(acc);
    mfma_stage_bf<NB>(acc, g, ring, slot, lane, false, nullptr, roff, 0);
    if (a.dres) {
      f32x4 r[NB];
      load_rows<NB>(r, a.dres + rowc * D, lg);
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[t] += r[t];
    }
    store_rows<NB, false>(acc, a.dx, roff, lg);
    if (FIRST == F_HEADS2) {
      zero_tile<NB>(acc);
      mfma_stage_bf<NB>(acc, g, ring, slot, lane, false, nullptr, roff, 0);
      store_rows<NB, false>(acc, a.dx2, roff, lg);
    }
  } else if (FIRST != F_NONE) {
    const float mh = row_amax<NB>(g);
    note_amax(brow, a.nstage, mh, lane);
    const RowScale rs = scale_of(mh);
    mfma_stage<NB, true, 1, LONE>(acc, g, rs, ring, slot, lane, pending, roff, 1, 0, nullptr, row, a.R);
    pending = nullptr;
    if (a.dres) {
      f32x4 r[NB];
      load_rows<NB>(r, a.dres + rowc * D, lg);
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[t] += r[t];
    }
    if (FIRST == F_HEADS2) {
      f32x4 acc2[NB];
      mfma_stage<NB, true, 1, LONE>(acc2, g, rs, ring, slot, lane);
      store_rows<NB, false>(acc, a.dx, roff, lg);
      store_rows<NB, false>(acc2, a.dx2, roff, lg);
    } else {
      store_rows<NB, false>(acc, a.dx, roff, lg);
    }
  }
  if (FIRST == F_NONE && a.gmax[a.nstage]) note_amax(brow, a.nstage, row_amax<NB>(g), lane);   // uniform
  if constexpr (BF) store_rows_bf16<NB>(g, pending, roff, lg);
  else store_rows<NB, false>(g, pending, roff, lg);
  }  // tile loop
  flush_bounds(a.gmax, kMaxStages + 1, brow, wave, lane);
}

// ------------------------------------------------------------------ small launches: feature-split backward chain ----
// k_chain_bwd with the features of a 16-row tile split over four waves (see k_fs_fwd).  The LayerNorm backward needs sums
// over the whole row in the association of k_chain_bwd (row_sum, then the sequential fmaf chain): every wave reads the full
// dy / y rows (L2-resident at these sizes) and repeats that arithmetic, then keeps its own feature blocks.  Bit-identical
// to k_chain_bwd.
template <int GIN, int FIRST>
__global__ __launch_bounds__(256) void k_fs_bwd(ChainBwdArgs a) {
  constexpr int NB = 8, D = 128;
  __shared__ FsLds L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lg = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * 16 + (lane & 15);
  const bool live = row < a.R;
  const int64_t rowc = live ? row : 0;
  FsPack pa, pb;
  fs_request(pa, a.wseq[0], w, lane);
  f32x4 own[2], acc[2];
  if (GIN == G_SMALL) {  // g = (dy . W_out) masked by the last hidden activation
#pragma unroll
    for (int i = 0; i < 2; ++i) own[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.C; ++c) {
      const float dv = a.dy[rowc * a.C + c];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float4 wv = *reinterpret_cast<const float4*>(a.wout + c * D + 16 * (2 * w + i) + 4 * lg);
        own[i][0] = fmaf(dv, wv.x, own[i][0]);
        own[i][1] = fmaf(dv, wv.y, own[i][1]);
        own[i][2] = fmaf(dv, wv.z, own[i][2]);
        own[i][3] = fmaf(dv, wv.w, own[i][3]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 mv = *reinterpret_cast<const float4*>(a.mask_in + rowc * D + 16 * (2 * w + i) + 4 * lg);
      own[i][0] = mv.x > 0.f ? own[i][0] : 0.f;
      own[i][1] = mv.y > 0.f ? own[i][1] : 0.f;
      own[i][2] = mv.z > 0.f ? own[i][2] : 0.f;
      own[i][3] = mv.w > 0.f ? own[i][3] : 0.f;
    }
  } else {  // G_ROWS_LN: LayerNorm backward (no affine): dz = rstd * (dy - mean(dy) - y * mean(dy * y)) on the FULL row
    f32x4 gf[NB], yf[NB];
    load_rows<NB>(gf, a.dy + rowc * D, lg);
    load_rows<NB>(yf, a.yln + rowc * D, lg);
    const float rs = a.rstd[rowc];
    const float m1 = row_sum<NB>(gf) * (1.f / D);
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) s2 = fmaf(gf[t][r], yf[t][r], s2);
    s2 = group_sum(s2);
    const float m2 = s2 * (1.f / D);
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) gf[t][r] = rs * (gf[t][r] - m1 - yf[t][r] * m2);
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // own feature blocks 2w, 2w+1 (w is wave-uniform: a select over the register tile)
      own[i] = gf[i];
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (w == q) own[i] = gf[2 * q + i];
    }
  }
  auto store_own = [&](float* base, const f32x4 (&v)[2]) {   // a layer gradient: rows [R, D] fp32, own quarter
    if (!base || !live) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4*>(base + row * D + 16 * (2 * w + i) + 4 * lg));
  };
  FsPieces x;
  RowScale rs{};
  auto enter = [&](int k) {   // the gradient entering pack k: store, bound, row scale, pieces
    store_own(a.gstore[k], own);
    if (k > 0) lds_barrier();   // the pieces of the previous gradient have been read by everybody
    const float m = fs_row_max(L, fs_amax2(own), w, lane);
    fs_note(a.gmax[k], m, w, lane);
    rs = scale_of(m);
    fs_publish(L, x, own, rs.s, w, lane);
  };
  auto stage = [&](FsPack& cur, FsPack& nxt, int q, int k) {   // dgrad through layer k, masked by the ReLU sign bits of its input activation
    unsigned mb = 0xffu;
    if (a.mask[k]) mb = reinterpret_cast<const unsigned char*>(a.mask[k] + pad_rows(a.R) * D)[(rowc * 4 + lg) * 4 + w];
    fs_stage<true, 1>(acc, cur, x, rs.E, lane, &nxt, q + 1 < a.nseq ? a.wseq[q + 1] : nullptr, w);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int keep = __builtin_amdgcn_sbfe((int)mb, 4 * i + r, 1);
        own[i][r] = __uint_as_float(__float_as_uint(acc[i][r]) & (unsigned)keep);
      }
  };
  // the two pack register sets alternate with STATIC roles (a run-time choice between them would put both in scratch)
  auto finish = [&](FsPack& cur, FsPack& nxt, int q) {
    if (FIRST == F_NONE) {
      if (a.gmax[a.nstage]) {   // uniform
        lds_barrier();
        fs_note(a.gmax[a.nstage], fs_row_max(L, fs_amax2(own), w, lane), w, lane);
      }
      store_own(a.gstore[a.nstage], own);
      return;
    }
    enter(a.nstage);
    fs_stage<true, 1>(acc, cur, x, rs.E, lane, &nxt, q + 1 < a.nseq ? a.wseq[q + 1] : nullptr, w);
    if (a.dres && live) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] += *reinterpret_cast<const f32x4*>(a.dres + row * D + 16 * (2 * w + i) + 4 * lg);
    }
    if (live)
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(a.dx + row * D + 16 * (2 * w + i) + 4 * lg) = acc[i];
    if (FIRST == F_HEADS2) {
      fs_stage<true, 1>(acc, nxt, x, rs.E, lane);
      if (live)
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(a.dx2 + row * D + 16 * (2 * w + i) + 4 * lg) = acc[i];
    }
  };
  for (int k = 0;;) {
    if (k == a.nstage) { finish(pa, pb, k); break; }
    enter(k);
    stage(pa, pb, k, k);
    ++k;
    if (k == a.nstage) { finish(pb, pa, k); break; }
    enter(k);
    stage(pb, pa, k, k);
    ++k;
  }
}

}  // namespace
