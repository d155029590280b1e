// The software-pipelined edge MLP chains, k_edge_fwd / k_edge_bwd (NB = 8 / 16, fp32).  Same rules as chain_kernels.h.
#pragma once
#include "chain_dev.h"

namespace {

// store_pair_stream for the pipelined edge kernels: the tensor is non-null and padded (no tests), and the per-lane
// part of both addresses is a 32-bit byte offset WITHIN THE TILE, computed once per kernel (the tile's base is uniform
// 64-bit scalar arithmetic), so a pair costs its DPP exchange and two stores with SGPR base + VGPR offset + immediate.
struct PairOff { unsigned a, b; };
template <int NB>
__device__ __forceinline__ PairOff pair_offsets(int64_t row, int lane) {
  constexpr int D = NB * 16;
  const bool hi = (lane & 8) != 0;
  const int64_t rowA = row - (lane & 8);
  return PairOff{unsigned((rowA * D + 4 * (lane >> 4) + (hi ? 16 : 0)) * 4), unsigned(((rowA + 8) * D + 4 * (lane >> 4) + (hi ? 0 : 16)) * 4)};
}
template <int NB>
__device__ __forceinline__ void store_pair_nt(const f32x4 (&v)[NB], float* base, PairOff off, int lane, int t) {
  using i32x4 = __attribute__((ext_vector_type(4))) int;
  const bool hi = (lane & 8) != 0;
  const i32x4 own = __builtin_bit_cast(i32x4, v[t + 1]);
  i32x4 got;
#pragma unroll
  for (int r = 0; r < 4; ++r) got[r] = __builtin_amdgcn_update_dpp(own[r], own[r], 0x128, 0xf, 0xf, false);
  const f32x4 x = __builtin_bit_cast(f32x4, got);
  const f32x4 dA = hi ? x : v[t], dB = hi ? v[t] : x;
  char* b = reinterpret_cast<char*>(base) + 64 * t;   // uniform
  __builtin_nontemporal_store(dA, reinterpret_cast<f32x4*>(b + off.a));
  __builtin_nontemporal_store(dB, reinterpret_cast<f32x4*>(b + off.b));
}

// ------------------------------------------------------------- edge MLP chains, software-pipelined ----
// The edge MLP (IN_EDGE / OUT_LN forward, G_EDGE_LN / F_NONE backward) is ~45 % of the training step.  In k_chain_fwd /
// k_chain_bwd every A-fragment pair is read from LDS right before its MFMAs (the 128-VGPR budget of two workgroups
// per CU leaves no room to prefetch), so an in-order wave exposes one LDS round trip per pair.
// Here a wave owns RB row blocks of 16 rows: ONE fragment pair feeds 2 RB x {2, 1} MFMAs, the next pair is in
// flight while they run, 2 RB independent accumulator chains interleave (no dependent back-to-back MFMAs), and the
// workgroup barrier + bias reads are paid once per RB x 64 rows.  RB = 2 at D = 128 (one workgroup per CU, 256-VGPR
// budget), RB = 1 at D = 256 (the 32 + 32 blocks of one row block already fill the budget).
// The arithmetic (order of the three partial products per accumulator, chain.h) is exactly mfma_stage's: bit-identical.
// The VALU work of a stage, cut into STEPS of 2-4 operations that are placed by hand between the MFMA pairs of the
// chunk before the one that needs them (sched_barrier fences keep hipcc from regrouping them: left alone it emits the
// split of a K block as one lump during which the matrix pipe drains, and its IGroupLP pipelines (sched_group_barrier)
// either explode in compile time or silently skip some regions).  Per row block:
//   P0..P3  streaming store of feature blocks 2c, 2c + 1 of the activation: DPP exchange (2 steps), select + store (2)
//   S0..S7  fp16 pieces of K block c + 1: per dword (two features) {h}, {l}  (two v_fma_mix each)
//   M0..M7  (last chunk of a saved activation instead of S) ReLU sign bits, then the store of the words
struct Pieces { unsigned h[4], l[4]; };
__device__ __forceinline__ u32x4 vec4(const unsigned (&d)[4]) { return u32x4{d[0], d[1], d[2], d[3]}; }
struct StepState { int got[4]; };

// SAVE: 0 nothing is stored; 1 the activation as fp32 rows (128-byte streaming pairs) + sign bits.
template <int NB, int RB, int SAVE, bool MASK>
__device__ __forceinline__ void valu_step(int s, int c, const f32x4 (&act)[RB][NB], Pieces (&pc)[RB][2], StepState (&st)[RB],
                                          const RowScale (&rs)[RB], unsigned (&mword)[RB][mask_words<NB>()], float* store_base,
                                          unsigned* bits_base, const PairOff (&off)[RB], const unsigned (&moff)[RB], int lane) {
  constexpr int W = mask_words<NB>(), NP = SAVE ? 4 : 0, PER = NP + 8;
  const int rb = s / PER, q = s % PER;
  if (rb >= RB) return;
  const bool last = c + 1 == Ring<NB>::NCH;
  if (q < NP) {   // ---- P steps
    const f32x4& own = act[rb][2 * c + 1];
    const bool hi = (lane & 8) != 0;
    if (q < 2) {
#pragma unroll
      for (int r = 2 * q; r < 2 * q + 2; ++r) {
        const int x = __float_as_int(own[r]);
        st[rb].got[r] = __builtin_amdgcn_update_dpp(x, x, 0x128, 0xf, 0xf, false);   // row_ror:8: partner's block 2c + 1
      }
    } else {
      const f32x4& mine = act[rb][2 * c];
      f32x4 d;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float g = __int_as_float(st[rb].got[r]);
        d[r] = (q == 2) ? (hi ? g : mine[r]) : (hi ? mine[r] : g);
      }
      char* b = reinterpret_cast<char*>(store_base) + 128 * c;   // uniform; feature blocks 2c, 2c + 1
      __builtin_nontemporal_store(d, reinterpret_cast<f32x4*>(b + (q == 2 ? off[rb].a : off[rb].b)));
    }
    return;
  }
  const int ss = q - NP;
  if (!last) {    // ---- S steps: K block c + 1 -> pc[rb][(c + 1) & 1]
    const int v = ss >> 1, kb2 = c + 1;
    Pieces& o = pc[rb][kb2 & 1];
    const float x0 = act[rb][2 * kb2 + (v >> 1)][2 * (v & 1)], x1 = act[rb][2 * kb2 + (v >> 1)][2 * (v & 1) + 1];
    if ((ss & 1) == 0) {
      asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(o.h[v]) : "v"(x0), "v"(rs[rb].s));
      asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(o.h[v]) : "v"(x1), "v"(rs[rb].s));
    } else {
      asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(o.l[v]) : "v"(x0), "v"(rs[rb].s), "v"(o.h[v]));
      asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(o.l[v]) : "v"(x1), "v"(rs[rb].s), "v"(o.h[v]));
    }
  } else if (SAVE && MASK) {   // ---- M steps: highest element first, one shift-and-append per element (store_mask_bits)
    constexpr int EPS = (4 * NB + 7) / 8;
#pragma unroll
    for (int i = ss * EPS; i < (ss + 1) * EPS && i < 4 * NB; ++i) {
      const int e = 4 * NB - 1 - i;
      mword[rb][e >> 5] = __builtin_amdgcn_alignbit(mword[rb][e >> 5], 0u - __float_as_uint(act[rb][e >> 2][e & 3]), 31);
    }
    if (ss == 7) {
      unsigned* bits = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(bits_base) + moff[rb]);
#pragma unroll
      for (int w = 0; w < W; ++w) bits[w] = mword[rb][w];   // rows past R land in the padding (chain.h: act_floats)
    }
  }
}

// ZERO / FIN as in mfma_stage: ZERO = the accumulators start from zero (else they continue the raw sums of the previous
// call: same row scales, pack of the same weight scale); FIN = 0 leave raw sums, 1 un-scale, 2 un-scale + bias.
// `rs_ext` (nullable): row scales decided by the caller (a Linear over two concatenated sources); else the row maxima of
// `act` are taken here and noted in the running bounds (`brow`, stage index `stage`).
template <int NB, int RB, int SAVE, bool MASK, bool ZERO, int FIN, bool LONE = false>
__device__ __forceinline__ void stage_rb(f32x4 (&acc)[RB][NB], const f32x4 (&act)[RB][NB], float4* lds, Slot& slot, int lane,
                                         float* store_base, unsigned* bits_base, const PairOff (&off)[RB], const unsigned (&moff)[RB],
                                         unsigned* brow, int stage, const RowScale* rs_ext = nullptr,
                                         unsigned long long* waited = nullptr) {   // experiments: cycles at the chunk barriers
  using Rg = Ring<NB>;
  constexpr int W = mask_words<NB>();
  constexpr int NSLOT = (NB / 2) * 3 * RB;            // MFMA pairs per chunk
  constexpr int NSTEP = RB * ((SAVE ? 4 : 0) + 8);    // VALU steps per chunk
  static_assert(NSTEP <= NSLOT, "at most one step per MFMA pair");
  Pieces pc[RB][2];                                   // pieces of K blocks c (slot c & 1) and c + 1
  StepState st[RB];
  RowScale rs[RB];
  unsigned mword[RB][W];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    if (rs_ext) {
      rs[rb] = rs_ext[rb];
    } else {
      const float m = row_amax<NB>(act[rb]);
      note_amax(brow, stage, m, lane);
      rs[rb] = scale_of(m);
    }
    u32x4 h, l;
    split_block<NB>(act[rb], 0, rs[rb].s, h, l);
#pragma unroll
    for (int v = 0; v < 4; ++v) { pc[rb][0].h[v] = h[v]; pc[rb][0].l[v] = l[v]; }
#pragma unroll
    for (int w = 0; w < W; ++w) mword[rb][w] = 0;
  }
  int fw = 0;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if constexpr (LONE) {
    // ---- single-round launches (one workgroup per CU, one or two waves per SIMD, 256-register budget): nothing hides the
    // chunk barrier and the LDS round trip of a chunk's first fragments (~350 of ~900 cycles per chunk, profiles/census/
    // stage_lone.hip).  As in mfma_stage<LONE>: the wave passes the barrier of chunk c + 1 and requests its first fragments
    // at the START of chunk c's last block pair -- whose own fragments (plane l) were requested one pair early -- so the
    // round trip runs under six MFMAs per row block.  One barrier per chunk, in the same order; after barrier c + 1 this
    // wave has nothing left to read of chunk c (lds_barrier waits for its LDS reads), so the loader may overwrite it.
    static_assert(NB >= 4, "the early barrier needs two block pairs per chunk");
    const float4* cur = nullptr;
    const float4* body = nullptr;
    float4 f0, f1;
#pragma unroll
    for (int c = 0; c < Rg::NCH; ++c) {
      if (c == 0) {
        lds_barrier();
        cur = lds + slot.i * Rg::CH4;
        if (++slot.i == slot.nr) slot.i = 0;
        body = cur + kChunkHdrFloats / 4 + lane;
        f0 = body[0]; f1 = body[2 * 64];
        fw = int(__float_as_uint(reinterpret_cast<const float*>(cur)[kScaleSlot]) >> 23);
      }
      const int cb = c & 1;
      int islot = 0;
      auto pair = [&](int t, int rb, const float4& a0, const float4& a1, const unsigned (&piece)[4], bool first) {
        acc[rb][t] = mma(a0, vec4(piece), (ZERO && first && c == 0) ? zero : acc[rb][t]);
        acc[rb][t + 1] = mma(a1, vec4(piece), (ZERO && first && c == 0) ? zero : acc[rb][t + 1]);
        const int s = (islot * NSTEP + NSLOT - 1) / NSLOT;
        if (s < NSTEP && s * NSLOT / NSTEP == islot)
          valu_step<NB, RB, SAVE, MASK>(s, c, act, pc, st, rs, mword, store_base, bits_base, off, moff, lane);
        ++islot;
        __builtin_amdgcn_sched_barrier(0);
      };
      __builtin_amdgcn_sched_barrier(0);
      float4 m0 = f0, m1 = f1;   // plane l of the LAST block pair, requested one pair early
      float4 g0 = f0, g1 = f1;   // first fragments of the NEXT chunk
      const float4* ncur = cur;
      const float4* nbody = body;
#pragma unroll
      for (int t = 0; t < NB; t += 2) {
        float4 n0, n1;
        if (t == NB - 2) {
          n0 = m0; n1 = m1;
          if (c + 1 < Rg::NCH) {   // every read of this chunk has been issued: barrier of the next one, its first fragments
            lds_barrier();
            ncur = lds + slot.i * Rg::CH4;
            if (++slot.i == slot.nr) slot.i = 0;
            nbody = ncur + kChunkHdrFloats / 4 + lane;
            g0 = nbody[0]; g1 = nbody[2 * 64];
          }
        } else {
          n0 = body[(t * 2 + 1) * 64]; n1 = body[(t * 2 + 3) * 64];
          if (t == NB - 4) { m0 = body[((NB - 2) * 2 + 1) * 64]; m1 = body[((NB - 2) * 2 + 3) * 64]; }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].l, true);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].h, false);
        f0 = n0;
        f1 = n1;
        if (t + 2 < NB) {
          n0 = body[((t + 2) * 2) * 64];
          n1 = body[((t + 2) * 2 + 2) * 64];
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].h, false);
        f0 = n0;
        f1 = n1;
      }
      if (FIN != 0 && c == Rg::NCH - 1) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) finish_stage<NB, FIN == 2>(acc[rb], rs[rb].E, fw, reinterpret_cast<const float*>(cur), lane);
      }
      cur = ncur; body = nbody; f0 = g0; f1 = g1;
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < Rg::NCH; ++c) {
#ifdef BSMS_EXPERIMENTS
    if (waited) {
      const unsigned long long t0 = __builtin_amdgcn_s_memtime();
      lds_barrier();
      *waited += __builtin_amdgcn_s_memtime() - t0;
    } else
#endif
    lds_barrier();                                         // chunk has landed (and my reads of the last one are done)
    const float4* cur = lds + slot.i * Rg::CH4;
    if (++slot.i == slot.nr) slot.i = 0;
    const float4* body = cur + kChunkHdrFloats / 4 + lane;
    float4 f0 = body[0], f1 = body[2 * 64];                // pair (t = 0, plane h)
    if (c == 0) fw = int(__float_as_uint(reinterpret_cast<const float*>(cur)[kScaleSlot]) >> 23);
    const int cb = c & 1;
    int islot = 0;   // MFMA pair within the chunk
    // one MFMA pair (feature blocks t, t + 1 of row block rb, one plane combination), then the VALU step that rides with it
    auto pair = [&](int t, int rb, const float4& a0, const float4& a1, const unsigned (&piece)[4], bool first) {
      acc[rb][t] = mma(a0, vec4(piece), (ZERO && first && c == 0) ? zero : acc[rb][t]);
      acc[rb][t + 1] = mma(a1, vec4(piece), (ZERO && first && c == 0) ? zero : acc[rb][t + 1]);
      const int s = (islot * NSTEP + NSLOT - 1) / NSLOT;          // the step whose place is this pair, if any
      if (s < NSTEP && s * NSLOT / NSTEP == islot)
        valu_step<NB, RB, SAVE, MASK>(s, c, act, pc, st, rs, mword, store_base, bits_base, off, moff, lane);
      ++islot;
      __builtin_amdgcn_sched_barrier(0);
    };
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NB; t += 2) {
      float4 n0 = body[(t * 2 + 1) * 64], n1 = body[(t * 2 + 3) * 64];          // plane l of (t, t + 1): one pair ahead
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].l, true);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].h, false);
      f0 = n0;
      f1 = n1;
      if (t + 2 < NB) {                                                           // plane h of the next block pair
        n0 = body[((t + 2) * 2) * 64];
        n1 = body[((t + 2) * 2 + 2) * 64];
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) pair(t, rb, f0, f1, pc[rb][cb].h, false);
      f0 = n0;
      f1 = n1;
    }
    if (FIN != 0 && c == Rg::NCH - 1) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) finish_stage<NB, FIN == 2>(acc[rb], rs[rb].E, fw, reinterpret_cast<const float*>(cur), lane);
    }
  }
}

template <int NB, int RB>
struct EdgeTile {
  static constexpr int rows = kTileRows * RB;
  static constexpr int waves_per_eu = (NB * RB <= 8) ? 4 : 2;   // VGPR budget 128 / 256
  static constexpr int resident = (NB * RB <= 8) ? 2 : 1;       // workgroups per CU (see resident_per_cu)
};

// LONE: the instantiation for launches of at most one workgroup per CU (stage_rb<.., LONE>; 256-register budget)
template <int NB, int RB, int SAVE, bool LONE = false>
__global__ __launch_bounds__(kChainMaxThreads) __attribute__((amdgpu_waves_per_eu(LONE ? 2 : EdgeTile<NB, RB>::waves_per_eu)))
void k_edge_fwd(ChainFwdArgs a) {
  constexpr int D = NB * 16;
  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
  const int cw = int(blockDim.x >> 6) - a.nload, tile_rows = 16 * RB * cw;   // compute waves of this launch (launcher's choice); the last wave(s) load
  if (wave >= cw) {  // loader wave (uniform branch)
    loader_dispatch<NB>(a.nload, wave - cw, a.wseq, a.nseq, lds, lane, a.ntiles, a.nring, a.w0t);
    return;
  }
  const float rcpE = 1.f / float(a.E);
  // plan-order endpoints of this lane's rows in a tile; fetched one tile ahead (two registers per row block), so a tile
  // starts with its row gathers instead of a dependent index round trip
  auto fetch_endpoints = [&](int tile, int (&i)[RB], int (&j)[RB], int (&b)[RB]) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int64_t r = int64_t(tile) * tile_rows + wave * (16 * RB) + rb * 16 + (lane & 15);
      const EdgeRef e = edge_ref(unsigned(r < a.R ? r : 0), unsigned(a.E), rcpE);   // a lane past the end reads row 0
      i[rb] = a.src[e.q];
      j[rb] = a.dst[e.q];
      b[rb] = e.b;
    }
  };
  int ni[RB], nj[RB], nbat[RB];
  fetch_endpoints(blockIdx.x, ni, nj, nbat);
  lds_barrier();
  const float* w0t = reinterpret_cast<const float*>(lds);   // fiber weights (LDS side table, see k_chain_fwd)
  Slot slot{0, a.nring};
  float4* const ring = lds + Ring<NB>::PRE4;
  unsigned* brow = bound_row<NB>(lds, wave, lane, any_slot(a.amax));   // this wave's running magnitude bounds
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int64_t row[RB];
    PairOff off[RB];
    unsigned moff[RB];   // byte offset of this lane's sign-bit words
    f32x4 act[RB][NB], acc[RB][NB];
    float pi[RB][7], pj[RB][7];
#ifdef BSMS_EXPERIMENTS
    int stamp_i = 0;
    unsigned long long waited = 0;
    auto stamp = [&]() { if (a.timing && tid == 0 && stamp_i < 16) a.timing[int64_t(tile) * 16 + stamp_i++] = __builtin_amdgcn_s_memtime(); };
#else
    auto stamp = [] {};
#endif
    stamp();
    // ---- input stage: relu(Ps[src] + Pd[dst] + Wf . [pos_i - pos_j, |pos_i - pos_j|])   (ops/basic.py:70-92)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      row[rb] = int64_t(tile) * tile_rows + wave * (16 * RB) + rb * 16 + (lane & 15);
      off[rb] = pair_offsets<NB>(wave * (16 * RB) + rb * 16 + (lane & 15), lane);                         // within the tile
      moff[rb] = unsigned(((wave * (16 * RB) + rb * 16 + (lane & 15)) * (4 * mask_words<NB>()) + lg * mask_words<NB>()) * 4);
      const int i = ni[rb], j = nj[rb], b = nbat[rb];
      load_rows<NB>(act[rb], a.Ps + (int64_t(b) * a.N + i) * D, lg);
      load_rows<NB>(acc[rb], a.Pd + (int64_t(b) * a.N + j) * D, lg);
      const float* pb = a.pos + b * a.pos_bstride;
      if (a.p == 2) {   // uniform; the common widths load whole points
        const float2 xi = *reinterpret_cast<const float2*>(pb + int64_t(i) * 2), xj = *reinterpret_cast<const float2*>(pb + int64_t(j) * 2);
        pi[rb][0] = xi.x; pi[rb][1] = xi.y; pj[rb][0] = xj.x; pj[rb][1] = xj.y;
#pragma unroll
        for (int c = 2; c < 7; ++c) pi[rb][c] = pj[rb][c] = 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          const int cc = c < a.p ? c : 0;   // uniform clamp: the loads stay unconditional
          pi[rb][c] = pb[int64_t(i) * a.p + cc];
          pj[rb][c] = pb[int64_t(j) * a.p + cc];
        }
      }
    }
    if (tile + int(gridDim.x) < a.ntiles) fetch_endpoints(tile + gridDim.x, ni, nj, nbat);   // uniform; lands under the stages
    __builtin_amdgcn_sched_barrier(0);   // all gathers of the tile are in flight before the first use
    stamp();
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int t = 0; t < NB; ++t) act[rb][t] += acc[rb][t];
      float n2 = 0.f;
#pragma unroll
      for (int c = 0; c < 7; ++c)
        if (c < a.p) {
          const float rel = pi[rb][c] - pj[rb][c];
          n2 = fmaf(rel, rel, n2);
          axpy_features<NB>(act[rb], w0t + c * D, rel, lg);
        }
      const float nrm = sqrtf(n2);
      axpy_features<NB>(act[rb], w0t + a.p * D, nrm, lg);
      relu_into<NB>(act[rb], act[rb]);
      if (a.fiber_out && row[rb] < a.R && lg == 0) {   // one lane per row keeps the fiber for the backward (uniform: null in inference)
        float f[8];
#pragma unroll
        for (int c = 0; c < 7; ++c) f[c] = c < a.p ? pi[rb][c] - pj[rb][c] : (c == a.p ? nrm : 0.f);
        f[7] = a.p == 7 ? nrm : 0.f;
        const int ld = fiber_ld(a.p);
        float4* dst = reinterpret_cast<float4*>(a.fiber_out + row[rb] * ld);
        dst[0] = make_float4(f[0], f[1], f[2], f[3]);
        if (ld == 8) dst[1] = make_float4(f[4], f[5], f[6], f[7]);
      }
    }
    // ---- MFMA stages; the activation entering a stage is stored (values + sign bits) from inside that stage
    float* pending = a.store_in;   // uniform; non-null when SAVE (launcher)
    stamp();
    for (int l = 0; l < a.nstage; ++l) {
      float* st_tile = SAVE ? pending + int64_t(tile) * (tile_rows * D) : nullptr;   // uniform
      unsigned* bits_tile = SAVE ? reinterpret_cast<unsigned*>(pending + pad_rows(a.R) * D) + int64_t(tile) * (tile_rows * 4 * mask_words<NB>()) : nullptr;
#ifdef BSMS_EXPERIMENTS
      stage_rb<NB, RB, SAVE, true, true, 2, LONE>(acc, act, ring, slot, lane, st_tile, bits_tile, off, moff, brow, l, nullptr, a.timing ? &waited : nullptr);
#else
      stage_rb<NB, RB, SAVE, true, true, 2, LONE>(acc, act, ring, slot, lane, st_tile, bits_tile, off, moff, brow, l);   // acc = bias + W act
#endif
      stamp();
      if (l + 1 < a.nstage) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) relu_into<NB>(act[rb], acc[rb]);
        pending = a.store[l];
      }
    }
    // ---- LayerNorm(elementwise_affine=False), eps 1e-5  (ops/basic.py:18)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const float mean = row_sum<NB>(acc[rb]) * (1.f / D);
      float ss = 0.f;
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[rb][t][r] -= mean;
          ss = fmaf(acc[rb][t][r], acc[rb][t][r], ss);
        }
      ss = group_sum(ss);
      const float rstd = 1.f / sqrtf(ss * (1.f / D) + 1e-5f);
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rb][t][r] *= rstd;
      const int64_t roff = row[rb] < a.R ? row[rb] * D : -1;
      store_rows<NB, false>(acc[rb], a.yln, roff, lg);
      if (a.rstd && roff >= 0 && lg == 0) a.rstd[row[rb]] = rstd;
      store_rows<NB, false>(acc[rb], a.y, roff, lg, a.out_mode);
    }
    stamp();
#ifdef BSMS_EXPERIMENTS
    if (a.timing && tid == 0) a.timing[int64_t(tile) * 16 + 11] = waited;
#endif
  }
  if (SAVE) flush_bounds(a.amax, kMaxStages + 1, brow, wave, lane);
}

// STORE = false (the edge MLP is frozen, gmp.hip): the layer gradients gstore[0 .. nstage-1] have no reader (only the weight-gradient
// jobs read them) and are not written -- stage_rb<SAVE = 0>, the path of the inference forward with its shorter VALU step table;
// the last gradient, gstore[nstage] = gE[0], is stored as always (the scatter and the position gradient read it).  Same products
// in the same order: the gradients are bit-identical to the storing build's.
template <int NB, int RB, bool LONE = false, bool STORE = true>
__global__ __launch_bounds__(kChainMaxThreads) __attribute__((amdgpu_waves_per_eu(LONE ? 2 : EdgeTile<NB, RB>::waves_per_eu)))
void k_edge_bwd(ChainBwdArgs a) {
  constexpr int D = NB * 16, W = mask_words<NB>();
  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
  const int cw = int(blockDim.x >> 6) - a.nload, tile_rows = 16 * RB * cw;   // compute waves of this launch (launcher's choice); the last wave(s) load
  if (wave >= cw) {  // loader wave (uniform branch)
    loader_dispatch<NB>(a.nload, wave - cw, a.wseq, a.nseq, lds, lane, a.ntiles, a.nring);
    return;
  }
  const float rcpE = 1.f / float(a.E);
  auto fetch_targets = [&](int tile, int64_t (&node)[RB]) {   // node row (b * N + dst) of this lane's rows, one tile ahead
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int64_t r = int64_t(tile) * tile_rows + wave * (16 * RB) + rb * 16 + (lane & 15);
      const EdgeRef e = edge_ref(unsigned(r < a.R ? r : 0), unsigned(a.E), rcpE);
      node[rb] = int64_t(e.b) * a.N + a.dst[e.q];
    }
  };
  int64_t nnode[RB];
  fetch_targets(blockIdx.x, nnode);
  Slot slot{0, a.nring};
  float4* const ring = lds + Ring<NB>::PRE4;
  unsigned* brow = bound_row<NB>(lds, wave, lane, any_slot(a.gmax));   // this wave's running magnitude bounds
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int64_t row[RB], rowc[RB];
    PairOff off[RB];
    unsigned moff[RB];
    f32x4 g[RB][NB], acc[RB][NB];
    float rs[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {   // autograd of scatter_sum: gather the node gradient by target; y, rstd of the row
      row[rb] = int64_t(tile) * tile_rows + wave * (16 * RB) + rb * 16 + (lane & 15);
      rowc[rb] = row[rb] < a.R ? row[rb] : 0;
      off[rb] = pair_offsets<NB>(wave * (16 * RB) + rb * 16 + (lane & 15), lane);   // within the tile
      moff[rb] = 0;
      load_rows<NB>(g[rb], a.dy + nnode[rb] * D, lg);
      load_rows<NB>(acc[rb], a.yln + rowc[rb] * D, lg);
      rs[rb] = a.rstd[rowc[rb]];
    }
    if (tile + int(gridDim.x) < a.ntiles) fetch_targets(tile + gridDim.x, nnode);   // uniform; lands under the stages
    __builtin_amdgcn_sched_barrier(0);   // all loads in flight before the first use
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {   // LayerNorm backward (no affine): dz = rstd * (dy - mean(dy) - y * mean(dy * y))
      const float m1 = row_sum<NB>(g[rb]) * (1.f / D);
      float s2 = 0.f;
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s2 = fmaf(g[rb][t][r], acc[rb][t][r], s2);
      s2 = group_sum(s2);
      const float m2 = s2 * (1.f / D);
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) g[rb][t][r] = rs[rb] * (g[rb][t][r] - m1 - acc[rb][t][r] * m2);
    }
    float* pending = a.gstore[0];   // uniform, non-null when STORE (launcher): the gradient entering a stage is stored inside it
    for (int k = 0; k < a.nstage; ++k) {
      unsigned mbits[RB][W];   // ReLU sign bits of the activation that masks this stage's output, loaded ahead of the stage
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int w = 0; w < W; ++w)
          mbits[rb][w] = reinterpret_cast<const unsigned*>(a.mask[k] + pad_rows(a.R) * D)[rowc[rb] * (4 * W) + lg * W + w];
#ifdef BSMS_EXPERIMENTS   // ablation bound of the fused dataflow (profiles/r05_fusion_bound.txt): the layer gradients of every tile land on tile 0
      float* const gtile = STORE ? pending + int64_t(a.ablate ? 0 : tile) * (tile_rows * D) : nullptr;
#else
      float* const gtile = STORE ? pending + int64_t(tile) * (tile_rows * D) : nullptr;
#endif
      stage_rb<NB, RB, STORE ? 1 : 0, false, true, 1, LONE>(acc, g, ring, slot, lane, gtile, nullptr, off, moff, brow, k);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int t = 0; t < NB; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {   // bit -> all-ones / zero mask (one v_bfe_i32), then one and
            const int keep = __builtin_amdgcn_sbfe((int)mbits[rb][(4 * t + r) >> 5], (4 * t + r) & 31, 1);
            g[rb][t][r] = __uint_as_float(__float_as_uint(acc[rb][t][r]) & (unsigned)keep);
          }
      pending = a.gstore[k + 1];
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {  // gE[0]: read next by the scatter kernel, plain stores (stay in L2 / the memory-side cache)
      if (a.gmax[a.nstage]) note_amax(brow, a.nstage, row_amax<NB>(g[rb]), lane);   // uniform
      store_rows<NB, false>(g[rb], pending, row[rb] < a.R ? row[rb] * D : -1, lg);
    }
  }
  flush_bounds(a.gmax, kMaxStages + 1, brow, wave, lane);
}

}  // namespace
