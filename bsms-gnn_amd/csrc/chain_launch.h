// Host side of the chain kernels: launch shapes, the choice of the kernel variant, and the two entry points of a width,
// launch_chain_fwd_nb<NB> / launch_chain_bwd_nb<NB> (chain.h), which chain_d*.hip instantiates explicitly.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "chain_edge.h"
#include "chain_kernels.h"

namespace {

// Workgroups of 5 waves the chip keeps resident per CU at each width.  NOT the occupancy API's answer: the SPI
// accounts a 5-wave workgroup like an 8-wave one (census: 320 threads x 120 VGPRs -> 2 per CU where the API says 3;
// profiles/census).  A grid larger than the residency would only queue, a smaller one idles slots.
// D = 96 / 160 / 192 / 224 (NB = 6 / 10 / 12 / 14) keep ONE: their kernels are built for 256 VGPRs (chain_wpe) and the
// largest instantiations use more than 128 (D = 96: up to 137, the wider ones 140-230; two waves per SIMD and workgroup
// leave room for one), and from NB = 12 on the 3-slot ring alone (82 / 95 KB of LDS) would not fit twice into 160 KB
// (profiles/width_rates.txt: resource table).
template <int NB>
constexpr int resident_per_cu() { return NB <= 4 ? 4 : NB == 8 ? 2 : 1; }

// Compute waves per workgroup of a generic chain launch: 4 (64-row tiles), or up to 7 when that makes the launch fit ONE
// round of resident workgroups.  A workgroup streams the whole weight set once per tile (~23 us for the node MLP: the
// LDS-DMA rate of a CU), so a second, nearly empty round costs as much as the first: the level-0 node launches of the
// airfoil step (41 864 rows = 655 tiles of 64 on 512 slots) run as 437 tiles of 96 rows instead.  The SPI accounts a
// 5-wave workgroup like an 8-wave one anyway (resident_per_cu), so the extra waves use slots that were empty.
template <int NB>
int chain_compute_waves(int64_t R) {
  const int cus = device_cu_count();
  const int64_t slots = int64_t(cus) * resident_per_cu<NB>();
  if (resident_per_cu<NB>() >= 4 || ceil_div(R, kTileRows) <= slots) return kComputeWaves;   // D = 32 / 64: always 4
  const int64_t need = ceil_div(R, slots * 16);   // waves per workgroup for one round
  return need <= 7 ? (int)need : kComputeWaves;
}

template <int NB>
unsigned persistent_grid(int64_t ntiles) {
  const int cus = device_cu_count();
  return (unsigned)std::min<int64_t>(ntiles, int64_t(cus) * resident_per_cu<NB>());
}

// Launch shape knobs.  Production values are the defaults; experiment builds read them from the environment for
// same-box sweeps (BSMS_EDGE_CW, BSMS_EDGE_NL, BSMS_CHAIN_NL, BSMS_EDGE_CW16, BSMS_EDGE_NL16).
inline int knob(const char* name, int dflt) {
#ifdef BSMS_EXPERIMENTS
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

// experiment builds (same-box A/B, profiles/edge_prof.sh): BSMS_EDGE_RB = 0 keeps the edge MLP on k_chain_fwd / k_chain_bwd,
// 1 / 2 force the number of row blocks per wave
inline int edge_rb_mode() {
#ifdef BSMS_EXPERIMENTS
  static const int m = [] { const char* e = getenv("BSMS_EDGE_RB"); return e ? atoi(e) : -1; }();
  return m;
#else
  return -1;
#endif
}

// Compute waves per workgroup of an edge launch: 7 (+ the loader: 8 waves, 112 x RB rows per tile).  A tile streams the
// whole weight set of the MLP through the loader's LDS-DMA (one wave delivers a 1 KB piece per 60-185 cycles,
// profiles/census/ldsdma_rate.hip), and since the fp32 products take three MFMAs per fragment pair that stream, not the
// matrix pipe, paces a stage: 7 compute waves spread it over 1.75x the rows of 4 (same-box +2.5 % steps/s at D = 128 with
// the fp16 x 2 arithmetic; +4.3 % at D = 256 already with the bf16 x 3 one; profiles/r02_edge_levels.md, r03).
template <int NB>
int edge_compute_waves() {
  static const int cw = NB >= 16 ? knob("BSMS_EDGE_CW16", 7) : knob("BSMS_EDGE_CW", 7);
  return cw;
}
// Compute waves of ONE edge launch.  A persistent workgroup runs ceil(tiles / grid) tiles one after the other and a tile
// costs t0 + t1 * (rows per wave-set): the fixed part is the weight stream of the whole MLP, the rest scales with the rows.
// Seven waves minimise the fixed part per row, but a launch whose last round is nearly empty pays a whole tile for it:
// cylinder level 0 (90 112 rows, 512 slots) runs 2 rounds with 7, 6 waves and 3 with 5, 4 -- 6 waves win by the shorter
// tile (same-box sweep: 4 / 5 / 6 / 7 waves = 400.1 / 392.6 / 404.4 / 397.2 steps/s, exactly this model's order).  The
// slope t1 / t0 = 0.53 per wave with one row block per wave comes from the airfoil sweep (7 against 4 waves: +2.5 %).
template <int NB, int RB>
int pick_edge_waves(int64_t R) {
  const int fixed = edge_compute_waves<NB>();
#ifdef BSMS_EXPERIMENTS
  if (getenv(NB >= 16 ? "BSMS_EDGE_CW16" : "BSMS_EDGE_CW") || getenv("BSMS_EDGE_CW_FIXED")) return fixed;
#endif
  const double slope = (NB >= 16 ? 0.25 : 0.53) * RB;
  const int64_t slots = int64_t(device_cu_count()) * EdgeTile<NB, RB>::resident;
  auto cost_of = [&](int cw) {
    const int64_t tiles = ceil_div(R, int64_t(16) * RB * cw);
    const int64_t per = ceil_div(tiles, std::min<int64_t>(tiles, slots));
    return double(per) * (1.0 + slope * cw);
  };
  int best = fixed;
  double best_cost = cost_of(fixed) * 0.92;   // the model is coarse: leave the measured default unless it predicts a clear gain
  for (int cw = 6; cw >= 4; --cw) {
    const double cost = cost_of(cw);
    if (cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = cw; }
  }
  return best;
}
template <int NB>
int edge_loader_waves() {
  static const int nl = NB >= 16 ? knob("BSMS_EDGE_NL16", 1) : knob("BSMS_EDGE_NL", 1);
  return nl;
}
inline int chain_loader_waves() {
  static const int nl = knob("BSMS_CHAIN_NL", 1);
  return nl;
}

// Weight stream of a launch: loader waves and ring depth (Ring).  A launch that fits ONE round of workgroups (at most
// one workgroup per CU: the coarse mesh levels, most node-level launches) has the CU's whole LDS and nothing to overlap
// its chunk latency with: deep ring (up to 6 slots = 5 chunks in flight) fed by two loader waves.  Anything larger keeps
// 3 slots so that two workgroups share a CU.  Limits: compute + loader waves <= 8; (nr - 2) x pieces per loader <= 63
// (vmcnt field); ring + side tables <= 160 KB.
template <int NB, int PL = kPL>
int max_ring() { return (int)std::min<size_t>(6, (size_t(160) * 1024 - Ring<NB, PL>::PRE_FLOATS * sizeof(float)) / (Ring<NB, PL>::CHF * sizeof(float))); }
template <int NB, int PL = kPL>
void pick_stream(int64_t ntiles, int cw, int nload_default, int& nload, int& nring) {
  static const int deep = knob("BSMS_RING_DEEP", 6), lone_nl = knob("BSMS_LONE_NL", 2), shared = knob("BSMS_RING", 3);
  nload = std::max(1, std::min(nload_default, 8 - cw));
  nring = std::min(shared, max_ring<NB, PL>());
  if (ntiles <= device_cu_count()) {
    nload = std::max(nload, std::min(lone_nl, 8 - cw));
    nring = std::min(deep, max_ring<NB, PL>());
  }
  const int mine = (Ring<NB, PL>::PER + nload - 1) / nload;
  while (nring > 3 && (nring - 2) * mine > 63) --nring;
}

template <int NB>
size_t ring_lds_max() { return Ring<NB>::lds_bytes(max_ring<NB>()); }

template <int NB, int RB, int SAVE>
int launch_edge_fwd_t(ChainFwdArgs& a, hipStream_t s) {
  const int cw = pick_edge_waves<NB, RB>(a.R);
  a.ntiles = (int)ceil_div(a.R, 16 * RB * cw);
  pick_stream<NB>(a.ntiles, cw, edge_loader_waves<NB>(), a.nload, a.nring);
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, int64_t(device_cu_count()) * EdgeTile<NB, RB>::resident);
  const unsigned threads = (cw + a.nload) * 64;
  const size_t lds = Ring<NB>::lds_bytes(a.nring);
  static const int lone = knob("BSMS_EDGE_LONE", 1);
  if (lone && a.ntiles <= device_cu_count() && !a.timing)   // one round of workgroups: the variant that passes the chunk barrier early (stage_rb<LONE>)
    return launch_dyn_lds<k_edge_fwd<NB, RB, SAVE, true>>("edge_fwd", "single-round build", grid, threads, lds, ring_lds_max<NB>(), a, s);
  return launch_dyn_lds<k_edge_fwd<NB, RB, SAVE>>("edge_fwd", nullptr, grid, threads, lds, ring_lds_max<NB>(), a, s);
}

// the software-pipelined edge kernels take the production configuration only; anything else stays on k_chain_fwd
template <int NB>
bool launch_edge_fwd(ChainFwdArgs& a, hipStream_t s, int& rc) {
  if (a.bf16 || a.nstage < 1 || a.store_mode != 1 || a.resid || a.resid2 || edge_rb_mode() == 0 || a.R >= (int64_t(1) << 31)) return false;
  const bool save = a.store_in != nullptr;
  for (int l = 0; l + 1 < a.nstage; ++l)
    if ((a.store[l] != nullptr) != save) return false;
  constexpr int RBIG = NB == 8 ? 2 : 1;
  // Measured per level (profiles/r02_edge_levels.md): with several tiles per workgroup two workgroups per CU of one row
  // block per wave win the forward (the random row gathers of one hide under the other's MFMA stages); a launch that
  // fits one round of workgroups is faster with two row blocks per wave, and so is the whole backward (its loads are
  // sequential or local).  Below half a round of 128-row tiles the narrow tile keeps more CUs busy.
  const int64_t cus = device_cu_count(), rows1 = 16 * edge_compute_waves<NB>();   // rows of a tile with one row block per wave
  bool big = RBIG == 2 && a.R >= cus * rows1 && ceil_div(a.R, rows1) <= cus * EdgeTile<NB, 1>::resident;
  if (edge_rb_mode() > 0) big = RBIG == 2 && edge_rb_mode() == 2;
  if (big) rc = save ? launch_edge_fwd_t<NB, RBIG, 1>(a, s) : launch_edge_fwd_t<NB, RBIG, 0>(a, s);
  else rc = save ? launch_edge_fwd_t<NB, 1, 1>(a, s) : launch_edge_fwd_t<NB, 1, 0>(a, s);
  return true;
}

template <int NB, int RB, bool STORE>
int launch_edge_bwd_t(ChainBwdArgs& a, hipStream_t s) {
  const int cw = pick_edge_waves<NB, RB>(a.R);
  a.ntiles = (int)ceil_div(a.R, 16 * RB * cw);
  pick_stream<NB>(a.ntiles, cw, edge_loader_waves<NB>(), a.nload, a.nring);
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, int64_t(device_cu_count()) * EdgeTile<NB, RB>::resident);
  const unsigned threads = (cw + a.nload) * 64;
  const size_t lds = Ring<NB>::lds_bytes(a.nring);
  static const int lone = knob("BSMS_EDGE_LONE", 1);
  if (lone && a.ntiles <= device_cu_count())   // see launch_edge_fwd_t
    return launch_dyn_lds<k_edge_bwd<NB, RB, true, STORE>>("edge_bwd", STORE ? "single-round build" : "single-round no-store build", grid, threads, lds, ring_lds_max<NB>(), a, s);
  return launch_dyn_lds<k_edge_bwd<NB, RB, false, STORE>>("edge_bwd", STORE ? nullptr : "no-store build", grid, threads, lds, ring_lds_max<NB>(), a, s);
}

template <int NB>
bool launch_edge_bwd(ChainBwdArgs& a, hipStream_t s, int& rc) {
  if (a.bf16 || a.nstage < 1 || a.store_mode != 1 || edge_rb_mode() == 0 || a.R >= (int64_t(1) << 31)) return false;
  // the layer gradients gstore[0 .. nstage-1]: all kept, or none (a frozen edge MLP: the no-store build; tile, ring and single-round
  // choices are the storing launch's).  The last gradient, gstore[nstage], always has a reader.
  if (!a.gstore[a.nstage]) return false;
  const bool store = a.gstore[0] != nullptr;
  for (int k = 0; k < a.nstage; ++k)
    if ((a.gstore[k] != nullptr) != store || !a.mask[k]) return false;
  constexpr int RBIG = NB == 8 ? 2 : 1;
  bool big = RBIG == 2 && a.R >= int64_t(device_cu_count()) * 16 * edge_compute_waves<NB>();   // see launch_edge_fwd
  if (edge_rb_mode() > 0) big = RBIG == 2 && edge_rb_mode() == 2;
  if (store) rc = big ? launch_edge_bwd_t<NB, RBIG, true>(a, s) : launch_edge_bwd_t<NB, 1, true>(a, s);
  else rc = big ? launch_edge_bwd_t<NB, RBIG, false>(a, s) : launch_edge_bwd_t<NB, 1, false>(a, s);
  return true;
}

// Compute waves per workgroup of the bf16 edge chains (generic kernels, 16 rows per wave).  Round 4, same-box with the
// experiment build (profiles/r04_bfcw.sh): 7 waves against 4 -- airfoil batch 8 bf16 222.4 -> 230.1, bf16_nodes 231.5 -> 241.5,
// surface B=2 bf16 105.2 -> 110.9 / bf16_nodes 111.6 -> 118.0 steps/s (a workgroup streams the weights once per tile: 112 rows
// per pass instead of 64); a launch that fits one round of 64-row tiles keeps 4 (batch 1: 614 against 597 steps/s with 7).
template <int NB>
int bf_edge_waves(int64_t R) {
  static const int forced = knob("BSMS_BFEDGE_CW", 0);
  if (forced > 0) return forced;
  return R > int64_t(device_cu_count()) * resident_per_cu<NB>() * 16 * kComputeWaves ? 7 : kComputeWaves;
}

// Which kernel runs a forward chain, first match wins:
//   1. the pipelined edge kernel (launch_edge_fwd: NB = 8 / 16, fp32 edge MLP in its production configuration);
//   2. the feature-split kernel (NB = 8, fp32, at most kFsMaxRows rows);
//   3. the TIMING variant when the caller asks for stamps (NB = 8 edge chain; experiment builds: also the single-round node chain);
//   4. the bf16 variant (edge and node MLPs at NB = 8 / 16; bf16 anywhere else is an error);
//   5. the single-round (LONE) variant, NB >= 8, when the launch fits one workgroup per CU or is the [x, x2] Linear below;
//   6. the ring kernel.
template <int NB, int IN, int OUT>
int launch_fwd_t(const ChainFwdArgs& a0, hipStream_t s) {
  ChainFwdArgs a = a0;
  a.nseq = 0;
  for (int l = 0; l < a.nstage; ++l) {  // the loader follows exactly the compute waves' stage order
    a.wseq[a.nseq++] = a.wp[l];
    if (IN == IN_ROWS2 && l == 0) a.wseq[a.nseq++] = a.wp0b;
  }
  if constexpr ((NB == 8 || NB == 16) && IN == IN_EDGE && OUT == OUT_LN) {
    int rc = BSMS_OK;
    if (launch_edge_fwd<NB>(a, s, rc)) return rc;
  }
  if constexpr (NB == 8 && (IN == IN_ROWS || IN == IN_ROWS2 || IN == IN_SMALL)) {   // small launches
    static const int fs_rows = knob("BSMS_FS_ROWS", kFsMaxRows);
    if (!a.bf16 && a.R <= fs_rows && a.nseq >= 1 && a.nseq <= kMaxStages + 1) {
      hipLaunchKernelGGL((k_fs_fwd<IN, OUT>), dim3((unsigned)ceil_div(a.R, 16)), dim3(256), 0, s, a);
      BSMS_LAUNCH_CHECK();
      return BSMS_OK;
    }
  }
  // ---- launch shape of the ring kernel and its variants
  int cw = (IN == IN_EDGE) ? bf_edge_waves<NB>(a.R) : chain_compute_waves<NB>(a.R);
  a.ntiles = (int)ceil_div(a.R, 16 * cw);
  // One Linear over [x, x2] added into y (the input gradient through the two edge projections, gmp.hip): three more dependent row
  // loads per tile than a plain chain and only two packs of MFMAs to hide them under.  The single-round build keeps x2 in registers
  // (one round trip instead of three) -- so this launch always takes it, one 7-wave workgroup per CU striding over the tiles
  // (round 6, profiles/r06_rows2.txt).
  bool rows2_lone = false;
  if constexpr (NB == 8 && IN == IN_ROWS2 && OUT == OUT_PLAIN) {
    static const int on = knob("BSMS_ROWS2_LONE", 1);
    if (on && !a.bf16 && a.nstage == 1 && a.ntiles > device_cu_count()) {
      rows2_lone = true;
      cw = 7;
      a.ntiles = (int)ceil_div(a.R, 16 * cw);
    }
  }
  const int64_t stream_tiles = rows2_lone ? std::min<int64_t>(a.ntiles, device_cu_count()) : a.ntiles;   // ring depth / loaders of a one-workgroup-per-CU launch
  if (a.bf16) pick_stream<NB, 1>(stream_tiles, cw, chain_loader_waves(), a.nload, a.nring);
  else pick_stream<NB>(stream_tiles, cw, chain_loader_waves(), a.nload, a.nring);
  const unsigned grid = rows2_lone ? (unsigned)stream_tiles : persistent_grid<NB>(a.ntiles);   // (rows2_lone: fp32 OUT_PLAIN, always the LONE variant)
  const unsigned threads = (cw + a.nload) * 64;
  // the bf16 precision's chunks are one plane: its ring may be deeper than the fp32 one at the same D, size it as what it is
  const size_t lds = a.bf16 ? Ring<NB, 1>::lds_bytes(a.nring) : Ring<NB>::lds_bytes(a.nring), lds_max = ring_lds_max<NB>();
  // ---- the variant
  if constexpr (NB == 8 && IN == IN_EDGE) {   // the only production instantiation with stamps
    if (a.timing) return launch_dyn_lds<k_chain_fwd<NB, IN, OUT, true>>("chain_fwd", "timing build", grid, threads, lds, lds_max, a, s);
  }
#ifdef BSMS_EXPERIMENTS
  if constexpr (NB == 8 && IN == IN_ROWS2 && OUT == OUT_LN) {   // phase stamps of a single-round node chain (profiles/lone_timeline.py)
    if (a.timing && a.ntiles <= device_cu_count())
      return launch_dyn_lds<k_chain_fwd<NB, IN, OUT, true, false, true>>("chain_fwd", "timing build", grid, threads, lds, lds_max, a, s);
  }
#endif
  if constexpr ((NB == 8 || NB == 16) && (IN == IN_EDGE || IN == IN_ROWS2) && OUT == OUT_LN) {   // the bf16 arithmetic: edge MLP (BSMS_BF16), node MLP (BSMS_BF16_NODES)
    if (a.bf16) return launch_dyn_lds<k_chain_fwd<NB, IN, OUT, false, true>>("chain_fwd", "bf16 build", grid, threads, lds, lds_max, a, s);
  }
  BSMS_REQUIRE(!a.bf16, BSMS_E_UNSUPPORTED, "chain_fwd: bf16 precision is built for the edge and node MLPs at D = 128 / 256 only");
  // (D = 96 has no single-round build: its single-round launches stay on the ring kernel, which saves a set of instantiations)
  if constexpr (NB >= 8) {   // one round of workgroups = a single wave per SIMD: the variant that prefetches its fragments (mfma_stage)
    if (a.ntiles <= device_cu_count() || rows2_lone)
      return launch_dyn_lds<k_chain_fwd<NB, IN, OUT, false, false, true>>("chain_fwd", "single-round build", grid, threads, lds, lds_max, a, s);
  }
  return launch_dyn_lds<k_chain_fwd<NB, IN, OUT>>("chain_fwd", nullptr, grid, threads, lds, lds_max, a, s);
}
// Only the combinations the path uses are instantiated (each is a large unrolled kernel).
template <int NB>
int launch_fwd_n(int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s) {
#define BSMS_FWD(I, O) \
  if (in_mode == I && out_mode == O) return launch_fwd_t<NB, I, O>(a, s)
  BSMS_FWD(IN_ROWS, OUT_PLAIN);   // x W^T
  BSMS_FWD(IN_ROWS, OUT_PLAIN2);  // the two node pre-projections of the edge MLP
  BSMS_FWD(IN_ROWS2, OUT_PLAIN);  // its input gradient
  BSMS_FWD(IN_EDGE, OUT_LN);      // edge MLP
  BSMS_FWD(IN_ROWS2, OUT_LN);     // node MLP on [x, aggr]
  BSMS_FWD(IN_SMALL, OUT_LN);     // encoder
  BSMS_FWD(IN_ROWS, OUT_SMALL);   // decoder
  BSMS_FWD(IN_ROWS, OUT_LN);      // generic D -> D MLP
#undef BSMS_FWD
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "chain_fwd: in/out mode (%d,%d) not built", in_mode, out_mode);
}

// Which kernel runs a backward chain, first match wins:
//   1. the feature-split kernel (NB = 8, fp32, at most kFsMaxRowsBwd rows);
//   2. the pipelined edge kernel (launch_edge_bwd: NB = 8 / 16, fp32 edge MLP in its production configuration; its no-store
//      build when the layer gradients gstore[0 .. nstage-1] are all null);
//   3. the bf16 variant (edge MLP; node MLP of BSMS_BF16_NODES; NB = 8 / 16; bf16 anywhere else is an error);
//   4. the single-round (LONE) variant, NB >= 8, when the launch fits one workgroup per CU;
//   5. the ring kernel.
template <int NB, int GIN, int FIRST>
int launch_bwd_t(const ChainBwdArgs& a0, hipStream_t s) {
  ChainBwdArgs a = a0;
  a.nseq = 0;
  for (int k = 0; k < a.nstage; ++k) a.wseq[a.nseq++] = a.wpt[k];
  if (FIRST != F_NONE) a.wseq[a.nseq++] = a.wh0;
  if (FIRST == F_HEADS2) a.wseq[a.nseq++] = a.wh1;
  if constexpr (NB == 8 && (GIN == G_ROWS_LN || GIN == G_SMALL)) {   // small launches (see launch_fwd_t)
    static const int fs_rows = knob("BSMS_FS_ROWS_BWD", kFsMaxRowsBwd);
    if (!a.bf16 && a.R <= fs_rows && a.nseq >= 1) {
      hipLaunchKernelGGL((k_fs_bwd<GIN, FIRST>), dim3((unsigned)ceil_div(a.R, 16)), dim3(256), 0, s, a);
      BSMS_LAUNCH_CHECK();
      return BSMS_OK;
    }
  }
  if constexpr ((NB == 8 || NB == 16) && GIN == G_EDGE_LN && FIRST == F_NONE) {
    int rc = BSMS_OK;
    if (launch_edge_bwd<NB>(a, s, rc)) return rc;
  }
  // ---- launch shape of the ring kernel and its variants
  const int cw = (GIN == G_EDGE_LN) ? bf_edge_waves<NB>(a.R) : chain_compute_waves<NB>(a.R);
  a.ntiles = (int)ceil_div(a.R, 16 * cw);
  if (a.bf16) pick_stream<NB, 1>(a.ntiles, cw, chain_loader_waves(), a.nload, a.nring);
  else pick_stream<NB>(a.ntiles, cw, chain_loader_waves(), a.nload, a.nring);
  const unsigned grid = persistent_grid<NB>(a.ntiles), threads = (cw + a.nload) * 64;
  const size_t lds = a.bf16 ? Ring<NB, 1>::lds_bytes(a.nring) : Ring<NB>::lds_bytes(a.nring), lds_max = ring_lds_max<NB>();   // see launch_fwd_t
  // ---- the variant
  constexpr bool kEdgeMlp = GIN == G_EDGE_LN && FIRST == F_NONE, kNodeMlp = GIN == G_ROWS_LN && FIRST == F_HEADS2;
  if constexpr ((NB == 8 || NB == 16) && (kEdgeMlp || kNodeMlp)) {
    if (a.bf16) return launch_dyn_lds<k_chain_bwd<NB, GIN, FIRST, true>>("chain_bwd", kEdgeMlp ? "bf16 build" : "bf16 node build", grid, threads, lds, lds_max, a, s);
  }
  BSMS_REQUIRE(!a.bf16, BSMS_E_UNSUPPORTED, "chain_bwd: bf16 precision is built for the edge and node MLPs at D = 128 / 256 only");
  if constexpr (NB >= 8) {   // see launch_fwd_t
    if (a.ntiles <= device_cu_count())
      return launch_dyn_lds<k_chain_bwd<NB, GIN, FIRST, false, true>>("chain_bwd", "single-round build", grid, threads, lds, lds_max, a, s);
  }
  return launch_dyn_lds<k_chain_bwd<NB, GIN, FIRST>>("chain_bwd", nullptr, grid, threads, lds, lds_max, a, s);
}
template <int NB>
int launch_bwd_n(int gin, int first, const ChainBwdArgs& a, hipStream_t s) {
#define BSMS_BWD(G, F) \
  if (gin == G && first == F) return launch_bwd_t<NB, G, F>(a, s)
  BSMS_BWD(G_ROWS_LN, F_HEADS2);  // node MLP
  BSMS_BWD(G_EDGE_LN, F_NONE);    // edge MLP
  BSMS_BWD(G_ROWS_LN, F_NONE);    // encoder
  BSMS_BWD(G_SMALL, F_HEADS1);    // decoder
  BSMS_BWD(G_ROWS_LN, F_HEADS1);  // generic D -> D MLP
#undef BSMS_BWD
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "chain_bwd: grad/first mode (%d,%d) not built", gin, first);
}

}  // namespace

namespace bsms {
template <int NB>
int launch_chain_fwd_nb(int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s) { return launch_fwd_n<NB>(in_mode, out_mode, a, s); }
template <int NB>
int launch_chain_bwd_nb(int gin, int first, const ChainBwdArgs& a, hipStream_t s) { return launch_bwd_n<NB>(gin, first, a, s); }
}  // namespace bsms
