// Host side of the chain kernels.  The choice of a launch is DATA: plan_fwd / plan_bwd map a ChainLaunchKey (what the choice reads
// from the arguments) and a CU count to a ChainLaunch (family, variant, shape) without touching the device; launch_fwd_t /
// launch_bwd_t build the key, call them and run ONE switch from the record to the instantiation; chain_launch_query_nb answers
// bsms_chain_launch_query from the same two functions.  The entry points of a width, launch_chain_fwd_nb<NB> /
// launch_chain_bwd_nb<NB> / chain_launch_query_nb<NB> (chain.h), are instantiated explicitly by chain_d*.hip.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

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
// the same for the edge kernels with `rb` row blocks per wave (chain_edge.h)
template <int NB>
constexpr int edge_resident(int rb) { return rb == 2 ? EdgeTile<NB, 2>::resident : EdgeTile<NB, 1>::resident; }

// THE one-round predicate: `tiles` fit one round of `room` workgroups (room = the CU count: at most one workgroup per CU)
inline bool one_round(int64_t tiles, int64_t room) { return tiles <= room; }

// Compute waves per workgroup of a generic chain launch: 4 (64-row tiles), or up to 7 when that makes the launch fit ONE
// round of resident workgroups.  A workgroup streams the whole weight set once per tile (~23 us for the node MLP: the
// LDS-DMA rate of a CU), so a second, nearly empty round costs as much as the first: the level-0 node launches of the
// airfoil step (41 864 rows = 655 tiles of 64 on 512 slots) run as 437 tiles of 96 rows instead.  The SPI accounts a
// 5-wave workgroup like an 8-wave one anyway (resident_per_cu), so the extra waves use slots that were empty.
template <int NB>
int chain_compute_waves(int64_t R, int cus) {
  const int64_t slots = int64_t(cus) * resident_per_cu<NB>();
  if (resident_per_cu<NB>() >= 4 || one_round(ceil_div(R, kTileRows), slots)) return kComputeWaves;   // D = 32 / 64: always 4
  const int64_t need = ceil_div(R, slots * 16);   // waves per workgroup for one round
  return need <= 7 ? (int)need : kComputeWaves;
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
template <int NB>
int pick_edge_waves(int64_t R, int rb, int cus) {
  const int fixed = edge_compute_waves<NB>();
#ifdef BSMS_EXPERIMENTS
  if (getenv(NB >= 16 ? "BSMS_EDGE_CW16" : "BSMS_EDGE_CW") || getenv("BSMS_EDGE_CW_FIXED")) return fixed;
#endif
  const double slope = (NB >= 16 ? 0.25 : 0.53) * rb;
  const int64_t slots = int64_t(cus) * edge_resident<NB>(rb);
  auto cost_of = [&](int cw) {
    const int64_t tiles = ceil_div(R, int64_t(16) * rb * cw);
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

// Compute waves per workgroup of the bf16 edge chains (generic kernels, 16 rows per wave).  Round 4, same-box with the
// experiment build (profiles/r04_bfcw.sh): 7 waves against 4 -- airfoil batch 8 bf16 222.4 -> 230.1, bf16_nodes 231.5 -> 241.5,
// surface B=2 bf16 105.2 -> 110.9 / bf16_nodes 111.6 -> 118.0 steps/s (a workgroup streams the weights once per tile: 112 rows
// per pass instead of 64); a launch that fits one round of 64-row tiles keeps 4 (batch 1: 614 against 597 steps/s with 7).
template <int NB>
int bf_edge_waves(int64_t R, int cus) {
  static const int forced = knob("BSMS_BFEDGE_CW", 0);
  if (forced > 0) return forced;
  return R > int64_t(cus) * resident_per_cu<NB>() * 16 * kComputeWaves ? 7 : kComputeWaves;
}

template <int NB, int PL = kPL>
int max_ring() { return (int)std::min<size_t>(6, (size_t(160) * 1024 - Ring<NB, PL>::PRE_FLOATS * sizeof(float)) / (Ring<NB, PL>::CHF * sizeof(float))); }
template <int NB>
size_t ring_lds_max() { return Ring<NB>::lds_bytes(max_ring<NB>()); }

// THE launch shape of the edge and ring kernels: `cw` compute waves of `rows_per_wave` rows make a tile; persistent workgroups,
// `resident` per CU, stride over the tiles (`per_cu`: exactly one per CU, whatever the tile count -- the [x, x2] Linear of plan_fwd).
// Weight stream: loader waves and ring depth (Ring<NB, PL>; PL = 1: the one-plane chunks of the bf16 precision, whose ring may be
// deeper than the fp32 one at the same D and is sized as what it is).  A launch that fits ONE round of workgroups (at most one
// workgroup per CU: the coarse mesh levels, most node-level launches) has the CU's whole LDS and nothing to overlap its chunk
// latency with: deep ring (up to 6 slots = 5 chunks in flight) fed by two loader waves.  Anything larger keeps 3 slots so that two
// workgroups share a CU.  Limits: compute + loader waves <= 8; (nr - 2) x pieces per loader <= 63 (vmcnt field); ring + side
// tables <= 160 KB.
template <int NB, int PL>
void launch_shape(ChainLaunch& l, int64_t R, int rows_per_wave, int cw, int nload_default, int resident, bool per_cu, int cus) {
  static const int deep = knob("BSMS_RING_DEEP", 6), lone_nl = knob("BSMS_LONE_NL", 2), shared = knob("BSMS_RING", 3);
  l.cw = cw;
  l.ntiles = (int)ceil_div(R, rows_per_wave * cw);
  l.nload = std::max(1, std::min(nload_default, 8 - cw));
  l.nring = std::min(shared, max_ring<NB, PL>());
  if (per_cu || one_round(l.ntiles, cus)) {
    l.nload = std::max(l.nload, std::min(lone_nl, 8 - cw));
    l.nring = std::min(deep, max_ring<NB, PL>());
  }
  const int mine = (Ring<NB, PL>::PER + l.nload - 1) / l.nload;
  while (l.nring > 3 && (l.nring - 2) * mine > 63) --l.nring;
  l.grid = (unsigned)std::min<int64_t>(l.ntiles, int64_t(cus) * (per_cu ? 1 : resident));
  l.threads = (cw + l.nload) * 64;
  l.lds = Ring<NB, PL>::lds_bytes(l.nring);
  l.lds_max = ring_lds_max<NB>();
}
// ... of the generic ring kernels (16 rows per wave)
template <int NB>
void ring_shape(ChainLaunch& l, const ChainLaunchKey& k, int cw, bool per_cu, int cus) {
  l.family = CHAIN_RING;
  if (k.bf16) launch_shape<NB, 1>(l, k.R, 16, cw, chain_loader_waves(), resident_per_cu<NB>(), per_cu, cus);
  else launch_shape<NB, kPL>(l, k.R, 16, cw, chain_loader_waves(), resident_per_cu<NB>(), per_cu, cus);
}
// ... of the software-pipelined edge kernels (`rb` row blocks of 16 rows per wave)
template <int NB>
void edge_shape(ChainLaunch& l, const ChainLaunchKey& k, int rb, int cus) {
  l.family = CHAIN_EDGE;
  l.rb = rb;
  launch_shape<NB, kPL>(l, k.R, 16 * rb, pick_edge_waves<NB>(k.R, rb, cus), edge_loader_waves<NB>(), edge_resident<NB>(rb), false, cus);
}
inline void fs_shape(ChainLaunch& l, const ChainLaunchKey& k) {   // the feature-split kernels: one workgroup of 4 waves per 16 rows, static LDS
  l.family = CHAIN_FS;
  l.cw = 4;
  l.ntiles = (int)ceil_div(k.R, 16);
  l.grid = (unsigned)l.ntiles;
  l.threads = 256;
}

// Which variants are built (each is a large unrolled kernel: only the combinations the path uses): plan_* set a flag, and the launch
// path names the instantiation, under the same condition
constexpr bool has_edge_kernels(int NB) { return NB == 8 || NB == 16; }
constexpr int edge_rb_max(int NB) { return NB == 8 ? 2 : 1; }   // two row blocks per wave are built at D = 128 only
constexpr bool has_lone(int NB) { return NB >= 8; }             // D = 96 has no single-round build: its single-round launches stay on the ring kernel
constexpr bool has_fs_fwd(int NB, int IN) { return NB == 8 && (IN == IN_ROWS || IN == IN_ROWS2 || IN == IN_SMALL); }
constexpr bool has_fs_bwd(int NB, int GIN) { return NB == 8 && (GIN == G_ROWS_LN || GIN == G_SMALL); }
constexpr bool has_timing(int NB, int IN) { return NB == 8 && IN == IN_EDGE; }   // the only production instantiation with stamps
constexpr bool has_bf16_fwd(int NB, int IN, int OUT) { return (NB == 8 || NB == 16) && (IN == IN_EDGE || IN == IN_ROWS2) && OUT == OUT_LN; }   // edge MLP (BSMS_BF16), node MLP (BSMS_BF16_NODES)
constexpr bool has_bf16_bwd(int NB, int GIN, int FIRST) { return (NB == 8 || NB == 16) && ((GIN == G_EDGE_LN && FIRST == F_NONE) || (GIN == G_ROWS_LN && FIRST == F_HEADS2)); }

inline ChainLaunchKey key_of(const ChainFwdArgs& a) {   // (after wseq / nseq are built)
  ChainLaunchKey k{};
  k.R = a.R; k.nstage = a.nstage; k.nseq = a.nseq; k.bf16 = a.bf16 != 0; k.store_mode = a.store_mode; k.timing = a.timing != nullptr;
  k.resid = a.resid || a.resid2;
  int set = a.store_in != nullptr, all = 1;
  for (int l = 0; l + 1 < std::min(a.nstage, kMaxStages); ++l, ++all) set += a.store[l] != nullptr;
  k.act_stores = set == 0 ? CHAIN_STORES_NONE : set == all ? CHAIN_STORES_ALL : CHAIN_STORES_MIXED;
  return k;
}
inline ChainLaunchKey key_of(const ChainBwdArgs& a) {
  ChainLaunchKey k{};
  k.R = a.R; k.nstage = a.nstage; k.nseq = a.nseq; k.bf16 = a.bf16 != 0; k.store_mode = a.store_mode;
  const int n = std::max(0, std::min(a.nstage, kMaxStages));   // (the entries bound nstage; the key never reads past the tables)
  k.glast = a.gstore[n] != nullptr;
  int set = 0;
  k.masks = 1;
  for (int q = 0; q < n; ++q) { set += a.gstore[q] != nullptr; k.masks &= a.mask[q] != nullptr; }
  k.gstores = set == 0 ? CHAIN_STORES_NONE : set == n ? CHAIN_STORES_ALL : CHAIN_STORES_MIXED;
  return k;
}

// Which kernel runs a forward chain, first match wins.
template <int NB, int IN, int OUT>
ChainLaunch plan_fwd(const ChainLaunchKey& k, int cus) {
  ChainLaunch l{};
  l.what = "chain_fwd";
  // 1. the pipelined edge kernel: NB = 8 / 16, the fp32 edge MLP in its production configuration only (activation stores all kept
  //    or none); anything else stays on k_chain_fwd
  if constexpr (has_edge_kernels(NB) && IN == IN_EDGE && OUT == OUT_LN) {
    if (!k.bf16 && k.nstage >= 1 && k.store_mode == 1 && !k.resid && edge_rb_mode() != 0 && k.R < (int64_t(1) << 31) &&
        k.act_stores != CHAIN_STORES_MIXED) {
      // Measured per level (profiles/r02_edge_levels.md): with several tiles per workgroup two workgroups per CU of one row
      // block per wave win the forward (the random row gathers of one hide under the other's MFMA stages); a launch that
      // fits one round of workgroups is faster with two row blocks per wave, and so is the whole backward (its loads are
      // sequential or local).  Below half a round of 128-row tiles the narrow tile keeps more CUs busy.
      const int64_t rows1 = 16 * edge_compute_waves<NB>();   // rows of a tile with one row block per wave
      bool big = edge_rb_max(NB) == 2 && k.R >= cus * rows1 && one_round(ceil_div(k.R, rows1), int64_t(cus) * edge_resident<NB>(1));
      if (edge_rb_mode() > 0) big = edge_rb_max(NB) == 2 && edge_rb_mode() == 2;
      l.what = "edge_fwd";
      edge_shape<NB>(l, k, big ? 2 : 1, cus);
      l.save = k.act_stores == CHAIN_STORES_ALL;
      static const int lone = knob("BSMS_EDGE_LONE", 1);
      l.lone = lone && one_round(l.ntiles, cus) && !k.timing;   // one round of workgroups: the variant that passes the chunk barrier early (stage_rb<LONE>)
      l.build = l.lone ? "single-round build" : nullptr;
      return l;
    }
  }
  // 2. the feature-split kernel: NB = 8, fp32, small launches (at most kFsMaxRows rows)
  if constexpr (has_fs_fwd(NB, IN)) {
    static const int fs_rows = knob("BSMS_FS_ROWS", kFsMaxRows);
    if (!k.bf16 && k.R <= fs_rows && k.nseq >= 1 && k.nseq <= kMaxStages + 1) { fs_shape(l, k); return l; }
  }
  // ---- the ring kernel and its variants
  int cw = (IN == IN_EDGE) ? bf_edge_waves<NB>(k.R, cus) : chain_compute_waves<NB>(k.R, cus);
  // One Linear over [x, x2] added into y (the input gradient through the two edge projections, gmp.hip): three more dependent row
  // loads per tile than a plain chain and only two packs of MFMAs to hide them under.  The single-round build keeps x2 in registers
  // (one round trip instead of three) -- so this launch always takes it, one 7-wave workgroup per CU striding over the tiles
  // (round 6, profiles/r06_rows2.txt; fp32 OUT_PLAIN: it reaches rule 5 below).
  bool rows2_lone = false;
  if constexpr (NB == 8 && IN == IN_ROWS2 && OUT == OUT_PLAIN) {
    static const int on = knob("BSMS_ROWS2_LONE", 1);
    rows2_lone = on && !k.bf16 && k.nstage == 1 && !one_round(ceil_div(k.R, 16 * cw), cus);
    if (rows2_lone) cw = 7;
  }
  ring_shape<NB>(l, k, cw, rows2_lone, cus);
  // 3. the TIMING variant when the caller asks for stamps: the NB = 8 edge chain ...
  if constexpr (has_timing(NB, IN)) {
    if (k.timing) { l.timing = true; l.build = "timing build"; return l; }
  }
#ifdef BSMS_EXPERIMENTS
  if constexpr (NB == 8 && IN == IN_ROWS2 && OUT == OUT_LN) {   // ... experiment builds: phase stamps of a single-round node chain (profiles/lone_timeline.py)
    if (k.timing && one_round(l.ntiles, cus)) { l.timing = l.lone = true; l.build = "timing build"; return l; }
  }
#endif
  // 4. the bf16 variant: edge MLP (BSMS_BF16) and node MLP (BSMS_BF16_NODES) at NB = 8 / 16; bf16 anywhere else is an error
  if (k.bf16) {
    if constexpr (has_bf16_fwd(NB, IN, OUT)) { l.bf16 = true; l.build = "bf16 build"; }
    else l.family = CHAIN_UNBUILT;   // the launch path and the query refuse it (chain_refuse)
    return l;
  }
  // 5. the single-round (LONE) variant, NB >= 8, when the launch fits one workgroup per CU (a single wave per SIMD: the variant that
  //    prefetches its fragments, mfma_stage) or is the [x, x2] Linear above
  if constexpr (has_lone(NB)) {
    if (one_round(l.ntiles, cus) || rows2_lone) { l.lone = true; l.build = "single-round build"; return l; }
  }
  return l;   // 6. the ring kernel
}

// Which kernel runs a backward chain, first match wins.
template <int NB, int GIN, int FIRST>
ChainLaunch plan_bwd(const ChainLaunchKey& k, int cus) {
  ChainLaunch l{};
  l.what = "chain_bwd";
  // 1. the feature-split kernel: NB = 8, fp32, small launches (at most kFsMaxRowsBwd rows)
  if constexpr (has_fs_bwd(NB, GIN)) {
    static const int fs_rows = knob("BSMS_FS_ROWS_BWD", kFsMaxRowsBwd);
    if (!k.bf16 && k.R <= fs_rows && k.nseq >= 1) { fs_shape(l, k); return l; }
  }
  // 2. the pipelined edge kernel: NB = 8 / 16, the fp32 edge MLP in its production configuration.  The layer gradients
  //    gstore[0 .. nstage-1]: all kept, or none (a frozen edge MLP: the no-store build; tile, ring and single-round choices are the
  //    storing launch's).  The last gradient, gstore[nstage], always has a reader.
  if constexpr (has_edge_kernels(NB) && GIN == G_EDGE_LN && FIRST == F_NONE) {
    if (!k.bf16 && k.nstage >= 1 && k.store_mode == 1 && edge_rb_mode() != 0 && k.R < (int64_t(1) << 31) && k.glast &&
        k.gstores != CHAIN_STORES_MIXED && k.masks) {
      bool big = edge_rb_max(NB) == 2 && k.R >= int64_t(cus) * 16 * edge_compute_waves<NB>();   // see plan_fwd
      if (edge_rb_mode() > 0) big = edge_rb_max(NB) == 2 && edge_rb_mode() == 2;
      l.what = "edge_bwd";
      edge_shape<NB>(l, k, big ? 2 : 1, cus);
      l.store = k.gstores == CHAIN_STORES_ALL;
      static const int lone = knob("BSMS_EDGE_LONE", 1);
      l.lone = lone && one_round(l.ntiles, cus);   // see plan_fwd
      l.build = l.lone ? (l.store ? "single-round build" : "single-round no-store build") : (l.store ? nullptr : "no-store build");
      return l;
    }
  }
  // ---- the ring kernel and its variants
  ring_shape<NB>(l, k, (GIN == G_EDGE_LN) ? bf_edge_waves<NB>(k.R, cus) : chain_compute_waves<NB>(k.R, cus), false, cus);
  // 3. the bf16 variant: edge MLP; node MLP of BSMS_BF16_NODES; NB = 8 / 16; bf16 anywhere else is an error
  if (k.bf16) {
    if constexpr (has_bf16_bwd(NB, GIN, FIRST)) { l.bf16 = true; l.build = GIN == G_EDGE_LN ? "bf16 build" : "bf16 node build"; }
    else l.family = CHAIN_UNBUILT;
    return l;
  }
  // 4. the single-round (LONE) variant, NB >= 8, when the launch fits one workgroup per CU (see plan_fwd)
  if constexpr (has_lone(NB)) {
    if (one_round(l.ntiles, cus)) { l.lone = true; l.build = "single-round build"; return l; }
  }
  return l;   // 5. the ring kernel
}

inline int chain_refuse(const ChainLaunch& l) {
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "%s: bf16 precision is built for the edge and node MLPs at D = 128 / 256 only", l.what);
}

// From the record to the instantiation
#define BSMS_RUN(...) return launch_dyn_lds<__VA_ARGS__>(l.what, l.build, l.grid, l.threads, l.lds, l.lds_max, a, s)
template <int NB, int RB>
int run_edge(const ChainLaunch& l, const ChainFwdArgs& a, hipStream_t s) {
  if (l.save && l.lone) BSMS_RUN(k_edge_fwd<NB, RB, 1, true>);
  if (l.save) BSMS_RUN(k_edge_fwd<NB, RB, 1>);
  if (l.lone) BSMS_RUN(k_edge_fwd<NB, RB, 0, true>);
  BSMS_RUN(k_edge_fwd<NB, RB, 0>);
}
template <int NB, int RB>
int run_edge(const ChainLaunch& l, const ChainBwdArgs& a, hipStream_t s) {
  if (l.store && l.lone) BSMS_RUN(k_edge_bwd<NB, RB, true, true>);
  if (l.store) BSMS_RUN(k_edge_bwd<NB, RB, false, true>);
  if (l.lone) BSMS_RUN(k_edge_bwd<NB, RB, true, false>);
  BSMS_RUN(k_edge_bwd<NB, RB, false, false>);
}
template <int NB, int IN, int OUT>
int launch_fwd_t(const ChainFwdArgs& a0, hipStream_t s) {
  ChainFwdArgs a = a0;
  a.nseq = 0;
  for (int l = 0; l < a.nstage; ++l) {  // the loader follows exactly the compute waves' stage order
    a.wseq[a.nseq++] = a.wp[l];
    if (IN == IN_ROWS2 && l == 0) a.wseq[a.nseq++] = a.wp0b;
  }
  const ChainLaunch l = plan_fwd<NB, IN, OUT>(key_of(a), device_cu_count());
  a.ntiles = l.ntiles; a.nload = l.nload; a.nring = l.nring;
  if (l.family == CHAIN_UNBUILT) return chain_refuse(l);
  if constexpr (has_fs_fwd(NB, IN)) {
    if (l.family == CHAIN_FS) {
      hipLaunchKernelGGL((k_fs_fwd<IN, OUT>), dim3(l.grid), dim3(l.threads), 0, s, a);
      BSMS_LAUNCH_CHECK();
      return BSMS_OK;
    }
  }
  if constexpr (has_edge_kernels(NB) && IN == IN_EDGE && OUT == OUT_LN) {
    if (l.family == CHAIN_EDGE) return l.rb == 2 ? run_edge<NB, edge_rb_max(NB)>(l, a, s) : run_edge<NB, 1>(l, a, s);
  }
  if constexpr (has_timing(NB, IN)) {
    if (l.timing) BSMS_RUN(k_chain_fwd<NB, IN, OUT, true>);
  }
#ifdef BSMS_EXPERIMENTS
  if constexpr (NB == 8 && IN == IN_ROWS2 && OUT == OUT_LN) {
    if (l.timing) BSMS_RUN(k_chain_fwd<NB, IN, OUT, true, false, true>);
  }
#endif
  if constexpr (has_bf16_fwd(NB, IN, OUT)) {
    if (l.bf16) BSMS_RUN(k_chain_fwd<NB, IN, OUT, false, true>);
  }
  if constexpr (has_lone(NB)) {
    if (l.lone) BSMS_RUN(k_chain_fwd<NB, IN, OUT, false, false, true>);
  }
  BSMS_RUN(k_chain_fwd<NB, IN, OUT>);
}

template <int NB, int GIN, int FIRST>
int launch_bwd_t(const ChainBwdArgs& a0, hipStream_t s) {
  ChainBwdArgs a = a0;
  a.nseq = 0;
  for (int k = 0; k < a.nstage; ++k) a.wseq[a.nseq++] = a.wpt[k];
  if (FIRST != F_NONE) a.wseq[a.nseq++] = a.wh0;
  if (FIRST == F_HEADS2) a.wseq[a.nseq++] = a.wh1;
  const ChainLaunch l = plan_bwd<NB, GIN, FIRST>(key_of(a), device_cu_count());
  a.ntiles = l.ntiles; a.nload = l.nload; a.nring = l.nring;
  if (l.family == CHAIN_UNBUILT) return chain_refuse(l);
  if constexpr (has_fs_bwd(NB, GIN)) {
    if (l.family == CHAIN_FS) {
      hipLaunchKernelGGL((k_fs_bwd<GIN, FIRST>), dim3(l.grid), dim3(l.threads), 0, s, a);
      BSMS_LAUNCH_CHECK();
      return BSMS_OK;
    }
  }
  if constexpr (has_edge_kernels(NB) && GIN == G_EDGE_LN && FIRST == F_NONE) {
    if (l.family == CHAIN_EDGE) return l.rb == 2 ? run_edge<NB, edge_rb_max(NB)>(l, a, s) : run_edge<NB, 1>(l, a, s);
  }
  if constexpr (has_bf16_bwd(NB, GIN, FIRST)) {
    if (l.bf16) BSMS_RUN(k_chain_bwd<NB, GIN, FIRST, true>);
  }
  if constexpr (has_lone(NB)) {
    if (l.lone) BSMS_RUN(k_chain_bwd<NB, GIN, FIRST, false, true>);
  }
  BSMS_RUN(k_chain_bwd<NB, GIN, FIRST>);
}
#undef BSMS_RUN

// The mode pairs that are built: f(in, out) / f(gin, first) gets them as integral constants
template <class F>
int with_fwd_modes(int in_mode, int out_mode, F&& f) {
#define BSMS_FWD(I, O) \
  if (in_mode == I && out_mode == O) return f(std::integral_constant<int, I>{}, std::integral_constant<int, O>{})
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
template <class F>
int with_bwd_modes(int gin, int first, F&& f) {
#define BSMS_BWD(G, F_) \
  if (gin == G && first == F_) return f(std::integral_constant<int, G>{}, std::integral_constant<int, F_>{})
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
int launch_chain_fwd_nb(int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s) {
  return with_fwd_modes(in_mode, out_mode, [&](auto i, auto o) { return launch_fwd_t<NB, decltype(i)::value, decltype(o)::value>(a, s); });
}
template <int NB>
int launch_chain_bwd_nb(int gin, int first, const ChainBwdArgs& a, hipStream_t s) {
  return with_bwd_modes(gin, first, [&](auto g, auto f) { return launch_bwd_t<NB, decltype(g)::value, decltype(f)::value>(a, s); });
}
template <int NB>
int chain_launch_query_nb(int backward, int mode_a, int mode_b, const ChainLaunchKey& k, int cus, ChainLaunch* out) {
  const int rc = backward ? with_bwd_modes(mode_a, mode_b, [&](auto g, auto f) { *out = plan_bwd<NB, decltype(g)::value, decltype(f)::value>(k, cus); return int(BSMS_OK); })
                          : with_fwd_modes(mode_a, mode_b, [&](auto i, auto o) { *out = plan_fwd<NB, decltype(i)::value, decltype(o)::value>(k, cus); return int(BSMS_OK); });
  return rc || out->family != CHAIN_UNBUILT ? rc : chain_refuse(*out);
}
}  // namespace bsms
