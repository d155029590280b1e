// Host-side pieces shared by the orchestration units (gmp.hip, mlp.hip, bsgmp.hip): the bump allocator behind every buffer layout,
// the experiment switches and the pack-table helpers.  No kernel translation unit includes this header.
#pragma once
#include "chain.h"

namespace bsms {

struct Carver {  // identical walk for size queries (base == nullptr) and real buffers
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(reinterpret_cast<char*>(b)) {}
  float* take(size_t nfloat) { return reinterpret_cast<float*>(take_bytes(nfloat * sizeof(float))); }
  char* take_bytes(size_t n) {
    char* p = base ? base + off : nullptr;
    off += align_up(n);
    return p;
  }
};

// fp32: every multiple of 32 (the K block of a weight chunk: an even number of 16-feature MFMA blocks) up to 256; wider
// rows do not fit the chain kernels' LDS ring (chain.hip: max_ring).  The bf16 precisions: 128 / 256 (GmpShape::check).
inline bool supported_D(int64_t D) { return D % 32 == 0 && D >= 32 && D <= 256; }

// the 2 (H + 1) gradient entries of one MLP: 1 all there, 0 all null (the MLP is frozen), -1 some of each
inline int grads_state(float* const* g, int n) {
  if (!g) return 0;
  int live = 0;
  for (int i = 0; i < n; ++i) live += g[i] != nullptr;
  return live == n ? 1 : (live == 0 ? 0 : -1);
}

// Experiment switches exist only in a library built with -DBSMS_EXPERIMENTS (BSMS_EXPERIMENTS=1 python
// bsms-gnn_amd/build.py; used by profiles/experiments.py, tile_timeline.py, ab.sh): the production build has no
// environment variable or exported setter that could change kernel behaviour.  The bits of BSMS_DEBUG_FLAGS /
// bsms_debug_set_flags (bit 4 is not in use):
enum DebugFlag : int {
  DBG_NO_ACT_STORES = 1 << 0,     // edge forward: none of the activation stores the backward needs (timing runs only)
  DBG_PLAIN_STORES = 1 << 1,      // edge chains: plain instead of non-temporal activation / layer-gradient stores
  DBG_NT_OUTPUT = 1 << 2,         // edge forward: the final y goes out with non-temporal stores too
  DBG_NO_SIDE_LANES = 1 << 3,     // backward: no side lanes, every launch on the caller's stream
  DBG_NO_LANE2 = 1 << 5,          // backward: no second side lane (its launches stay on the caller's stream)
  DBG_NO_SIGN_BITS = 1 << 6,      // edge forward: saved activations without their sign bits
  DBG_UNPAIRED_STORES = 1 << 7,   // edge chains: unpaired 64-byte store pieces
  DBG_BWD_STORE_MODE2 = 1 << 8,   // edge backward: layer-gradient store mode 2
  DBG_TIME_NODE_CHAIN = 1 << 9,   // the stamp buffer goes to the node forward chain instead of the edge one
  DBG_NO_EDGE_WGRAD = 1 << 10,    // backward: the weight-gradient jobs of edge Linears 1..H are dropped
  DBG_NO_GRAD_STREAM = 1 << 11,   // edge backward: gE[1..H] are not streamed to HBM (with bits 0 and 10: the traffic a fused backward would not have)
  DBG_NO_PREPACK = 1 << 12,       // no prepack kernel (the ceiling of the pack group, profiles/pack_group_rates.txt); see prepack_table
};
#ifdef BSMS_EXPERIMENTS
extern int g_debug_flags;              // gmp.hip: BSMS_DEBUG_FLAGS, bsms_debug_set_flags
extern unsigned long long* g_timing;   // gmp.hip: bsms_debug_set_timing
extern const int g_node_bf3;           // gmp.hip: BSMS_NODE_BF3 (see there)
#else
constexpr int g_debug_flags = 0;
constexpr unsigned long long* g_timing = nullptr;
constexpr int g_node_bf3 = 1;
#endif
inline bool dbg(DebugFlag f) { return (g_debug_flags & f) != 0; }

// The per-call prepack of one table.  Experiment builds, DBG_NO_PREPACK: no prepack kernel -- the packs of an earlier step stay where
// they are, stale but valid -- while the bound slots are still cleared.  The bit skips EVERY prepack from the moment it is set: set it
// with bsms_debug_set_flags after a first step has written the packs, never through BSMS_DEBUG_FLAGS at start-up (the packs would
// never be written).
inline int prepack_table(const PackTable& t, hipStream_t s) {
  if (dbg(DBG_NO_PREPACK)) {
    if (t.zero) BSMS_HIP_CHECK(hipMemsetAsync(t.zero, 0, size_t(kBoundSlots) * kBoundWidth * sizeof(float), s));
    return BSMS_OK;
  }
  return launch_prepack(t, s);
}

inline void add_pack(PackTable& t, const float* W, int ld, int row0, int col0, int N, int K, int kind, float* dst, const float* bias) {
  PackDesc& d = t.d[t.n++];
  d.W = W; d.bias = bias; d.dst = dst; d.ld = ld; d.row0 = row0; d.col0 = col0; d.N = N; d.K = K; d.kind = kind;
}

}  // namespace bsms
