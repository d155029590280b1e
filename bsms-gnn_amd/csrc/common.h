// Shared host-side helpers for libbsms_hip.so (error reporting, plan struct, launch geometry).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/bsms_hip.h"

namespace bsms {

void set_error(const char* fmt, ...);

#define BSMS_FAIL(code, ...)        \
  do {                              \
    ::bsms::set_error(__VA_ARGS__); \
    return (code);                  \
  } while (0)

#define BSMS_REQUIRE(cond, code, ...)         \
  do {                                        \
    if (!(cond)) BSMS_FAIL(code, __VA_ARGS__); \
  } while (0)

#define BSMS_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) BSMS_FAIL(BSMS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define BSMS_LAUNCH_CHECK()                                                                  \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) BSMS_FAIL(BSMS_E_HIP, "kernel launch: %s", hipGetErrorString(e_)); \
  } while (0)

inline hipStream_t as_stream(bsms_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Internal fork/join helper: one non-blocking side stream + two events per device, created lazily and kept for
// the life of the process.  A fork makes the side stream wait for everything queued on `main` so far; a join makes
// `main` wait for the side stream.  Stream-wait-event takes a snapshot, so the events are safely reused per call,
// and both operations are legal inside HIP-graph capture.
struct SideLane {
  hipStream_t stream = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  hipEvent_t done_ev[2] = {nullptr, nullptr};   // "everything queued on the lane up to here has run", two slots
  bool uncovered[2] = {false, false};           // the slot has been marked and neither waited for nor covered by a chained mark since
};
constexpr int kSideLanes = 2;
int side_lane(SideLane** out, int which, hipStream_t caller);   // for the current device; `which` < kSideLanes; `caller`: see plan.hip (capture)
int side_fork(SideLane* lane, hipStream_t main);     // side waits for main
int side_join(SideLane* lane, hipStream_t main);     // main waits for side
// Deferred join: side_mark records "the lane's work so far" into slot 0/1; side_wait_mark makes `main` wait for what
// that slot recorded last (callers only wait on slots they marked themselves: a stale record from an earlier call
// would be an event from outside an ongoing graph capture).  The U-Net backward lets the weight gradients of block k run
// under the gradient chain of block k+1 and only waits for them before block k+2 reuses their scratch (bsgmp.hip).
int side_mark(SideLane* lane, int slot);
int side_wait_mark(SideLane* lane, int slot, hipStream_t main);
int side_mark_chain(SideLane* a, SideLane* b, int slot);   // b's mark covers a's: wait for b only
// side_wait_mark, but only if the lane's `slot` holds an OPEN mark: one that no wait and no later chained mark covers yet (a deferred
// bsms_mlp_bwd_ex marks lane 0 alone; the U-Net blocks behind it normally cover that mark -- unless they are all frozen and run no
// lane).  Test and wait are one critical section.  SideLane::uncovered is HOST state: it follows the order of the calls on the host,
// not stream order, and is shared by every caller of the device like the lanes themselves.  A call that fails between a mark and its
// join leaves the flag set; the next bsms_side_lanes_join then waits for that (recorded) event once more, which is harmless.
int side_wait_open_mark(SideLane* lane, int slot, hipStream_t main);
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int kMaxC = 8;   // state / field channels of a row, in every library: what the kernels hold in registers per row

// Per-DEVICE launch state: hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the device that is current
// when it is called, and the CU count is a property of that device -- a process driving several devices (not the one-process-per-GPU
// layout of dp.py, but legal at the C ABI) must not reuse the first device's answers.  Both are cached per device index; the
// races are benign (two threads may set the same attribute / read the same count twice).
constexpr int kMaxDevices = 64;
inline int current_device_index() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  return dev >= 0 && dev < kMaxDevices ? dev : 0;
}
struct DynLdsAttr {
  int state[kMaxDevices] = {};   // 0: not asked on this device yet; 1 + hipError_t afterwards
  hipError_t ensure(const void* fn, int bytes) {
    int& st = state[current_device_index()];
    if (st == 0) st = 1 + int(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return hipError_t(st - 1);
  }
};
#ifdef __HIPCC__
// One launch of a kernel that takes dynamic LDS beyond the default limit.  The first launch of a kernel on a device raises its
// LDS limit to `lds_max` (the most any launch of it asks for; DynLdsAttr keeps one answer per kernel and device), so only
// kernels that run get the attribute.  `what` names the launcher and `build` the variant (null: the plain kernel) in the error text.
template <auto Kernel, class Args>
int launch_dyn_lds(const char* what, const char* build, unsigned grid, unsigned threads, size_t lds, size_t lds_max, const Args& a, hipStream_t s) {
  static DynLdsAttr attr_dev;
  const hipError_t attr = attr_dev.ensure(reinterpret_cast<const void*>(Kernel), (int)lds_max);
  if (build) BSMS_REQUIRE(attr == hipSuccess, BSMS_E_HIP, "%s: cannot reserve %zu bytes of LDS (%s)", what, lds_max, build);
  BSMS_REQUIRE(attr == hipSuccess, BSMS_E_HIP, "%s: cannot reserve %zu bytes of LDS", what, lds_max);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, s, a);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}
// std_with_epsilon() of a normaliser from its statistics, op for op (normalizer.py:40-52): sim.hip and errsum.hip, both compiled
// with -ffp-contract=off
__device__ __forceinline__ double std_eps(double mean, double meansq, double eps) {
  double s = sqrt(meansq - mean * mean);       // torch: sqrt(E2 - mean ** 2); pow(x, 2) is x * x
  if (isnan(s)) s = 0.0;                       // nan_to_num
  else if (isinf(s)) s = s > 0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
  return s > eps ? s : eps;                    // torch.max(std, eps)
}
#endif
inline int device_cu_count() {
  static int cus[kMaxDevices] = {};
  const int dev = current_device_index();
  if (cus[dev] <= 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) { (void)hipGetLastError(); v = 256; }
    cus[dev] = v;
  }
  return cus[dev];
}

// ---- internal entry points shared between translation units (not part of the C ABI)
// rowsum.hip: bsms_edge_conv + fused addend
int edge_conv_add(const bsms_plan* p, const float* x, int64_t B, int64_t D, const float* ew, int aggregating, int pooled,
                  float* out, const float* addend, hipStream_t stream);
// posgrad.hip: the position gradient of one GMP block from its first edge gradient gE[0] (plan order; bf16 rows when
// `g_bf16`) and the saved fiber rows; `scratch` holds pos_edge_scratch_bytes(B, E, p).  grad_pos [B,N,p] (pos_bstride != 0)
// or [N,p] (0, summed over the batch) is overwritten, or added to when `accumulate`.
size_t pos_edge_scratch_bytes(int64_t B, int64_t E, int64_t p);
int gmp_pos_grad(const bsms_plan* plan, const void* gE0, bool g_bf16, const float* fiber, const float* W0_edge, int64_t B,
                 int64_t D, int64_t p, int64_t pos_bstride, float* grad_pos, bool accumulate, float* scratch, hipStream_t s);
// out [R,K] = G [R,D] . W[:, 0:K] (W [D,K] row-major): the input gradient of an MLP whose first Linear is narrow (K <= 8)
int narrow_input_grad(const float* G, int64_t R, int64_t D, const float* W, int K, float* out, hipStream_t s);
// posgrad.hip: db = column sums of the LayerNorm backward of dy, in fp32 (D = 128 / 256); `part`: ln_bias_grad_work_floats(D) floats of scratch
size_t ln_bias_grad_work_floats(int64_t D);
int ln_bias_grad(const float* dy, const float* yln, const float* rstd, int64_t R, int64_t D, float* part, float* db, hipStream_t s);
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// bsms_plan_concat (plan.hip: host side; rowsum.hip: the kernel -- plan.hip is also compiled as plain C++ for the sanitizer build):
// the index blocks of up to kCatParts plans copied into the blocks of their block-diagonal union, node / edge / pooled offsets added
constexpr size_t kIdxAlign = 64;   // int32 elements (256 bytes) between the arrays of a plan's index block
// The padding words between the arrays are written (0; -1 behind ids / inv) in a plan bsms_plan_create / bsms_plan_set_pool uploaded and UNDEFINED in one
// bsms_plan_concat built (its blocks come from the recycling pool and the kernel writes the logical words only): no kernel reads an
// index array past its logical end (tests/test_hip_plan_concat.py builds unions in recycled blocks and runs the row sums on them).
#ifdef __HIPCC__
#define BSMS_HD __host__ __device__
#else
#define BSMS_HD
#endif
BSMS_HD inline size_t idx_pad(size_t n) { return (n + kIdxAlign - 1) / kIdxAlign * kIdxAlign; }
// THE layout of a plan's two index blocks (the arrays: see bsms_plan below), the one statement every reader and writer takes its
// offsets from -- the host builds and the plan's own pointers (plan.hip), the union's allocations and k_plan_concat (rowsum.hip).
// Word offsets of the arrays, each array padded to kIdxAlign, in block order; `words`: the block's length.
struct MainLayout { size_t rowptr, t_rowptr, src, dst, perm, t_dst, t_eid, t_pos, words; };
struct PoolLayout { size_t ids, inv, k_rowptr, k_src, k_eid, p_rowptr, p_src, p_eid, k_w, p_w, words; };
BSMS_HD inline MainLayout main_layout(size_t N, size_t E) {
  const size_t nN = idx_pad(N + 1), nE = idx_pad(E);
  MainLayout l;
  l.rowptr = 0; l.t_rowptr = l.rowptr + nN; l.src = l.t_rowptr + nN; l.dst = l.src + nE; l.perm = l.dst + nE;
  l.t_dst = l.perm + nE; l.t_eid = l.t_dst + nE; l.t_pos = l.t_eid + nE; l.words = l.t_pos + nE;
  return l;
}
BSMS_HD inline PoolLayout pool_layout(size_t N, size_t Nk, size_t Ek, size_t Ep) {
  const size_t nEk = idx_pad(Ek), nEp = idx_pad(Ep);
  PoolLayout l;
  l.ids = 0; l.inv = l.ids + idx_pad(Nk); l.k_rowptr = l.inv + idx_pad(N); l.k_src = l.k_rowptr + idx_pad(Nk + 1); l.k_eid = l.k_src + nEk;
  l.p_rowptr = l.k_eid + nEk; l.p_src = l.p_rowptr + idx_pad(N + 1); l.p_eid = l.p_src + nEp; l.k_w = l.p_eid + nEp; l.p_w = l.k_w + nEk;
  l.words = l.p_w + nEp;
  return l;
}
// the arrays of a block at `base` (I: int32_t or const int32_t; k_w / p_w are float words, given as words here)
template <class I> struct MainPtrs { I *rowptr, *t_rowptr, *src, *dst, *perm, *t_dst, *t_eid, *t_pos; };
template <class I> struct PoolPtrs { I *ids, *inv, *k_rowptr, *k_src, *k_eid, *p_rowptr, *p_src, *p_eid, *k_w, *p_w; };
template <class I> BSMS_HD inline MainPtrs<I> main_ptrs(I* base, size_t N, size_t E) {
  const MainLayout l = main_layout(N, E);
  return {base + l.rowptr, base + l.t_rowptr, base + l.src, base + l.dst, base + l.perm, base + l.t_dst, base + l.t_eid, base + l.t_pos};
}
template <class I> BSMS_HD inline PoolPtrs<I> pool_ptrs(I* base, size_t N, size_t Nk, size_t Ek, size_t Ep) {
  const PoolLayout l = pool_layout(N, Nk, Ek, Ep);
  return {base + l.ids, base + l.inv, base + l.k_rowptr, base + l.k_src, base + l.k_eid, base + l.p_rowptr, base + l.p_src, base + l.p_eid,
          base + l.k_w, base + l.p_w};
}
constexpr int kCatParts = 16;
struct CatPart {
  const int32_t *blk, *pool;               // the part's two device blocks (pool: null when no part has one)
  int32_t N, E, Nk, Ek, Ep;                // its sizes ...
  int32_t n_off, e_off, k_off, ek_off, ep_off;   // ... and where it starts in the union
};
struct CatArgs {
  CatPart part[kCatParts];
  int nparts;
  int32_t *out_blk, *out_pool;             // blocks of the union, laid out for (N, E, Nk, Ek, Ep) below
  int32_t N, E, Nk, Ek, Ep;
  int has_w;                               // copy the gathered edge weights k_w / p_w too (every part is bound)
  int64_t* coo_out;                        // nullable: [2, E] int64 edge list of the union in the CALLER's edge order
  int64_t* ids_out;                        // nullable: [Nk] int64 kept ids of the union
};
int launch_plan_concat(const CatArgs& a, hipStream_t s) __attribute__((weak));   // rowsum.hip (absent from the host-only sanitizer library)

}  // namespace bsms

// One mesh level in HBM.  All arrays int32, owned by the plan.
//   dst-sorted CSR ("plan order" q = 0..E-1, stable w.r.t. the caller's edge order):
//     rowptr[N+1]; src[q], dst[q] node ids; perm[q] = caller's edge id of plan slot q
//   src-sorted transpose (slot t = 0..E-1, stable):
//     t_rowptr[N+1]; t_dst[t] target node; t_eid[t] caller's edge id; t_pos[t] plan slot q
//   pooling (optional): ids[Nk] kept fine ids (ascending), inv[N] fine -> coarse or -1
struct bsms_plan {
  int64_t N = 0, E = 0, Nk = 0;
  int64_t min_out_degree = 0, max_source = -1;
  int64_t max_in_degree = 0, max_out_degree = 0;   // bound the scatter sums of a bounded tensor (wgrad.hip: operand scales)
  int32_t *rowptr = nullptr, *src = nullptr, *dst = nullptr, *perm = nullptr;
  int32_t *t_rowptr = nullptr, *t_dst = nullptr, *t_eid = nullptr, *t_pos = nullptr;
  int32_t *ids = nullptr, *inv = nullptr;
  // pooled transitions, compacted (built by bsms_plan_set_pool; plan.hip).  restrict: CSR over the KEPT rows only,
  //   k_rowptr[Nk+1]; k_src[q] fine source node; k_eid[q] caller's edge id -- the slots of kept row ids[k] in plan order.
  // prolong: CSR over ALL fine rows by source with the slots whose target is not kept dropped (they add nothing),
  //   p_rowptr[N+1]; p_src[t] COARSE row of the target (inv[t_dst]); p_eid[t] caller's edge id.
  // k_w / p_w: the edge weights in those slot orders, filled by bsms_plan_bind_edge_weights (w_bound = the `ew` they were
  // gathered from): a transition kernel then reads index + weight as two coalesced streams instead of chasing
  // rows -> rowptr -> (xidx, widx) -> (xmap, w) through four dependent round trips.
  int32_t *k_rowptr = nullptr, *k_src = nullptr, *k_eid = nullptr, *p_rowptr = nullptr, *p_src = nullptr, *p_eid = nullptr;
  float *k_w = nullptr, *p_w = nullptr;
  int64_t Ek = 0, Ep = 0;
  const float* w_bound = nullptr;
  std::vector<int32_t> host;                         // host copy of the index block (set_pool derives the compact lists from it); released by the first
                                                     // bsms_plan_set_pool -- a later re-pool reads the block back from the device (host_words int32)
  size_t host_words = 0;
  int32_t *block = nullptr, *pool_block = nullptr;   // the two device allocations the pointers above point into
  size_t block_cap = 0, pool_cap = 0;                // their capacities in bytes (plan.hip recycles them)
  int device = 0;                                    // the device the blocks live on (current device at bsms_plan_create)
  // bsms_plan_concat only: recorded on the caller's stream behind the kernels that write the blocks.  The HOST readers of the blocks
  // (bsms_plan_export*, bsms_plan_set_pool) wait for it: their plain hipMemcpy is not ordered against a non-blocking stream.  Null
  // for a plan bsms_plan_create built (its upload is complete when the call returns).
  hipEvent_t written = nullptr;
};
