// What the kernels of the edge-difference adjoint share: the launch arguments, what an edge reads of one of its
// ends, mu_e * omega_e, and the ONE copy of the adjoint's gather loop -- k_edge_bwd (edgediff.hip: bsms_edge_diff_bwd) and
// k_edge_objective_bwd (ext/edge_objective.hip: bsms_sim_edge_objective_bwd) both run `edge_gather`.  Both files are compiled with
// -ffp-contract=off.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace bsms {
namespace edge {

constexpr int kMaxP = 3;                                // position columns
constexpr int kBwdThreads = 256;                        // rows per block of the backward

struct EdgeArgs {
  const int32_t *rowptr, *src;                          // incoming edges of plan row n: src[rowptr[n] .. rowptr[n+1])
  const int32_t *t_rowptr, *t_dst;                      // outgoing edges of plan row n (backward only)
  const float *pred, *target, *mask, *pos;              // row 0 of segment 0
  int64_t row0, seg_rows, pieces;                       // the window of the plan; blocks per segment
  int64_t pred_stride, target_stride, mask_stride, pos_stride;   // rows between the segments
  int64_t blk0;                                         // global index of this launch's first block
  int p;
};

// C (and with it every loop below) is a compile-time constant: the rows of pred / target load as one or two wide loads (global
// loads need dword alignment only) and nothing inside the edge loop branches -- with C, the position width or the window test as
// run-time branches hipcc waits for every load before it issues the next one.
template <int C>
struct Node {                                           // what an edge reads of one of its ends
  float d[C], t[C], x[kMaxP], m;
};

template <int C, bool kQuot>
__device__ __forceinline__ Node<C> load_node(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ mask,
                                             const float* __restrict__ pos, int p, int64_t r) {
  Node<C> n;
  float pr[C];
#pragma unroll
  for (int c = 0; c < C; ++c) pr[c] = pred[r * C + c];
#pragma unroll
  for (int c = 0; c < C; ++c) n.t[c] = target[r * C + c];
#pragma unroll
  for (int c = 0; c < C; ++c) n.d[c] = pr[c] - n.t[c];              // the fp32 subtraction of bsms_error_sums
  n.m = mask[r];
  if (kQuot) {                                          // p in 1..3: the columns past p re-read column 0 (in bounds); edge_weight drops them
    const float* x = pos + r * p;
    n.x[0] = x[0];
    n.x[1] = x[p > 1 ? 1 : 0];
    n.x[2] = x[p > 2 ? 2 : 0];
  } else {
    n.x[0] = n.x[1] = n.x[2] = 0.f;
  }
  return n;
}

// mu_e * omega_e of the edge between `a` and `b`; `mu` returns mu_e alone (what ME counts).  An edge without length ("quotient")
// has both 0.
template <int C, bool kQuot>
__device__ __forceinline__ double edge_weight(const Node<C>& a, const Node<C>& b, int p, double& mu) {
  mu = double(a.m) * double(b.m);
  if (!kQuot) return mu;
  double l2 = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxP; ++k) {
    const double dx = double(a.x[k]) - double(b.x[k]);
    const double sq = dx * dx;
    l2 = k < p ? l2 + sq : l2;                          // a select: the sum runs over the p columns in order
  }
  const bool flat = l2 == 0.0;
  const double w = 1.0 / (flat ? 1.0 : l2);
  mu = flat ? 0.0 : mu;
  return flat ? 0.0 : mu * w;
}

// U consecutive slots of a row per step: all index loads, then all neighbour loads, then the terms strictly in slot order.  A slot
// past the row's end, or one whose other end lies outside the window, loads the row itself (in bounds, in cache) and is dropped by
// a select: the accumulators see exactly the additions of the edges that count, in CSR order.
template <int C>
struct Batch {                                          // neighbour rows in flight per lane
  static constexpr int kSums = C <= 4 ? 4 : C <= 6 ? 2 : 1;     // 1024 threads leave 128 registers, 2 (1 + 2C) of them accumulators
  static constexpr int kBwd = C <= 4 ? 4 : 2;
};

// acc[c] = sum over the incoming edges of row r in CSR order, then its outgoing edges in transpose order, of mu omega (d_rc - d_other,c):
// ONE fp64 accumulator per element.  The one copy of the adjoint's gather loop: k_edge_bwd and k_edge_objective_bwd both run it.
template <int C, bool kQuot>
__device__ __forceinline__ void edge_gather(const EdgeArgs& a, const float* __restrict__ pred, const float* __restrict__ target,
                                            const float* __restrict__ mask, const float* __restrict__ pos, int64_t r, const Node<C>& me,
                                            double (&acc)[C]) {
  constexpr int U = Batch<C>::kBwd;
  const int in0 = a.rowptr[a.row0 + r], in1 = a.rowptr[a.row0 + r + 1];
  const int out0 = a.t_rowptr[a.row0 + r], out1 = a.t_rowptr[a.row0 + r + 1];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {                // incoming edges in CSR order, then outgoing edges in transpose order
    const int32_t* __restrict__ nbr = half ? a.t_dst : a.src;
    const int q0 = half ? out0 : in0, q1 = half ? out1 : in1;
    for (int q = q0; q < q1; q += U) {
      int64_t o[U];
      bool counts[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool live = q + u < q1;
        o[u] = int64_t(nbr[live ? q + u : q]) - a.row0;
        counts[u] = live && o[u] >= 0 && o[u] < a.seg_rows;
        o[u] = counts[u] ? o[u] : r;
      }
      Node<C> other[U];
#pragma unroll
      for (int u = 0; u < U; ++u) other[u] = load_node<C, kQuot>(pred, target, mask, pos, a.p, o[u]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        double mu;
        const double mw = edge_weight<C, kQuot>(other[u], me, a.p, mu);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double nxt = acc[c] + mw * (double(me.d[c]) - double(other[u].d[c]));
          acc[c] = counts[u] ? nxt : acc[c];
        }
      }
    }
  }
}

}  // namespace edge
}  // namespace bsms
