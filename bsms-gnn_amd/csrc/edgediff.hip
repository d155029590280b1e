// Edge-difference (discrete H1) error sums and their adjoint (include/bsms_hip.h: bsms_edge_diff_sums, bsms_edge_diff_bwd; DESIGN.md
// 4.21).  Per segment s (a sample of a batch, or a time step of a rolled-out trajectory) over the directed edges e = (i -> j) of the
// plan's rows [row0, row0 + seg_rows) whose BOTH ends lie in that window:
//   mu_e = double(m_i) * double(m_j)     omega_e = 1 ("difference") | 1 / l2_e, l2_e = sum_k (double(pos_ik) - double(pos_jk))^2
//   ("quotient"; an edge with l2_e == 0 has mu_e = omega_e = 0)
//   ME = sum mu_e    DE[c] = sum mu_e omega_e (d_ic - d_jc)^2    TE[c] = sum mu_e omega_e (t_ic - t_jc)^2,   d = fl32(pred - target)
// d takes the ONE fp32 rounding of bsms_error_sums; every product and sum after it is fp64.
// Deterministic, no atomics.  Sums: row r owns its INCOMING edges (the plan's dst-sorted CSR, stable in the caller's edge order) and
// adds them one after the other; the rows are reduced by the piece sum of piece_sum.h -- pieces of kPieceRows rows,
// one row per thread, sixteen waves.  A segment's row therefore depends on its own rows and edges only: not on S, the
// strides, its neighbours in the launch, or on whether the plan is the mesh's own or a block-diagonal union around it.
// Backward: thread r owns grad[s, r, :]; per element ONE fp64 accumulator, incoming edges in CSR order, then outgoing edges in
// transpose order, times 2 * coef[s, c] in fp64, ONE rounding to fp32.
// An edge whose other end lies outside the window is not read: its index is replaced by the row's own (a load that is in bounds and
// in cache) and its term is dropped by a select, so the loop carries no branch and the index / row loads of consecutive edges stay
// independent.
// The gather loop of the backward is `edge_gather` (edge_gather.h): ext/edge_objective.hip runs the same copy.
// Compiled with -ffp-contract=off (build.py): the sums keep the roundings of separate fp64 multiplies and adds.
#include "edge_gather.h"
#include "piece_sum.h"

#pragma clang fp contract(off)

using namespace bsms;
using namespace bsms::edge;

namespace {

constexpr int kMaxCols = 1 + 2 * kMaxC;                 // ME | DE | TE
constexpr int kPieceRows = 1024;                        // rows of a segment per block of the sums: one row per thread, sixteen waves
constexpr int64_t kMaxBlocksPerLaunch = int64_t(1) << 21;   // 2^31 threads: below the 2^32 work items of one dispatch

template <int C, bool kQuot>
__global__ __launch_bounds__(kPieceRows) void k_edge_pieces(const EdgeArgs a, double* __restrict__ partials) {
  constexpr int ncol = 1 + 2 * C, U = Batch<C>::kSums;
  const psum::Split at = psum::split(a.blk0, a.pieces);
  const int64_t s = at.seg, piece = at.piece;
  const float* pred = a.pred + s * a.pred_stride * C;
  const float* target = a.target + s * a.target_stride * C;
  const float* mask = a.mask + s * a.mask_stride;
  const float* pos = kQuot ? a.pos + s * a.pos_stride * a.p : nullptr;

  double acc[ncol];
#pragma unroll
  for (int k = 0; k < ncol; ++k) acc[k] = 0.0;
  const int64_t r = piece * kPieceRows + int(threadIdx.x);          // row inside the segment
  if (r < a.seg_rows) {
    const int q0 = a.rowptr[a.row0 + r], q1 = a.rowptr[a.row0 + r + 1];
    const Node<C> me = load_node<C, kQuot>(pred, target, mask, pos, a.p, r);
    for (int q = q0; q < q1; q += U) {                  // CSR order = the caller's edge order
      int64_t o[U];
      bool counts[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool live = q + u < q1;
        o[u] = int64_t(a.src[live ? q + u : q]) - a.row0;
        counts[u] = live && o[u] >= 0 && o[u] < a.seg_rows;
        o[u] = counts[u] ? o[u] : r;
      }
      Node<C> other[U];
#pragma unroll
      for (int u = 0; u < U; ++u) other[u] = load_node<C, kQuot>(pred, target, mask, pos, a.p, o[u]);
      __builtin_amdgcn_sched_barrier(0);                // every neighbour load is in flight before the first add
#pragma unroll
      for (int u = 0; u < U; ++u) {
        double mu;
        const double mw = edge_weight<C, kQuot>(other[u], me, a.p, mu);
        acc[0] = counts[u] ? acc[0] + mu : acc[0];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double dd = double(other[u].d[c]) - double(me.d[c]);
          const double td = double(other[u].t[c]) - double(me.t[c]);
          const double de = acc[1 + c] + mw * (dd * dd), te = acc[1 + C + c] + mw * (td * td);
          acc[1 + c] = counts[u] ? de : acc[1 + c];
          acc[1 + C + c] = counts[u] ? te : acc[1 + C + c];
        }
      }
    }
  }
  psum::block_sum<kPieceRows>(acc, psum::Dense<ncol>(), partials + at.blk * ncol);
}

// grad[s, r, c] = fl32(2 coef[s, c] * (sum over incoming, then outgoing edges of mu omega (d_rc - d_other,c))); one thread per row
template <int C, bool kQuot>
__global__ __launch_bounds__(kBwdThreads) void k_edge_bwd(const EdgeArgs a, const double* __restrict__ coef, int accumulate,
                                                         float* __restrict__ grad, int64_t grad_stride) {
  const psum::Split at = psum::split(a.blk0, a.pieces);
  const int64_t s = at.seg, r = at.piece * kBwdThreads + int(threadIdx.x);
  if (r >= a.seg_rows) return;
  const float* pred = a.pred + s * a.pred_stride * C;
  const float* target = a.target + s * a.target_stride * C;
  const float* mask = a.mask + s * a.mask_stride;
  const float* pos = kQuot ? a.pos + s * a.pos_stride * a.p : nullptr;
  const Node<C> me = load_node<C, kQuot>(pred, target, mask, pos, a.p, r);
  double acc[C];
  edge_gather<C, kQuot>(a, pred, target, mask, pos, r, me, acc);
  float* g = grad + (s * grad_stride + r) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float v = float((2.0 * coef[s * C + c]) * acc[c]);        // the one rounding to fp32
    g[c] = accumulate ? g[c] + v : v;
  }
}

template <int C>
void launch_pieces(bool quot, unsigned nb, hipStream_t s, const EdgeArgs& a, double* partials) {
  if (quot) hipLaunchKernelGGL((k_edge_pieces<C, true>), dim3(nb), dim3(kPieceRows), 0, s, a, partials);
  else hipLaunchKernelGGL((k_edge_pieces<C, false>), dim3(nb), dim3(kPieceRows), 0, s, a, partials);
}

template <int C>
void launch_bwd(bool quot, unsigned nb, hipStream_t s, const EdgeArgs& a, const double* coef, int accumulate, float* grad, int64_t grad_stride) {
  if (quot) hipLaunchKernelGGL((k_edge_bwd<C, true>), dim3(nb), dim3(kBwdThreads), 0, s, a, coef, accumulate, grad, grad_stride);
  else hipLaunchKernelGGL((k_edge_bwd<C, false>), dim3(nb), dim3(kBwdThreads), 0, s, a, coef, accumulate, grad, grad_stride);
}

inline int64_t pieces_of(int64_t seg_rows) { return ceil_div(seg_rows, kPieceRows); }

// The checks both entries share, in the order of bsms_error_sums; fills `a` when there is work.  Returns BSMS_OK with *go = false when
// S == 0.
int edge_args(const char* who, const bsms_plan* plan, int64_t row0, int64_t seg_rows, const float* pred, const float* target,
              const float* mask, const float* pos, int64_t S, int64_t C, int64_t p, int weighting, int64_t pred_stride,
              int64_t target_stride, int64_t mask_stride, int64_t pos_stride, EdgeArgs* a, bool* go) {
  *go = false;
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: C=%lld (C in 1..8)", who, (long long)C);
  BSMS_REQUIRE(weighting == BSMS_EDGE_DIFFERENCE || weighting == BSMS_EDGE_QUOTIENT, BSMS_E_UNSUPPORTED, "%s: weighting=%d (0 or 1)", who,
               weighting);
  const bool quot = weighting == BSMS_EDGE_QUOTIENT;
  BSMS_REQUIRE(!quot || (p >= 1 && p <= kMaxP), BSMS_E_UNSUPPORTED, "%s: p=%lld (p in 1..3 with the quotient weighting)", who, (long long)p);
  BSMS_REQUIRE(S >= 0 && seg_rows >= 0 && seg_rows <= INT32_MAX && row0 >= 0, BSMS_E_INVALID_ARG,
               "%s: S=%lld row0=%lld seg_rows=%lld (seg_rows in 0..2^31-1)", who, (long long)S, (long long)row0, (long long)seg_rows);
  BSMS_REQUIRE(pred_stride >= 0 && target_stride >= 0 && mask_stride >= 0 && pos_stride >= 0, BSMS_E_INVALID_ARG,
               "%s: negative segment stride (%lld, %lld, %lld, %lld)", who, (long long)pred_stride, (long long)target_stride,
               (long long)mask_stride, (long long)pos_stride);
  if (S == 0) return BSMS_OK;
  BSMS_REQUIRE(plan, BSMS_E_INVALID_ARG, "%s: plan is null", who);
  BSMS_REQUIRE(row0 + seg_rows <= plan->N, BSMS_E_SHAPE, "%s: rows [%lld, %lld) are not a window of a plan of %lld rows", who,
               (long long)row0, (long long)(row0 + seg_rows), (long long)plan->N);
  BSMS_REQUIRE(seg_rows == 0 || (pred && target && mask && (pos || !quot)), BSMS_E_INVALID_ARG, "%s: null argument", who);
  a->rowptr = plan->rowptr; a->src = plan->src; a->t_rowptr = plan->t_rowptr; a->t_dst = plan->t_dst;
  a->pred = pred; a->target = target; a->mask = mask; a->pos = quot ? pos : nullptr;
  a->row0 = row0; a->seg_rows = seg_rows; a->pieces = pieces_of(seg_rows);
  a->pred_stride = pred_stride; a->target_stride = target_stride; a->mask_stride = mask_stride; a->pos_stride = pos_stride;
  a->blk0 = 0;
  a->p = quot ? int(p) : 0;
  *go = true;
  return BSMS_OK;
}

}  // namespace

extern "C" size_t bsms_edge_diff_work_bytes(int64_t S, int64_t seg_rows) {
  if (S < 0 || seg_rows < 0) return 0;
  return size_t(std::max<int64_t>(S, 1)) * size_t(std::max<int64_t>(pieces_of(seg_rows), 1)) * kMaxCols * sizeof(double) + 256;
}

extern "C" int bsms_edge_diff_sums(const bsms_plan_t* plan, int64_t row0, int64_t seg_rows, const float* pred, const float* target,
                                   const float* mask, const float* pos, int64_t S, int64_t C, int64_t p, int weighting,
                                   int64_t pred_stride, int64_t target_stride, int64_t mask_stride, int64_t pos_stride, double* sums,
                                   void* work, bsms_stream_t stream) {
  EdgeArgs a;
  bool go;
  if (int rc = edge_args("edge_diff_sums", plan, row0, seg_rows, pred, target, mask, pos, S, C, p, weighting, pred_stride, target_stride,
                         mask_stride, pos_stride, &a, &go))
    return rc;
  if (!go) return BSMS_OK;
  BSMS_REQUIRE(sums && (a.pieces == 0 || work), BSMS_E_INVALID_ARG, "edge_diff_sums: null argument");
  const int ncol = 1 + 2 * int(C);
  // the finishing kernel runs one thread per output element in one dispatch
  BSMS_REQUIRE(S <= (int64_t(1) << 30) / ncol, BSMS_E_UNSUPPORTED, "edge_diff_sums: S=%lld segments of %d sums exceed one dispatch", (long long)S, ncol);
  hipStream_t s = as_stream(stream);
  double* partials = reinterpret_cast<double*>(work);
  const int64_t blocks = S * a.pieces;
  const int rc = psum::for_block_slices(blocks, kMaxBlocksPerLaunch, [&](int64_t first, unsigned nb) {
    a.blk0 = first;
    psum::by_channels(int(C), [&](auto c) { launch_pieces<decltype(c)::value>(weighting == BSMS_EDGE_QUOTIENT, nb, s, a, partials); });
  });
  if (rc) return rc;
  psum::launch_finish(partials, S, a.pieces, ncol, ncol, sums, s);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_edge_diff_bwd(const bsms_plan_t* plan, int64_t row0, int64_t seg_rows, const float* pred, const float* target,
                                  const float* mask, const float* pos, int64_t S, int64_t C, int64_t p, int weighting,
                                  int64_t pred_stride, int64_t target_stride, int64_t mask_stride, int64_t pos_stride, const double* coef,
                                  int accumulate, float* grad, int64_t grad_stride, bsms_stream_t stream) {
  EdgeArgs a;
  bool go;
  if (int rc = edge_args("edge_diff_bwd", plan, row0, seg_rows, pred, target, mask, pos, S, C, p, weighting, pred_stride, target_stride,
                         mask_stride, pos_stride, &a, &go))
    return rc;
  if (!go || seg_rows == 0) return BSMS_OK;
  BSMS_REQUIRE(coef && grad, BSMS_E_INVALID_ARG, "edge_diff_bwd: null argument");
  BSMS_REQUIRE(grad_stride >= seg_rows, BSMS_E_INVALID_ARG, "edge_diff_bwd: grad_stride=%lld is shorter than a segment (%lld rows)",
               (long long)grad_stride, (long long)seg_rows);
  hipStream_t s = as_stream(stream);
  a.pieces = ceil_div(seg_rows, kBwdThreads);            // blocks per segment: one thread per row
  const int64_t blocks = S * a.pieces;
  return psum::for_block_slices(blocks, kMaxBlocksPerLaunch, [&](int64_t first, unsigned nb) {
    a.blk0 = first;
    psum::by_channels(int(C), [&](auto c) {
      launch_bwd<decltype(c)::value>(weighting == BSMS_EDGE_QUOTIENT, nb, s, a, coef, accumulate, grad, grad_stride);
    });
  });
}
