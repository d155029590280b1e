// Masked error sums for evaluation (include/bsms_hip.h: bsms_error_sums): what the reference's `Trainer.get_error`
// (trainer/trainer.py:254-269) and its rollout driver (rollout.py:99-107) reduce on the host after copying prediction, target and
// mask there.  Per segment s (a sample of a batch, or a time step of a rolled-out trajectory) over its seg_rows rows:
//   M = sum m    SE[c] = sum m * d_c^2    AE[c] = sum m * |d_c|    TT[c] = sum m * target_c^2,   d = fl32(pred - target)
// d takes the ONE fp32 rounding of the reference's subtraction; every product and sum after it is fp64.
// Deterministic, no atomics: the piece sum of piece_sum.h over pieces of kPieceRows rows, a thread adding its rows
// in ascending order.  A segment's sums therefore depend on its own rows only -- not on S, on the strides, or on what else is in
// the launch.  What is this file's: what a row adds (SumErrors / SumRobust), the argument checks and the entries.
// bsms_error_sums_w (node-weighted training objectives) is the same code with mu = double(m) * double(weight) in m's place.
// bsms_robust_sums (robust training objectives) is the same code again with another POLICY for what a row adds: one
// column S[c] = sum mu * rho(d_c / s_c) per channel in place of the three of the evaluation (SumErrors / SumRobust below).
// Compiled with -ffp-contract=off (build.py): the sums keep the roundings of separate fp64 multiplies and adds.
#include "piece_sum.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kMaxCols = 1 + 3 * kMaxC;                 // M | SE | AE | TT
constexpr int kThreads = 256;                           // four waves of 64
constexpr int kRowsPerThread = 4;
constexpr int kPieceRows = kThreads * kRowsPerThread;   // 1024 rows of a segment per block
constexpr int64_t kMaxBlocksPerLaunch = int64_t(1) << 22;   // 2^30 threads: below the 2^32 work items of one dispatch

struct ErrArgs {
  const float *pred, *target, *mask;
  int64_t seg_rows, pieces;                             // pieces per segment = ceil(seg_rows / kPieceRows)
  int64_t pred_stride, target_stride, mask_stride;      // rows between the segments
  int64_t blk0;                                         // global index of this launch's first block (= segment * pieces + piece)
  int C;
};

// What a row accumulates -- the policy of error_piece.  kGroups columns per channel behind M; `add` forms them for one element from
// mu, d = double(fl32(pred - target)) and the target, each into acc[1 + g * kMaxC + c].
struct SumErrors {                                      // M | SE | AE | TT (bsms_error_sums, bsms_error_sums_w)
  static constexpr int kGroups = 3;
  __device__ __forceinline__ void prepare(int) {}
  __device__ __forceinline__ void add(double* acc, int c, double m, double dd, double td) const {
    acc[1 + c] += m * (dd * dd);
    acc[1 + kMaxC + c] += m * fabs(dd);
    acc[1 + 2 * kMaxC + c] += m * (td * td);
  }
};

struct SumRobust {                                      // M | S, S[c] = sum mu * rho(d_c / s_c) (bsms_robust_sums)
  static constexpr int kGroups = 1;
  const double *mean, *meansq, *eps, *delta;            // the target normaliser (read when normalized) and delta[C] (read when huber)
  int normalized, huber;
  double s[kMaxC], dl[kMaxC];                           // filled by prepare: every thread forms the C scales itself
  __device__ __forceinline__ void prepare(int C) {
    const double e = normalized ? *eps : 0.0;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      s[c] = (normalized && c < C) ? std_eps(mean[c], meansq[c], e) : 1.0;      // x / 1.0 is exact: physical MAE IS the AE column
      dl[c] = (huber && c < C) ? delta[c] : 0.0;
    }
  }
  __device__ __forceinline__ void add(double* acc, int c, double m, double dd, double) const {
    const double u = dd / s[c], au = fabs(u);
    double rho = au;                                    // mae
    if (huber) rho = au <= dl[c] ? 0.5 * (u * u) : dl[c] * (au - 0.5 * dl[c]);
    acc[1 + c] += m * rho;
  }
};

// The accumulators of a thread are M and kGroups blocks of kMaxC channels; the output columns are M and kGroups blocks of C.
template <int kGroups>
struct ChannelCols {
  int C;
  __device__ __forceinline__ bool live(int k) const { return k == 0 || (k - 1) % kMaxC < C; }
  __device__ __forceinline__ int ncol() const { return 1 + kGroups * C; }
  __device__ __forceinline__ int slot(int col) const { return col == 0 ? 0 : 1 + ((col - 1) / C) * kMaxC + (col - 1) % C; }
};

// One piece of one segment.  kWeighted (bsms_error_sums_w): the row's mask is multiplied by its weight in fp64 before anything
// else sees it -- with a unit weight the product IS the mask, so every later operation is the unweighted kernel's.
template <bool kWeighted, class Policy>
__device__ __forceinline__ void error_piece(const ErrArgs& a, const float* __restrict__ row_weights, int64_t weight_stride,
                                            double* __restrict__ partials, Policy pol) {
  constexpr int kCols = 1 + Policy::kGroups * kMaxC;    // accumulators of a thread: M, then kGroups blocks of kMaxC channels
  const int C = a.C;
  pol.prepare(C);
  const psum::Split at = psum::split(a.blk0, a.pieces);
  const int64_t s = at.seg, piece = at.piece;
  const float* pred = a.pred + s * a.pred_stride * C;
  const float* target = a.target + s * a.target_stride * C;
  const float* mask = a.mask + s * a.mask_stride;
  const float* omega = kWeighted ? row_weights + s * weight_stride : nullptr;

  double acc[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) acc[k] = 0.0;
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int64_t r = piece * kPieceRows + j * kThreads + int(threadIdx.x);     // row inside the segment
    if (r < a.seg_rows) {
      double m = double(mask[r]);
      if (kWeighted) m = m * double(omega[r]);         // mu = double(mask) * double(weight)
      acc[0] += m;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < C) {
          const float t = target[r * C + c];
          const float d = pred[r * C + c] - t;          // the fp32 subtraction of the reference
          pol.add(acc, c, m, double(d), double(t));
        }
      }
    }
  }
  const ChannelCols<Policy::kGroups> cols{C};
  psum::block_sum<kThreads>(acc, cols, partials + at.blk * cols.ncol());
}

__global__ __launch_bounds__(kThreads) void k_error_pieces(const ErrArgs a, double* __restrict__ partials) {
  error_piece<false>(a, nullptr, 0, partials, SumErrors());
}

__global__ __launch_bounds__(kThreads) void k_error_pieces_w(const ErrArgs a, const float* __restrict__ row_weights,
                                                             int64_t weight_stride, double* __restrict__ partials) {
  error_piece<true>(a, row_weights, weight_stride, partials, SumErrors());
}

__global__ __launch_bounds__(kThreads) void k_robust_pieces(const ErrArgs a, const SumRobust pol, double* __restrict__ partials) {
  error_piece<false>(a, nullptr, 0, partials, pol);
}

__global__ __launch_bounds__(kThreads) void k_robust_pieces_w(const ErrArgs a, const SumRobust pol, const float* __restrict__ row_weights,
                                                              int64_t weight_stride, double* __restrict__ partials) {
  error_piece<true>(a, row_weights, weight_stride, partials, pol);
}

inline int64_t pieces_of(int64_t seg_rows) { return ceil_div(seg_rows, kPieceRows); }

}  // namespace

extern "C" size_t bsms_error_sums_work_bytes(int64_t S, int64_t seg_rows) {
  if (S < 0 || seg_rows < 0) return 0;
  return size_t(std::max<int64_t>(S, 1)) * size_t(std::max<int64_t>(pieces_of(seg_rows), 1)) * kMaxCols * sizeof(double) + 256;
}

namespace {

// All three entries: the checks in their documented order, the piece launches, the finish.  `row_weights` == nullptr with weighted ==
// false is bsms_error_sums, launch for launch.  `robust` (bsms_robust_sums): the SumRobust policy, rows of `sums` sums_stride apart.
int error_sums_impl(const char* who, bool weighted, const float* pred, const float* target, const float* mask,
                    const float* row_weights, int64_t S, int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride,
                    int64_t mask_stride, int64_t weight_stride, double* sums, void* work, bsms_stream_t stream,
                    const SumRobust* robust = nullptr, int64_t sums_stride = 0) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: C=%lld (C in 1..8)", who, (long long)C);
  const int ncol = robust ? 1 + int(C) : 1 + 3 * int(C);
  if (!robust) sums_stride = ncol;
  BSMS_REQUIRE(S >= 0 && seg_rows >= 0 && seg_rows <= INT32_MAX, BSMS_E_INVALID_ARG, "%s: S=%lld seg_rows=%lld (seg_rows in 0..2^31-1)", who,
               (long long)S, (long long)seg_rows);
  BSMS_REQUIRE(pred_stride >= 0 && target_stride >= 0 && mask_stride >= 0 && weight_stride >= 0, BSMS_E_INVALID_ARG,
               "%s: negative segment stride (%lld, %lld, %lld, %lld)", who, (long long)pred_stride, (long long)target_stride,
               (long long)mask_stride, (long long)weight_stride);
  BSMS_REQUIRE(sums_stride >= ncol, BSMS_E_INVALID_ARG, "%s: sums_stride=%lld is shorter than one row (%d)", who, (long long)sums_stride, ncol);
  if (S == 0) return BSMS_OK;
  const int64_t pieces = pieces_of(seg_rows);
  BSMS_REQUIRE(sums && (pieces == 0 || (pred && target && mask && work && (row_weights || !weighted))), BSMS_E_INVALID_ARG,
               "%s: null argument", who);
  BSMS_REQUIRE(!robust || ((!robust->normalized || (robust->mean && robust->meansq && robust->eps)) && (!robust->huber || robust->delta)),
               BSMS_E_INVALID_ARG, "%s: null argument (the statistics of the normalized space, delta of the Huber loss)", who);
  // the finishing kernel runs one thread per output element in one dispatch
  BSMS_REQUIRE(S <= (int64_t(1) << 30) / ncol, BSMS_E_UNSUPPORTED, "%s: S=%lld segments of %d sums exceed one dispatch", who, (long long)S, ncol);
  hipStream_t s = as_stream(stream);
  double* partials = reinterpret_cast<double*>(work);
  ErrArgs a;
  a.pred = pred; a.target = target; a.mask = mask;
  a.seg_rows = seg_rows; a.pieces = pieces;
  a.pred_stride = pred_stride; a.target_stride = target_stride; a.mask_stride = mask_stride;
  a.C = int(C);
  const int64_t blocks = S * pieces;     // < 2^20 * 2^21 at the documented limits: no overflow
  const int rc = psum::for_block_slices(blocks, kMaxBlocksPerLaunch, [&](int64_t first, unsigned nb) {
    a.blk0 = first;
    if (robust && weighted) hipLaunchKernelGGL(k_robust_pieces_w, dim3(nb), dim3(kThreads), 0, s, a, *robust, row_weights, weight_stride, partials);
    else if (robust) hipLaunchKernelGGL(k_robust_pieces, dim3(nb), dim3(kThreads), 0, s, a, *robust, partials);
    else if (weighted) hipLaunchKernelGGL(k_error_pieces_w, dim3(nb), dim3(kThreads), 0, s, a, row_weights, weight_stride, partials);
    else hipLaunchKernelGGL(k_error_pieces, dim3(nb), dim3(kThreads), 0, s, a, partials);
  });
  if (rc) return rc;
  psum::launch_finish(partials, S, pieces, ncol, sums_stride, sums, s);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

}  // namespace

extern "C" int bsms_error_sums(const float* pred, const float* target, const float* mask, int64_t S, int64_t seg_rows, int64_t C,
                               int64_t pred_stride, int64_t target_stride, int64_t mask_stride, double* sums, void* work,
                               bsms_stream_t stream) {
  return error_sums_impl("error_sums", false, pred, target, mask, nullptr, S, seg_rows, C, pred_stride, target_stride, mask_stride, 0, sums,
                         work, stream);
}

// bsms_error_sums with a weight per row (include/bsms_hip.h): mu = double(mask) * double(weight) takes the mask's place in every sum.
extern "C" int bsms_error_sums_w(const float* pred, const float* target, const float* mask, const float* row_weights, int64_t S,
                                 int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride, int64_t mask_stride,
                                 int64_t weight_stride, double* sums, void* work, bsms_stream_t stream) {
  return error_sums_impl("error_sums_w", true, pred, target, mask, row_weights, S, seg_rows, C, pred_stride, target_stride, mask_stride,
                         weight_stride, sums, work, stream);
}

// The per-channel sums of the robust training objectives (include/bsms_hip.h): the pieces, block sum and finish of
// bsms_error_sums with S[c] = sum mu * rho(double(d_c) / s_c) as the one column per channel.
extern "C" int bsms_robust_sums(const float* pred, const float* target, const float* mask, const float* row_weights, int64_t S,
                                int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride, int64_t mask_stride,
                                int64_t weight_stride, const double* mean, const double* meansq, const double* std_eps_dev,
                                const double* delta, int space, int rkind, double* sums, int64_t sums_stride, void* work,
                                bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "robust_sums: C=%lld (C in 1..8)", (long long)C);
  BSMS_REQUIRE((space == BSMS_LOSS_PHYSICAL || space == BSMS_LOSS_NORMALIZED) && (rkind == BSMS_ROBUST_MAE || rkind == BSMS_ROBUST_HUBER),
               BSMS_E_UNSUPPORTED, "robust_sums: space=%d rkind=%d (each 0 or 1)", space, rkind);
  SumRobust pol;
  pol.mean = mean; pol.meansq = meansq; pol.eps = std_eps_dev; pol.delta = delta;
  pol.normalized = int(space == BSMS_LOSS_NORMALIZED);
  pol.huber = int(rkind == BSMS_ROBUST_HUBER);
  for (int c = 0; c < kMaxC; ++c) pol.s[c] = pol.dl[c] = 0.0;      // formed on the device (SumRobust::prepare)
  return error_sums_impl("robust_sums", row_weights != nullptr, pred, target, mask, row_weights, S, seg_rows, C, pred_stride, target_stride,
                         mask_stride, weight_stride, sums, work, stream, &pol, sums_stride);
}
