// Masked error sums for evaluation (include/bsms_hip.h: bsms_error_sums): what the reference's `Trainer.get_error`
// (trainer/trainer.py:254-269) and its rollout driver (rollout.py:99-107) reduce on the host after copying prediction, target and
// mask there.  Per segment s (a sample of a batch, or a time step of a rolled-out trajectory) over its seg_rows rows:
//   M = sum m    SE[c] = sum m * d_c^2    AE[c] = sum m * |d_c|    TT[c] = sum m * target_c^2,   d = fl32(pred - target)
// d takes the ONE fp32 rounding of the reference's subtraction; every product and sum after it is fp64.
// Deterministic, no atomics: a segment is cut into pieces of kPieceRows rows counted from ITS first row; k_error_pieces reduces a
// piece (per thread: its rows in ascending order; per wave: a fixed shuffle tree; per block: the four waves in order) and
// k_error_finish adds the pieces of a segment in index order.  A segment's sums therefore depend on its own rows only -- not on
// S, on the strides, or on what else is in the launch.
// bsms_error_sums_w (node-weighted training objectives) is the same code with mu = double(m) * double(weight) in m's place.
// Compiled with -ffp-contract=off (build.py): the sums keep the roundings of separate fp64 multiplies and adds.
#include "common.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kMaxC = 8;                                // state channels (sim.hip and batch.hip keep the same bound)
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

// One piece of one segment.  kWeighted (bsms_error_sums_w): the row's mask is multiplied by its weight in fp64 before anything
// else sees it -- with a unit weight the product IS the mask, so every later operation is the unweighted kernel's.
template <bool kWeighted>
__device__ __forceinline__ void error_piece(const ErrArgs& a, const float* __restrict__ row_weights, int64_t weight_stride,
                                            double* __restrict__ partials) {
  __shared__ double red[kThreads / 64][kMaxCols];
  const int C = a.C, ncol = 1 + 3 * C;
  const int64_t blk = a.blk0 + int64_t(blockIdx.x);
  const int64_t s = blk / a.pieces, piece = blk - s * a.pieces;
  const float* pred = a.pred + s * a.pred_stride * C;
  const float* target = a.target + s * a.target_stride * C;
  const float* mask = a.mask + s * a.mask_stride;
  const float* omega = kWeighted ? row_weights + s * weight_stride : nullptr;

  double acc[kMaxCols];
#pragma unroll
  for (int k = 0; k < kMaxCols; ++k) acc[k] = 0.0;
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
          const double dd = double(d), td = double(t);
          acc[1 + c] += m * (dd * dd);
          acc[1 + kMaxC + c] += m * fabs(dd);
          acc[1 + 2 * kMaxC + c] += m * (td * td);
        }
      }
    }
  }
  // fixed trees: lanes of a wave by shuffle, then the four waves in order
  const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
#pragma unroll
  for (int k = 0; k < kMaxCols; ++k) {
    const int c = (k - 1) % kMaxC;                      // channel of column k (k >= 1)
    if (k == 0 || c < C) {
      double v = acc[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][k] = v;
    }
  }
  __syncthreads();
  if (int(threadIdx.x) < ncol) {
    const int col = int(threadIdx.x);                   // output column: 0 | 1 + c | 1 + C + c | 1 + 2C + c
    const int k = col == 0 ? 0 : 1 + ((col - 1) / C) * kMaxC + (col - 1) % C;
    double v = red[0][k];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) v += red[w][k];
    partials[blk * ncol + col] = v;
  }
}

__global__ __launch_bounds__(kThreads) void k_error_pieces(const ErrArgs a, double* __restrict__ partials) {
  error_piece<false>(a, nullptr, 0, partials);
}

__global__ __launch_bounds__(kThreads) void k_error_pieces_w(const ErrArgs a, const float* __restrict__ row_weights,
                                                             int64_t weight_stride, double* __restrict__ partials) {
  error_piece<true>(a, row_weights, weight_stride, partials);
}

// sums[s, col] = the pieces of segment s added in index order (zero pieces: zeros); one thread per output element
__global__ __launch_bounds__(kThreads) void k_error_finish(const double* __restrict__ partials, int64_t S, int64_t pieces, int ncol,
                                                          double* __restrict__ sums) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  if (i >= S * ncol) return;
  const int64_t s = i / ncol;
  const int col = int(i - s * ncol);
  const double* p = partials + s * pieces * ncol + col;
  double v = 0.0;
#pragma unroll 8
  for (int64_t k = 0; k < pieces; ++k) v += p[k * ncol];
  sums[i] = v;
}

inline int64_t pieces_of(int64_t seg_rows) { return ceil_div(seg_rows, kPieceRows); }

}  // namespace

extern "C" size_t bsms_error_sums_work_bytes(int64_t S, int64_t seg_rows) {
  if (S < 0 || seg_rows < 0) return 0;
  return size_t(std::max<int64_t>(S, 1)) * size_t(std::max<int64_t>(pieces_of(seg_rows), 1)) * kMaxCols * sizeof(double) + 256;
}

namespace {

// Both entries: the checks in their documented order, the piece launches, the finish.  `row_weights` == nullptr with weighted == false
// is bsms_error_sums, launch for launch.
int error_sums_impl(const char* who, bool weighted, const float* pred, const float* target, const float* mask,
                    const float* row_weights, int64_t S, int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride,
                    int64_t mask_stride, int64_t weight_stride, double* sums, void* work, bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: C=%lld (C in 1..8)", who, (long long)C);
  BSMS_REQUIRE(S >= 0 && seg_rows >= 0 && seg_rows <= INT32_MAX, BSMS_E_INVALID_ARG, "%s: S=%lld seg_rows=%lld (seg_rows in 0..2^31-1)", who,
               (long long)S, (long long)seg_rows);
  BSMS_REQUIRE(pred_stride >= 0 && target_stride >= 0 && mask_stride >= 0 && weight_stride >= 0, BSMS_E_INVALID_ARG,
               "%s: negative segment stride (%lld, %lld, %lld, %lld)", who, (long long)pred_stride, (long long)target_stride,
               (long long)mask_stride, (long long)weight_stride);
  if (S == 0) return BSMS_OK;
  const int64_t pieces = pieces_of(seg_rows);
  BSMS_REQUIRE(sums && (pieces == 0 || (pred && target && mask && work && (row_weights || !weighted))), BSMS_E_INVALID_ARG,
               "%s: null argument", who);
  const int ncol = 1 + 3 * int(C);
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
  for (int64_t first = 0; first < blocks; first += kMaxBlocksPerLaunch) {
    a.blk0 = first;
    const unsigned nb = unsigned(std::min(kMaxBlocksPerLaunch, blocks - first));
    if (weighted) hipLaunchKernelGGL(k_error_pieces_w, dim3(nb), dim3(kThreads), 0, s, a, row_weights, weight_stride, partials);
    else hipLaunchKernelGGL(k_error_pieces, dim3(nb), dim3(kThreads), 0, s, a, partials);
    BSMS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_error_finish, dim3(unsigned(ceil_div(S * ncol, kThreads))), dim3(kThreads), 0, s, (const double*)partials, S, pieces,
                     ncol, sums);
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
