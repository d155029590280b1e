// The one deterministic fp64 piece sum behind the evaluation sums (errsum.hip), the edge-difference sums
// (edgediff.hip), the dataset moments (stats/moments.hip) and the edge fold (ext/edge_objective.hip).  The rule, no atomics anywhere:
//   1. a segment is cut into pieces counted from ITS OWN first row (`split`), one block per piece;
//   2. a thread adds what is its own in ascending order (the callers' part), `block_sum` adds the lanes of a wave by a fixed shuffle
//      tree 32, 16, .., 1 and then the waves in order, and stores one partial per column and piece;
//   3. `k_piece_finish` adds the pieces of a segment in index order (`add_in_order`);
//   4. `k_row_fold` adds the rows of the segments in ascending order, where a caller wants one row for them all.
// Every addition and its place in the order are fixed by the segment's own rows: its sums are bit-identical whatever S, the strides,
// the neighbours in the launch or the grouping into launches (`for_block_slices`) are.  Every file that includes this is compiled with
// -ffp-contract=off (build.py).
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

namespace bsms {
namespace psum {

// Which accumulator slots of a thread are output columns.  Dense: slot k is column k.  (errsum.hip keeps its slots kMaxC apart and
// its columns C apart: its own policy.)
template <int kCols>
struct Dense {
  __device__ __forceinline__ bool live(int) const { return true; }
  __device__ __forceinline__ int ncol() const { return kCols; }
  __device__ __forceinline__ int slot(int col) const { return col; }
};

// out[col] = the block's sum of acc[cols.slot(col)]: the lanes of a wave by the shuffle tree, then the waves in order.
template <int kThreads, int kSlots, class Cols>
__device__ __forceinline__ void block_sum(const double (&acc)[kSlots], const Cols cols, double* __restrict__ out) {
  __shared__ double red[kThreads / 64][kSlots];
  const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    if (cols.live(k)) {
      double v = acc[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][k] = v;
    }
  }
  __syncthreads();
  if (int(threadIdx.x) < cols.ncol()) {
    const int col = int(threadIdx.x), k = cols.slot(col);
    double v = red[0][k];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) v += red[w][k];
    out[col] = v;
  }
}

// p[0] + p[stride] + .. in index order (none: 0): loads ahead, adds in order
__device__ __forceinline__ double add_in_order(const double* __restrict__ p, int64_t n, int64_t stride) {
  double v = 0.0;
#pragma unroll 8
  for (int64_t k = 0; k < n; ++k) v += p[k * stride];
  return v;
}

namespace {   // the kernels and their launchers: a copy with internal linkage in every translation unit that launches one

// sums[s, col] = the pieces of segment s added in index order (zero pieces: zeros); one thread per output element.  Rows of `sums`
// are sums_stride doubles apart (>= ncol; what lies between the rows is not written).
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_piece_finish(const double* __restrict__ partials, int64_t S, int64_t pieces, int ncol,
                                                          int64_t sums_stride, double* __restrict__ sums) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  if (i >= S * ncol) return;
  const int64_t s = i / ncol;
  const int col = int(i - s * ncol);
  sums[s * sums_stride + col] = add_in_order(partials + s * pieces * ncol + col, pieces, ncol);
}

// out[col] = sum_s rows[s * ld + col] for col < ncols: the rows in ascending order, one thread per column
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_row_fold(const double* __restrict__ rows, int64_t S, int64_t ncols, int64_t ld,
                                                      double* __restrict__ out) {
  const int64_t col = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  if (col < ncols) out[col] = add_in_order(rows + col, S, ld);
}

// (templates, so that a translation unit holds only the kernels it launches)
template <int kThreads = 256>
void launch_finish(const double* partials, int64_t S, int64_t pieces, int ncol, int64_t sums_stride, double* sums, hipStream_t s) {
  hipLaunchKernelGGL(k_piece_finish<kThreads>, dim3(unsigned(ceil_div(S * ncol, kThreads))), dim3(kThreads), 0, s, partials, S, pieces, ncol,
                     sums_stride, sums);
}

template <int kThreads = 64>
void launch_fold(const double* rows, int64_t S, int64_t ncols, int64_t ld, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_row_fold<kThreads>, dim3(unsigned(ceil_div(ncols, kThreads))), dim3(kThreads), 0, s, rows, S, ncols, ld, out);
}

}  // namespace

// Block blk0 + blockIdx.x of a launch over S * pieces blocks: which segment, and which piece (or row block) of it
struct Split {
  int64_t blk, seg, piece;
};
__device__ __forceinline__ Split split(int64_t blk0, int64_t pieces) {
  const int64_t blk = blk0 + int64_t(blockIdx.x), seg = blk / pieces;
  return {blk, seg, blk - seg * pieces};
}

// launch(first, nb) over [0, blocks) in slices of at most max_blocks blocks (a dispatch holds fewer than 2^32 work items), the launch
// check after each
template <class Launch>
int for_block_slices(int64_t blocks, int64_t max_blocks, Launch&& launch) {
  for (int64_t first = 0; first < blocks; first += max_blocks) {
    launch(first, unsigned(std::min(max_blocks, blocks - first)));
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}

// f(std::integral_constant<int, C>) for C in 1..8 (checked by the caller): the one switch that picks a template instance by channel count
template <class F>
void by_channels(int C, F&& f) {
  switch (C) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 8>()); break;
  }
}

}  // namespace psum
}  // namespace bsms
