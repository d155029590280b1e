/* bsms_hip_stats.h -- C ABI of libbsms_hip_stats.so, the second companion of libbsms_hip.so (bsms_hip.h).
 *
 * The surfaces of libbsms_hip.so and of libbsms_hip_ext.so (bsms_hip_ext.h) are closed: their entries are pinned one by one.  The
 * dataset statistics are declared here and built into a third shared library, which links against the first: the same conventions
 * (extern "C", caller-owned device pointers, `stream` as void*, 0 or a negative bsms_status, the message behind bsms_last_error() of
 * libbsms_hip.so).  Load libbsms_hip.so first, or let the loader find it next to this library (the link carries $ORIGIN as its run
 * path).  Nothing here is called by the training step: a process that never asks for statistics never loads this library. */
#ifndef BSMS_HIP_STATS_H
#define BSMS_HIP_STATS_H
#include "bsms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Normaliser moments of resident trajectories: the exact first and second moments of what the reference's
 * Normalizer._accumulate samples during warm-up -- the network's inputs [state | type] and its targets, the deltas -- over EVERY
 * pair of frames (t, t+1) of a table of trajectories, in one streaming pass.
 *
 * A table entry is one trajectory: `state` [T, n, C] with contiguous frames, `type` one column [n] shared by the frames
 * (type_stride == 0) or one per frame [T, n] (type_stride == n), and the pairs (t, t+1) for t = frame0 .. frame0 + frames - 1.  The
 * CALLER guarantees that frame frame0 + frames exists: frames + 1 frames of state are read, frames of type.
 *
 * bsms_moment_sums writes row s of `sums` (DEVICE double [S, W], W = 4C + 4) for entry s, over its R = frames * n rows (t, i):
 *   [ R | M | SX[0..C) | ST | QX[0..C) | QT | SD[0..C) | QD[0..C) ]
 *   m    = 1 if type[t, i] equals one of the n_valid codes of `valid_types` (HOST), else 0 -- the rule of bsms_batch_assemble
 *   R    = frames * n,   M = sum m
 *   x    = double(state[t, i, c]):                 SX[c] = sum x,          QX[c] = sum x * x
 *   y    = double(type[t, i]):                     ST    = sum y,          QT    = sum y * y
 *   d    = fl32(state[t+1, i, c] - state[t, i, c]) -- the ONE fp32 rounding of the reference's delta, as bsms_error_sums takes it
 *                                                  SD[c] = sum double(d),  QD[c] = sum double(d) * double(d)
 * Every product and sum after the loads (and that one subtraction) is a separate fp64 operation.  Nothing but M looks at the mask:
 * the reference's normalisers see every row.  An entry with frames * n == 0 yields a row of zeros.  `sums` is overwritten, never
 * added to.
 *
 * Determinism: no atomics.  A frame is read as a flat array of E = n * C floats.  An entry is cut into PIECES: slab j (the elements
 * [1024 j, 1024 (j + 1)) of every frame) x frame chunk k (the pairs frame0 + 32 k .. frame0 + 32 k + 31), piece index k * slabs + j.
 * One block of 256 threads reduces a piece: thread i owns the four elements 1024 j + i + 256 q (q = 0..3) and walks the chunk's
 * frames in ascending order through a ring of four frames in registers (two being summed, two in flight), so every frame is read
 * once (a chunk re-reads its first frame: 1/32 more).  Per frame the type terms of the rows whose first channel the thread owns are
 * added up in the order of q and then to the thread's M, ST and QT; at the end the thread's four elements fold into the channel
 * columns in the order of q; the lanes of a wave combine by a fixed shuffle tree,
 * the four waves in order.  A second kernel adds the pieces of an entry in index order.  A row is therefore a fixed function of the
 * entry's own (n, frames, C) and data: bit-identical from run to run, whatever S is, whatever else the table holds, and wherever the
 * entry falls in the launch chunking below.
 *
 * Launches: the table travels as kernel arguments, at most 64 entries per launch pair (fewer when their pieces would exceed the work
 * area); `work` (DEVICE, bsms_moment_work_bytes(max_rows) bytes, max_rows >= the largest frames * n of the table; its contents on
 * entry do not matter) holds the pieces of ONE launch and is reused by the next in stream order, so its size does not grow with S.
 * Nothing is allocated, synchronised or read back: capturable.
 *
 * Checks, all before any device call, in this order: C in 1..8 and n_valid in 1..4 (BSMS_E_UNSUPPORTED); S >= 0
 * (BSMS_E_INVALID_ARG); S == 0 returns BSMS_OK and touches nothing; null trajs / valid_types / sums / work (BSMS_E_INVALID_ARG); per
 * entry n, frame0, frames >= 0, type_stride 0 or n, no null field where frames * n > 0 (BSMS_E_INVALID_ARG), frames * n < 2^40
 * (BSMS_E_SHAPE).
 *
 * bsms_moment_fold adds the S rows of `sums` [S, W] into out [W]: ascending index order, fp64, one thread per column, no atomics;
 * S == 0 writes zeros.  W in 1..65536 (BSMS_E_UNSUPPORTED); S < 0 or a null pointer (sums may be NULL with S == 0) gives
 * BSMS_E_INVALID_ARG; all before any device call.  One launch, capturable.  It is not tied to the layout above: any [S, W] fp64. */
typedef struct {
  const float* state; /* DEVICE [T, n, C], frames contiguous */
  const float* type;  /* DEVICE [n] (type_stride == 0) or [T, n] (type_stride == n) */
  int64_t n, frame0, frames, type_stride;
} bsms_moment_traj;

size_t bsms_moment_work_bytes(int64_t max_rows /* largest frames * n of the table */);
int bsms_moment_sums(const bsms_moment_traj* trajs /* HOST [S] */, int64_t S, int64_t C, const float* valid_types /* HOST */,
                     int64_t n_valid, double* sums /* DEVICE [S, 4C + 4] */, void* work, bsms_stream_t stream);
int bsms_moment_fold(const double* sums /* [S, W] */, int64_t S, int64_t W, double* out /* [W] */, bsms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_STATS_H */
