/* bsms_hip_sample.h -- C ABI of libbsms_hip_sample.so, the third companion of libbsms_hip.so (bsms_hip.h).
 *
 * The surfaces of libbsms_hip.so, libbsms_hip_ext.so (bsms_hip_ext.h) and libbsms_hip_stats.so (bsms_hip_stats.h) are closed.  The
 * sampling of nodal fields on a 2-D cell complex -- locate points in the triangles, interpolate linearly -- is declared here and
 * built into a fourth shared library, which links against the first: the same conventions (extern "C", caller-owned device
 * pointers, `stream` as void*, 0 or a negative bsms_status, the message behind bsms_last_error() of libbsms_hip.so).  Load
 * libbsms_hip.so first, or let the loader find it next to this library (the link carries $ORIGIN as its run path).  Nothing here is
 * called by the training step: a process that never samples a field never loads this library.
 *
 * GEOMETRY CONTRACT.  Positions are fp32 [N, 2] with a row stride `pos_stride` (in floats, >= 2), promoted to
 * fp64; triangles are int32 [T, 3] = (a, b, c), contiguous.  For a query point q in fp64
 *   orient(u, v, q) = (v.x - u.x) * (q.y - u.y) - (v.y - u.y) * (q.x - u.x)
 *   e0 = orient(b, c, q),  e1 = orient(c, a, q),  e2 = orient(a, b, q),  A = orient(a, b, c)
 * every difference, product and the final subtraction a separate fp64 operation (no contraction).  A triangle CONTAINS q iff
 * A != 0, A is finite and e_i * sign(A) >= 0 for i = 0, 1, 2: edges and vertices are inclusive, either orientation is accepted, a
 * zero-area triangle and a triangle with a NaN or infinite vertex contain nothing.  A triangle that names a node outside [0, N)
 * contains nothing either.  The OWNER of q is the lowest triangle index that contains it, or -1.  The interpolated value of a
 * nodal field f at q is
 *   s = (e0 + e1) + e2,   w_i = e_i / s,   fl32((w0 * f[a] + w1 * f[b]) + w2 * f[c])
 * in fp64 from the promoted fp32 nodal values, rounded once.  Pixel (j, i) of a W x H grid has its centre at
 *   (x0 + (i + 0.5) * dx,  y0 + (j + 0.5) * dy)
 * computed in fp64 from the double arguments (i + 0.5 is exact; one product, one sum).  dx and dy are finite and non-zero; a
 * negative step is allowed.
 *
 * Common checks, before any device call: null pointers (an array of no elements may be null), N, T, P >= 0, pos_stride >= 2, W and
 * H in 1..32768, x0, y0 finite, dx, dy finite and non-zero (BSMS_E_INVALID_ARG); N, T <= 2^31 - 2 (BSMS_E_SHAPE).  Nothing is
 * allocated, synchronised or read back: every entry is capturable.
 *
 * bsms_raster_owner writes owner [H, W] (int32) for the pixel centres of the grid.  Triangle-driven: a triangle visits the pixel
 * centres of its bounding box -- widened by one pixel on every side against the rounding of the index computation, clipped to the
 * grid through clamped conversions (a box that misses the grid, or whose bounds are not ordered numbers, is empty) -- and takes
 * atomicMin(owner[j, i], t), as unsigned 32-bit words with -1 = 0xFFFFFFFF above every index, wherever it contains the centre.  The
 * entry initialises the image itself, so its contents on entry do not matter, and the result does not depend on the schedule.
 * Three ways to walk a box, by its pixel count n: n <= small_box: the eight lanes that hold the triangle; n <= 16384: the 64 lanes of
 * the triangle's wave, one box after the other; above: the triangle is appended to a list in `work` and a second kernel spreads
 * each listed box over the whole grid of 256 blocks (a list that is full leaves the triangle to its wave).  small_box <= 0 selects
 * the measured default.  `work`: bsms_raster_work_bytes() bytes, contents on entry do not matter.
 *
 * bsms_point_owner writes owner [P] for query points q [P, 2] (fp64, contiguous): one wave per point strides the triangles, every
 * lane keeps the lowest index it found, a shuffle tree takes the minimum.  Brute force, P * T containment tests.
 *
 * bsms_field_gather interpolates S sets of C channels at the samples whose owners are given: fields[s * set_stride + n * row_stride
 * + c] (fp32, strides in floats, set_stride any value, row_stride >= C) is read in place.  points == NULL: the W x H grid, owner
 * [H, W], out [S, C, H, W]; points != NULL: q [P, 2], owner [P], out [S, P, C] (W, H, x0, y0, dx, dy are then ignored).  One thread per
 * sample computes the weights once and reuses them over the S * C values; a sample whose owner is not in [0, T), or whose owner is
 * a triangle that names no valid nodes, gets `fill` (NaN allowed).  The weights are those of the contract whether or not the owner
 * contains the sample.  C in 1..8 (BSMS_E_UNSUPPORTED), S >= 0, row_stride >= C. */
#ifndef BSMS_HIP_SAMPLE_H
#define BSMS_HIP_SAMPLE_H
#include "bsms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t bsms_raster_work_bytes(void);
int bsms_raster_owner(const float* pos /* [N, pos_stride] */, int64_t pos_stride, int64_t N, const int32_t* tris /* [T, 3] */, int64_t T,
                      int64_t W, int64_t H, double x0, double y0, double dx, double dy, int64_t small_box, int32_t* owner /* [H, W] */,
                      void* work, bsms_stream_t stream);
int bsms_point_owner(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const double* points /* [P, 2] */,
                     int64_t P, int32_t* owner /* [P] */, bsms_stream_t stream);
int bsms_field_gather(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* owner,
                      const double* points /* [P, 2] or NULL: the grid */, int64_t P, int64_t W, int64_t H, double x0, double y0, double dx,
                      double dy, const float* fields, int64_t S, int64_t C, int64_t set_stride, int64_t row_stride, float fill,
                      float* out, bsms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_SAMPLE_H */
