/* bsms_hip_diffop.h -- C ABI of libbsms_hip_diffop.so, the fifth companion of libbsms_hip.so (bsms_hip.h).
 *
 * The surfaces of libbsms_hip.so and of the four other companions (bsms_hip_ext.h, bsms_hip_stats.h, bsms_hip_sample.h,
 * bsms_hip_query.h) are closed.  The P1 gradient of nodal fields on a 2-D triangle complex -- per cell, recovered at the nodes, its
 * squared sums (the H1 seminorm of an error field, the divergence and the vorticity of a velocity pair) and their adjoint -- is
 * declared here and built into a sixth shared library, which links against the first: the same conventions (extern "C",
 * caller-owned device pointers, `stream` as void*, 0 or a negative bsms_status, the message behind bsms_last_error() of
 * libbsms_hip.so).  Load libbsms_hip.so first, or let the loader find it next to this library (the link carries $ORIGIN as its run
 * path).  Nothing here is called by the training step: a process that never differentiates a field never loads this library.
 *
 * GEOMETRY CONTRACT.  Positions are fp32 [N, 2] with a row stride `pos_stride` (in floats, >= 2), promoted to
 * fp64; triangles are int32 [T, 3] = (a, b, c), contiguous.  Every difference, product, sum and quotient below is a separate fp64
 * operation in the order written (no contraction):
 *   A2    = orient(a, b, c) = (x_b - x_a) * (y_c - y_a) - (y_b - y_a) * (x_c - x_a)        (orient of bsms_hip_sample.h)
 *   kx    = (y_b - y_c,  y_c - y_a,  y_a - y_b)      ky = (x_c - x_b,  x_a - x_c,  x_b - x_a)      (the edge normals of the corners)
 *   nx(f) = (f_a * kx_0 + f_b * kx_1) + f_c * kx_2      ny(f) = (f_a * ky_0 + f_b * ky_1) + f_c * ky_2
 *   G(f)  = (nx(f) / A2, ny(f) / A2)                 the P1 gradient of the nodal field f on the triangle
 *   a_t   = |A2| * 0.5                               its area
 *   b_k   = (kx_k / A2, ky_k / A2)                   the gradient of the hat function of corner k
 * A triangle is VALID iff its three nodes lie in [0, N) and A2 is finite and non-zero; either orientation is accepted (the sampler's
 * rule).  An invalid triangle gets `fill` where a per-triangle value is written and adds nothing to any node value, sum or gradient;
 * nothing is read from `pos` or a field for a triangle that names a node outside the mesh.  Fields are read in place as
 * fields[s * set_stride + n * row_stride + c] (fp32, strides in floats, row_stride >= C, set_stride any value).  C in 1..8
 * (BSMS_E_UNSUPPORTED otherwise, checked before any pointer), S >= 0, N, T <= 2^31 - 2 (BSMS_E_SHAPE).
 *
 * Common checks, before any device call: C, then N, T >= 0, pos_stride >= 2, S >= 0, row strides >= C, null pointers (an array of no
 * elements may be null) (BSMS_E_INVALID_ARG).  Nothing is allocated, synchronised or read back: every entry is capturable.
 *
 * The node -> triangle INCIDENCE is a CSR: inc_ptr int32 [N + 1], inc_tri int32 [nnz], the triangles of node n at inc_tri[inc_ptr[n]
 * .. inc_ptr[n + 1]) in ascending triangle index, each once.  The kernels clamp the range to [0, nnz), skip an entry outside [0, T)
 * and skip a triangle that does not contain the node (its first corner equal to n counts), so a wrong list cannot reach memory
 * outside the arrays.  A node OWNS its sums: one thread adds them in the list's order, there are no atomics, and every result is
 * bit-identical run to run.
 *
 * bsms_cell_gradient writes out [S, T, C, 2] = fl32(G(f_{s,c})), `fill` on invalid triangles.  One thread per triangle and group of
 * eight sets: the geometry once, reused over the group's values.
 *
 * bsms_node_gradient writes out [S, N, C, 2], the area-weighted recovery
 *   g_n = (sum_t sign(A2_t) * n_t(f)) / (sum_t |A2_t|)            over the valid triangles t of n's list, in list order
 * numerator (from 0.0, term by term; sign(A2) * n is exact) and denominator in fp64, ONE division and ONE rounding to fp32 per
 * component; a node with no valid incident triangle gets `fill`.  A thread owns one node and a group of sets.  A node whose list is
 * longer than `long_list` entries is left to its wave, whose lanes then take one (set, channel) element each and walk the same list
 * in the same order: the result does not depend on `long_list`.  long_list <= 0 selects the default.
 *
 * bsms_cell_gradient_sums writes, per segment s, sums[s, :] = [ A | GE[0..C) | GT[0..C) | DP | DT | WE | WT ] (DEVICE double, rows of
 * 1 + 2C + 4) over the valid triangles:
 *   d     = fl32(pred - target)                      ONE fp32 rounding, as in bsms_error_sums; t = target; p = pred
 *   mu_t  = (double(m[a]) * double(m[b])) * double(m[c])        mask == NULL: 1.  mask[s * mask_stride + n]; mask_stride 0: one mask
 *   w_t   = mu_t * a_t
 *   A     = sum w_t
 *   GE[c] = sum w_t * (G(d_c).x * G(d_c).x + G(d_c).y * G(d_c).y)            GT[c]: the same of t_c
 *   div(f)  = G(f_cu).x + G(f_cv).y                  curl(f) = G(f_cv).x - G(f_cu).y
 *   DP = sum w_t * (div(p) * div(p))     DT: of t     WE = sum w_t * (curl(d) * curl(d))     WT: of t
 * cu < 0: no velocity pair, the last four columns are zeros (cv is ignored); otherwise cu != cv, both in [0, C).  pred and target have
 * their own set and row strides.  The sums follow csrc/piece_sum.h and nothing else: the triangles of a segment in pieces of 1024
 * counted from its own first triangle, one triangle per thread, block_sum per piece, k_piece_finish over the pieces.  A segment's row
 * is bit-identical whatever S, the strides or its neighbours in the launch.  S == 0 touches nothing; T == 0 writes rows of zeros.
 * `work`: bsms_cell_gradient_work_bytes(S, T) bytes; neither its contents nor those of `sums` on entry matter.
 *
 * bsms_cell_gradient_bwd is the exact adjoint, with respect to pred, of J_s = sum_c k_c GE[c] + k_D DP + k_W WE with coef DEVICE
 * double [S, C + 2] = [k_0 .. k_{C-1} | k_D | k_W]; the fl32 rounding of d is taken as the identity.  Node-owned through the
 * incidence: thread (s, n) keeps one fp64 accumulator per channel, starts them at 0.0 and, for every valid triangle t of n's list
 * in list order, with k the corner of t that is n,
 *   acc[c]  += (w_t * k_c) * (G(d_c).x * b_k.x + G(d_c).y * b_k.y)            c = 0 .. C-1 in order
 *   acc[cu] += (w_t * k_D) * (div(p) * b_k.x)          acc[cv] += (w_t * k_D) * (div(p) * b_k.y)
 *   acc[cu] += (w_t * k_W) * (curl(d) * (-b_k.y))      acc[cv] += (w_t * k_W) * (curl(d) * b_k.x)
 * (the last two lines with a velocity pair only), then grad[(s * grad_stride + n) * C + c] = fl32(2.0 * acc[c]): ONE rounding,
 * stored, or added in fp32 to what is there when `accumulate` != 0.  grad_stride >= N rows.  A zero mask on any corner and a zero
 * coefficient give exact zero terms (of finite fields). */
#ifndef BSMS_HIP_DIFFOP_H
#define BSMS_HIP_DIFFOP_H
#include "bsms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int bsms_cell_gradient(const float* pos /* [N, pos_stride] */, int64_t pos_stride, int64_t N, const int32_t* tris /* [T, 3] */, int64_t T,
                       const float* fields, int64_t S, int64_t C, int64_t set_stride, int64_t row_stride, float fill,
                       float* out /* [S, T, C, 2] */, bsms_stream_t stream);
int bsms_node_gradient(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* inc_ptr /* [N + 1] */,
                       const int32_t* inc_tri /* [nnz] */, int64_t nnz, const float* fields, int64_t S, int64_t C, int64_t set_stride,
                       int64_t row_stride, float fill, int64_t long_list, float* out /* [S, N, C, 2] */, bsms_stream_t stream);
size_t bsms_cell_gradient_work_bytes(int64_t S, int64_t T);
int bsms_cell_gradient_sums(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const float* pred,
                            int64_t pred_set_stride, int64_t pred_row_stride, const float* target, int64_t target_set_stride,
                            int64_t target_row_stride, const float* mask, int64_t mask_stride, int64_t S, int64_t C, int64_t cu, int64_t cv,
                            double* sums /* [S, 1 + 2C + 4] */, void* work, bsms_stream_t stream);
int bsms_cell_gradient_bwd(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* inc_ptr,
                           const int32_t* inc_tri, int64_t nnz, const float* pred, int64_t pred_set_stride, int64_t pred_row_stride,
                           const float* target, int64_t target_set_stride, int64_t target_row_stride, const float* mask, int64_t mask_stride,
                           int64_t S, int64_t C, int64_t cu, int64_t cv, const double* coef /* [S, C + 2] */, int accumulate,
                           float* grad /* [S, grad_stride, C] */, int64_t grad_stride, bsms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_DIFFOP_H */
