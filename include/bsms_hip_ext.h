/* bsms_hip_ext.h -- C ABI of libbsms_hip_ext.so, the companion of libbsms_hip.so (bsms_hip.h).
 *
 * The surface of libbsms_hip.so is closed: its entries, their argument counts and bsms_abi_version() == 4 are pinned one by one.
 * Entries that come later are declared here and built into a second shared library, which links against the first: the same
 * conventions (extern "C", caller-owned device pointers, `stream` as void*, 0 or a negative bsms_status, the message behind
 * bsms_last_error() of libbsms_hip.so), the same plans (bsms_plan_t of bsms_plan_create) and the same device code underneath.
 * Load libbsms_hip.so first, or let the loader find it next to this library (the link carries $ORIGIN as its run path). */
#ifndef BSMS_HIP_EXT_H
#define BSMS_HIP_EXT_H
#include "bsms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Training: the objective with an edge-difference term.
 * J = L + lambda * T: L the pointwise loss of bsms_sim_objective_bwd, T the edge-difference (discrete H1) term from
 * the sums of bsms_edge_diff_sums over ALL samples of the batch (and, under data parallelism, all ranks):
 *   H = sum_c a_c DE[c] / (ME C),   T = H (BSMS_LOSS_MSE) | sqrt(H) (BSMS_LOSS_RMSE),   a_c exactly those of bsms_sim_objective_bwd.
 *
 * bsms_edge_diff_fold adds the S rows [ME | DE | TE] of bsms_edge_diff_sums into ONE row out = [ ME | DE[0..C) ] (DEVICE double
 * [1 + C]): out[0] = sum_s ME_s, out[1 + c] = sum_s DE_s[c], the segments in ascending index order in fp64, one thread per column, no
 * atomics; S == 0 writes zeros.  C in 1..8 (BSMS_E_UNSUPPORTED); S < 0 or a null pointer (sums may be NULL with S == 0) gives
 * BSMS_E_INVALID_ARG; all before any device call.  One launch, capturable.
 *
 * bsms_sim_edge_objective_bwd is bsms_sim_objective_bwd with the edge term: ONE launch over the R = S * seg_rows rows of pred /
 * target / mask [R(, C)] and pos [R, p]; segment s is rows [s * seg_rows, (s + 1) * seg_rows) of each, and its graph is `plan`, which
 * has exactly seg_rows rows (the window of bsms_edge_diff_bwd with row0 = 0).  Thread r owns row r.  `sums` = [M | SE] as there;
 * `edge_sums` = [ME | DE], the fold's row (all-reduced by the caller under data parallelism).  Per row, in this order:
 *   a_c, MC, Q, L, G, sd_c    exactly as bsms_sim_objective_bwd forms them (sd_c = the target normaliser's std)
 *   MEC  = edge_sums[0] * double(C);   H = sum_c (a_c * edge_sums[1 + c] / MEC), c ascending;   T = rmse ? sqrt(H) : H
 *   loss_out = float(L + edge_lambda * T);   parts_out = { float(L), float(T) } (nullable float[2]);   chan_out as there
 *   k_c  = rmse ? (edge_lambda * a_c) / ((2.0 * T) * MEC) : (edge_lambda * a_c) / MEC                                (fp64)
 *   acc_c = ONE fp64 accumulator: the row's incoming edges in CSR order, then its outgoing edges in transpose order, of
 *           mu_e w_e (d[r,c] - d[other,c]) -- the loop of bsms_edge_diff_bwd: the same mu, w and zero-length rule, d = fl32(pred - target)
 *   ge   = float((2.0 * k_c) * acc_c)                                  (one rounding, as bsms_edge_diff_bwd)
 *   gp   = (d * m) * float(G a_c);   gp = gp + ge;   gp = w * gp;   gp = gp + carry   (carried rows, as bsms_sim_unroll_bwd)
 *   g_pred = gp;   grad_norm_pred = float(double(gp * m) * sd_c)
 * Every fp32 operation is a separate rounding.  With edge_lambda == 0 every output has the value bsms_sim_objective_bwd writes.
 * ME == 0, and T == 0 under rmse, are not guarded, like M == 0 there.  The gradient of w_e with respect to pos is not formed.
 * Checks, in this order, all before any device call: C in 1..8, weighting 0 or 1, p in 1..3 with BSMS_EDGE_QUOTIENT, space and kind
 * in {0, 1} (BSMS_E_UNSUPPORTED, before any pointer is looked at); S >= 1, seg_rows >= 1, S * seg_rows < 2^31, edge_lambda finite
 * and >= 0, a null plan, null required pointers, half a carried pair (BSMS_E_INVALID_ARG); seg_rows != the plan's rows
 * (BSMS_E_SHAPE).  No allocation, no synchronisation, nothing read back: capturable. */
int bsms_edge_diff_fold(const double* sums /* [S, 1 + 2C] */, int64_t S, int64_t C, double* out /* [1 + C] */, bsms_stream_t stream);
int bsms_sim_edge_objective_bwd(const bsms_plan_t* plan, int64_t seg_rows, int64_t S, const float* pred, const float* target,
                                const float* mask, const float* pos /* nullable with BSMS_EDGE_DIFFERENCE */, int64_t C, int64_t p,
                                int weighting, const double* mean, const double* meansq, const double* std_eps,
                                const double* in_mean /* nullable */, const double* in_meansq /* nullable */,
                                const double* in_std_eps /* nullable */, const double* sums, const double* edge_sums,
                                const double* channel_weights /* nullable */, int space, int kind, double edge_lambda, float w,
                                const float* g_pred_next /* nullable */, const float* g_norm_in_next /* nullable */,
                                float* loss_out /* nullable */, float* parts_out /* nullable */, float* chan_out /* nullable */,
                                float* g_pred /* nullable */, float* grad_norm_pred, bsms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_EXT_H */
