// The objective with an edge-difference term (include/bsms_hip_ext.h: bsms_edge_diff_fold, bsms_sim_edge_objective_bwd),
// built into the companion library libbsms_hip_ext.so: the surface of libbsms_hip.so is closed (its entries are pinned one by one),
// so entries that come later live here, on the same plans, error reporting and device code.
// The fold is the row fold of piece_sum.h over the columns [ME | DE] of the segments' rows.  The backward is the row of k_sim_objective_bwd
// (sim.hip; objective_row.h: the one head and the one tail) with the adjoint's gather (edge_gather.h: the one copy k_edge_bwd runs too) added to the loss
// gradient in front of the step weight.  Compiled with -ffp-contract=off (build.py).
#include <cmath>

#include "../edge_gather.h"
#include "../objective_row.h"
#include "../piece_sum.h"
#include "../../../include/bsms_hip_ext.h"

#pragma clang fp contract(off)

using namespace bsms;
using namespace bsms::edge;

namespace {

// The objective with an edge term, backward (include/bsms_hip_ext.h: bsms_sim_edge_objective_bwd): the row of
// k_sim_objective_bwd (objective_row.h: the one head and the one tail) with the edge term's gradient added to the loss gradient before the
// step weight.  Thread gr owns row gr of the R = S * seg_rows rows; segment s = gr / seg_rows, the plan's row r = gr - s * seg_rows.
struct EdgeObjArgs {
  LossBwdArgs row;                                      // sums = fp64 [M | SE]
  const double* edge_sums;                              // [ME | DE] (the fold's row)
  float* parts_out;
  double lambda;
  int64_t R;
  int normalized, rmse;
};

template <int C, bool kQuot>
__global__ __launch_bounds__(kBwdThreads) void k_edge_objective_bwd(const EdgeArgs a, const EdgeObjArgs o) {
  const int64_t gr = int64_t(blockIdx.x) * kBwdThreads + int(threadIdx.x);
  const bool row = gr < o.R;                            // (the thread of row 0 always has one: R >= 1)
  // the gather first: while its loads are in flight a lane holds its own row and the accumulators, not the 2C coefficients
  Node<C> me{};
  double acc[C];
  if (row) {
    const int s = int(gr) / int(a.seg_rows), r = int(gr) - s * int(a.seg_rows);      // R < 2^31 (checked): 32-bit division
    const int64_t row0 = int64_t(s) * a.seg_rows;                     // first row of the segment
    const float* pred = a.pred + row0 * C;
    const float* target = a.target + row0 * C;
    const float* mask = a.mask + row0;
    const float* pos = kQuot ? a.pos + row0 * a.p : nullptr;
    me = load_node<C, kQuot>(pred, target, mask, pos, a.p, r);
    edge_gather<C, kQuot>(a, pred, target, mask, pos, r, me, acc);
  }
  const double* sums = static_cast<const double*>(o.row.sums);
  const double e = *o.row.eps;
  const double MC = sums[0] * double(C);
  double sd[C], ac[C];
  double Q = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const ObjectiveChannel ch = objective_channel(c, o.row.mean, o.row.meansq, e, sums, o.row.weights, o.normalized, MC);
    sd[c] = ch.sd;
    ac[c] = ch.a;
    if (gr == 0 && o.row.chan_out) o.row.chan_out[c] = float(ch.term);
    Q += ch.term;
  }
  const double loss = objective_loss(Q, o.rmse);
  const double G = objective_scale(loss, MC, o.rmse);
  const double MEC = o.edge_sums[0] * double(C);
  double H = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) H += ac[c] * o.edge_sums[1 + c] / MEC;
  const double T = o.rmse ? sqrt(H) : H;
  if (gr == 0) {
    if (o.row.loss_out) *o.row.loss_out = float(loss + o.lambda * T);
    if (o.parts_out) { o.parts_out[0] = float(loss); o.parts_out[1] = float(T); }
  }
  if (!row) return;
  const float m = me.m;
  const LossBwdCarry carry = loss_bwd_carry(o.row, m);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double k = o.rmse ? (o.lambda * ac[c]) / ((2.0 * T) * MEC) : (o.lambda * ac[c]) / MEC;
    const float ge = float((2.0 * k) * acc[c]);                     // one rounding, as k_edge_bwd
    const float coef = float(G * ac[c]);
    float gp = me.d[c] * m * coef;
    gp = gp + ge;
    objective_tail(gp, m, carry, gr, c, C, sd[c], o.row);
  }
}

template <int C>
void launch_objective_bwd(bool quot, unsigned nb, hipStream_t s, const EdgeArgs& a, const EdgeObjArgs& o) {
  if (quot) hipLaunchKernelGGL((k_edge_objective_bwd<C, true>), dim3(nb), dim3(kBwdThreads), 0, s, a, o);
  else hipLaunchKernelGGL((k_edge_objective_bwd<C, false>), dim3(nb), dim3(kBwdThreads), 0, s, a, o);
}

}  // namespace

extern "C" int bsms_edge_diff_fold(const double* sums, int64_t S, int64_t C, double* out, bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "edge_diff_fold: C=%lld (C in 1..8)", (long long)C);
  BSMS_REQUIRE(S >= 0, BSMS_E_INVALID_ARG, "edge_diff_fold: S=%lld", (long long)S);
  BSMS_REQUIRE(out && (sums || S == 0), BSMS_E_INVALID_ARG, "edge_diff_fold: null argument");
  psum::launch_fold(sums, S, 1 + C, 1 + 2 * C, out, as_stream(stream));     // out[0] = sum_s ME_s, out[1 + c] = sum_s DE_s[c]
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

// The checks in the order of the header: what is unsupported before any pointer is looked at, then the arguments, then the plan's shape.
extern "C" int bsms_sim_edge_objective_bwd(const bsms_plan_t* plan, int64_t seg_rows, int64_t S, const float* pred, const float* target,
                                           const float* mask, const float* pos, int64_t C, int64_t p, int weighting, const double* mean,
                                           const double* meansq, const double* std_eps_dev, const double* in_mean,
                                           const double* in_meansq, const double* in_std_eps_dev, const double* sums,
                                           const double* edge_sums, const double* channel_weights, int space, int kind,
                                           double edge_lambda, float w, const float* g_pred_next, const float* g_norm_in_next,
                                           float* loss_out, float* parts_out, float* chan_out, float* g_pred, float* grad_norm_pred,
                                           bsms_stream_t stream) {
  const char* who = "sim_edge_objective_bwd";
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: C=%lld (C in 1..8)", who, (long long)C);
  BSMS_REQUIRE(weighting == BSMS_EDGE_DIFFERENCE || weighting == BSMS_EDGE_QUOTIENT, BSMS_E_UNSUPPORTED, "%s: weighting=%d (0 or 1)", who,
               weighting);
  const bool quot = weighting == BSMS_EDGE_QUOTIENT;
  BSMS_REQUIRE(!quot || (p >= 1 && p <= kMaxP), BSMS_E_UNSUPPORTED, "%s: p=%lld (p in 1..3 with the quotient weighting)", who, (long long)p);
  if (int rc = check_space_kind(who, space, kind)) return rc;
  BSMS_REQUIRE(S >= 1 && seg_rows >= 1 && seg_rows <= INT32_MAX && S <= INT32_MAX / seg_rows, BSMS_E_INVALID_ARG,
               "%s: S=%lld seg_rows=%lld (each >= 1, S * seg_rows below 2^31)", who, (long long)S, (long long)seg_rows);
  BSMS_REQUIRE(std::isfinite(edge_lambda) && edge_lambda >= 0.0, BSMS_E_INVALID_ARG, "%s: edge_lambda=%g (finite and >= 0)", who, edge_lambda);
  BSMS_REQUIRE(plan, BSMS_E_INVALID_ARG, "%s: plan is null", who);
  BSMS_REQUIRE(pred && target && mask && (pos || !quot) && mean && meansq && std_eps_dev && sums && edge_sums && grad_norm_pred,
               BSMS_E_INVALID_ARG, "%s: null argument", who);
  if (int rc = check_carry(who, g_pred_next, g_norm_in_next, in_mean, in_meansq, in_std_eps_dev, g_pred)) return rc;
  BSMS_REQUIRE(seg_rows == plan->N, BSMS_E_SHAPE, "%s: seg_rows=%lld, the plan has %lld rows", who, (long long)seg_rows, (long long)plan->N);
  EdgeArgs a{};
  a.rowptr = plan->rowptr; a.src = plan->src; a.t_rowptr = plan->t_rowptr; a.t_dst = plan->t_dst;
  a.pred = pred; a.target = target; a.mask = mask; a.pos = quot ? pos : nullptr;
  a.row0 = 0; a.seg_rows = seg_rows; a.pieces = 0;
  a.pred_stride = a.target_stride = a.mask_stride = a.pos_stride = seg_rows;
  a.blk0 = 0;
  a.p = quot ? int(p) : 0;
  EdgeObjArgs o{};
  o.row = {mean, meansq, std_eps_dev, in_mean, in_meansq, in_std_eps_dev, sums, channel_weights, w, g_pred_next, g_norm_in_next, loss_out,
           chan_out, g_pred, grad_norm_pred};
  o.edge_sums = edge_sums; o.parts_out = parts_out; o.lambda = edge_lambda; o.R = S * seg_rows;
  o.normalized = int(space == BSMS_LOSS_NORMALIZED); o.rmse = int(kind == BSMS_LOSS_RMSE);
  const unsigned nb = unsigned(ceil_div(o.R, kBwdThreads));
  hipStream_t s = as_stream(stream);
  psum::by_channels(int(C), [&](auto c) { launch_objective_bwd<decltype(c)::value>(quot, nb, s, a, o); });
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}
