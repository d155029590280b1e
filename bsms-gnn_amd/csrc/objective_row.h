// The two ends of a row of the objective backward that sim.hip (sim_objective_bwd_row: bsms_sim_objective_bwd, _w) and
// ext/edge_objective.hip (k_edge_objective_bwd: bsms_sim_edge_objective_bwd) share -- ONE copy of the arithmetic, so the two entries agree bit for bit
// wherever the edge term adds nothing.  Both files are compiled with -ffp-contract=off.
//   objective_channel / objective_loss / objective_scale: sd_c, a_c, the terms of Q, loss and G from the fp64 sums [M | SE]
//   objective_tail: gp = w * gp, + the carried gradient, g_pred, and the way out through the fp64 de-normalisation
#pragma once
#include "common.h"

namespace bsms {

// Channel c of the head: sd_c (the target normaliser's std), a_c = w_c or w_c / sd_c^2, and the channel's term a_c SE_c / MC of Q.
// The callers keep sd_c and a_c in arrays of their own and add the terms in ascending c: a function that handed the arrays back in
// a struct left them in scratch memory in the kernels whose C is a run-time value (168 bytes per lane in k_sim_objective_bwd).
struct ObjectiveChannel {
  double sd, a, term;
};

__device__ __forceinline__ ObjectiveChannel objective_channel(int c, const double* mean, const double* meansq, double e, const double* sums,
                                                              const double* weights, int normalized, double MC) {
  ObjectiveChannel ch;
  ch.sd = std_eps(mean[c], meansq[c], e);
  const double wc = weights ? weights[c] : 1.0;
  ch.a = normalized ? wc / (ch.sd * ch.sd) : wc;
  ch.term = ch.a * sums[1 + c] / MC;
  return ch;
}

// loss = Q (mse) or sqrt(Q) (rmse); G = 2 / MC (mse) or 1 / (loss MC) (rmse)
__device__ __forceinline__ double objective_loss(double Q, int rmse) { return rmse ? sqrt(Q) : Q; }
__device__ __forceinline__ double objective_scale(double loss, double MC, int rmse) { return rmse ? 1.0 / (loss * MC) : 2.0 / MC; }

// Element (r, c): `gp` is the loss gradient before the step weight.  carried: g_pred_next != nullptr && m != 0.
__device__ __forceinline__ void objective_tail(float gp, float w, float m, bool carried, int64_t r, int c, int C, double sd,
                                               const double* in_mean, const double* in_meansq, double ie, const float* g_pred_next,
                                               const float* g_norm_in_next, float* g_pred, float* grad_norm_pred) {
  gp = w * gp;
  if (carried) {
    const float through_norm = float(double(g_norm_in_next[r * (C + 1) + c]) / std_eps(in_mean[c], in_meansq[c], ie));
    const float g_state = g_pred_next[r * C + c] + through_norm;
    gp = gp + g_state;
  }
  if (g_pred) g_pred[r * C + c] = gp;
  const float gd = gp * m;
  grad_norm_pred[r * C + c] = float(double(gd) * sd);
}

}  // namespace bsms
