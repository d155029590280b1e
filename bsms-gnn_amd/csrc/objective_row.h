// What every loss-gradient entry shares -- sim.hip: bsms_sim_loss_bwd, _unroll_bwd, _objective_bwd, _objective_bwd_w,
// _robust_bwd; ext/edge_objective.hip: bsms_sim_edge_objective_bwd -- in ONE copy, so the entries agree bit for bit wherever they coincide
// (DESIGN.md 4.10, 4.11, 4.19, 4.20, 4.22).  Every file that includes this one is compiled with -ffp-contract=off.
//   LossBwdArgs: the statistics, sums, step weight, carried pair and outputs of an entry, as one kernel argument
//   objective_channel / objective_loss / objective_scale: sd_c, a_c, the terms of Q, loss and G from the fp64 sums [M | SE]
//   loss_bwd_carry / objective_tail: gp = w * gp, + the carried gradient, g_pred, and the way out through the fp64 de-normalisation
//   check_carry / check_space_kind: the refusals the entries share, with the entry's name in front
#pragma once
#include "common.h"

namespace bsms {

// Pointers and scalars only: per-channel arrays stay local arrays of the kernels (see objective_channel).
struct LossBwdArgs {
  const double *mean, *meansq, *eps;                 // the target normaliser
  const double *in_mean, *in_meansq, *in_eps;        // the input normaliser: read only with a carried pair
  const void* sums;                                  // fp32 [S, M] (k_sim_pair_bwd) or fp64 [M | SE] / [M | S] (the row kernels)
  const double* weights;                             // channel weights, or null for unit weights
  float w;                                           // the step weight
  const float *g_pred_next, *g_norm_in_next;         // the carried pair, or both null
  float *loss_out, *chan_out, *g_pred, *grad_norm_pred;
};

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

// Row r of mask m takes the carried gradient iff a pair is given and m != 0: Dirichlet rows took in_0, not pred_k.
struct LossBwdCarry {
  bool on;
  double ie;
};

__device__ __forceinline__ LossBwdCarry loss_bwd_carry(const LossBwdArgs& o, float m) {
  return {o.g_pred_next != nullptr && m != 0.f, o.g_pred_next ? *o.in_eps : 0.0};
}

// Element (r, c) of a row of C channels: `gp` is the loss gradient before the step weight, `sd` the target normaliser's std_c.
// Step k+1's state columns reach its loss twice: through the identity term of pred = state + delta * mask (g_pred_next) and through
// the encoder's input, behind the fp64 input normalisation (g_norm_in_next / std_in).
__device__ __forceinline__ void objective_tail(float gp, float m, LossBwdCarry carry, int64_t r, int c, int C, double sd, const LossBwdArgs& o) {
  gp = o.w * gp;
  if (carry.on) {
    const float through_norm = float(double(o.g_norm_in_next[r * (C + 1) + c]) / std_eps(o.in_mean[c], o.in_meansq[c], carry.ie));
    const float g_state = o.g_pred_next[r * C + c] + through_norm;
    gp = gp + g_state;
  }
  if (o.g_pred) o.g_pred[r * C + c] = gp;
  const float gd = gp * m;                                   // through `delta * mask`
  o.grad_norm_pred[r * C + c] = float(double(gd) * sd);      // through the fp64 de-normalisation
}

// The refusals of the carried pair, in every entry behind its own unsupported, null-pointer and period checks.  Header-inline: the
// companion library is a shared object of its own.
inline int check_carry(const char* who, const float* g_pred_next, const float* g_norm_in_next, const double* in_mean, const double* in_meansq,
                       const double* in_eps, const float* g_pred) {
  BSMS_REQUIRE((g_pred_next == nullptr) == (g_norm_in_next == nullptr), BSMS_E_INVALID_ARG,
               "%s: the carried pair (g_pred_next, g_norm_in_next) is given together or not at all", who);
  BSMS_REQUIRE(!g_pred_next || (in_mean && in_meansq && in_eps), BSMS_E_INVALID_ARG,
               "%s: a carried gradient needs the input normaliser's statistics", who);
  BSMS_REQUIRE(!g_pred || (g_pred != g_pred_next), BSMS_E_INVALID_ARG, "%s: g_pred aliases g_pred_next", who);
  return BSMS_OK;
}

inline int check_space_kind(const char* who, int space, int kind) {
  BSMS_REQUIRE((space == BSMS_LOSS_PHYSICAL || space == BSMS_LOSS_NORMALIZED) && (kind == BSMS_LOSS_MSE || kind == BSMS_LOSS_RMSE),
               BSMS_E_UNSUPPORTED, "%s: space=%d kind=%d (each 0 or 1)", who, space, kind);
  return BSMS_OK;
}

}  // namespace bsms
