// Model-level glue of BSMS_Simulator (models/model.py:127-164) and the masked-RMSE loss (trainer/trainer.py:96-97) as
// small fused kernels: prologue, epilogue, and the loss gradients (pair sums, squared-objective row, robust row: one tail, objective_row.h).  In the reference (and in the autograd mirror, bsms-gnn_amd/model.py) this is ~40
// element-wise / reduction launches per training step on [B,N,<=4] tensors -- ~0.35 ms of a 7 ms step on the GPU and
// most of the host time that is not the engine's own.  The arithmetic is kept op for op:
//   normalise    float( (double(x) - mean) / std ),  std = max(nan_to_num(sqrt(E[x^2] - mean^2)), eps)   (fp64, normalizer.py:40-52,88-90)
//   de-normalise float( double(y) * std + mean )                                                        (normalizer.py:80-83)
//   integrate    pred = state + delta * mask                                                            (model.py:160-163)
//   loss         sqrt( sum(se * mask) / sum(mask) / C )                                                 (trainer.py:96-97)
// This file is compiled with -ffp-contract=off (build.py): a fused multiply-add would change the fp64 roundings.
#include "common.h"
#include "objective_row.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

// node_in [R, C+p+1] = [state(C) | mesh_pos(p) | node_type(1)]  ->  norm_in [R, C+1] = normalised [state | type], pos [R,p]
__global__ __launch_bounds__(256) void k_sim_prologue(const float* node_in, int64_t R, int C, int p, const double* mean,
                                                      const double* meansq, const double* eps, float* norm_in, float* pos) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= R) return;
  const int W = C + p + 1;
  const float* row = node_in + r * W;
  const double e = *eps;
  for (int c = 0; c <= C; ++c) {
    const float x = c < C ? row[c] : row[W - 1];
    norm_in[r * (C + 1) + c] = float((double(x) - mean[c]) / std_eps(mean[c], meansq[c], e));
  }
  for (int c = 0; c < p; ++c) pos[r * p + c] = row[C + c];
}

// de-normalise, mask, integrate; optional loss partial sums; optional next rollout input
__global__ __launch_bounds__(256) void k_sim_epilogue(const float* norm_pred, const float* node_in, const float* mask,
                                                      const float* target, int64_t R, int C, int p, const double* mean,
                                                      const double* meansq, const double* eps, float* pred, float* next_in,
                                                      const float* ic, float2* partials) {
  __shared__ float2 red[256];
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  float s_se = 0.f, s_m = 0.f;
  if (r < R) {
    const int W = C + p + 1;
    const double e = *eps;
    const float m = mask[r];
    float pr[kMaxC], tail[kMaxC + 1];
    for (int c = 0; c < C; ++c) {
      const float delta = float(double(norm_pred[r * C + c]) * std_eps(mean[c], meansq[c], e) + mean[c]);
      const float dm = delta * m;
      pr[c] = node_in[r * W + c] + dm;
    }
    if (next_in)
      for (int c = 0; c <= p; ++c) tail[c] = node_in[r * W + C + c];    // read before a possibly aliasing write
    for (int c = 0; c < C; ++c) pred[r * C + c] = pr[c];
    if (target) {
      for (int c = 0; c < C; ++c) {
        const float d = pr[c] - target[r * C + c];
        const float se = d * d;
        s_se += se * m;
      }
      s_m = m;
    }
    if (next_in) {   // rollout_utils.py:57-62: next = cat[pred, mesh_pos | type]; Dirichlet nodes (mask == 0) keep the IC
      for (int c = 0; c < C; ++c) next_in[r * W + c] = (m == 0.f) ? ic[r * W + c] : pr[c];
      for (int c = 0; c <= p; ++c) next_in[r * W + C + c] = (m == 0.f) ? ic[r * W + C + c] : tail[c];
    }
  }
  if (partials) {
    red[threadIdx.x] = make_float2(s_se, s_m);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {   // fixed tree: deterministic
      if (threadIdx.x < s) {
        red[threadIdx.x].x += red[threadIdx.x + s].x;
        red[threadIdx.x].y += red[threadIdx.x + s].y;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
  }
}

__global__ __launch_bounds__(256) void k_sim_sum_partials(const float2* partials, int n, float* sums) {
  __shared__ double2 red[256];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { a += partials[i].x; b += partials[i].y; }
  red[threadIdx.x] = make_double2(a, b);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[threadIdx.x].x += red[threadIdx.x + s].x;
      red[threadIdx.x].y += red[threadIdx.x + s].y;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[0] = float(red[0].x); sums[1] = float(red[0].y); }
}

// The masked RMSE on the fp32 pair `sums` = [S, M] of bsms_sim_epilogue: loss = sqrt(S / M / C) from the (possibly all-reduced) sums,
// and one step k of its (K-step) gradient w.r.t. the decoder output, through the one tail of objective_row.h: the step weight and
// the gradient carried back from step k+1 through in_{k+1} = where(mask == 0, in_0, cat[pred_k, ...]) (utils/rollout_utils.py:57-62).
// bsms_sim_loss_bwd is the launch with w = 1.0f, no carried pair and no g_pred: 1.0f * x is exact, so the single step's gradient
// is (d * m) * coef to the bit, as if the product were not there (tests/test_hip_unroll.py::test_sim_unroll_bwd_kernel).
__global__ __launch_bounds__(256) void k_sim_pair_bwd(const float* pred, const float* target, const float* mask, int64_t R, int C,
                                                      const LossBwdArgs o) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const float* sums = static_cast<const float*>(o.sums);
  const float S = sums[0], M = sums[1];
  const float loss = sqrtf(S / M / float(C));
  if (r == 0 && o.loss_out) *o.loss_out = loss;
  if (r >= R) return;
  const double e = *o.eps;
  const float m = mask[r];
  const float coef = 1.f / (loss * M * float(C));           // dL/dS * 2 = 1 / (L M C)
  const LossBwdCarry carry = loss_bwd_carry(o, m);
  for (int c = 0; c < C; ++c) {
    const float gp = (pred[r * C + c] - target[r * C + c]) * m * coef;   // dL/dpred
    objective_tail(gp, m, carry, r, c, C, std_eps(o.mean[c], o.meansq[c], e), o);
  }
}

}  // namespace

extern "C" int bsms_sim_prologue(const float* node_in, int64_t R, int64_t C, int64_t p, const double* mean,
                                 const double* meansq, const double* std_eps_dev, float* norm_in, float* pos,
                                 bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 0 && C >= 1 && C <= kMaxC && p >= 1 && p <= 7, BSMS_E_UNSUPPORTED, "sim_prologue: R=%lld C=%lld p=%lld",
               (long long)R, (long long)C, (long long)p);
  if (R == 0) return BSMS_OK;
  BSMS_REQUIRE(node_in && mean && meansq && std_eps_dev && norm_in && pos, BSMS_E_INVALID_ARG, "sim_prologue: null argument");
  hipLaunchKernelGGL(k_sim_prologue, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), node_in, R, (int)C,
                     (int)p, mean, meansq, std_eps_dev, norm_in, pos);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" size_t bsms_sim_work_bytes(int64_t R) { return size_t(ceil_div(std::max<int64_t>(R, 1), 256)) * sizeof(float2) + 256; }

extern "C" int bsms_sim_epilogue(const float* norm_pred, const float* node_in, const float* mask, const float* target,
                                 int64_t R, int64_t C, int64_t p, const double* mean, const double* meansq,
                                 const double* std_eps_dev, float* pred, float* next_in, const float* ic, float* sums,
                                 void* work, bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 0 && C >= 1 && C <= kMaxC && p >= 1 && p <= 7, BSMS_E_UNSUPPORTED, "sim_epilogue: R=%lld C=%lld p=%lld",
               (long long)R, (long long)C, (long long)p);
  BSMS_REQUIRE(!sums || (target && work), BSMS_E_INVALID_ARG, "sim_epilogue: the loss sums need target and work");
  BSMS_REQUIRE(!next_in || ic, BSMS_E_INVALID_ARG, "sim_epilogue: next_in needs the initial condition");
  hipStream_t s = as_stream(stream);
  if (R == 0) {
    if (sums) BSMS_HIP_CHECK(hipMemsetAsync(sums, 0, 2 * sizeof(float), s));
    return BSMS_OK;
  }
  BSMS_REQUIRE(norm_pred && node_in && mask && mean && meansq && std_eps_dev && pred, BSMS_E_INVALID_ARG, "sim_epilogue: null argument");
  const unsigned nb = (unsigned)ceil_div(R, 256);
  float2* partials = sums ? reinterpret_cast<float2*>(work) : nullptr;
  hipLaunchKernelGGL(k_sim_epilogue, dim3(nb), dim3(256), 0, s, norm_pred, node_in, mask, target, R, (int)C, (int)p, mean, meansq,
                     std_eps_dev, pred, next_in, ic, partials);
  BSMS_LAUNCH_CHECK();
  if (sums) {
    hipLaunchKernelGGL(k_sim_sum_partials, dim3(1), dim3(256), 0, s, (const float2*)partials, (int)nb, sums);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}

extern "C" int bsms_sim_loss_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C,
                                 const double* mean, const double* meansq, const double* std_eps_dev, const float* sums,
                                 float* loss_out, float* grad_norm_pred, bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 1 && C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "sim_loss_bwd: R=%lld C=%lld", (long long)R, (long long)C);
  BSMS_REQUIRE(pred && target && mask && mean && meansq && std_eps_dev && sums && grad_norm_pred, BSMS_E_INVALID_ARG,
               "sim_loss_bwd: null argument");
  const LossBwdArgs o{mean, meansq, std_eps_dev, nullptr, nullptr, nullptr, sums, nullptr, 1.0f, nullptr, nullptr, loss_out, nullptr, nullptr,
                      grad_norm_pred};
  hipLaunchKernelGGL(k_sim_pair_bwd, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), pred, target, mask, R, (int)C, o);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_sim_unroll_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C,
                                   const double* mean, const double* meansq, const double* std_eps_dev, const double* in_mean,
                                   const double* in_meansq, const double* in_std_eps_dev, const float* sums, float w,
                                   const float* g_pred_next, const float* g_norm_in_next, float* loss_out, float* g_pred,
                                   float* grad_norm_pred, bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 1 && C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "sim_unroll_bwd: R=%lld C=%lld", (long long)R, (long long)C);
  BSMS_REQUIRE(pred && target && mask && mean && meansq && std_eps_dev && sums && grad_norm_pred, BSMS_E_INVALID_ARG,
               "sim_unroll_bwd: null argument");
  if (int rc = check_carry("sim_unroll_bwd", g_pred_next, g_norm_in_next, in_mean, in_meansq, in_std_eps_dev, g_pred)) return rc;
  const LossBwdArgs o{mean, meansq, std_eps_dev, in_mean, in_meansq, in_std_eps_dev, sums, nullptr, w, g_pred_next, g_norm_in_next, loss_out,
                      nullptr, g_pred, grad_norm_pred};
  hipLaunchKernelGGL(k_sim_pair_bwd, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), pred, target, mask, R, (int)C, o);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

namespace {

// One step k of the K-step input gradient G = dJ / d in_0 (include/bsms_hip.h: bsms_sim_input_grad), folded into grad_in
// [R, C+p+1] in the column layout of node_in.  t = float(double(g_norm_in) / std_in) is the way back through the fp64 input
// normalisation, formed as objective_tail (objective_row.h) forms the carried one.  Thread r owns row r, the map of every k_sim_* kernel: a
// row is at most 17 floats in and 16 out, a wave covers 64 consecutive rows, so every cache line it touches is used in full
// over the column loop; the launch is glue (launch-bound), not a streaming kernel worth an element-per-lane map.
__global__ __launch_bounds__(256) void k_sim_input_grad(const float* g_pred, const float* g_norm_in, const float* g_pos,
                                                        const float* mask, int64_t R, int C, int p, const double* in_mean,
                                                        const double* in_meansq, const double* in_eps, int first_step,
                                                        int overwrite, float* grad_in) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= R) return;
  const int W = C + p + 1;
  const double ie = *in_eps;
  const float m = mask[r];
  float* out = grad_in + r * W;
  for (int c = 0; c <= C; ++c) {
    const float t = float(double(g_norm_in[r * (C + 1) + c]) / std_eps(in_mean[c], in_meansq[c], ie));
    float contrib;
    if (c == C) contrib = t;                                          // node type: every step, every row
    else if (first_step) contrib = g_pred[r * C + c] + t;             // in_0 is step 0's input on every row
    else contrib = (m == 0.f) ? t : 0.f;                              // later steps: only the rows that took in_0 again
    float* o = out + (c < C ? c : W - 1);
    *o = overwrite ? contrib : *o + contrib;
  }
  for (int c = 0; c < p; ++c) {                                       // positions: every step, every row
    const float contrib = g_pos[r * p + c];
    out[C + c] = overwrite ? contrib : out[C + c] + contrib;
  }
}

}  // namespace

extern "C" int bsms_sim_input_grad(const float* g_pred, const float* g_norm_in, const float* g_pos, const float* mask, int64_t R,
                                   int64_t C, int64_t p, const double* in_mean, const double* in_meansq,
                                   const double* in_std_eps_dev, int first_step, int overwrite, float* grad_in,
                                   bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 1 && C >= 1 && C <= kMaxC && p >= 1 && p <= 7, BSMS_E_UNSUPPORTED, "sim_input_grad: R=%lld C=%lld p=%lld",
               (long long)R, (long long)C, (long long)p);
  BSMS_REQUIRE(g_norm_in && g_pos && mask && in_mean && in_meansq && in_std_eps_dev && grad_in, BSMS_E_INVALID_ARG,
               "sim_input_grad: null argument");
  BSMS_REQUIRE(!first_step || g_pred, BSMS_E_INVALID_ARG, "sim_input_grad: the first step (k == 0) needs g_pred");
  hipLaunchKernelGGL(k_sim_input_grad, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), g_pred, g_norm_in, g_pos,
                     mask, R, (int)C, (int)p, in_mean, in_meansq, in_std_eps_dev, first_step ? 1 : 0, overwrite ? 1 : 0, grad_in);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

namespace {

// k_sim_pair_bwd for the family of objectives (include/bsms_hip.h: bsms_sim_objective_bwd, _w).  `sums` = [M | SE[0..C)] in fp64
// (bsms_error_sums); every thread forms the C per-channel coefficients G * a_c from it in fp64 and rounds each to fp32 once.
// No guard for M == 0 or loss == 0, as in k_sim_pair_bwd: the non-finite coefficient reaches the output.  The head (coefficients) and
// the tail (step weight, carry, way out) of a row live in objective_row.h, shared with the edge objective's backward
// (ext/edge_objective.hip).  `row_weights` (bsms_sim_objective_bwd_w): row r's loss gradient carries mu = m * row_weights[r % period],
// ONE fp32 product formed first, so (d * mu) * coef is the unweighted (d * m) * coef whenever the weight is 1; nullptr: mu IS m (no
// product), the launch of bsms_sim_objective_bwd.  The mask of the carry and of the way out stays m.
__global__ __launch_bounds__(256) void k_sim_objective_bwd(const float* pred, const float* target, const float* mask,
                                                           const float* row_weights, int64_t weight_period, int64_t R, int C,
                                                           int normalized, int rmse, const LossBwdArgs o) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const double* sums = static_cast<const double*>(o.sums);
  const double e = *o.eps;
  const double MC = sums[0] * double(C);
  double sd[kMaxC], a[kMaxC];
  double Q = 0.0;
  for (int c = 0; c < C; ++c) {
    const ObjectiveChannel ch = objective_channel(c, o.mean, o.meansq, e, sums, o.weights, normalized, MC);
    sd[c] = ch.sd;
    a[c] = ch.a;
    if (r == 0 && o.chan_out) o.chan_out[c] = float(ch.term);
    Q += ch.term;
  }
  const double loss = objective_loss(Q, rmse);
  if (r == 0 && o.loss_out) *o.loss_out = float(loss);
  if (r >= R) return;
  const double G = objective_scale(loss, MC, rmse);
  const float m = mask[r];
  const float mu = row_weights ? m * row_weights[r % weight_period] : m;
  const LossBwdCarry carry = loss_bwd_carry(o, m);
  for (int c = 0; c < C; ++c) {
    const float coef = float(G * a[c]);
    const float gp = (pred[r * C + c] - target[r * C + c]) * mu * coef;
    objective_tail(gp, m, carry, r, c, C, sd[c], o);
  }
}

// k_sim_objective_bwd for the robust objectives (include/bsms_hip.h: bsms_sim_robust_bwd).  `sums` = [M | S[0..C)]
// (bsms_robust_sums), loss = sum_c w_c S_c / (M C): linear in the sums, so the coefficient of a row is fl32(w_c / (M C s_c)) whatever
// the sums hold, and only the loss-gradient term differs: psi(u) = sign(u) or clamp(u, -delta, delta) of u = double(d) / s_c takes
// d's place.  mu and the tail are that kernel's.
__global__ __launch_bounds__(256) void k_sim_robust_bwd(const float* pred, const float* target, const float* mask,
                                                        const float* row_weights, int64_t weight_period, int64_t R, int C,
                                                        const double* delta, int normalized, int huber, const LossBwdArgs o) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const double* sums = static_cast<const double*>(o.sums);
  const double e = *o.eps;
  const double MC = sums[0] * double(C);
  double sd[kMaxC], sc[kMaxC], dl[kMaxC];
  float coef[kMaxC];
  double loss = 0.0;
  for (int c = 0; c < C; ++c) {
    sd[c] = std_eps(o.mean[c], o.meansq[c], e);
    sc[c] = normalized ? sd[c] : 1.0;
    dl[c] = huber ? delta[c] : 0.0;
    const double wc = o.weights ? o.weights[c] : 1.0;
    const double term = wc * sums[1 + c] / MC;
    if (r == 0 && o.chan_out) o.chan_out[c] = float(term);
    loss += term;
    coef[c] = float(wc / (MC * sc[c]));
  }
  if (r == 0 && o.loss_out) *o.loss_out = float(loss);
  if (r >= R) return;
  const float m = mask[r];
  const float mu = row_weights ? m * row_weights[r % weight_period] : m;
  const LossBwdCarry carry = loss_bwd_carry(o, m);
  for (int c = 0; c < C; ++c) {
    const double u = double(pred[r * C + c] - target[r * C + c]) / sc[c];
    double psi = u;                                                     // |u| <= delta; u == 0 (sign(0) = 0); a NaN stays one
    if (huber) psi = u > dl[c] ? dl[c] : (u < -dl[c] ? -dl[c] : u);
    else if (u > 0.0) psi = 1.0;
    else if (u < 0.0) psi = -1.0;
    objective_tail(float(psi) * mu * coef[c], m, carry, r, c, C, sd[c], o);
  }
}

// bsms_sim_objective_bwd and its `_w` form (`weighted`: a weight per row, required, with its period): one list of checks -- each
// weighted argument directly behind the check it belongs to -- and one launch.
int sim_objective_bwd(const char* who, bool weighted, const float* pred, const float* target, const float* mask, const float* row_weights,
                      int64_t weight_period, int64_t R, int64_t C, int space, int kind, const LossBwdArgs& o, bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 1 && C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: R=%lld C=%lld", who, (long long)R, (long long)C);
  if (int rc = check_space_kind(who, space, kind)) return rc;
  BSMS_REQUIRE(pred && target && mask && (row_weights || !weighted) && o.mean && o.meansq && o.eps && o.sums && o.grad_norm_pred,
               BSMS_E_INVALID_ARG, "%s: null argument", who);
  BSMS_REQUIRE(!weighted || (weight_period >= 1 && weight_period <= R && R % weight_period == 0), BSMS_E_INVALID_ARG,
               "%s: weight_period=%lld does not divide R=%lld", who, (long long)weight_period, (long long)R);
  if (int rc = check_carry(who, o.g_pred_next, o.g_norm_in_next, o.in_mean, o.in_meansq, o.in_eps, o.g_pred)) return rc;
  hipLaunchKernelGGL(k_sim_objective_bwd, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), pred, target, mask,
                     weighted ? row_weights : nullptr, weighted ? weight_period : 1, R, (int)C, int(space == BSMS_LOSS_NORMALIZED),
                     int(kind == BSMS_LOSS_RMSE), o);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

}  // namespace

extern "C" int bsms_sim_objective_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C,
                                      const double* mean, const double* meansq, const double* std_eps_dev, const double* in_mean,
                                      const double* in_meansq, const double* in_std_eps_dev, const double* sums,
                                      const double* channel_weights, int space, int kind, float w, const float* g_pred_next,
                                      const float* g_norm_in_next, float* loss_out, float* chan_out, float* g_pred,
                                      float* grad_norm_pred, bsms_stream_t stream) {
  return sim_objective_bwd("sim_objective_bwd", false, pred, target, mask, nullptr, 1, R, C, space, kind,
                           {mean, meansq, std_eps_dev, in_mean, in_meansq, in_std_eps_dev, sums, channel_weights, w, g_pred_next,
                            g_norm_in_next, loss_out, chan_out, g_pred, grad_norm_pred},
                           stream);
}

extern "C" int bsms_sim_objective_bwd_w(const float* pred, const float* target, const float* mask, const float* row_weights,
                                        int64_t weight_period, int64_t R, int64_t C, const double* mean, const double* meansq,
                                        const double* std_eps_dev, const double* in_mean, const double* in_meansq,
                                        const double* in_std_eps_dev, const double* sums, const double* channel_weights, int space,
                                        int kind, float w, const float* g_pred_next, const float* g_norm_in_next, float* loss_out,
                                        float* chan_out, float* g_pred, float* grad_norm_pred, bsms_stream_t stream) {
  return sim_objective_bwd("sim_objective_bwd_w", true, pred, target, mask, row_weights, weight_period, R, C, space, kind,
                           {mean, meansq, std_eps_dev, in_mean, in_meansq, in_std_eps_dev, sums, channel_weights, w, g_pred_next,
                            g_norm_in_next, loss_out, chan_out, g_pred, grad_norm_pred},
                           stream);
}

// The robust objectives' backward (include/bsms_hip.h): the checks of bsms_sim_objective_bwd_w in its order, with `row_weights`
// nullable (then weight_period is not looked at) and `delta` among the required pointers under BSMS_ROBUST_HUBER.
extern "C" int bsms_sim_robust_bwd(const float* pred, const float* target, const float* mask, const float* row_weights,
                                   int64_t weight_period, int64_t R, int64_t C, const double* mean, const double* meansq,
                                   const double* std_eps_dev, const double* in_mean, const double* in_meansq,
                                   const double* in_std_eps_dev, const double* sums, const double* channel_weights,
                                   const double* delta, int space, int rkind, float w, const float* g_pred_next,
                                   const float* g_norm_in_next, float* loss_out, float* chan_out, float* g_pred,
                                   float* grad_norm_pred, bsms_stream_t stream) {
  BSMS_REQUIRE(R >= 1 && C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "sim_robust_bwd: R=%lld C=%lld", (long long)R, (long long)C);
  BSMS_REQUIRE((space == BSMS_LOSS_PHYSICAL || space == BSMS_LOSS_NORMALIZED) && (rkind == BSMS_ROBUST_MAE || rkind == BSMS_ROBUST_HUBER),
               BSMS_E_UNSUPPORTED, "sim_robust_bwd: space=%d rkind=%d (each 0 or 1)", space, rkind);
  BSMS_REQUIRE(pred && target && mask && mean && meansq && std_eps_dev && sums && grad_norm_pred &&
                   (delta || rkind != BSMS_ROBUST_HUBER),
               BSMS_E_INVALID_ARG, "sim_robust_bwd: null argument");
  BSMS_REQUIRE(!row_weights || (weight_period >= 1 && weight_period <= R && R % weight_period == 0), BSMS_E_INVALID_ARG,
               "sim_robust_bwd: weight_period=%lld does not divide R=%lld", (long long)weight_period, (long long)R);
  if (int rc = check_carry("sim_robust_bwd", g_pred_next, g_norm_in_next, in_mean, in_meansq, in_std_eps_dev, g_pred)) return rc;
  const LossBwdArgs o{mean, meansq, std_eps_dev, in_mean, in_meansq, in_std_eps_dev, sums, channel_weights, w, g_pred_next, g_norm_in_next,
                      loss_out, chan_out, g_pred, grad_norm_pred};
  hipLaunchKernelGGL(k_sim_robust_bwd, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, as_stream(stream), pred, target, mask,
                     row_weights, row_weights ? weight_period : 1, R, (int)C, delta, int(space == BSMS_LOSS_NORMALIZED),
                     int(rkind == BSMS_ROBUST_HUBER), o);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

namespace {

// The coefficients of one fold of gradient accumulation (include/bsms_hip.h: bsms_accum_coef).  One block; thread k
// owns unroll step k: its sums, its row of `running`, its entry of loss_out.  The pair (a, b) is step 0's (the mask, and so the
// factor, is shared by the K steps wherever a scalar factor exists).  Everything is fp64 until the single rounding of a, b and the
// losses to fp32; a_c and std are formed as k_sim_objective_bwd forms them.  No guard for m == 0 or a zero loss, as there.
struct AccumCoefArgs {
  const void* sums;
  int64_t stride;
  const double *mean, *meansq, *eps, *weights;
  double* running;
  float *coef, *loss_out;
  int64_t t;
  int row, C, normalized, rmse, mean_reduction, K;
};

__global__ __launch_bounds__(64) void k_accum_coef(AccumCoefArgs p) {
  for (int k = threadIdx.x; k < p.K; k += 64) {
    double m, n;
    if (p.row) {
      const double* s = reinterpret_cast<const double*>(p.sums) + int64_t(k) * p.stride;
      const double e = p.normalized ? *p.eps : 0.0;
      m = s[0];
      n = 0.0;
      for (int c = 0; c < p.C; ++c) {
        const double wc = p.weights ? p.weights[c] : 1.0;
        double a = wc;
        if (p.normalized) {
          const double sd = std_eps(p.mean[c], p.meansq[c], e);
          a = wc / (sd * sd);
        }
        n += a * s[1 + c];
      }
    } else {
      const float* s = reinterpret_cast<const float*>(p.sums) + int64_t(k) * p.stride;
      n = double(s[0]);
      m = double(s[1]);
    }
    const double Cd = double(p.C);
    const double q = n / (m * Cd);
    const double l = p.rmse ? sqrt(q) : q;
    double* run = p.running + 3 * k;
    double a = 0.0, b = 1.0, Mc = m, Nc = n, Lc = l;
    if (p.t > 0) {
      const double Mp = run[0], Np = run[1], Lp = run[2];
      Mc = Mp + m;
      Nc = Np + n;
      if (p.mean_reduction) {
        const double td = double(p.t), t1 = double(p.t + 1);
        Lc = (Lp * td + l) / t1;
        a = td / t1;
        b = 1.0 / t1;
      } else {
        const double Qc = Nc / (Mc * Cd);
        Lc = p.rmse ? sqrt(Qc) : Qc;
        if (p.rmse) {
          const double den = Lc * Mc;
          a = (Lp * Mp) / den;
          b = (l * m) / den;
        } else {
          a = Mp / Mc;
          b = m / Mc;
        }
      }
    }
    run[0] = Mc; run[1] = Nc; run[2] = Lc;
    p.loss_out[k] = float(Lc);
    if (k == 0) { p.coef[0] = float(a); p.coef[1] = float(b); }
  }
}

}  // namespace

extern "C" int bsms_accum_coef(const void* sums, int layout, int64_t sums_stride, int64_t C, const double* mean, const double* meansq,
                               const double* std_eps_dev, const double* channel_weights, int space, int kind, int reduction,
                               int64_t t, int64_t K, double* running, float* coef, float* loss_out, bsms_stream_t stream) {
  BSMS_REQUIRE(K >= 1 && K <= 4096 && C >= 1 && C <= kMaxC && t >= 0, BSMS_E_UNSUPPORTED, "accum_coef: K=%lld C=%lld t=%lld",
               (long long)K, (long long)C, (long long)t);
  BSMS_REQUIRE((layout == BSMS_ACCUM_SUMS_PAIR || layout == BSMS_ACCUM_SUMS_ROW) &&
                   (space == BSMS_LOSS_PHYSICAL || space == BSMS_LOSS_NORMALIZED) && (kind == BSMS_LOSS_MSE || kind == BSMS_LOSS_RMSE) &&
                   (reduction == BSMS_ACCUM_BATCH || reduction == BSMS_ACCUM_MEAN),
               BSMS_E_UNSUPPORTED, "accum_coef: layout=%d space=%d kind=%d reduction=%d (each 0 or 1)", layout, space, kind, reduction);
  const bool row = layout == BSMS_ACCUM_SUMS_ROW;
  BSMS_REQUIRE(sums_stride >= (row ? 1 + C : 2), BSMS_E_SHAPE, "accum_coef: sums_stride=%lld is shorter than one entry (%lld)",
               (long long)sums_stride, (long long)(row ? 1 + C : 2));
  BSMS_REQUIRE(sums && running && coef && loss_out, BSMS_E_INVALID_ARG, "accum_coef: null argument");
  const bool normalized = row && space == BSMS_LOSS_NORMALIZED;
  BSMS_REQUIRE(!normalized || (mean && meansq && std_eps_dev), BSMS_E_INVALID_ARG,
               "accum_coef: the normalized space needs the target normaliser's statistics");
  AccumCoefArgs p{};
  p.sums = sums; p.stride = sums_stride; p.mean = mean; p.meansq = meansq; p.eps = std_eps_dev;
  p.weights = row ? channel_weights : nullptr;
  p.running = running; p.coef = coef; p.loss_out = loss_out; p.t = t;
  p.row = int(row); p.C = (int)C; p.normalized = int(normalized); p.rmse = int(kind == BSMS_LOSS_RMSE);
  p.mean_reduction = int(reduction == BSMS_ACCUM_MEAN); p.K = (int)K;
  hipLaunchKernelGGL(k_accum_coef, dim3(1), dim3(64), 0, as_stream(stream), p);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}
