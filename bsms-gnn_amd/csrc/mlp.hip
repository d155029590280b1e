// Host orchestration of a whole MLP (encoder / decoder: bsms_mlp_*), forward and backward, as sequences of the chain / wgrad
// kernels, and its pack table in a pack group (bsms_pack_group_add_mlp).
#include "host_orch.h"

using namespace bsms;

namespace {

enum MlpKind { MLP_SMALL_LN, MLP_ROWS_LN, MLP_ROWS_SMALL, MLP_BAD };
MlpKind mlp_kind(int64_t in_dim, int64_t D, int64_t out_dim, int layer_norm) {
  const bool in_small = in_dim >= 1 && in_dim <= 8 && in_dim != D, in_rows = in_dim == D;
  if (layer_norm && out_dim == D) return in_small ? MLP_SMALL_LN : (in_rows ? MLP_ROWS_LN : MLP_BAD);
  if (!layer_norm && out_dim >= 1 && out_dim <= 8 && in_rows) return MLP_ROWS_SMALL;
  return MLP_BAD;
}

struct MlpSaved {
  float *act[kMaxStages], *yln, *rstd;
  float *w[kMaxStages + 1], *wt[kMaxStages + 1], *w0t;
  float* bound;   // training: magnitude bounds, [st] tensor entering forward MFMA stage st, [16 + k] gradient entering backward stage k
  size_t bytes;
};
MlpSaved carve_mlp_saved(void* base, int64_t R, int64_t D, int H, bool training) {
  Carver c(base);
  MlpSaved s{};
  if (training) {
    for (int l = 0; l < H; ++l) s.act[l] = c.take(act_floats(size_t(R), D));
    s.yln = c.take(size_t(R) * D);
    s.rstd = c.take(size_t(R));
    s.bound = c.take(size_t(kBoundSlots) * kBoundWidth);
  }
  for (int l = 0; l <= H; ++l) { s.w[l] = c.take(pack_floats(D)); if (training) s.wt[l] = c.take(pack_floats(D)); }
  s.w0t = c.take(size_t(16) * D);
  s.bytes = c.off;
  return s;
}
struct MlpWork {
  float* g[kMaxStages + 1];
  char *wg, *sw;
  size_t bytes;
};
MlpWork carve_mlp_work(void* base, int64_t R, int64_t D, int H) {
  Carver c(base);
  MlpWork w{};
  for (int l = 0; l <= H; ++l) w.g[l] = c.take(pad_rows(size_t(R)) * D);
  w.wg = c.take_bytes(wgrad_work_bytes((int)D, 0));
  w.sw = c.take_bytes(small_wgrad_work_bytes((int)D));
  w.bytes = c.off;
  return w;
}

int check_mlp(int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int H, int layer_norm, const char* who) {
  BSMS_REQUIRE(supported_D(D), BSMS_E_UNSUPPORTED, "%s: latent width D=%lld not supported (a multiple of 32, 32..256)", who, (long long)D);
  BSMS_REQUIRE(H >= 1 && H < kMaxStages, BSMS_E_UNSUPPORTED, "%s: hidden=%d (1..%d)", who, H, kMaxStages - 1);
  BSMS_REQUIRE(R >= 0, BSMS_E_SHAPE, "%s: R=%lld", who, (long long)R);
  BSMS_REQUIRE(mlp_kind(in_dim, D, out_dim, layer_norm) != MLP_BAD, BSMS_E_UNSUPPORTED,
               "%s: MLP shape in=%lld D=%lld out=%lld ln=%d not supported", who, (long long)in_dim, (long long)D,
               (long long)out_dim, layer_norm);
  return BSMS_OK;
}

// THE definition of "which packs an MLP has" (bsms_mlp_fwd_ex and the pack group)
PackTable mlp_pack_table(const MlpSaved& sv, MlpKind kind, int64_t in_dim, int64_t D, int H, bool training, const float* const* params) {
  PackTable t{};
  const int lfirst = (kind == MLP_SMALL_LN) ? 1 : 0;          // first Linear that runs on the MFMA
  const int llast = (kind == MLP_ROWS_SMALL) ? H - 1 : H;     // last one
  if (kind == MLP_SMALL_LN) add_pack(t, params[0], (int)in_dim, 0, 0, (int)D, (int)in_dim, PACK_TRANSPOSE, sv.w0t, nullptr);
  for (int l = lfirst; l <= llast; ++l) {
    add_pack(t, params[2 * l], (int)D, 0, 0, (int)D, (int)D, PACK_FRAG, sv.w[l], params[2 * l + 1]);
    if (training) add_pack(t, params[2 * l], (int)D, 0, 0, (int)D, (int)D, PACK_FRAG_T, sv.wt[l], nullptr);
  }
  t.zero = training ? sv.bound : nullptr;
  return t;
}

}  // namespace

extern "C" size_t bsms_mlp_saved_bytes(int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden) {
  (void)in_dim; (void)out_dim;
  if (hidden < 1 || hidden >= kMaxStages) return 0;
  return carve_mlp_saved(nullptr, R, D, hidden, true).bytes;
}
extern "C" size_t bsms_mlp_work_bytes(int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden) {
  (void)in_dim; (void)out_dim;
  if (hidden < 1 || hidden >= kMaxStages) return 0;
  return carve_mlp_work(nullptr, R, D, hidden).bytes;
}

extern "C" int bsms_mlp_fwd(const float* x, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int H, int layer_norm,
                            const float* const* params, float* y, void* saved, void* work, bsms_stream_t stream) {
  return bsms_mlp_fwd_ex(x, R, in_dim, D, out_dim, H, layer_norm, params, y, saved, work, 0, stream);
}

extern "C" int bsms_mlp_fwd_ex(const float* x, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int H, int layer_norm,
                               const float* const* params, float* y, void* saved, void* work, int flags, bsms_stream_t stream) {
  int rc = check_mlp(R, in_dim, D, out_dim, H, layer_norm, "mlp_fwd");
  if (rc) return rc;
  BSMS_REQUIRE((x && y) || R == 0, BSMS_E_INVALID_ARG, "mlp_fwd: null argument");
  BSMS_REQUIRE(params != nullptr && (saved != nullptr || work != nullptr), BSMS_E_INVALID_ARG, "mlp_fwd: null argument");
  hipStream_t s = as_stream(stream);
  const MlpKind kind = mlp_kind(in_dim, D, out_dim, layer_norm);
  const bool training = saved != nullptr;     // saved == NULL: inference (packs live in `work`)
  MlpSaved sv = carve_mlp_saved(training ? saved : work, R, D, H, training);

  const int lfirst = (kind == MLP_SMALL_LN) ? 1 : 0;          // first Linear that runs on the MFMA
  const int llast = (kind == MLP_ROWS_SMALL) ? H - 1 : H;     // last one
  // BSMS_MLP_REUSE_PACKS: the packs are there already (and, in training, the bound slots cleared): an earlier inference call, or a pack group
  if (!(flags & BSMS_MLP_REUSE_PACKS) && (rc = prepack_table(mlp_pack_table(sv, kind, in_dim, D, H, training, params), s))) return rc;

  ChainFwdArgs a{};
  a.R = R; a.x = x;
  int st = 0;
  if (kind == MLP_SMALL_LN) {
    a.K0 = (int)in_dim; a.w0t = sv.w0t; a.bias_in = params[1]; a.store_in = training ? sv.act[0] : nullptr;
  }
  for (int l = lfirst; l <= llast; ++l, ++st) {
    a.wp[st] = reinterpret_cast<const float4*>(sv.w[l]);
    a.store[st] = (training && l < H) ? sv.act[l] : nullptr;
  }
  a.nstage = st;
  a.y = y;
  if (training && !g_node_bf3) for (int k = 0; k < st; ++k) a.amax[k] = sv.bound + size_t(k) * kBoundWidth;
  if (kind == MLP_ROWS_SMALL) {
    a.wout = params[2 * H]; a.bout = params[2 * H + 1]; a.C = (int)out_dim;
    return launch_chain_fwd((int)D, IN_ROWS, OUT_SMALL, a, s);
  }
  a.yln = training ? sv.yln : nullptr; a.rstd = training ? sv.rstd : nullptr;
  return launch_chain_fwd((int)D, kind == MLP_SMALL_LN ? IN_SMALL : IN_ROWS, OUT_LN, a, s);
}

extern "C" int bsms_pack_group_add_mlp(bsms_pack_group_t* group, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int H,
                                       int layer_norm, const float* const* params, void* saved, void* work) {
  PackGroup* g;
  int rc = pack_group_open(group, "pack_group_add_mlp", &g);
  if (rc || (rc = check_mlp(R, in_dim, D, out_dim, H, layer_norm, "pack_group_add_mlp"))) return rc;
  BSMS_REQUIRE(params != nullptr && (saved != nullptr || work != nullptr), BSMS_E_INVALID_ARG, "pack_group_add_mlp: null argument");
  for (int i = 0; i < 2 * (H + 1); ++i) BSMS_REQUIRE(params[i] != nullptr, BSMS_E_INVALID_ARG, "pack_group_add_mlp: parameter %d is null", i);
  const bool training = saved != nullptr;
  MlpSaved sv = carve_mlp_saved(training ? saved : work, R, D, H, training);
  pack_group_append(*g, mlp_pack_table(sv, mlp_kind(in_dim, D, out_dim, layer_norm), in_dim, D, H, training, params));
  return BSMS_OK;
}

extern "C" int bsms_mlp_bwd(const float* x, const float* grad_y, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim,
                            int H, int layer_norm, const float* const* params, const void* saved, void* work,
                            float* grad_x, float* const* grads, bsms_stream_t stream) {
  return bsms_mlp_bwd_ex(x, grad_y, R, in_dim, D, out_dim, H, layer_norm, params, saved, work, grad_x, grads, 0, stream);
}

extern "C" int bsms_mlp_bwd_ex(const float* x, const float* grad_y, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim,
                               int H, int layer_norm, const float* const* params, const void* saved, void* work,
                               float* grad_x, float* const* grads, int flags, bsms_stream_t stream) {
  int rc = check_mlp(R, in_dim, D, out_dim, H, layer_norm, "mlp_bwd");
  if (rc) return rc;
  BSMS_REQUIRE(params && saved && work, BSMS_E_INVALID_ARG, "mlp_bwd: null argument");
  BSMS_REQUIRE((x && grad_y) || R == 0, BSMS_E_INVALID_ARG, "mlp_bwd: null tensor");
  // grads == NULL (or every entry null): the MLP is frozen -- only the input gradient is formed
  const int gstate = grads_state(grads, 2 * (H + 1));
  BSMS_REQUIRE(gstate >= 0, BSMS_E_INVALID_ARG, "mlp_bwd: the gradient entries are partly null (an MLP is frozen as a whole: all %d "
               "entries null, or none)", 2 * (H + 1));
  const bool live = gstate == 1;
  if (!live && !grad_x) return BSMS_OK;   // nothing to compute
  hipStream_t s = as_stream(stream);
  const MlpKind kind = mlp_kind(in_dim, D, out_dim, layer_norm);
  BSMS_REQUIRE(kind == MLP_SMALL_LN || grad_x, BSMS_E_INVALID_ARG, "mlp_bwd: grad_x is null");
  MlpSaved sv = carve_mlp_saved(const_cast<void*>(saved), R, D, H, true);
  MlpWork wk = carve_mlp_work(work, R, D, H);

  // g[l] = gradient w.r.t. the output of Linear_l (pre-activation)
  ChainBwdArgs a{};
  a.R = R; a.dy = grad_y;
  int top;  // Linear index whose output gradient enters the chain
  if (kind == MLP_ROWS_SMALL) {
    a.wout = params[2 * H]; a.C = (int)out_dim; a.mask_in = sv.act[H - 1];
    top = H - 1;
  } else {
    a.yln = sv.yln; a.rstd = sv.rstd;
    top = H;
  }
  // frozen: the layer gradients have no reader -- but g[0] of the encoder shape, which the narrow input gradient multiplies
  a.gstore[0] = live ? wk.g[top] : nullptr;
  int k = 0;
  for (int l = top; l >= 1; --l, ++k) {   // dgrad stages run Linear_top .. Linear_1
    a.wpt[k] = reinterpret_cast<const float4*>(sv.wt[l]);
    a.mask[k] = sv.act[l - 1];
    a.gstore[k + 1] = (live || (l == 1 && kind == MLP_SMALL_LN)) ? wk.g[l - 1] : nullptr;
  }
  a.nstage = k;
  if (!g_node_bf3 && live) for (int q = 0; q <= k; ++q) a.gmax[q] = sv.bound + size_t(16 + q) * kBoundWidth;
  if (kind == MLP_SMALL_LN) {
    rc = launch_chain_bwd((int)D, G_ROWS_LN, F_NONE, a, s);
    // optional input gradient (a caller differentiating w.r.t. the encoder's input): g0 . W0, narrow (posgrad.hip)
    if (!rc && grad_x) rc = narrow_input_grad(wk.g[0], R, D, params[0], (int)in_dim, grad_x, s);
  } else {
    a.wh0 = reinterpret_cast<const float4*>(sv.wt[0]);
    a.dx = grad_x;
    rc = launch_chain_bwd((int)D, kind == MLP_ROWS_SMALL ? G_SMALL : G_ROWS_LN, F_HEADS1, a, s);
  }
  if (rc || !live) return rc;   // frozen: no weight gradient, no side lane, no mark

  // BSMS_BWD_DEFER_JOIN: grad_x is complete in stream order here; the weight gradients go to side lane 0 and the caller
  // joins later (bsms_side_lanes_join) -- the fused step runs the decoder's weight gradients under the U-Net's first block
  if (flags & BSMS_BWD_DEFER_JOIN) {
    SideLane* lane = nullptr;
    if ((rc = side_lane(&lane, 0, s)) || (rc = side_fork(lane, s))) return rc;
    s = lane->stream;
  }
  WgradJob jobs[kMaxWgradJobs] = {};
  int nj = 0;
  for (int l = (kind == MLP_SMALL_LN ? 1 : 0); l <= top; ++l) {
    WgradJob& j = jobs[nj++];
    j.G = wk.g[l]; j.A = (l == 0) ? x : sv.act[l - 1];
    j.dW = grads[2 * l]; j.db = grads[2 * l + 1];
    j.R = R; j.ldg = j.lda = j.ldw = (int)D; j.col0 = 0;
    j.g_bound = g_node_bf3 ? nullptr : sv.bound + size_t(16 + (top - l)) * kBoundWidth;                          // g[l] = gstore[top - l]
    j.a_bound = g_node_bf3 ? nullptr : sv.bound + size_t(l - (kind == MLP_SMALL_LN ? 1 : 0)) * kBoundWidth;    // the tensor entering the forward stage of Linear l
    j.g_mul = j.a_mul = 1.f;
  }
  if ((rc = launch_wgrad((int)D, jobs, nj, wk.wg, s, 0))) return rc;

  SmallWgradArgs sa{};
  sa.R = R; sa.D = (int)D;
  if (kind == MLP_SMALL_LN) {          // dW0[f][k] = sum_r g0[r][f] x[r][k] ; db0 = colsum g0
    sa.G = wk.g[0]; sa.S = x; sa.S_cols = (int)in_dim;
    sa.out = grads[0]; sa.os = 1; sa.of = in_dim; sa.colsum = grads[1];
    rc = launch_small_wgrad(sa, wk.sw, s);
  } else if (kind == MLP_ROWS_SMALL) {        // dW_H[c][f] = sum_r dy[r][c] a_{H-1}[r][f] ; db_H = colsum dy
    sa.G = sv.act[H - 1]; sa.S = grad_y; sa.S_cols = (int)out_dim;
    sa.out = grads[2 * H]; sa.os = D; sa.of = 1; sa.colsum_S = grads[2 * H + 1];
    rc = launch_small_wgrad(sa, wk.sw, s);
  }
  if (rc) return rc;
  if (flags & BSMS_BWD_DEFER_JOIN) {   // visible to bsms_side_lanes_join even if nothing else uses the lane afterwards
    SideLane* lane = nullptr;
    if ((rc = side_lane(&lane, 0, s)) || (rc = side_mark(lane, 0))) return rc;
  }
  return BSMS_OK;
}
