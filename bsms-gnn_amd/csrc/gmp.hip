// Host orchestration of one coarse C-ABI entry: a whole GMP block (ops/basic.py:26-98), forward and backward, as sequences of
// the chain / rowsum / wgrad kernels.  (A whole MLP: mlp.hip; the U-Net of blocks: bsgmp.hip; the descriptor of a block call: gmp_block.h.)
//
// GMP forward (H = hidden layers):
//   prepack            all weight matrices of the block -> MFMA fragment order (one launch; kept for bwd)
//   proj  x2           Ps = x Wi^T + b0,  Pd = x Wj^T         (the first edge Linear split by linearity:
//                      W0 [fiber | x_i | x_j] = Wf fiber + Wi x_i + Wj x_j, so 2 D^2 MACs per NODE
//                      instead of per EDGE; ops/basic.py:90 concatenation order [fiber, x_i, x_j])
//   edge chain         relu(Ps[i] + Pd[j] + Wf fiber) -> H-1 x (Linear, ReLU) -> Linear -> LayerNorm
//   segment sum        aggr[b,n] = sum of messages into n (dst-sorted CSR, no atomics)
//   node chain         [x, aggr] -> MLP -> LayerNorm -> + x
// GMP backward mirrors it: node chain bwd -> edge chain bwd -> segment sums of the edge gradient by
// source and by target -> all weight gradients in one batched split-K launch -> input gradient.
#include <cstdlib>

#include "gmp_block.h"

using namespace bsms;

// ================================================================================== experiment switches (host_orch.h)
// BSMS_EDGE_FUSED=0: the fused edge backward (efuse.hip) -- THE path of the bf16 precisions at D = 128, hidden = 3 -- off for A/B runs.
// BSMS_EDGE_FWD_RES=0: the generic ring kernel instead of efwd.hip (profiles/r05_efwd_ab.sh).
// BSMS_NODE_BF3: weight-gradient jobs whose `A` operand is a CALLER's tensor -- every job of bsms_mlp_bwd, and in a GMP block the x half
// of the first node Linear and the two projections (A = x) -- run the range-free three-way bf16 split (wgrad.hip: BF3, six products)
// instead of fp16 x 2 pieces with one scale per tensor: a caller's columns may differ by any factor (VERDICT
// round 4 item 2).  The other node-level jobs multiply the block's own post-ReLU activations / LayerNorm-bounded sums, like
// the edge-level ones, and keep the three-product arithmetic: all node-level jobs range-free measured 0 on the airfoil step
// but -2.6 % / -7.5 % on the cylinder steps (dense / block-diagonal), where the side lane is co-critical
// (profiles/r05_node_bf3_ab.txt).  0 none / 1 this / 2 all node-level jobs.
#ifdef BSMS_EXPERIMENTS
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
namespace bsms {
int g_debug_flags = env_int("BSMS_DEBUG_FLAGS", 0);
unsigned long long* g_timing = nullptr;
const int g_node_bf3 = env_int("BSMS_NODE_BF3", 1);
}  // namespace bsms
static const int g_edge_fused = env_int("BSMS_EDGE_FUSED", 1);
static const int g_edge_fwd_res = env_int("BSMS_EDGE_FWD_RES", 1);
extern "C" void bsms_debug_set_flags(int flags) { g_debug_flags = flags; }  // not in bsms_hip.h: experiments only
extern "C" void bsms_debug_set_timing(unsigned long long* dev_buf) { g_timing = dev_buf; }
#else
constexpr int g_edge_fused = 1;
constexpr int g_edge_fwd_res = 1;
#endif

// ================================================================================== the shape of a block
// Pure functions of the shape: size queries and calls agree.  (edge_fused_supported never holds for BSMS_F32: efuse.hip is built for
// the bf16 precisions; its pos_dim limit is the bf16 constraint of check().)
bool GmpShape::fused() const { return training && g_edge_fused && edge_fused_supported(D, H, 1, precision); }
bool GmpShape::edge_fwd_resident() const { return g_edge_fwd_res && edge_fwd_res_supported(D, H, p, precision) && (!training || fused()); }

int GmpShape::check(const char* who) const {
  BSMS_REQUIRE(supported_D(D), BSMS_E_UNSUPPORTED, "%s: latent width D=%lld not supported (a multiple of 32, 32..256)", who, (long long)D);
  BSMS_REQUIRE(p >= 1 && p <= 7, BSMS_E_UNSUPPORTED, "%s: pos_dim=%lld (1..7)", who, (long long)p);
  BSMS_REQUIRE(H >= 1 && H < kMaxStages, BSMS_E_UNSUPPORTED, "%s: hidden=%d (1..%d)", who, H, kMaxStages - 1);
  BSMS_REQUIRE(B >= 0, BSMS_E_SHAPE, "%s: B=%lld", who, (long long)B);
  BSMS_REQUIRE(B * std::max(E, N) * D < (int64_t(1) << 40), BSMS_E_SHAPE, "%s: tensor too large", who);
  BSMS_REQUIRE(precision == BSMS_F32 || precision == BSMS_BF16 || precision == BSMS_BF16_NODES, BSMS_E_UNSUPPORTED, "%s: precision %d", who, precision);
  BSMS_REQUIRE(!bf() || ((D == 128 || D == 256) && p <= 3), BSMS_E_UNSUPPORTED, "%s: bf16 precision needs D = 128 / 256 and pos_dim <= 3", who);
  return BSMS_OK;
}

namespace {

// ================================================================================== GMP layout
struct GmpSaved {
  float *e_act[kMaxStages], *e_y, *e_rstd, *aggr, *e_fiber;
  float *e_Ps, *e_Pd;   // fused edge backward of the bf16 precisions (efuse.hip): the two node projections are kept for the backward's recompute
  float *n_act[kMaxStages], *n_yln, *n_rstd;
  // packs (fragment order)
  float *e_wi, *e_wj, *e_wft, *e_w[kMaxStages], *e_wt[kMaxStages], *e_wit, *e_wjt;
  float* e_wr[kMaxStages];   // fused edge backward: PACK_ROWS_BF16 images of the D x D edge Linears (efuse.hip)
  float *n_w0x, *n_w0a, *n_w[kMaxStages], *n_wt[kMaxStages], *n_w0xt, *n_w0at;
  // magnitude bounds (training; chain.h: kBoundSlots floats, zeroed by the block's prepack): [0..7] tensor entering edge
  // forward stage l (e_act[l]); [8..15] node forward stage l ([8]: x and aggr jointly, [8 + l]: n_act[l - 1]);
  // [16..23] gradient entering edge backward stage k (gE[H - k]; [16 + H]: gE[0]); [24..31] node backward (gN[H - k])
  float* bound;
  size_t bytes;
};
// s.training: everything the backward needs.  Inference: only the messages, the aggregate and the forward packs, carved from the
// scratch buffer instead -- the packs from `packs_base` where one is given (GmpCall::packs_base).
GmpSaved carve_gmp_saved(void* base, const GmpShape& s, void* packs_base) {
  Carver c(base);
  GmpSaved v{};
  const int64_t D = s.D;
  const int H = s.H;
  const bool training = s.training, fused = s.fused();
  const size_t re = size_t(s.B) * s.E, rn = size_t(s.B) * s.N, dd = pack_floats(D);
  const size_t edge_act = s.bf() ? pad_rows(re) * (size_t(D) / 2 + mask_words_per_row(D)) : act_floats(re, D);
  if (training && !fused)
    for (int l = 0; l < H; ++l) v.e_act[l] = c.take(edge_act);
  if (fused) { v.e_Ps = c.take(rn * D); v.e_Pd = c.take(rn * D); }
  v.e_y = c.take(s.bf() ? re * D / 2 : re * D);
  if (training) v.e_rstd = c.take(re);
  if (training) v.e_fiber = c.take(re * 8);   // [B*E, fiber_ld(p)]: sized for the widest pitch (p is not part of the size query)
  v.aggr = c.take(rn * D);
  if (training) {
    for (int l = 0; l < H; ++l) v.n_act[l] = c.take(s.bfn() ? pad_rows(rn) * (size_t(D) / 2 + mask_words_per_row(D)) : act_floats(rn, D));
    v.n_yln = c.take(rn * D);
    v.n_rstd = c.take(rn);
    v.bound = c.take(size_t(kBoundSlots) * kBoundWidth);
  }
  Carver cp(packs_base);
  Carver& k = packs_base ? cp : c;
  v.e_wi = k.take(dd); v.e_wj = k.take(dd); v.e_wft = k.take(size_t(8) * D);
  if (training) { v.e_wit = k.take(dd); v.e_wjt = k.take(dd); }
  // transposed packs: the unfused backward; row images: the fused one (efuse.hip)
  for (int l = 1; l <= H; ++l) { v.e_w[l] = k.take(dd); if (training && !fused) v.e_wt[l] = k.take(dd); if (fused) v.e_wr[l] = k.take(size_t(D) * 72); }
  v.n_w0x = k.take(dd); v.n_w0a = k.take(dd);
  if (training) { v.n_w0xt = k.take(dd); v.n_w0at = k.take(dd); }
  for (int l = 1; l <= H; ++l) { v.n_w[l] = k.take(dd); if (training) v.n_wt[l] = k.take(dd); }
  v.bytes = c.off;
  return v;
}

struct GmpWork {
  float *Ps, *Pd;                    // fwd
  float *gN[kMaxStages + 1], *daggr; // bwd
  float *gE[kMaxStages + 1], *dPs, *dPd;
  char *wg, *wg2, *sw;
  size_t sw_bytes;
  float* ef_part;   // fused edge backward: per-workgroup partial weight gradients (efuse.hip)
  size_t bytes;
};
// can a precision of this build take the fused edge backward at this width and depth?  (The work size query has no precision argument.)
bool edge_fused_possible(GmpShape s) {
  s.training = true;
  s.precision = BSMS_BF16;
  if (s.fused()) return true;
  s.precision = BSMS_BF16_NODES;
  return s.fused();
}
GmpWork carve_gmp_work(void* base, const GmpShape& s) {
  Carver c(base);
  GmpWork w{};
  const int64_t D = s.D;
  const size_t re = size_t(s.B) * s.E, rn = size_t(s.B) * s.N;
  w.Ps = c.take(rn * D); w.Pd = c.take(rn * D);
  w.dPs = w.Ps; w.dPd = w.Pd;  // the backward reuses the two projection buffers for their gradients
  for (int l = 0; l <= s.H; ++l) w.gN[l] = c.take(pad_rows(rn) * D);   // written tile-wise by the backward chains
  w.daggr = c.take(rn * D);
  for (int l = 0; l <= s.H; ++l) w.gE[l] = c.take(pad_rows(re) * D);
  w.wg = c.take_bytes(wgrad_work_bytes((int)D, 0));
  w.wg2 = c.take_bytes(wgrad_work_bytes((int)D, 0));   // second split-K area: two wgrad launches run concurrently
  w.sw_bytes = small_wgrad_work_bytes_rows((int)D, s.B * s.N);   // one partial block per workgroup of the fused scatter kernel
  w.sw = c.take_bytes(w.sw_bytes);
  // one partial per workgroup of the fused edge backward: min(tiles, CUs) x 198 KB instead of 52 MB for every set
  w.ef_part = edge_fused_possible(s) ? c.take(edge_fused_part_floats(int64_t(re))) : nullptr;
  w.bytes = c.off;
  return w;
}

// where the saved tensors / packs of a call live (see carve_gmp_saved); inference: in the gradient scratch
GmpSaved locate_saved(const GmpCall& c, const GmpWork& wk) {
  return c.saved ? carve_gmp_saved(c.saved, c, nullptr) : carve_gmp_saved(wk.gN[0], c, c.packs_base);
}

// THE definition of "which packs a GMP block has" (the per-call prepack and the pack group both build their tables here)
PackTable block_pack_table(const GmpSaved& sv, const GmpCall& c) {
  const int D = (int)c.D, p1 = int(c.p + 1), H = c.H, nl = H + 1;
  const bool training = c.training, bf = c.bf(), bfn = c.bfn();
  const float* const* pn = c.params;            // mlp_node: W_l = pn[2l], b_l = pn[2l+1]
  const float* const* pe = c.params + 2 * nl;   // mlp_edge
  const int ldE0 = 2 * D + p1;
  PackTable t{};
  add_pack(t, pe[0], ldE0, 0, p1, D, D, PACK_FRAG, sv.e_wi, pe[1]);
  add_pack(t, pe[0], ldE0, 0, p1 + D, D, D, PACK_FRAG, sv.e_wj, nullptr);
  add_pack(t, pe[0], ldE0, 0, 0, D, p1, PACK_TRANSPOSE, sv.e_wft, nullptr);
  if (training) {   // grad_x += dPs Wi + dPd Wj runs as ONE Linear over [dPs, dPd]: the two packs share their scale (chain.h: mate)
    add_pack(t, pe[0], ldE0, 0, p1, D, D, PACK_FRAG_T, sv.e_wit, nullptr);
    add_pack(t, pe[0], ldE0, 0, p1 + D, D, D, PACK_FRAG_T, sv.e_wjt, nullptr);
    t.d[t.n - 2].mate = t.n;        // 1 + index of the other
    t.d[t.n - 1].mate = t.n - 1;
  }
  for (int l = 1; l <= H; ++l) {   // the D x D Linears of the edge MLP: bf16 operands in the bf16 precision
    add_pack(t, pe[2 * l], D, 0, 0, D, D, PACK_FRAG, sv.e_w[l], pe[2 * l + 1]);
    t.d[t.n - 1].bf16 = bf;
    if (training && sv.e_wt[l]) { add_pack(t, pe[2 * l], D, 0, 0, D, D, PACK_FRAG_T, sv.e_wt[l], nullptr); t.d[t.n - 1].bf16 = bf; }
    if (training && sv.e_wr[l]) add_pack(t, pe[2 * l], D, 0, 0, D, D, PACK_ROWS_BF16, sv.e_wr[l], nullptr);   // fused edge backward (efuse.hip)
  }
  // first node Linear over [x, aggr]: two packs, one scale; the bias rides in the second one (where the stage finishes).
  // BSMS_BF16_NODES: one-plane packs of the rounded weights; a bf16 stage STARTS from its pack's bias (chunk 0 header), so
  // the bias rides in the first pack there
  add_pack(t, pn[0], 2 * D, 0, 0, D, D, PACK_FRAG, sv.n_w0x, bfn ? pn[1] : nullptr);
  add_pack(t, pn[0], 2 * D, 0, D, D, D, PACK_FRAG, sv.n_w0a, bfn ? nullptr : pn[1]);
  t.d[t.n - 2].mate = t.n;
  t.d[t.n - 1].mate = t.n - 1;
  t.d[t.n - 2].bf16 = t.d[t.n - 1].bf16 = bfn;
  if (training) {
    add_pack(t, pn[0], 2 * D, 0, 0, D, D, PACK_FRAG_T, sv.n_w0xt, nullptr);
    add_pack(t, pn[0], 2 * D, 0, D, D, D, PACK_FRAG_T, sv.n_w0at, nullptr);
    t.d[t.n - 2].bf16 = t.d[t.n - 1].bf16 = bfn;
  }
  for (int l = 1; l <= H; ++l) {
    add_pack(t, pn[2 * l], D, 0, 0, D, D, PACK_FRAG, sv.n_w[l], pn[2 * l + 1]);
    t.d[t.n - 1].bf16 = bfn;
    if (training) { add_pack(t, pn[2 * l], D, 0, 0, D, D, PACK_FRAG_T, sv.n_wt[l], nullptr); t.d[t.n - 1].bf16 = bfn; }
  }
  t.zero = training ? sv.bound : nullptr;
  return t;
}

// the descriptor of an ABI call on a single block (fp32)
GmpCall abi_call(const bsms_plan_t* plan, int64_t B, int64_t D, int64_t p, int H, const float* const* params, void* saved, void* work) {
  GmpCall c;
  c.B = B; c.D = D; c.p = p; c.H = H; c.params = params;
  c.bind(plan, saved, work, nullptr);
  return c;
}
GmpShape abi_shape(int64_t B, int64_t N, int64_t E, int64_t D, int H) {
  GmpShape s;
  s.B = B; s.N = N; s.E = E; s.D = D; s.H = H;
  return s;
}

}  // namespace

// Frozen MLPs: which of a block's two MLPs get their weight gradients.  A host check, before any launch.
int bsms::gmp_check_grads(float* const* grads, int H, int precision, const char* who, bool* node_live, bool* edge_live, bool frozen_bf16) {
  const int n = 2 * (H + 1);
  const int ns = grads_state(grads, n), es = grads_state(grads ? grads + n : nullptr, n);
  BSMS_REQUIRE(ns >= 0 && es >= 0, BSMS_E_INVALID_ARG, "%s: the gradient entries of the %s MLP are partly null (an MLP is frozen as a whole: all "
               "%d entries null, or none)", who, ns < 0 ? "node" : "edge", n);
  BSMS_REQUIRE(precision == BSMS_F32 || frozen_bf16 || (ns == 1 && es == 1), BSMS_E_UNSUPPORTED, "%s: null gradient entries (a frozen MLP) need the fp32 "
               "precision: the fused edge backward of the bf16 precisions forms its weight gradients on chip", who);
  *node_live = ns == 1;
  *edge_live = es == 1;
  return BSMS_OK;
}

// =================================================================================== sizes and packs
size_t bsms::gmp_saved_bytes(const GmpShape& s) {
  if (s.H < 1 || s.H >= kMaxStages) return 0;
  return carve_gmp_saved(nullptr, s, nullptr).bytes;
}
extern "C" size_t bsms_gmp_saved_bytes(int64_t B, int64_t N, int64_t E, int64_t D, int hidden) {
  return gmp_saved_bytes(abi_shape(B, N, E, D, hidden));
}
extern "C" size_t bsms_gmp_work_bytes(int64_t B, int64_t N, int64_t E, int64_t D, int hidden) {
  if (hidden < 1 || hidden >= kMaxStages) return 0;
  return carve_gmp_work(nullptr, abi_shape(B, N, E, D, hidden)).bytes;
}
extern "C" size_t bsms_gmp_pos_work_bytes(int64_t B, int64_t E, int64_t p) {
  if (B < 0 || E < 0 || p < 1 || p > 7) return 0;
  return std::max<size_t>(pos_edge_scratch_bytes(B, E, p), 256);
}

size_t bsms::gmp_pack_bytes(int64_t D, int hidden) {   // inference packs of one block (upper bound: every take() is 256-byte aligned)
  return (size_t(2 * hidden + 4) * (pack_floats(D) * sizeof(float) + 256)) + size_t(8) * D * sizeof(float) + 256;
}

int bsms::gmp_prepack(const GmpCall& c, hipStream_t s) {
  return prepack_table(block_pack_table(locate_saved(c, carve_gmp_work(c.work, c)), c), s);
}
int bsms::gmp_pack_group_add(PackGroup* g, const GmpCall& c) {
  int rc = c.check("pack_group_add_bsgmp");
  if (rc) return rc;
  for (int i = 0; i < 4 * (c.H + 1); ++i)
    BSMS_REQUIRE(c.params[i] != nullptr, BSMS_E_INVALID_ARG, "pack_group_add_bsgmp: parameter %d of a block is null", i);
  if (!g) return BSMS_OK;   // checks only
  pack_group_append(*g, block_pack_table(locate_saved(c, carve_gmp_work(c.work, c)), c));
  return BSMS_OK;
}

// =================================================================================== forward
extern "C" int bsms_gmp_fwd(const bsms_plan_t* plan, const float* x, const float* pos, int64_t B, int64_t D, int64_t p,
                            int64_t pos_bstride, int H, const float* const* params, float* out, void* saved,
                            void* work, bsms_stream_t stream) {
  GmpCall c = abi_call(plan, B, D, p, H, params, saved, work);
  c.x = x; c.pos = pos; c.pos_bstride = pos_bstride;
  return gmp_fwd_core(c, out, nullptr, true, as_stream(stream));
}

int bsms::gmp_fwd_core(const GmpCall& c, float* out, const float* resid2, bool do_prepack, hipStream_t s) {
  BSMS_REQUIRE(c.plan != nullptr, BSMS_E_INVALID_ARG, "gmp_fwd: plan is null");
  int rc = c.check("gmp_fwd");
  if (rc) return rc;
  BSMS_REQUIRE(c.x && c.pos && c.params && out && c.work, BSMS_E_INVALID_ARG, "gmp_fwd: null argument");
  const bsms_plan* plan = c.plan;
  const int64_t B = c.B, N = c.N, E = c.E, D = c.D, p = c.p;
  const int H = c.H;
  const bool bf = c.bf(), bfn = c.bfn(), training = c.training, fused = c.fused();
  GmpWork wk = carve_gmp_work(c.work, c);
  GmpSaved sv = locate_saved(c, wk);
  if (do_prepack && (rc = prepack_table(block_pack_table(sv, c), s))) return rc;
  float* const Ps = fused ? sv.e_Ps : wk.Ps;   // the fused backward recomputes the edge activations: the projections are kept instead
  float* const Pd = fused ? sv.e_Pd : wk.Pd;

  // node pre-projections
  {
    ChainFwdArgs a{};
    a.R = B * N; a.x = c.x; a.nstage = 2;   // both projections in one launch (OUT_PLAIN2); bias b0 rides in the first pack
    a.wp[0] = reinterpret_cast<const float4*>(sv.e_wi); a.y = Ps;
    a.wp[1] = reinterpret_cast<const float4*>(sv.e_wj); a.y2 = Pd;
    if ((rc = launch_chain_fwd((int)D, IN_ROWS, OUT_PLAIN2, a, s))) return rc;
  }
  // edge MLP + LayerNorm
  if (c.edge_fwd_resident()) {
    EdgeFwdResArgs a{};
    a.R = B * E; a.E = (int32_t)E; a.N = (int32_t)N; a.src = plan->src; a.dst = plan->dst;
    a.Ps = Ps; a.Pd = Pd; a.pos = c.pos; a.pos_bstride = c.pos_bstride; a.p = (int)p; a.wft = sv.e_wft;
    for (int l = 1; l <= 3; ++l) a.wp[l - 1] = reinterpret_cast<const float4*>(sv.e_w[l]);
    a.y = sv.e_y; a.rstd = training ? sv.e_rstd : nullptr; a.fiber_out = training ? sv.e_fiber : nullptr;
    if ((rc = launch_edge_fwd_res(a, s))) return rc;
  } else {
    ChainFwdArgs a{};
    a.R = B * E; a.K0 = int(p + 1); a.w0t = sv.e_wft; a.store_in = fused ? nullptr : sv.e_act[0];
    a.src = plan->src; a.dst = plan->dst; a.E = (int32_t)E; a.N = (int32_t)N;
    a.Ps = Ps; a.Pd = Pd; a.pos = c.pos; a.pos_bstride = c.pos_bstride; a.p = (int)p;
    a.fiber_out = training ? sv.e_fiber : nullptr;
    a.bf16 = bf;
    a.nstage = H;
    for (int st = 0; st < H; ++st) {
      a.wp[st] = reinterpret_cast<const float4*>(sv.e_w[st + 1]);
      a.store[st] = (training && !fused && st < H - 1) ? sv.e_act[st + 1] : nullptr;
    }
    a.y = sv.e_y; a.rstd = sv.e_rstd;
    if (training && !bf) for (int st = 0; st < H; ++st) a.amax[st] = sv.bound + size_t(st) * kBoundWidth;
    a.timing = dbg(DBG_TIME_NODE_CHAIN) ? nullptr : g_timing;
    a.store_mode = (dbg(DBG_PLAIN_STORES) ? 0 : 1) | (dbg(DBG_NO_SIGN_BITS) ? 4 : 0) | (dbg(DBG_UNPAIRED_STORES) ? 8 : 0);   // non-temporal stores
    a.out_mode = dbg(DBG_NT_OUTPUT) ? 1 : 0;
    if (dbg(DBG_NO_ACT_STORES)) {
      a.store_in = nullptr;
      for (int st = 0; st < H; ++st) a.store[st] = nullptr;
    }
    if ((rc = launch_chain_fwd((int)D, IN_EDGE, OUT_LN, a, s))) return rc;
  }
  // aggregation (scatter_sum over targets, ops/basic.py:94)
  if ((rc = bf ? rowsum_plan_order_bf16(plan, sv.e_y, B, D, sv.aggr, s) : rowsum_plan_order(plan, sv.e_y, B, D, sv.aggr, s))) return rc;
  // node MLP + LayerNorm + residual
  {
    ChainFwdArgs a{};
    a.R = B * N; a.x = c.x; a.x2 = sv.aggr; a.nstage = H + 1;
    a.wp[0] = reinterpret_cast<const float4*>(sv.n_w0x);
    a.wp0b = reinterpret_cast<const float4*>(sv.n_w0a);
    a.store[0] = training ? sv.n_act[0] : nullptr;
    for (int st = 1; st <= H; ++st) {
      a.wp[st] = reinterpret_cast<const float4*>(sv.n_w[st]);
      a.store[st] = (training && st < H) ? sv.n_act[st] : nullptr;
    }
    a.y = out; a.yln = sv.n_yln; a.rstd = sv.n_rstd; a.resid = c.x; a.resid2 = resid2;
    a.bf16 = bfn;
    if (g_node_bf3 < 2) {   // bounds for the fp16 x 2 weight-gradient jobs of the node Linears
      if (training && !bfn) for (int st = 0; st <= H; ++st) a.amax[st] = sv.bound + size_t(8 + st) * kBoundWidth;
      else if (training) a.amax[0] = sv.bound + size_t(8) * kBoundWidth;   // BSMS_BF16_NODES: only [x, aggr] feed an fp32 weight-gradient job
    }
    a.store_mode = 1;
    a.timing = dbg(DBG_TIME_NODE_CHAIN) ? g_timing : nullptr;
    if ((rc = launch_chain_fwd((int)D, IN_ROWS2, OUT_LN, a, s))) return rc;
  }
  return BSMS_OK;
}

// =================================================================================== backward
extern "C" int bsms_gmp_bwd(const bsms_plan_t* plan, const float* x, const float* pos, const float* grad_out, int64_t B,
                            int64_t D, int64_t p, int64_t pos_bstride, int H, const float* const* params,
                            const void* saved, void* work, float* grad_x, float* const* grads, bsms_stream_t stream) {
  GmpCall c = abi_call(plan, B, D, p, H, params, const_cast<void*>(saved), work);
  c.x = x; c.pos = pos; c.pos_bstride = pos_bstride;
  return gmp_bwd_core(c, grad_out, grad_x, grads, GmpBwdOpts{}, as_stream(stream));
}

extern "C" int bsms_gmp_bwd_pos(const bsms_plan_t* plan, const float* x, const float* pos, const float* grad_out, int64_t B,
                                int64_t D, int64_t p, int64_t pos_bstride, int H, const float* const* params,
                                const void* saved, void* work, float* grad_x, float* const* grads, float* grad_pos, void* pos_work,
                                bsms_stream_t stream) {
  BSMS_REQUIRE(p >= 1 && p <= 7, BSMS_E_INVALID_ARG, "gmp_bwd_pos: pos_dim=%lld (1..7)", (long long)p);
  BSMS_REQUIRE(!grad_pos || pos_work, BSMS_E_INVALID_ARG, "gmp_bwd_pos: grad_pos needs pos_work (bsms_gmp_pos_work_bytes)");
  GmpCall c = abi_call(plan, B, D, p, H, params, const_cast<void*>(saved), work);
  c.x = x; c.pos = pos; c.pos_bstride = pos_bstride;
  GmpBwdOpts o;
  o.grad_pos = grad_pos; o.pos_work = pos_work;
  return gmp_bwd_core(c, grad_out, grad_x, grads, o, as_stream(stream));
}

// deferred-join mode: does lane 1's mark cover lane 0's (side_mark_chain)?  True unless an experiment switch disables a lane.
bool bsms::gmp_marks_chained() { return !dbg(DBG_NO_SIDE_LANES) && !dbg(DBG_NO_LANE2); }

namespace {
// joins (or marks) a side lane on EVERY exit path of gmp_bwd_core: an error return between fork and join would
// otherwise leave the lane dangling, which also breaks an in-progress HIP-graph capture
struct LaneScope {
  SideLane* lane = nullptr;
  hipStream_t main;
  int slot;
  explicit LaneScope(hipStream_t m, int defer_slot) : main(m), slot(defer_slot) {}
  int finish() {
    SideLane* l = lane;
    lane = nullptr;
    if (!l) return BSMS_OK;
    return slot < 0 ? side_join(l, main) : side_mark(l, slot);
  }
  ~LaneScope() { if (lane) side_join(lane, main); }
};

// The backward of one block, in stages over one context.  The stages run in the order of gmp_bwd_core below and nowhere else: the
// order of their launches, forks and joins ON THE HOST is itself tuned.
//
// After the two backward chains, independent strands run CONCURRENTLY (fork/join on internal side streams):
//   lane 0: the MFMA-bound batched weight gradients of all D x D layers (reads gE[1..H], gN[*], saved activations)
//   main:   the HBM-bound strand -- scatter of gE[0] to the two projections and finally the input gradient
//   lane 1: the remaining weight gradients of the first edge Linear (fiber columns + bias, the x-columns once dPs / dPd exist), so
//           that the caller's stream only carries what grad_x depends on: gE[0] -> dPs, dPd -> grad_x
// They touch disjoint outputs; main joins the side streams before returning (or marks them: GmpBwdOpts::defer_slot), so callers see
// ordinary semantics.  (Forking the node-layer gradients earlier, against the edge backward chain, measured SLOWER: two MFMA-bound
// kernels contend; an MFMA-bound kernel against HBM-bound ones is the pairing that pays: +5.6 % steps/s.)
// A lane with nothing to run (frozen MLPs) is neither forked nor joined.
struct GmpBwd {
  const GmpCall& c;
  const float* grad_out;
  float* grad_x;
  const GmpBwdOpts& o;
  hipStream_t s;               // the caller's stream
  // frozen MLPs: `nlive` / `elive` = the node / edge MLP gets its weight gradients.  Nothing that only serves a frozen MLP's dW / db
  // is launched, and the backward chains do not store the layer gradients that only those launches read
  bool nlive, elive;
  float* const* gn;            // the node / edge MLP's gradient entries; null: frozen
  float* const* ge;
  GmpSaved sv;
  GmpWork wk;
  int ef_nwg = 0;              // workgroups (= partials) of the fused edge backward
  LaneScope scope1, scope2;    // lane 0 / lane 1, once forked

  const int64_t B = c.B, N = c.N, E = c.E, D = c.D, p = c.p;
  const int H = c.H, ldE0 = int(2 * c.D + c.p + 1);
  const bool bf = c.bf(), bfn = c.bfn(), fused = c.fused();
  const bool overlap = !dbg(DBG_NO_SIDE_LANES);
  const bool x_job_on_lane2 = nlive && g_node_bf3 == 1;   // the x half of the first node Linear rides with the projections (lane0_wgrads)
  const bool overlap2 = overlap && !dbg(DBG_NO_LANE2) && (elive || x_job_on_lane2);

  GmpBwd(const GmpCall& call, const float* grad_out_, float* grad_x_, float* const* grads, bool node_live, bool edge_live,
         const GmpBwdOpts& opts, hipStream_t stream)
      : c(call), grad_out(grad_out_), grad_x(grad_x_), o(opts), s(stream), nlive(node_live), elive(edge_live),
        gn(node_live ? grads : nullptr), ge(edge_live ? grads + 2 * (call.H + 1) : nullptr),
        sv(carve_gmp_saved(call.saved, call, nullptr)), wk(carve_gmp_work(call.work, call)), scope1(stream, opts.defer_slot),
        scope2(stream, opts.defer_slot) {}

  float* GN(int i) const { return gn ? gn[i] : nullptr; }   // a frozen MLP's jobs stay in the tables (they shape the launch, chain.h:
  float* GE(int i) const { return ge ? ge[i] : nullptr; }   // launch_wgrad `skip_mask`) but are not run and have no target
  const float* bd(int slot) const { return sv.bound + size_t(slot) * kBoundWidth; }
  // no bounds = the range-free arithmetic: the job over the caller's x (g_node_bf3 >= 1), every node-level job (2)
  const float* nbd(int slot, int level) const { return g_node_bf3 >= level ? nullptr : bd(slot); }
  // one D x D weight-gradient job over `R` rows; every operand comes with a magnitude bound from the chain kernel that produced or
  // consumed it (GmpSaved::bound), or with none
  WgradJob job(const float* G, const float* A, float* dW, float* db, int64_t R, int ldw, int col0, const float* gb, const float* ab) const {
    WgradJob j{};
    j.G = G; j.A = A; j.dW = dW; j.db = db; j.R = R; j.ldg = (int)D; j.lda = (int)D; j.ldw = ldw; j.col0 = col0; j.bf16 = 0;
    j.g_bound = gb; j.a_bound = ab; j.g_mul = j.a_mul = 1.f;
    return j;
  }

  // node MLP backward: grad_x = grad_out (residual) + g0 W0x ; daggr = g0 W0a
  int node_chain() {
    ChainBwdArgs a{};
    a.R = B * N; a.dy = grad_out; a.yln = sv.n_yln; a.rstd = sv.n_rstd; a.store_mode = 1;
    a.nstage = H;
    a.gstore[0] = nlive ? wk.gN[H] : nullptr;   // frozen: no gN[l] has a reader (dx / dx2 leave the heads from registers)
    for (int k = 0; k < H; ++k) {
      a.wpt[k] = reinterpret_cast<const float4*>(sv.n_wt[H - k]);
      a.mask[k] = sv.n_act[H - k - 1];
      a.gstore[k + 1] = nlive ? wk.gN[H - k - 1] : nullptr;
    }
    a.wh0 = reinterpret_cast<const float4*>(sv.n_w0xt);
    a.wh1 = reinterpret_cast<const float4*>(sv.n_w0at);
    a.dx = grad_x; a.dx2 = wk.daggr; a.dres = grad_out;
    a.bf16 = bfn;
    if (g_node_bf3 < 2 && nlive) {   // (only weight-gradient jobs read the bounds)
      if (!bfn) for (int k = 0; k <= H; ++k) a.gmax[k] = sv.bound + size_t(24 + k) * kBoundWidth;
      else a.gmax[H] = sv.bound + size_t(24 + H) * kBoundWidth;   // BSMS_BF16_NODES: only gN[0] (fp32) feeds an fp32 weight-gradient job
    }
    const int rc = launch_chain_bwd((int)D, G_ROWS_LN, F_HEADS2, a, s);
    if (rc || !bfn || !nlive) return rc;
    // BSMS_BF16_NODES: gN[H] is stored as bf16 rows for the weight-gradient products, and the last node Linear's bias gradient used to
    // be the column sum of those rounded rows: 2^-9 of the fp32 sum at any depth.  It is summed from the unrounded LayerNorm backward
    // instead (posgrad.hip: ln_bias_grad; lane0_wgrads gives that job no db).  On the caller's stream, in front of the forks: grad_out
    // belongs to the caller, who may rewrite it while the lanes still run, and the split-K area is this block's own until lane 0 starts.
    BSMS_REQUIRE(ln_bias_grad_work_floats(D) * sizeof(float) <= wgrad_work_bytes((int)D, 0), BSMS_E_SHAPE, "gmp_bwd: bias-gradient partials exceed the split-K area");
    return ln_bias_grad(grad_out, sv.n_yln, sv.n_rstd, B * N, D, reinterpret_cast<float*>(wk.wg), gn[2 * H + 1], s);
  }

  // edge MLP backward (gradient of the aggregation = gather by target)
  int edge_chain() {
    if (fused) {   // recompute + LayerNorm backward + dgrad + the weight gradients of Linears 1..H on chip (efuse.hip)
      EdgeFusedBwdArgs a{};
      a.R = B * E; a.E = (int32_t)E; a.N = (int32_t)N; a.src = c.plan->src; a.dst = c.plan->dst;
      a.Ps = sv.e_Ps; a.Pd = sv.e_Pd; a.fiber = sv.e_fiber; a.wft = sv.e_wft; a.p = (int)p;
      const float* const* pe = c.params + 2 * (H + 1);
      for (int l = 1; l <= 3; ++l) { a.wr[l - 1] = reinterpret_cast<const float4*>(sv.e_wr[l]); a.b[l - 1] = pe[2 * l + 1]; }
      a.dy = wk.daggr; a.y = sv.e_y; a.rstd = sv.e_rstd; a.g0 = wk.gE[0];
      a.gmax = g_node_bf3 ? nullptr : sv.bound + size_t(16 + H) * kBoundWidth;   // only the projections' weight gradients used it
      a.timing = g_timing;
      // a frozen edge MLP (BSMS_BWD_FROZEN_BF16): the data-only kernel -- the same rows of g_0, no gradient waves, no partials, no
      // bound (its only reader, the projections' weight-gradient jobs, is skipped)
      if (!elive) { a.gmax = nullptr; return launch_edge_data_bwd(a, s); }
      a.part = wk.ef_part;
      return launch_edge_fused_bwd(a, &ef_nwg, s);
    }
    ChainBwdArgs a{};
    a.R = B * E; a.dy = wk.daggr; a.yln = sv.e_y; a.rstd = sv.e_rstd;
    a.store_mode = (dbg(DBG_PLAIN_STORES) ? 0 : dbg(DBG_BWD_STORE_MODE2) ? 2 : 1) | (dbg(DBG_UNPAIRED_STORES) ? 8 : 0);
    a.dst = c.plan->dst; a.E = (int32_t)E; a.N = (int32_t)N;
    a.bf16 = bf;
    a.nstage = H;
    a.gstore[0] = elive ? wk.gE[H] : nullptr;   // frozen: gE[1..H] have no reader; gE[0] keeps two (the scatter, the position gradient)
    for (int k = 0; k < H; ++k) {
      a.wpt[k] = reinterpret_cast<const float4*>(sv.e_wt[H - k]);
      a.mask[k] = sv.e_act[H - k - 1];
      a.gstore[k + 1] = (elive || k + 1 == H) ? wk.gE[H - k - 1] : nullptr;
    }
    // (a frozen edge MLP notes no bounds: the jobs that read them, the projections' included, are gone)
    if (elive && !bf) for (int k = 0; k <= (g_node_bf3 ? H - 1 : H); ++k) a.gmax[k] = sv.bound + size_t(16 + k) * kBoundWidth;   // gE[0] feeds only the projections' jobs
    else if (elive && !g_node_bf3) a.gmax[H] = sv.bound + size_t(16 + H) * kBoundWidth;   // bf16 precision: only gE[0] (fp32 scatter sums dPs / dPd feed fp32 weight-gradient jobs)
    a.ablate = dbg(DBG_NO_GRAD_STREAM) ? 1 : 0;
    return launch_chain_bwd((int)D, G_EDGE_LN, F_NONE, a, s);
  }

  // lane 0: fork, then the weight gradients of every D x D Linear but the ones that ride on lane 1, in ONE launch
  int lane0_wgrads() {
    if (!nlive && !elive) return BSMS_OK;
    int rc;
    hipStream_t ws = s;
    if (overlap) {
      SideLane* lane = nullptr;
      if ((rc = side_lane(&lane, 0, s)) || (rc = side_fork(lane, s))) return rc;
      ws = lane->stream;
      scope1.lane = lane;
    }
    WgradJob jobs[kMaxWgradJobs] = {};
    int nj = 0;
    unsigned skip = 0;
    if (fused && elive) {   // the edge Linears' gradients were accumulated by the fused kernel: only the fixed-order sum of its partials is left
      float* const dWs[3] = {ge[2], ge[4], ge[6]};
      float* const dbs[3] = {ge[3], ge[5], ge[7]};
      if ((rc = launch_edge_fused_reduce(wk.ef_part, ef_nwg, dWs, dbs, ws))) return rc;
    }
    for (int l = 1; l <= H && !fused && !dbg(DBG_NO_EDGE_WGRAD); ++l) {   // edge Linears: bf16 gradient and activation tensors in the bf16 precision
      jobs[nj++] = job(wk.gE[l], sv.e_act[l - 1], GE(2 * l), GE(2 * l + 1), B * E, (int)D, 0, bd(16 + (H - l)), bd(l - 1));
      jobs[nj - 1].bf16 = bf;
      if (!elive) skip |= 1u << (nj - 1);
    }
    for (int l = 1; l <= H; ++l) {   // node Linears 1..H: bf16 tensors in BSMS_BF16_NODES
      jobs[nj++] = job(wk.gN[l], sv.n_act[l - 1], GN(2 * l), (bfn && l == H) ? nullptr : GN(2 * l + 1), B * N, (int)D, 0, nbd(24 + (H - l), 2), nbd(8 + l, 2));   // (bfn, l == H: node_chain)
      jobs[nj - 1].bf16 = bfn;
      if (!nlive) skip |= 1u << (nj - 1);
    }
    // the job over the caller's x (with the first node Linear's bias gradient): range-free arithmetic = another launch, so
    // at level 1 it rides in lane 1's launch with the two projections (all three range-free) and this lane stays ONE launch of
    // three-product jobs -- two launches here cost the cylinder steps 1.6 % / 6 % (side lane co-critical, r05_node_bf3_ab.txt)
    if (g_node_bf3 != 1) {
      jobs[nj++] = job(wk.gN[0], c.x, GN(0), GN(1), B * N, int(2 * D), 0, nbd(24 + H, 1), nbd(8, 1));
      if (!nlive) skip |= 1u << (nj - 1);
    }
    jobs[nj++] = job(wk.gN[0], sv.aggr, GN(0), nullptr, B * N, int(2 * D), (int)D, nbd(24 + H, 2), nbd(8, 2));
    if (!nlive) skip |= 1u << (nj - 1);
    return launch_wgrad((int)D, jobs, nj, wk.wg, ws, skip);
  }

  // main: gE[0] -> dPs, dPd, the gradient of the first edge Linear w.r.t. the two per-node projections -- and, in the same pass over
  // gE[0], the partial sums of its fiber columns and bias (rowsum.hip: k_rowsum_pair_fiber).  Lane 1: the small reduction of those
  // partials and the x-columns of W0_edge (the two projections' weight gradients).
  int scatter_strand() {
    int rc;
    SideLane* lane2 = nullptr;
    hipStream_t s2 = s;
    if (overlap2) {   // (its first fork is only needed by the separate-pass path; the fused-scatter path forks once, below)
      if ((rc = side_lane(&lane2, 1, s))) return rc;
      s2 = lane2->stream;
    }
    SmallWgradArgs sw{};
    sw.G = wk.gE[0]; sw.S = sv.e_fiber; sw.S_cols = int(p + 1); sw.S_ld = fiber_ld(p);   // the fiber rows the forward kept
    sw.p = (int)p;
    if (elive) { sw.out = ge[0]; sw.colsum = ge[1]; }
    sw.os = 1; sw.of = ldE0;
    sw.R = B * E; sw.D = (int)D;
    int nwg = 0;
    // a frozen edge MLP: only the scatter is left -- the plain pair, which sums every row's slots in the same order as the fused
    // kernel (rowsum.hip: rowsum_body / fiber_batch), so dPs / dPd are bit-identical
    if (!elive) {
      if ((rc = rowsum_source_and_target(c.plan, wk.gE[0], B, D, wk.dPs, wk.dPd, s, bf))) return rc;
    } else if ((rc = rowsum_source_target_fiber(c.plan, wk.gE[0], B, D, wk.dPs, wk.dPd, sv.e_fiber, fiber_ld(p), int(p + 1),
                                                reinterpret_cast<float*>(wk.sw), small_wgrad_part_blocks(wk.sw_bytes, (int)D), &nwg, s, bf))) return rc;
    BSMS_REQUIRE(nwg > 0 || !bf || !elive, BSMS_E_UNSUPPORTED, "gmp_bwd: bf16 precision needs the fused scatter kernel (D = 128 / 256, pos_dim <= 3)");
    if (nwg == 0 && elive) {   // shape not built into the fused kernel (D < 128, pos_dim > 3): separate passes
      if (overlap2) {
        if ((rc = side_fork(lane2, s))) return rc;
        scope2.lane = lane2;
      }
      if ((rc = rowsum_source_and_target(c.plan, wk.gE[0], B, D, wk.dPs, wk.dPd, s))) return rc;
      if ((rc = launch_small_wgrad(sw, wk.sw, s2))) return rc;
    }
    if (overlap2) {   // lane 1 waits for dPs / dPd (and the partials)
      if ((rc = side_fork(lane2, s))) return rc;
      scope2.lane = lane2;
    }
    if (nwg > 0 && (rc = launch_small_reduce(sw, wk.sw, nwg, s2))) return rc;
    if (!elive && !x_job_on_lane2) return BSMS_OK;
    // dPs / dPd are sums of at most max-degree rows of gE[0]; x is covered by the joint bound of the node chain's input
    const float* const gb = g_node_bf3 ? nullptr : bd(16 + H);
    const float* const ab = g_node_bf3 ? nullptr : bd(8);
    WgradJob jobs[3] = {};
    jobs[0] = job(wk.dPs, c.x, GE(0), nullptr, B * N, ldE0, int(p + 1), gb, ab);
    jobs[1] = job(wk.dPd, c.x, GE(0), nullptr, B * N, ldE0, int(p + 1 + D), gb, ab);
    jobs[0].g_mul = float(std::max<int64_t>(c.plan->max_out_degree, 1));   // scatter by source
    jobs[1].g_mul = float(std::max<int64_t>(c.plan->max_in_degree, 1));    // scatter by target
    int nj = 2;
    unsigned skip = elive ? 0u : 3u;   // a frozen edge MLP: the two projection jobs only shape the launch
    if (g_node_bf3 == 1) {   // + the x half of the first node Linear (lane0_wgrads)
      jobs[nj++] = job(wk.gN[0], c.x, GN(0), GN(1), B * N, int(2 * D), 0, nullptr, nullptr);
      if (!nlive) skip |= 1u << (nj - 1);
    }
    return launch_wgrad((int)D, jobs, nj, wk.wg2, s2, skip);
  }

  // grad_x += dPs Wi + dPd Wj
  int input_grad() {
    ChainFwdArgs a{};
    a.R = B * N; a.x = wk.dPs; a.x2 = wk.dPd; a.nstage = 1;
    a.wp[0] = reinterpret_cast<const float4*>(sv.e_wit);
    a.wp0b = reinterpret_cast<const float4*>(sv.e_wjt);
    a.y = grad_x; a.accumulate = 1;
    return launch_chain_fwd((int)D, IN_ROWS2, OUT_PLAIN, a, s);
  }

  // position gradient (posgrad.hip): on the caller's stream, so gE[0] is read before a later block reuses this scratch set
  int pos_grad() {
    if (!o.grad_pos) return BSMS_OK;
    return gmp_pos_grad(c.plan, wk.gE[0], bf, sv.e_fiber, c.params[2 * (H + 1)], B, D, p, c.pos_bstride, o.grad_pos, o.pos_accumulate,
                        reinterpret_cast<float*>(o.pos_work), s);
  }

  // join, or -- deferred -- mark: one event covers both lanes (lane 1's mark waits for lane 0's).  The mark covers whichever lanes
  // ran: none (everything frozen) marks nothing; lane 0 alone -- experiment builds only -- is chained into lane 1's slot all the same,
  // since callers wait for lane 1's mark (gmp_marks_chained)
  int finish() {
    int rc;
    if (o.defer_slot >= 0 && scope1.lane) {
      SideLane *a = scope1.lane, *b = scope2.lane;
      if (!b && (rc = side_lane(&b, 1, s))) return rc;
      scope1.lane = scope2.lane = nullptr;
      return side_mark_chain(a, b, o.defer_slot);
    }
    if ((rc = scope1.finish()) || (rc = scope2.finish())) return rc;
    return BSMS_OK;
  }
};
}  // namespace

int bsms::gmp_bwd_core(const GmpCall& c, const float* grad_out, float* grad_x, float* const* grads, const GmpBwdOpts& o, hipStream_t s) {
  BSMS_REQUIRE(c.plan != nullptr, BSMS_E_INVALID_ARG, "gmp_bwd: plan is null");
  int rc = c.check("gmp_bwd");
  if (rc) return rc;
  BSMS_REQUIRE(c.x && c.pos && grad_out && c.params && c.saved && c.work && grad_x, BSMS_E_INVALID_ARG, "gmp_bwd: null argument");
  bool nlive = true, elive = true;
  if ((rc = gmp_check_grads(grads, c.H, c.precision, "gmp_bwd", &nlive, &elive, o.frozen_bf16))) return rc;
  GmpBwd b(c, grad_out, grad_x, grads, nlive, elive, o, s);   // (an error return below joins the lanes forked so far: LaneScope)
  if ((rc = b.node_chain()) || (rc = b.edge_chain()) || (rc = b.lane0_wgrads()) || (rc = b.scatter_strand()) || (rc = b.input_grad()) ||
      (rc = b.pos_grad()))
    return rc;
  return b.finish();
}
