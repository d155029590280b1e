/* bsms_hip.h -- C ABI of libbsms_hip.so: the MI355X (gfx950) engine for the BSMS-GNN hot path.
 *
 * The reference (Eydcao/BSMS-GNN @ 2024_10_08) has no FFI layer: its hot path sits behind the
 * Python nn.Module API of src/ops + src/models.  This header is the boundary a maintainer would
 * bind instead (ctypes stub in INTEGRATION.md); each entry names the reference code it replaces
 * (paths relative to /root/reference/src).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  Every call returns 0 (BSMS_OK) or a
 *     negative bsms_status; bsms_last_error() gives a thread-local message.  Never throws/exits.
 *   - All tensor arguments are CALLER-OWNED DEVICE pointers: fp32, row-major, contiguous,
 *     16-byte aligned.  The library never allocates, frees or synchronises on the data path; the
 *     one exception is bsms_plan_create/destroy, which own the small integer index buffers of a
 *     mesh level (lifetime = plan).  Scratch ("work") and saved-for-backward ("saved") buffers are
 *     caller-provided; their sizes come from the *_bytes() queries.
 *   - Every launch goes to the hipStream_t passed as `stream` (void* here so C callers need no HIP
 *     headers).  Re-entrant and thread-safe per stream.  Global state: the thread-local error string and,
 *     per device, two lazily created internal side streams (+ two events each) that bsms_gmp_bwd uses to
 *     overlap its weight-gradient kernels with its gradient scatters (forked from and joined back into
 *     `stream` inside the call, also legal under HIP-graph capture).
 *     The FIRST call that needs a side stream creates it and checks once, with a few device fills on a temporary
 *     64 MB allocation (~1 ms), that it does not share its hardware queue with the default stream or the other side
 *     stream -- HIP places streams on four hardware queues and two streams on one queue run in order.
 *     If `stream` is being CAPTURED at that first call the check is skipped (it allocates and synchronises, which would
 *     invalidate the capture): the side stream is created plainly and may share a queue -- less overlap, same results.
 *     Run one eager call before capturing to get the checked streams.
 *   - Arithmetic: fp32 in, fp32 out, fp32 accumulation.  Matrix products run on the f16 matrix cores as three
 *     partial products of two-way fp16 splits (11 + 11 significand bits) of power-of-two-scaled fp32 operands.
 *     Forward and input-gradient products scale per activation ROW and per weight MATRIX: the result is at least as
 *     accurate as an fp32 fused-multiply-add chain and as v_mfma_f32_16x16x4_f32 over the whole fp32 range
 *     (chain.h; profiles/census/f16split.hip; tests/test_hip_parity.py).  The WEIGHT gradients reduce over rows, so a
 *     scale cannot vary by row.  NODE-level weight gradients (node MLP, the two projections of the first edge Linear,
 *     bsms_mlp_bwd -- every job whose operand may be a caller's tensor) use the RANGE-FREE arithmetic: the exact
 *     three-way bf16 split (8 + 8 + 8 bits, fp32's exponent range, no scale), six partial products: a feature column
 *     1e-7 of the tensor's maximum is as accurate as in fp32 arithmetic (test_weight_gradient_precision_per_column).
 *     EDGE-level weight gradients of the fp32 GMP (85 % of the weight-gradient work; all six range-free would cost 3.8 % of
 *     the step, profiles/r05_wgrad_bf3_ab.txt) keep fp16 x 2 pieces with one power-of-two scale per operand TENSOR from
 *     the magnitude bound the chain kernels record: an element within 2^-18 of its tensor's largest magnitude keeps all
 *     22 bits; below that the low piece is an fp16 subnormal and one bit is lost per octave.  Their operands are the edge
 *     MLP's own post-ReLU activations and layer gradients -- never a caller's tensor -- which span far less than 2^18 per
 *     tensor (measured at full size, tests/test_hip_fullsize.py: gradients as close to fp64 as the fp32 oracle's);
 *     test_edge_weight_gradient_envelope pins that envelope.
 *   - Edge lists follow the reference: g = int64 [2,E], g[0] = source i, g[1] = target j
 *     (ops/basic.py:66); aggregation target is j.  "Edge order" below = the caller's order of g.
 *   - `D` (latent width) of the MLP/GMP entries: a multiple of 32 (MFMA tile width), 32 <= D <= 256; the bf16
 *     precisions only at D = 128 / 256 (other widths: BSMS_E_UNSUPPORTED).
 *   - An MLP is `hidden` x (Linear,ReLU) + Linear (+LayerNorm, no affine, eps 1e-5)
 *     (ops/basic.py:6-23).  `params` is a HOST array of 2*(hidden+1) device pointers in state_dict
 *     order: seq.0.weight, seq.0.bias, seq.2.weight, seq.2.bias, ...  Weights are [out,in] row-major
 *     exactly as torch.nn.Linear stores them.  `grads` arrays have the same order and shapes and
 *     are OVERWRITTEN (not accumulated).
 *   - `hidden`: 1 <= hidden <= 7 in every entry that takes one.  Outside that range the calls return
 *     BSMS_E_UNSUPPORTED before any launch and every size query -- a block's, an MLP's, the U-Net's -- returns 0.
 */
#ifndef BSMS_HIP_H
#define BSMS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  BSMS_OK = 0,
  BSMS_E_INVALID_ARG = -1,
  BSMS_E_SHAPE = -2,
  BSMS_E_UNSUPPORTED = -3,
  BSMS_E_HIP = -4
} bsms_status;

/* Precision of the tensors inside a GMP block (the *_p entries of the U-Net).  BSMS_F32 is the reference's arithmetic.
 * The other two are build extensions without a reference parity target (the reference has no mixed precision):
 * BSMS_BF16: the saved EDGE activations, the messages and the edge layer gradients are stored in HBM as bf16 (round to
 *   nearest even) and the D x D Linears of the edge MLP multiply bf16 operands (weights rounded once per call) with fp32
 *   accumulation; bias, ReLU, LayerNorm, the aggregation sums, every node-level tensor and kernel (projections, node
 *   MLP, transitions, skip connections), the encoder / decoder and all weight-gradient accumulators stay fp32.
 * BSMS_BF16_NODES (round 4): BSMS_BF16 plus the NODE MLP: its four Linears multiply bf16 operands (the rows [x, aggr] and
 *   the hidden activations rounded to bf16 as they enter a Linear, weights rounded once per call; fp32 accumulation,
 *   bias, ReLU, LayerNorm), its hidden activations are saved as bf16 and its layer gradients gN[1..H] are stored as bf16
 *   (one-product weight-gradient jobs); the block's input / output rows [B,N,D], the residual and skip additions, the
 *   projections, gN[0] and the weight gradient of the first node Linear (operands x, aggr in fp32) stay fp32, and so does the
 *   bias gradient of the LAST node Linear: the column sum of the unrounded LayerNorm backward, not of the rows of gN[H]. */
typedef enum { BSMS_F32 = 0, BSMS_BF16 = 1, BSMS_BF16_NODES = 2 } bsms_precision;

typedef struct bsms_plan bsms_plan_t; /* one mesh level: dst-sorted CSR + src-sorted transpose */
typedef void* bsms_stream_t;          /* hipStream_t */

int bsms_abi_version(void);           /* bumps when a signature changes */
const char* bsms_last_error(void);

/* ---------------------------------------------------------------- graph plan (host side) ----
 * Replaces the per-call index handling of utils/basic.py:312-343 (broadcast + scatter_add_) and
 * ops/basic.py:66-72,127-138 (x[:, i], x[:, j] gathers): the COO list is turned ONCE per mesh
 * into a destination-sorted CSR (stable, so each target sums its edges in the caller's edge
 * order, like a sequential scatter_add_) plus the source-sorted transpose used by the backward
 * gathers and the up-pass.  `coo_host` is a HOST pointer to int64 [2,E].  Indices must be
 * < 2^31.  bsms_plan_set_pool attaches the kept-node ids of the level (m_ids[l],
 * graph_wrappers/bsms_graph_wrapper.py:97-98; HOST int64 [Nk], ascending) for the fused
 * restrict / prolong kernels.
 * The index buffers of a plan are ONE device block, uploaded on a private stream (creating a plan does not wait for work
 * queued on the caller's streams).  bsms_plan_destroy / a second bsms_plan_set_pool hand the block to an internal pool
 * instead of hipFree (which would wait for the whole device): the caller guarantees that nothing using the plan is
 * still in flight, as for any buffer it owns.  bsms_plan_pool_trim releases the pooled blocks (waits for the device). */
int bsms_plan_create(const int64_t* coo_host, int64_t E, int64_t N, bsms_plan_t** out);
int bsms_plan_set_pool(bsms_plan_t* plan, const int64_t* ids_host, int64_t Nk);
/* Binds the DEVICE edge weights `ew` [E] (edge order; WeightedEdgeConv.cal_ew, ops/basic.py:142-167 -- mesh-static, the
 * reference recomputes them every forward, BSMS.py:73) to a plan with a pool: they are gathered once into the slot orders
 * of the two pooled transitions, and every later bsms_edge_conv(..., ew, ..., pooled = 1) / U-Net call that passes the
 * SAME pointer takes compact index + weight streams instead of four levels of dependent index loads.  The caller
 * guarantees that the content of `ew` is unchanged for as long as it passes that pointer; ew = NULL unbinds.  Results
 * are bit-identical to the unbound path.  A new bsms_plan_set_pool unbinds.  A plan already bound to ANOTHER non-null
 * pointer keeps that binding (captured HIP graphs and kernels still queued have the gathered copies baked in); the new
 * tensor then simply takes the unbound path.  To move a binding: bind NULL first, once nothing uses the old one.
 * Binding the pointer a plan is ALREADY bound to is a no-op (the copies are not gathered again): after changing the
 * content of `ew` in place, bind NULL and then `ew` again to refresh them.  The binding is by ADDRESS: the caller keeps
 * the bound tensor alive (and its address unrecycled) until it unbinds or destroys the plan;
 * bsms_plan_bound_edge_weights returns the pointer a plan is bound to (NULL: unbound) so that a host wrapper can tell
 * whether its bind call took effect and which tensor it has to keep alive. */
int bsms_plan_bind_edge_weights(bsms_plan_t* plan, const float* ew, bsms_stream_t stream);
const float* bsms_plan_bound_edge_weights(const bsms_plan_t* plan);
int bsms_plan_destroy(bsms_plan_t* plan);
int bsms_plan_pool_trim(void);
int64_t bsms_plan_num_nodes(const bsms_plan_t* plan);
int64_t bsms_plan_num_edges(const bsms_plan_t* plan);
int64_t bsms_plan_num_pooled(const bsms_plan_t* plan);  /* Nk, 0 if no pool attached */
int64_t bsms_plan_min_out_degree(const bsms_plan_t* plan);
int64_t bsms_plan_max_source(const bsms_plan_t* plan);  /* max(g[0]); degree() length-1, utils/basic.py:305 */
/* Block-diagonal union of `nparts` plans, built ON THE DEVICE from the parts' index blocks (one kernel per 16 parts on `stream`;
 * no host CSR build, no upload): the plan of a batch of DIFFERENT meshes -- the reference's variable-mesh path, PyG `Batch`
 * collation of datasets/base.py:325-349 consumed at models/model.py:194-200 -- from per-mesh plans that stay resident in HBM.
 * Equal, array for array, to bsms_plan_create on the offset-concatenated edge list + bsms_plan_set_pool on the offset kept ids
 * (all parts have pools, or none).  `ew_cat` (nullable): the DEVICE concatenation of the parts' bound edge-weight tensors, in part
 * order; every part must then be bound (bsms_plan_bind_edge_weights), the union is bound to `ew_cat` and its gathered weight
 * copies are the parts'.  `coo_out` (nullable): DEVICE int64 [2, E] that receives the union's edge list in the caller's edge
 * order; `ids_out` (nullable): DEVICE int64 [Nk], its kept ids (what PyG's Batch would have produced).  The arrays of the new
 * plan are complete in STREAM ORDER: use it on `stream`, or synchronise first.  The calls that read a plan's arrays on the HOST
 * (bsms_plan_export, bsms_plan_export_ex, bsms_plan_set_pool on the union) wait for that themselves. */
int bsms_plan_concat(const bsms_plan_t* const* parts, int nparts, const float* ew_cat, int64_t* coo_out, int64_t* ids_out,
                     bsms_stream_t stream, bsms_plan_t** out);
/* debug/test accessors: copy index arrays to HOST int32 buffers (sizes N+1, E, E, E). */
int bsms_plan_export(const bsms_plan_t* plan, int32_t* rowptr, int32_t* src_sorted,
                     int32_t* perm, int32_t* t_rowptr);
/* array `which` of a plan as int32 words on the HOST (host == NULL: only its length is returned; < 0: error):
 * 0 rowptr 1 src 2 dst 3 perm 4 t_rowptr 5 t_dst 6 t_eid 7 t_pos 8 ids 9 inv 10 k_rowptr 11 k_src 12 k_eid 13 p_rowptr 14 p_src
 * 15 p_eid 16 k_w 17 p_w (bit patterns of the gathered edge weights; length 0 while unbound).  Synchronises the device. */
int64_t bsms_plan_export_ex(const bsms_plan_t* plan, int which, int32_t* host);

/* ---------------------------------------------------------------- A1: edge aggregation ------
 * scatter_sum(src, index=g[1], dim=-2, dim_size=N)  (utils/basic.py:324-343, call site
 * ops/basic.py:94): out[b,n,:] = sum over edges e with g[1][e]==n of src[b,e,:], summed in edge
 * order.  plan_order=0: `src` rows are in the caller's edge order; 1: already dst-sorted
 * (plan order, what the fused GMP path produces).  The backward is the gather grad[b, g[1][e], :]
 * (autograd of scatter_add_), written in edge order. */
int bsms_segment_sum_fwd(const bsms_plan_t* plan, const float* src, int64_t B, int64_t D,
                         int plan_order, float* out, bsms_stream_t stream);
int bsms_segment_sum_bwd(const bsms_plan_t* plan, const float* grad_out, int64_t B, int64_t D,
                         float* grad_src, bsms_stream_t stream);
/* The aggregation of the BSMS_BF16 precision: `src_bf16` [B,E,D] bf16 in PLAN order (what the edge MLP of that precision
 * writes), fp32 sums in edge order, fp32 out [B,N,D].  D = 128 or 256. */
int bsms_segment_sum_bf16(const bsms_plan_t* plan, const void* src_bf16, int64_t B, int64_t D, float* out,
                          bsms_stream_t stream);

/* ---------------------------------------------------------------- A2+A6: cal_ew -------------
 * WeightedEdgeConv.cal_ew (ops/basic.py:142-167) incl. degree() (utils/basic.py:287-309):
 * ec[e] = (w[i]/deg[i]) / (sum_{e'->j} w[i']/deg[i'] + 1e-12), aggr_w[n] = that sum + 1e-12.
 * `w` [N], `ec` [E] in edge order, `aggr_w` [N]. */
int bsms_cal_ew(const bsms_plan_t* plan, const float* w, float* ec, float* aggr_w,
                bsms_stream_t stream);

/* ---------------------------------------------------------------- A5/A7/A8: transitions -----
 * WeightedEdgeConv.forward (ops/basic.py:107-140), optionally fused with the pooling gather
 * h[:, m_ids] (ops/BSMS.py:79-89) or with Unpool (ops/basic.py:176-201):
 *   aggregating=1, pooled=0: out[b,j,:] = sum_{e->j} ew[e]*x[b,i_e,:]          x,out [B,N,D]
 *   aggregating=1, pooled=1: only kept rows j = ids[k] ("restrict")       x [B,N,D], out [B,Nk,D]
 *   aggregating=0, pooled=0: out[b,i,:] = sum_{e: i_e=i} ew[e]*x[b,j_e,:]      x,out [B,N,D]
 *   aggregating=0, pooled=1: x is the coarse tensor [B,Nk,D], zero-filled unpooling is implied
 *                            ("prolong"): out[b,i,:] = sum_{e: i_e=i, j_e kept} ew[e]*x[b,inv[j_e],:]
 * Any D >= 1 (also used for positions, D = pos_dim).  `ew` [E] in edge order.  The backward of a
 * call w.r.t. x is the same entry with `aggregating` flipped (exact adjoint), same `pooled`. */
int bsms_edge_conv(const bsms_plan_t* plan, const float* x, int64_t B, int64_t D,
                   const float* ew, int aggregating, int pooled, float* out, bsms_stream_t stream);
/* standalone Unpool / pooling gather with a DEVICE int64 index (ops/basic.py:194-199, BSMS.py:79-83) */
int bsms_scatter_rows(const float* h, int64_t B, int64_t Nk, int64_t D, const int64_t* idx_dev,
                      int64_t N, float* out /* [B,N,D], zero-filled here */, bsms_stream_t stream);
int bsms_gather_rows(const float* x, int64_t B, int64_t N, int64_t D, const int64_t* idx_dev,
                     int64_t Nk, float* out /* [B,Nk,D] */, bsms_stream_t stream);

/* ---------------------------------------------------------------- A3: MLP -------------------
 * MLP.forward (ops/basic.py:6-23) over R rows: x [R,in_dim] -> y [R,out_dim].  Used for the
 * encoder (in_dim = out_dim_model+1, LN) and decoder (out_dim = C, no LN) of
 * models/model.py:20-22.  `saved` = NULL selects INFERENCE (nothing is kept for a backward; `work`
 * must then be non-NULL).  Supported shapes: (in_dim <= 8 or in_dim == D) and
 * (out_dim == D with layer_norm, or out_dim <= 8 without).  `saved` keeps the activations the backward
 * needs.  bsms_mlp_bwd: grad_x = NULL skips the input gradient (the encoder's input is data); a non-null grad_x gets it for
 * every supported shape, the narrow first Linear (in_dim <= 8) included -- a caller differentiating w.r.t. node_in.
 * FROZEN MLP (bsms_mlp_bwd / bsms_mlp_bwd_ex): `grads` = NULL, or all of its 2*(hidden+1) entries NULL, forms no
 * weight gradient -- only the backward chain (which then stores no layer gradient) and grad_x; no side lane is used or marked.
 * Some entries NULL and some not: BSMS_E_INVALID_ARG, checked on the host before any launch.  `grads` = NULL with grad_x = NULL
 * does nothing and returns BSMS_OK.  grad_x is bit-identical to the call with every gradient. */
size_t bsms_mlp_saved_bytes(int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden);
size_t bsms_mlp_work_bytes(int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden);
int bsms_mlp_fwd(const float* x, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden,
                 int layer_norm, const float* const* params, float* y, void* saved, void* work,
                 bsms_stream_t stream);
int bsms_mlp_bwd(const float* x, const float* grad_y, int64_t R, int64_t in_dim, int64_t D,
                 int64_t out_dim, int hidden, int layer_norm, const float* const* params,
                 const void* saved, void* work, float* grad_x /* nullable */,
                 float* const* grads, bsms_stream_t stream);
/* bsms_mlp_fwd with `flags`.  BSMS_MLP_REUSE_PACKS, inference (saved = NULL): the weight packs written into `work` by
 * the previous bsms_mlp_fwd / _ex call with the same shape and the same parameter VALUES are still there (a private
 * `work` buffer of an autoregressive caller: utils/rollout_utils.py:49-62 applies the same encoder / decoder every
 * step) -- the prepack launches are skipped.  Training (saved != NULL): the packs and the cleared bound slots are in `saved`
 * already, written by a pack group (bsms_pack_group_launch below) since the parameters last changed. */
enum { BSMS_MLP_REUSE_PACKS = 1 };
int bsms_mlp_fwd_ex(const float* x, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden,
                    int layer_norm, const float* const* params, float* y, void* saved, void* work,
                    int flags, bsms_stream_t stream);

/* ---------------------------------------------------------------- pack groups ---------------
 * Every forward entry re-lays its weights out for the matrix cores ("prepack") with one small launch per MLP / GMP block: 13 per
 * training step of the airfoil model, each a latency chain of 23-27 us.  The weights change once per step (at the optimizer), so a
 * training loop can pack ALL of them with one launch per step instead: build a group once, from the same arguments the forward
 * calls take, launch it once per step after the optimizer's update, and pass BSMS_MLP_REUSE_PACKS / `reuse` bit 0 to the
 * forwards.  Every pack, header and cleared bound slot is byte for byte what the forward's own prepack writes.
 *   create / add_*: host only, no device call.  add_mlp takes the arguments of bsms_mlp_fwd that decide its packs, add_bsgmp
 *     those of bsms_bsgmp_fwd_p (below); `saved` != NULL: the training layout (packs in `saved`), NULL: the inference layout
 *     (packs in `work`).  Checked as the forwards check them (BSMS_E_INVALID_ARG: a null group, table, plan or parameter,
 *     neither `saved` nor `work`; BSMS_E_UNSUPPORTED: width, hidden, pos_dim, MLP shape, precision; BSMS_E_SHAPE: sizes that do
 *     not fit); a refused call adds nothing.
 *   launch: the first one uploads the tables (a blocking copy: BSMS_E_INVALID_ARG on a capturing stream) and SEALS the group --
 *     a later add_* is BSMS_E_INVALID_ARG; when a parameter or buffer pointer, a shape or the precision changes, destroy the
 *     group and build a new one.  Later launches are one kernel on `stream` and may be captured into a graph (keep the group
 *     alive as long as the graph).  An empty group launches nothing.
 *   destroy: waits for the device; NULL is allowed. */
typedef struct bsms_pack_group bsms_pack_group_t;
int bsms_pack_group_create(bsms_pack_group_t** out);
void bsms_pack_group_destroy(bsms_pack_group_t* group);
int bsms_pack_group_add_mlp(bsms_pack_group_t* group, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int hidden,
                            int layer_norm, const float* const* params, void* saved, void* work);
int bsms_pack_group_add_bsgmp(bsms_pack_group_t* group, const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p,
                              int hidden, const float* const* params, void* saved, void* work, int precision);
int bsms_pack_group_launch(bsms_pack_group_t* group, bsms_stream_t stream);

/* ---------------------------------------------------------------- A4: GMP block -------------
 * GMP.forward (ops/basic.py:48-98) incl. both MLPs, the gathers, the fiber [pos_i-pos_j, |.|]
 * and the aggregation: out = mlp_node([x, scatter_sum(mlp_edge([fiber, x_i, x_j]), j)]) + x.
 * x,out [B,N,D]; pos [B,N,p] (pos_batch_stride = N*p) or [N,p] (pos_batch_stride = 0, the
 * `repeat` branch ops/basic.py:87-88); 1 <= p <= 7.  `params`: 2*(hidden+1) pointers of mlp_node
 * followed by 2*(hidden+1) of mlp_edge (state_dict order of a GMP module).  bsms_gmp_bwd gives no gradient w.r.t. pos (the
 * reference's training loop never asks for one); bsms_gmp_bwd_pos below does.  `saved` = NULL in
 * bsms_gmp_fwd selects INFERENCE (rollout, utils/rollout_utils.py:14-64): no activation is written for a backward, the
 * messages live in `work`.
 * FROZEN MLPs (bsms_gmp_bwd / bsms_gmp_bwd_pos): the 2*(hidden+1) `grads` entries of mlp_node, and those of
 * mlp_edge, may be NULL -- all of an MLP's entries or none; `grads` = NULL freezes both.  Nothing that only serves a frozen MLP's
 * weight gradients is launched (its split-K jobs, the fiber / bias sums of the first edge Linear, the two projection jobs), a
 * side lane with nothing to run is not used, and the backward chains do not store the layer gradients that only those launches
 * read (D = 128 / 256: the no-store build of the edge kernel).  grad_x, grad_pos and the other MLP's gradients are bit-identical
 * to the call with every entry.  A partly null MLP: BSMS_E_INVALID_ARG, on the host, before any launch.  fp32 only. */
size_t bsms_gmp_saved_bytes(int64_t B, int64_t N, int64_t E, int64_t D, int hidden);
size_t bsms_gmp_work_bytes(int64_t B, int64_t N, int64_t E, int64_t D, int hidden);
int bsms_gmp_fwd(const bsms_plan_t* plan, const float* x, const float* pos, int64_t B, int64_t D,
                 int64_t p, int64_t pos_batch_stride, int hidden, const float* const* params,
                 float* out, void* saved, void* work, bsms_stream_t stream);
int bsms_gmp_bwd(const bsms_plan_t* plan, const float* x, const float* pos, const float* grad_out,
                 int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                 const float* const* params, const void* saved, void* work, float* grad_x,
                 float* const* grads, bsms_stream_t stream);
/* bsms_gmp_bwd + the gradient w.r.t. the node positions (pos is an ordinary autograd input of the reference's GMP.forward,
 * ops/basic.py:77-85: shape sensitivity, mesh adaptation).  `grad_pos` has the layout of `pos` -- [B,N,p], or [N,p] summed over
 * the batch when pos_batch_stride = 0 -- and is OVERWRITTEN; `pos_work` is scratch of bsms_gmp_pos_work_bytes(B, E, p) bytes.
 * grad_pos = NULL: exactly bsms_gmp_bwd (same launches).  Returns BSMS_E_INVALID_ARG for p outside 1..7 and for a non-null
 * grad_pos with a null pos_work (checked before anything else, no GPU needed).  Cost: one more read of the first edge
 * gradient [B,E,D] + 2 x 16 or 32 bytes per edge; deterministic.
 * bsms_gmp_pos_work_bytes returns 0 for B < 0, E < 0 or p outside 1..7. */
size_t bsms_gmp_pos_work_bytes(int64_t B, int64_t E, int64_t p);
int bsms_gmp_bwd_pos(const bsms_plan_t* plan, const float* x, const float* pos, const float* grad_out,
                     int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                     const float* const* params, const void* saved, void* work, float* grad_x,
                     float* const* grads, float* grad_pos, void* pos_work, bsms_stream_t stream);

/* ---------------------------------------------------------------- A9: BSGMP (whole U-Net) ---
 * BSGMP.forward (ops/BSMS.py:39-104) in one call: down blocks + restrict, bottom block, prolong + up blocks + skip
 * connections.  `plans`: L+1 HOST pointers, levels 0..L; levels < L have their pool attached (bsms_plan_set_pool with
 * m_ids[l]) and plans[l]->Nk == nodes of level l+1.  `ew`: L HOST pointers to the DEVICE edge weights of levels 0..L-1
 * (cal_ew chain, BSMS.py:64,73,89 -- mesh-static, the caller caches them).  h,out [B,N_0,D]; pos [B,N_0,p]
 * (pos_batch_stride = N_0*p) or [N_0,p] (0).  `params`/`grads`: HOST arrays of (2L+1) x 4 (hidden+1) device
 * pointers, blocks in the order down_gmps[0..L-1], bottom_gmp, up_gmps[0..L-1] (up_gmps[i] acts on level L-1-i,
 * BSMS.py:96-101), each block laid out as for bsms_gmp_fwd.  `saved` = NULL selects inference.
 * FROZEN MLPs (every bsms_bsgmp_bwd* entry): per block as for bsms_gmp_bwd -- the node MLP's and the edge MLP's
 * `grads` entries all there or all NULL; `grads` = NULL freezes the whole U-Net (a data-only backward: grad_h, grad_pos).  Every
 * block's entries are checked on the host before the first launch: a partly null MLP is BSMS_E_INVALID_ARG, null entries with a
 * bf16 precision are BSMS_E_UNSUPPORTED unless `flags` has BSMS_BWD_FROZEN_BF16 (below).  grad_h, grad_pos and the remaining gradients are bit-identical to the call with every
 * entry.  A block whose two MLPs are frozen runs no side lane: under BSMS_BWD_DEFER_JOIN it marks nothing, and its
 * `block_done_events` entry (bsms_bsgmp_bwd_ev) is recorded on the CALLER's stream -- it orders the block itself, not the weight
 * gradients of earlier blocks or of a deferred bsms_mlp_bwd_ex; wait for the entry of a block that has weight gradients, or for
 * bsms_side_lanes_join. */
size_t bsms_bsgmp_saved_bytes(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden);
size_t bsms_bsgmp_work_bytes(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden);
/* `work` size for callers that only ever run INFERENCE forwards (saved == NULL; rollout_utils.py:14-64) with this buffer:
 * the forward's part of the layout without the backward's per-block scratch sets (airfoil batch 8: 1.4 GB against 4.7 GB).
 * A buffer of bsms_bsgmp_work_bytes serves inference calls too. */
size_t bsms_bsgmp_infer_work_bytes(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden);
int bsms_bsgmp_fwd(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                   int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                   const float* const* params, float* out, void* saved, void* work, bsms_stream_t stream);
/* As bsms_bsgmp_fwd, with `reuse` for INFERENCE calls (saved == NULL) that pass the same `work` buffer as their previous
 * call and let nothing else write to it: bit 0 = the weights are unchanged (skip the weight prepacks), bit 1 = pos and
 * the mesh are unchanged (skip the coarse positions).  The autoregressive rollout (utils/rollout_utils.py:49-62: fixed
 * weights, fixed mesh_pos) sets both from its second step on.
 * TRAINING calls (saved != NULL) take bit 0 only: the packs of every block and its cleared bound slots are in `saved` already,
 * written by a pack group (bsms_pack_group_launch) since the weights last changed and ahead of this call in stream order.  No
 * prepack is launched and the engine's pack lane is neither forked nor joined.  Bit 1 is ignored in training. */
int bsms_bsgmp_fwd_ex(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                      int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                      const float* const* params, float* out, void* saved, void* work, int reuse, bsms_stream_t stream);
/* The U-Net with a choice of precision (see bsms_precision): sizes, forward (+ reuse flags) and backward. */
size_t bsms_bsgmp_saved_bytes_p(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden, int precision);
int bsms_bsgmp_fwd_p(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                     int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden, const float* const* params,
                     float* out, void* saved, void* work, int reuse, int precision, bsms_stream_t stream);
int bsms_bsgmp_bwd_p(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                     const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                     const float* const* params, const void* saved, void* work, float* grad_h, float* const* grads,
                     int precision, bsms_stream_t stream);
int bsms_bsgmp_bwd(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                   const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                   const float* const* params, const void* saved, void* work, float* grad_h,
                   float* const* grads, bsms_stream_t stream);
/* bsms_bsgmp_bwd_p with `flags`.  BSMS_BWD_DEFER_JOIN: the weight gradients of the last blocks may still be running on
 * the engine's internal side streams when the call returns; `grad_h` is complete in stream order.  The caller may enqueue
 * work that touches neither `work` nor `grads` (the fused training step runs the encoder's backward there, with its own
 * scratch) and MUST call bsms_side_lanes_join(stream) before anything reads `grads`, reuses `work`, or the step ends. */
enum { BSMS_BWD_DEFER_JOIN = 1 };
/* ACTIVATION RECOMPUTATION: a forward / backward pair that keeps only the INPUT of every block between the two
 * calls, for long unrolled losses whose K steps each hold a `saved`.
 *   BSMS_FWD_LEAN, a bit of bsms_bsgmp_fwd_p's `reuse`: `saved` (non-null, else BSMS_E_INVALID_ARG) has the LEAN layout -- the
 *     inputs of the blocks on levels 1..L, the positions of levels 1..L and the inputs of the L up blocks, fp32 in every precision;
 *     bsms_bsgmp_saved_bytes_ex(.., BSMS_BWD_RECOMPUTE) bytes.  The blocks run as in inference, with their packs in the pack area of
 *     `work`; bits 0 / 1 of `reuse` keep their inference meaning for those packs (bit 1 is ignored).  `out` is bit-identical to the
 *     full forward's.
 *   BSMS_BWD_RECOMPUTE, a bit of `flags` of bsms_bsgmp_bwd_ex / _ev / _pos_ev: `saved` is the lean one of such a forward, `work`
 *     has bsms_bsgmp_work_bytes_ex(.., BSMS_BWD_RECOMPUTE) bytes.  In front of every block's backward its training forward runs again
 *     on `stream` (prepack included) from the stored input into one of two blobs at the end of `work`; block n of the backward uses
 *     blob n & 1 and first waits for the weight-gradient lanes of block n - 2, which read that blob.  Every gradient is bit-identical
 *     to the unflagged pair's; the price is one more U-Net forward.  `saved` is only read: any number of backwards may follow one
 *     forward.  `work` may be shared by any number of (forward, backward) pairs on one stream.  Under BSMS_BWD_DEFER_JOIN the blobs
 *     belong to the lanes until bsms_side_lanes_join, like the rest of `work`.
 * The `_ex` size queries take the backward's `flags`: 0 gives bsms_bsgmp_saved_bytes_p / bsms_bsgmp_work_bytes, bit for bit; unknown
 * bits or a bad shape give 0.  Unknown bits in `reuse` or `flags` of a call, and BSMS_BWD_RECOMPUTE without `saved`, are
 * BSMS_E_INVALID_ARG, checked before anything else.  The one-block bsms_gmp_* entries have no such mode. */
enum { BSMS_FWD_LEAN = 4 };
enum { BSMS_BWD_RECOMPUTE = 2 };
/* FROZEN MLPs IN THE bf16 PRECISIONS: a bit of `flags` of bsms_bsgmp_bwd_ex / _ev / _pos_ev.  With it, NULL `grads`
 * entries (frozen MLPs, as above) are accepted under BSMS_BF16 / BSMS_BF16_NODES for D = 128 / 256: a frozen edge MLP takes the
 * data-only edge backward, which forms no weight gradient on chip.  grad_h, grad_pos and the remaining gradients are bit-identical to
 * the call with every entry.  Without the bit such a call stays BSMS_E_UNSUPPORTED; in fp32 and with every entry there the bit
 * changes nothing.  The `_ex` size queries accept it and return the sizes they return without it. */
enum { BSMS_BWD_FROZEN_BF16 = 32 };
size_t bsms_bsgmp_saved_bytes_ex(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden, int precision,
                                 int flags);
size_t bsms_bsgmp_work_bytes_ex(const bsms_plan_t* const* plans, int L, int64_t B, int64_t D, int64_t p, int hidden, int precision,
                                int flags);
int bsms_bsgmp_bwd_ex(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                      const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                      const float* const* params, const void* saved, void* work, float* grad_h, float* const* grads,
                      int precision, int flags, bsms_stream_t stream);
/* bsms_bsgmp_bwd_ex with a hand-off for data-parallel callers that all-reduce their gradients in buckets WHILE the backward is
 * still running (the reference never got there: trainer/trainer.py:15-18 wraps nn.DataParallel and
 * train.py:16 disables it).  `block_done_events`: nullable HOST array of 2L+1 hipEvent_t (entries may be NULL), indexed by the
 * position of a block in the backward's EXECUTION order -- up_gmps[L-1] .. up_gmps[0] (levels 0 .. L-1), bottom_gmp,
 * down_gmps[L-1] .. down_gmps[0].  Event e is recorded on an internal side stream at the point where every weight gradient
 * of blocks 0..e -- and of a bsms_mlp_bwd_ex(BSMS_BWD_DEFER_JOIN) issued before this call -- has been written to `grads`:
 * a communication stream that waits for it may read those slots.  The events are the caller's (created without timing). */
int bsms_bsgmp_bwd_ev(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                      const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                      const float* const* params, const void* saved, void* work, float* grad_h, float* const* grads,
                      int precision, int flags, void* const* block_done_events, bsms_stream_t stream);
/* bsms_bsgmp_bwd_p + the gradient w.r.t. the level-0 positions `pos`, through every block and through the pooling of the
 * positions (pos_{l+1} = restrict_l(pos_l), BSMS.py:75,85-88; its adjoint is bsms_edge_conv with aggregating = 0):
 *   gpos_l = gpos(up block on l) + restrict_l^T(gpos_{l+1}) + gpos(down block l),  accumulated as the backward passes level l.
 * `grad_pos` has the layout of `pos` ([B,N_0,p], or [N_0,p] when pos_batch_stride = 0) and is OVERWRITTEN; `pos_work` is
 * scratch of bsms_bsgmp_pos_work_bytes(plans, L, B, p) bytes (edge scratch + the coarse levels' accumulators).  Any precision;
 * with the bf16 ones the block gradients are read from the bf16 edge gradients.  grad_pos = NULL: exactly bsms_bsgmp_bwd_p.
 * Same argument checks as bsms_gmp_bwd_pos; the size query returns 0 for null plans, B < 0 or p outside 1..7. */
size_t bsms_bsgmp_pos_work_bytes(const bsms_plan_t* const* plans, int L, int64_t B, int64_t p);
int bsms_bsgmp_bwd_pos(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                       const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                       const float* const* params, const void* saved, void* work, float* grad_h, float* const* grads,
                       int precision, float* grad_pos, void* pos_work, bsms_stream_t stream);
/* bsms_bsgmp_bwd_ev + the position gradient of bsms_bsgmp_bwd_pos in ONE call: `flags`, `block_done_events`, `grad_pos` and
 * `pos_work` together, each with the meaning it has in the entry it comes from.  grad_pos = NULL is exactly bsms_bsgmp_bwd_ev
 * (pos_work is ignored); flags = 0 with block_done_events = NULL is exactly bsms_bsgmp_bwd_pos.  With grad_pos: p in 1..7 and a
 * non-null pos_work, else BSMS_E_INVALID_ARG, before anything else is looked at.
 * The position kernels of a block run on the caller's stream before a later block reuses the scratch set, also under
 * BSMS_BWD_DEFER_JOIN: a block's position kernel and the adjoint of the position pooling are queued on `stream` inside the
 * block, behind its gradient strand; only the weight gradients go to the side lanes, and the deferred join leaves nothing but
 * those outstanding.  So `grad_pos` -- like `grad_h` -- is complete in stream order when the call returns, and `pos_work` may be
 * reused by the next call on the same stream without bsms_side_lanes_join in between. */
int bsms_bsgmp_bwd_pos_ev(const bsms_plan_t* const* plans, const float* const* ew, int L, const float* h, const float* pos,
                          const float* grad_out, int64_t B, int64_t D, int64_t p, int64_t pos_batch_stride, int hidden,
                          const float* const* params, const void* saved, void* work, float* grad_h, float* const* grads,
                          int precision, int flags, void* const* block_done_events, float* grad_pos /* nullable */,
                          void* pos_work /* nullable with grad_pos */, bsms_stream_t stream);
int bsms_side_lanes_join(bsms_stream_t stream);
/* Do two streams overlap?  HIP places its streams on a few hardware queues (four by default, by reference counts at creation time) and
 * two streams on one queue run in order, whatever their flags.  Returns 1 if work queued on `b` can overtake work queued on `a`, 0 if not
 * (or a == b), < 0 on error.  Probes with ~250 us of device fills on `a` and a small one on `b` over a temporary 64 MB allocation:
 * synchronises, not for the data path or graph capture.  The engine uses it for its own side streams; the host loader uses it to pick a
 * copy stream that really runs beside the compute stream (graph.py: _to_device_async; no counterpart in the reference, whose loader
 * copies on the compute stream, src/datasets/base.py via trainer/trainer.py:52-56). */
int bsms_streams_overlap(bsms_stream_t a, bsms_stream_t b);
/* bsms_mlp_bwd with `flags`.  BSMS_BWD_DEFER_JOIN: `grad_x` is complete in stream order when the call returns, the weight
 * gradients run on an internal side stream; same contract as above (`work`, `grads`, bsms_side_lanes_join). */
int bsms_mlp_bwd_ex(const float* x, const float* grad_y, int64_t R, int64_t in_dim, int64_t D, int64_t out_dim, int H,
                    int layer_norm, const float* const* params, const void* saved, void* work, float* grad_x,
                    float* const* grads, int flags, bsms_stream_t stream);


/* ---------------------------------------------------------------- A10-A12: model glue + loss -
 * BSMS_Simulator._forward (models/model.py:127-164) around encode / process / decode, the Normalizer arithmetic
 * (utils/normalizer.py:40-52,80-90: fp64, cast to fp32) and the masked RMSE (trainer/trainer.py:96-97), fused:
 *   bsms_sim_prologue  node_in [R, C+p+1] = [state(C) | mesh_pos(p) | node_type]  ->  norm_in [R, C+1] = normalised
 *                      [state | node_type] (model.py:43-46,153), pos [R,p] contiguous (model.py:62)
 *   bsms_sim_epilogue  norm_pred [R,C] (decoder output) -> pred = state + float(double(norm_pred) * std + mean) * mask
 *                      (model.py:160-163).  Optional: `sums` (device float[2]) <- (sum se*mask, sum mask) of the loss
 *                      against `target`; `next_in` [R, C+p+1] <- the next autoregressive input
 *                      where(mask == 0, ic, cat[pred, mesh_pos | type]) (utils/rollout_utils.py:57-62; may alias node_in).
 *   bsms_sim_loss_bwd  loss = sqrt(S / M / C) from `sums` (device; under data parallelism the caller all-reduces them
 *                      first, so the loss is the exact global one) and d loss / d norm_pred.
 * `mean`, `meansq`, `std_eps` are the DEVICE fp64 fields _E_data, _E_data_squared, std_eps of the reference's
 * Normalizer (state_dict layout); std = max(nan_to_num(sqrt(meansq - mean^2)), std_eps).  mask is [R] (the [B,N,1]
 * tensor of the reference, flat).  C <= 8.  Nothing here synchronises or reads device memory on the host. */
size_t bsms_sim_work_bytes(int64_t R);
int bsms_sim_prologue(const float* node_in, int64_t R, int64_t C, int64_t p, const double* mean, const double* meansq,
                      const double* std_eps, float* norm_in, float* pos, bsms_stream_t stream);
int bsms_sim_epilogue(const float* norm_pred, const float* node_in, const float* mask, const float* target /* nullable */,
                      int64_t R, int64_t C, int64_t p, const double* mean, const double* meansq, const double* std_eps,
                      float* pred, float* next_in /* nullable */, const float* ic /* nullable */, float* sums /* nullable */,
                      void* work, bsms_stream_t stream);
int bsms_sim_loss_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C, const double* mean,
                      const double* meansq, const double* std_eps, const float* sums, float* loss_out /* nullable */,
                      float* grad_norm_pred, bsms_stream_t stream);
/* One step k of an UNROLLED loss over K autoregressive steps (step.py), backward: bsms_sim_loss_bwd with the step weight `w`
 * and the gradient carried back from step k+1, whose input was in_{k+1} = where(mask == 0, in_0, cat[pred_k, mesh_pos | type])
 * (the rollout rule, utils/rollout_utils.py:57-62).  One launch per step, in the order k = K-1 .. 0:
 *   loss_k        = sqrt(S_k / M_k / C) from `sums` (written to loss_out, nullable; NOT weighted)
 *   g_pred_k      = w * ((pred_k - tar_k) * mask * coef_k) + carry_k          coef_k = 1 / (loss_k M_k C) as bsms_sim_loss_bwd forms it
 *   carry_k       = mask != 0 ? g_pred_next + float(double(g_norm_in_next[:, c]) / std_in[c]) : 0         (c < C)
 *   grad_norm_pred = float(double(g_pred_k * mask) * std_out)
 * `g_pred_next` [R,C] is the g_pred this entry wrote for step k+1, `g_norm_in_next` [R,C+1] the input gradient of step k+1's
 * encoder backward (bsms_mlp_bwd's grad_x; its node-type column is not used).  The pair is given together or not at all: both
 * NULL for the last step and for a detached ("pushforward") chain -- then, with w = 1, the result is bit for bit that of
 * bsms_sim_loss_bwd.  The identity term of pred = state + delta * mask acts on every row; the carry stops it on rows with
 * mask == 0, which took in_0.  `g_pred` (nullable: nobody carries further) must not alias g_pred_next.  mean / meansq / std_eps are
 * the TARGET normaliser's fields, in_* the INPUT normaliser's (needed with a carried pair only).  R >= 1 and C in 1..8
 * (BSMS_E_UNSUPPORTED otherwise), null pointers give BSMS_E_INVALID_ARG, all before any device call; the call allocates
 * nothing, does not synchronise and reads nothing back.  No atomics. */
int bsms_sim_unroll_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C, const double* mean,
                        const double* meansq, const double* std_eps, const double* in_mean /* nullable */,
                        const double* in_meansq /* nullable */, const double* in_std_eps /* nullable */, const float* sums, float w,
                        const float* g_pred_next /* nullable */, const float* g_norm_in_next /* nullable */,
                        float* loss_out /* nullable */, float* g_pred /* nullable */, float* grad_norm_pred, bsms_stream_t stream);
/* bsms_sim_unroll_bwd for a FAMILY of masked objectives: the same step weight, the same carried pair, the same
 * way out through the de-normalisation, with the loss chosen by `space`, `kind` and per-channel weights.  With d = fl32(pred - tar),
 * m = mask and std_c the TARGET normaliser's std (formed from mean / meansq / std_eps as everywhere in this section):
 *   sums            = [ M | SE[0..C) ]  DEVICE double, M = sum m, SE[c] = sum m d_c^2 -- the first 1 + C fields of a row of
 *                     bsms_error_sums (under data parallelism the caller all-reduces them first: the loss is the exact global one)
 *   a_c             = w_c (BSMS_LOSS_PHYSICAL)  or  w_c / std_c^2 (BSMS_LOSS_NORMALIZED); w = `channel_weights`, DEVICE double[C],
 *                     NULL = all ones.  fp64.
 *   Q               = sum_c a_c SE[c] / (M C)                                              (fp64)
 *   loss            = Q (BSMS_LOSS_MSE)  or  sqrt(Q) (BSMS_LOSS_RMSE), written to loss_out (nullable; fp32, NOT weighted by `w`)
 *   chan_out[c]     = a_c SE[c] / (M C)   (nullable float[C]: the per-channel terms of Q)
 *   g_pred_k        = w * (d * m * fl32(G a_c)) + carry_k,   G = 2 / (M C) (mse)  or  1 / (loss M C) (rmse), G a_c formed in fp64
 *   grad_norm_pred  = float(double(g_pred_k * mask) * std_c)
 * carry_k, g_pred_next, g_norm_in_next, g_pred and the rule that the pair is given together or not at all are those of
 * bsms_sim_unroll_bwd, as are in_mean / in_meansq / in_std_eps.  BSMS_LOSS_PHYSICAL + BSMS_LOSS_RMSE + unit weights is the loss of
 * bsms_sim_loss_bwd, from fp64 sums instead of an fp32 pair (equal to fp32 round-off, not bit for bit).  M == 0, and loss == 0
 * under rmse, are not guarded, as there: the non-finite coefficient shows in the outputs.
 * One launch, thread r owns row r and recomputes the C coefficients from `sums`; no atomics, no allocation, no synchronisation,
 * nothing read back: the call can be captured into a HIP graph.  R >= 1 and C in 1..8, then space and kind in {0, 1}
 * (BSMS_E_UNSUPPORTED otherwise, checked in this order before any pointer is looked at); null required pointers and half a
 * carried pair give BSMS_E_INVALID_ARG; all before any device call. */
enum { BSMS_LOSS_PHYSICAL = 0, BSMS_LOSS_NORMALIZED = 1 };   /* space */
enum { BSMS_LOSS_RMSE = 0, BSMS_LOSS_MSE = 1 };              /* kind */
int bsms_sim_objective_bwd(const float* pred, const float* target, const float* mask, int64_t R, int64_t C, const double* mean,
                           const double* meansq, const double* std_eps, const double* in_mean /* nullable */,
                           const double* in_meansq /* nullable */, const double* in_std_eps /* nullable */, const double* sums,
                           const double* channel_weights /* nullable */, int space, int kind, float w,
                           const float* g_pred_next /* nullable */, const float* g_norm_in_next /* nullable */,
                           float* loss_out /* nullable */, float* chan_out /* nullable */, float* g_pred /* nullable */,
                           float* grad_norm_pred, bsms_stream_t stream);
/* bsms_sim_objective_bwd for a NODE-WEIGHTED objective: every row carries a weight omega >= 0 (the measure its
 * node represents, or any other importance) and mu = m * omega takes the mask's place in the LOSS -- not in the carry and not on the
 * way out, which keep m: the mask also gates pred = state + delta * mask and the rollout rule, the weight does not.
 *   row_weights     DEVICE float, `weight_period` entries; row r reads row_weights[r % weight_period].  weight_period must divide R:
 *                   R gives a weight per row, N shares one mesh's weights between the B = R / N samples of a batch.
 *   sums            = [ M | SE[0..C) ] with M = sum mu, SE[c] = sum mu d_c^2: the leading fields of a row of bsms_error_sums_w
 *   a_c, Q, loss, chan_out, G    as bsms_sim_objective_bwd forms them, from the weighted sums
 *   g_pred_k        = w * ((d * fl32(m * omega)) * fl32(G a_c)) + carry_k
 *   grad_norm_pred  = float(double(g_pred_k * mask) * std_c)
 * ORDER of the fp32 operations: mu = m * omega first (one rounding; exact for a 0/1 mask), then d * mu, then * fl32(G a_c), then
 * * w, then + carry.  With omega == 1 mu IS m and every later operation is bsms_sim_objective_bwd's: unit weights reproduce that
 * entry bit for bit.  omega -> 2^k omega scales the sums, and so 1 / G, by 2^k exactly: loss_out, chan_out, g_pred and
 * grad_norm_pred keep their bits (short of overflow and of subnormals).
 * Everything else -- the carried pair, in_*, the unguarded M == 0 -- is that entry's, and so is the order of the checks: R >= 1 and C
 * in 1..8, then space and kind (BSMS_E_UNSUPPORTED, before any pointer is looked at); then null required pointers, `row_weights`
 * among them, then a weight_period that is < 1 or does not divide R, then half a carried pair (BSMS_E_INVALID_ARG); all before
 * any device call.  One launch; no atomics, no allocation, no synchronisation, nothing read back: capturable. */
int bsms_sim_objective_bwd_w(const float* pred, const float* target, const float* mask, const float* row_weights,
                             int64_t weight_period, int64_t R, int64_t C, const double* mean, const double* meansq,
                             const double* std_eps, const double* in_mean /* nullable */, const double* in_meansq /* nullable */,
                             const double* in_std_eps /* nullable */, const double* sums, const double* channel_weights /* nullable */,
                             int space, int kind, float w, const float* g_pred_next /* nullable */,
                             const float* g_norm_in_next /* nullable */, float* loss_out /* nullable */, float* chan_out /* nullable */,
                             float* g_pred /* nullable */, float* grad_norm_pred, bsms_stream_t stream);
/* bsms_sim_objective_bwd_w for the ROBUST objectives: masked MAE and Huber losses, which are linear in their
 * per-channel sums.  With d = fl32(pred - tar), mu = m (row_weights == NULL) or m * omega, s_c = 1 (BSMS_LOSS_PHYSICAL) or the TARGET
 * normaliser's std_c (BSMS_LOSS_NORMALIZED), u_c = double(d_c) / s_c and delta (DEVICE double[C], > 0, in the units of the space;
 * read with BSMS_ROBUST_HUBER only):
 *   rho(u)          = |u| (BSMS_ROBUST_MAE)   or   u^2 / 2 if |u| <= delta_c, else delta_c (|u| - delta_c / 2) (BSMS_ROBUST_HUBER)
 *   psi(u)          = sign(u), sign(0) = 0    or   clamp(u, -delta_c, delta_c)
 *   sums            = [ M | S[0..C) ]  DEVICE double, M = sum mu, S[c] = sum mu rho(u_c): the row bsms_robust_sums writes (all-reduced
 *                     first under data parallelism)
 *   loss            = sum_c w_c S[c] / (M C)  -> loss_out (fp32, NOT weighted by `w`; no square root);   chan_out[c] = w_c S[c] / (M C)
 *   g_pred_k        = w * ((fl32(psi(u_c)) * mu) * fl32(w_c / (M C s_c))) + carry_k
 *   grad_norm_pred  = float(double(g_pred_k * mask) * std_c)
 * `space` only chooses s_c: there is no 1 / std^2 on top.  ORDER of the fp32 operations: mu = m * omega (one rounding; skipped
 * without row_weights), then fl32(psi) * mu, then * fl32(w_c / (M C s_c)) -- the coefficient is formed in fp64 and rounded once --
 * then * w, then + carry.  With omega == 1 mu IS m: all-ones weights reproduce row_weights == NULL bit for bit.  omega -> 2^k omega
 * scales the sums by 2^k and the coefficient by 2^-k exactly: every output keeps its bits (short of overflow and of subnormals).
 * With row_weights == NULL weight_period is ignored.  The carry, the carried pair, in_*, the mask of the way out and the unguarded
 * M == 0 are bsms_sim_objective_bwd_w's, and so is the order of the checks: R >= 1 and C in 1..8, then space and rkind in {0, 1}
 * (BSMS_E_UNSUPPORTED, before any pointer is looked at); then null required pointers -- `delta` with BSMS_ROBUST_HUBER among
 * them --, then with row_weights a weight_period that is < 1 or does not divide R, then half a carried pair
 * (BSMS_E_INVALID_ARG); all before any device call.  One launch, thread r owns row r; no atomics, no allocation, no
 * synchronisation, nothing read back: capturable. */
enum { BSMS_ROBUST_MAE = 0, BSMS_ROBUST_HUBER = 1 };         /* rkind */
int bsms_sim_robust_bwd(const float* pred, const float* target, const float* mask, const float* row_weights /* nullable */,
                        int64_t weight_period, int64_t R, int64_t C, const double* mean, const double* meansq,
                        const double* std_eps, const double* in_mean /* nullable */, const double* in_meansq /* nullable */,
                        const double* in_std_eps /* nullable */, const double* sums, const double* channel_weights /* nullable */,
                        const double* delta /* nullable with BSMS_ROBUST_MAE */, int space, int rkind, float w,
                        const float* g_pred_next /* nullable */, const float* g_norm_in_next /* nullable */,
                        float* loss_out /* nullable */, float* chan_out /* nullable */, float* g_pred /* nullable */,
                        float* grad_norm_pred, bsms_stream_t stream);
/* The gradient of the K-step objective w.r.t. its INPUT, G = dJ / d in_0: one launch folds step k into
 * `grad_in` [R, C+p+1], which has the column layout of node_in = [state (C) | mesh_pos (p) | node_type].  in_0 reaches step k
 * through its positions and node type on every row, through its state on every row at k = 0, and at k > 0 through its state
 * on the rows with mask == 0 only (the rollout rule put in_0 there; the other rows took pred_{k-1}, and their gradient went
 * into the carry of bsms_sim_unroll_bwd).  With t[r,c] = float(double(g_norm_in[r,c]) / std_in[c]), c = 0..C, std_in formed from
 * in_mean / in_meansq / in_std_eps as everywhere in this section:
 *   state columns c < C:   first_step ? g_pred[r,c] + t[r,c]  :  (mask[r] == 0 ? t[r,c] : 0)
 *   position columns:      g_pos[r,:]
 *   type column:           t[r,C]
 *   grad_in = overwrite ? contribution : grad_in + contribution            (fp32)
 * `g_pred` [R,C] is what bsms_sim_unroll_bwd / bsms_sim_objective_bwd wrote for this step (read with first_step only: it is 0 on
 * rows with mask == 0, so the k = 0 line needs no row condition), `g_norm_in` [R,C+1] the grad_x of this step's encoder
 * backward, `g_pos` [R,p] the grad_pos of its U-Net backward.  Call it once per step in the order k = K-1 .. 0, with `overwrite`
 * on the first call (stale contents of grad_in, NaNs included, never reach the result) and `first_step` on the last; K = 1 is
 * one call with both.  Per element: one fp64 division rounded once to fp32, at most two fp32 additions.
 * One launch, thread r owns row r; no atomics, no allocation, no synchronisation, nothing read back: the call can be captured
 * into a HIP graph.  Checked in this order, all before any device call: R >= 1, C in 1..8 and p in 1..7 (BSMS_E_UNSUPPORTED
 * otherwise, before any pointer is looked at); then null required pointers -- a null g_pred with first_step is one of them --
 * give BSMS_E_INVALID_ARG. */
int bsms_sim_input_grad(const float* g_pred /* [R,C], required iff first_step */, const float* g_norm_in /* [R,C+1] */,
                        const float* g_pos /* [R,p] */, const float* mask /* [R] */, int64_t R, int64_t C, int64_t p,
                        const double* in_mean, const double* in_meansq, const double* in_std_eps,
                        int first_step /* k == 0 */, int overwrite /* the launch of k = K-1 */,
                        float* grad_in /* [R, C+p+1] */, bsms_stream_t stream);

/* ---------------------------------------------------------------- evaluation: masked error sums ---
 * The reductions behind the reference's evaluation figures -- `Trainer.get_error` (trainer/trainer.py:254-269: per-sample
 * target scale, mean and standard deviation of the masked absolute error) and the rollout driver's RMSEs (rollout.py:99-107)
 * -- which the reference takes on the host after copying prediction, target and mask there.  One call over S segments
 * (the samples of a batch, or the time steps of a rolled-out trajectory) of seg_rows rows each:
 *   sums[s, :] = [ M | SE[0..C) | AE[0..C) | TT[0..C) ]   (DEVICE double, row length 1 + 3C), over the rows r of segment s with
 *   d = fl32(pred - target) (ONE fp32 rounding, as the reference's subtraction) and m = mask:
 *     M = sum m    SE[c] = sum m * d_c^2    AE[c] = sum m * |d_c|    TT[c] = sum m * target_c^2    (products and sums in fp64)
 * Segment s reads pred + s * pred_stride * C, target + s * target_stride * C and mask + s * mask_stride: the strides count ROWS,
 * so a segment can be a column block of a wider tensor; a mask_stride of 0 shares one mask between all segments.  Rows inside
 * a segment are contiguous ([seg_rows, C] / [seg_rows]).
 * Limits: C in 1..8 (BSMS_E_UNSUPPORTED otherwise, checked before any pointer is looked at), seg_rows in 0..2^31-1, S >= 0
 * (at least 2^20 segments per call).  S == 0 returns BSMS_OK and touches nothing; seg_rows == 0 writes zeros; null pointers
 * with work to do give BSMS_E_INVALID_ARG.
 * The call allocates nothing, does not synchronise and reads nothing back: it can be captured into a HIP graph.  `work` holds
 * bsms_error_sums_work_bytes(S, seg_rows) bytes (non-decreasing in both arguments).
 * DETERMINISM: no atomics.  The rows of a segment are cut into pieces of 1024 rows counted from the segment's own first row,
 * each piece is reduced in a fixed tree, and a second kernel adds the pieces of a segment in index order -- a segment's sums
 * are bit-identical from run to run and do not depend on S, on the strides or on the other segments of the launch. */
size_t bsms_error_sums_work_bytes(int64_t S, int64_t seg_rows);
int bsms_error_sums(const float* pred, const float* target, const float* mask, int64_t S, int64_t seg_rows, int64_t C,
                    int64_t pred_stride, int64_t target_stride, int64_t mask_stride, double* sums, void* work,
                    bsms_stream_t stream);
/* bsms_error_sums with a weight per row: mu = double(mask) * double(omega) takes the mask's place in every sum,
 *     M = sum mu    SE[c] = sum mu * d_c^2    AE[c] = sum mu * |d_c|    TT[c] = sum mu * target_c^2
 * Segment s reads row_weights + s * weight_stride ([seg_rows] floats; weight_stride counts rows like mask_stride, 0 shares one weight
 * vector between all segments).  Everything else is bsms_error_sums': the one fp32 rounding of d, the pieces of 1024 rows and their
 * fixed trees, the finishing kernel, the limits, the checks and their order (a null row_weights with work to do is one of the null
 * pointers, a negative weight_stride one of the negative strides), `work` of bsms_error_sums_work_bytes(S, seg_rows) bytes; no
 * atomics, no allocation, no synchronisation, capturable.  The kernels are one template: with omega == 1 the sums are those of
 * bsms_error_sums bit for bit, with omega in {0, 1} those of bsms_error_sums under the mask m * omega.  The weights are not looked
 * at: negative or non-finite ones show in the sums. */
int bsms_error_sums_w(const float* pred, const float* target, const float* mask, const float* row_weights, int64_t S,
                      int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride, int64_t mask_stride,
                      int64_t weight_stride, double* sums, void* work, bsms_stream_t stream);
/* The sums of the ROBUST training objectives (rho, u_c, s_c, delta, mu as at bsms_sim_robust_bwd above): per segment
 *   sums + s * sums_stride = [ M | S[0..C) ],   M = sum mu,   S[c] = sum mu * rho(double(d_c) / s_c)      (products and sums in fp64)
 * with mu = double(m) (row_weights == NULL: the unweighted kernel) or double(m) * double(omega) as in bsms_error_sums_w -- all-ones
 * weights reproduce NULL bit for bit.  sums_stride >= 1 + C counts doubles; the fields of a row past 1 + C are NOT written (a caller
 * keeps rows of 1 + 3C there and sends them as one message).  mean / meansq / std_eps: the TARGET normaliser's, DEVICE double, read
 * with BSMS_LOSS_NORMALIZED only (nullable otherwise); delta: DEVICE double[C], read with BSMS_ROBUST_HUBER only.
 * The kernel IS bsms_error_sums_w's, with another policy for what a row adds: the one fp32 rounding of d, pieces of 1024 rows counted
 * from the segment's first row, per-thread rows in ascending order, the fixed shuffle tree, the four waves in order, the finishing
 * kernel -- so a segment's sums depend on its own rows only and are bit-identical from run to run, and with BSMS_LOSS_PHYSICAL +
 * BSMS_ROBUST_MAE S[c] is the AE[c] of bsms_error_sums(_w) on the same rows bit for bit (x / 1.0 is exact).  `work` holds
 * bsms_error_sums_work_bytes(S, seg_rows) bytes.  No atomics, no allocation, no synchronisation: capturable.
 * The loss sum_c w_c S[c] / (M C) is linear in the row, so bsms_accum_coef (below) with BSMS_ACCUM_SUMS_ROW, BSMS_LOSS_PHYSICAL and
 * BSMS_LOSS_MSE on these rows forms exactly the robust loss and its fold coefficients: the scaling by s_c is already inside S[c].
 * Checked in this order, all before any device call: C in 1..8, then space and rkind in {0, 1} (BSMS_E_UNSUPPORTED, before any pointer
 * is looked at); then the S / seg_rows / stride limits of bsms_error_sums_w and sums_stride >= 1 + C (BSMS_E_INVALID_ARG); S == 0
 * returns BSMS_OK; then null required pointers -- the statistics with BSMS_LOSS_NORMALIZED and delta with BSMS_ROBUST_HUBER among
 * them -- give BSMS_E_INVALID_ARG. */
int bsms_robust_sums(const float* pred, const float* target, const float* mask, const float* row_weights /* nullable */, int64_t S,
                     int64_t seg_rows, int64_t C, int64_t pred_stride, int64_t target_stride, int64_t mask_stride,
                     int64_t weight_stride, const double* mean /* nullable */, const double* meansq /* nullable */,
                     const double* std_eps /* nullable */, const double* delta /* nullable with BSMS_ROBUST_MAE */, int space,
                     int rkind, double* sums, int64_t sums_stride, void* work, bsms_stream_t stream);

/* ---------------------------------------------------------------- evaluation: edge-difference (discrete H1) sums ---
 * What bsms_error_sums is for the values of a field, these two entries are for its differences along the mesh edges (DESIGN.md
 * 4.21).  A segment is seg_rows consecutive rows of a field; its graph is the plan's rows [row0, row0 + seg_rows) with the directed
 * edges e = (i_e -> j_e) of the plan whose BOTH ends lie in that window (an edge with an end outside is skipped: not read, not
 * counted, in the sums and in both halves of the backward -- one mesh of a block-diagonal union is summed through the union's
 * plan).  A mesh edge listed in both directions counts twice.  With d = fl32(pred - target) (ONE fp32 rounding, as in
 * bsms_error_sums), t = target, m = mask, every product and sum in fp64:
 *   l2_e  = sum_k (double(pos[i_e,k]) - double(pos[j_e,k]))^2          mu_e = double(m[i_e]) * double(m[j_e])
 *   w_e   = 1 (BSMS_EDGE_DIFFERENCE: pos is not read and may be NULL, p is ignored)
 *         | 1 / l2_e (BSMS_EDGE_QUOTIENT; an edge with l2_e == 0 has mu_e = w_e = 0: it adds nothing to any field)
 *   sums[s, :] = [ ME | DE[0..C) | TE[0..C) ]   (DEVICE double, row length 1 + 2C)
 *     ME = sum_e mu_e     DE[c] = sum_e mu_e w_e (d[i_e,c] - d[j_e,c])^2     TE[c] = sum_e mu_e w_e (t[i_e,c] - t[j_e,c])^2
 * The data pointers address the segment's OWN first row (plan row n is local row n - row0): segment s reads pred + s * pred_stride
 * * C, target + s * target_stride * C, mask + s * mask_stride and pos + s * pos_stride * p; strides count rows, 0 shares one array
 * between all segments; rows inside a segment are contiguous ([seg_rows, C] / [seg_rows] / [seg_rows, p]).
 * bsms_edge_diff_bwd is the exact adjoint of sum_c k_c DE[c] with respect to pred, k = coef (DEVICE double [S, C]):
 *   grad[s, r, c] = fl32( 2 k_c * [ sum_{e: j_e = r} mu_e w_e (d[r,c] - d[i_e,c]) + sum_{e: i_e = r} mu_e w_e (d[r,c] - d[j_e,c]) ] )
 * stored (accumulate == 0) or added in fp32 to what grad holds (accumulate != 0); segment s writes grad + s * grad_stride * C,
 * grad_stride >= seg_rows rows.
 * Limits: C in 1..8, weighting 0 or 1, p in 1..3 with BSMS_EDGE_QUOTIENT (BSMS_E_UNSUPPORTED otherwise, all three checked before any
 * pointer is looked at); S >= 0, seg_rows in 0..2^31-1, row0 >= 0, no negative stride (BSMS_E_INVALID_ARG); S == 0 returns BSMS_OK
 * and touches nothing; then a null plan (BSMS_E_INVALID_ARG), row0 + seg_rows beyond the plan's rows (BSMS_E_SHAPE), null pointers
 * with work to do (BSMS_E_INVALID_ARG).  seg_rows == 0 writes rows of zeros (sums) and writes nothing (bwd).
 * The calls allocate nothing, do not synchronise and read nothing back: they can be captured into a HIP graph.  `work` holds
 * bsms_edge_diff_work_bytes(S, seg_rows) bytes (non-decreasing in both arguments).
 * DETERMINISM: no atomics.  Sums: row r owns its INCOMING edges and adds them one after the other in the plan's CSR order (the
 * caller's edge order); the rows are cut into pieces of 1024 counted from the segment's own first row, a piece is reduced with
 * per-thread rows in ascending order and a fixed tree, and a second kernel adds the pieces in index order -- a segment's row is
 * bit-identical from run to run, whatever S, the strides or its neighbours in the launch, and whether it is summed through its own
 * plan or as a window of a union.  Backward: one thread owns grad[s, r, :]; per element ONE fp64 accumulator, incoming edges in CSR
 * order first, then outgoing edges in transpose order, times 2 * coef[s, c] in fp64, ONE rounding to fp32. */
enum { BSMS_EDGE_DIFFERENCE = 0, BSMS_EDGE_QUOTIENT = 1 };   /* weighting */
size_t bsms_edge_diff_work_bytes(int64_t S, int64_t seg_rows);
int bsms_edge_diff_sums(const bsms_plan_t* plan, int64_t row0, int64_t seg_rows, const float* pred, const float* target,
                        const float* mask, const float* pos /* nullable with BSMS_EDGE_DIFFERENCE */, int64_t S, int64_t C, int64_t p,
                        int weighting, int64_t pred_stride, int64_t target_stride, int64_t mask_stride, int64_t pos_stride,
                        double* sums /* [S, 1 + 2C] */, void* work, bsms_stream_t stream);
int bsms_edge_diff_bwd(const bsms_plan_t* plan, int64_t row0, int64_t seg_rows, const float* pred, const float* target,
                       const float* mask, const float* pos /* nullable with BSMS_EDGE_DIFFERENCE */, int64_t S, int64_t C, int64_t p,
                       int weighting, int64_t pred_stride, int64_t target_stride, int64_t mask_stride, int64_t pos_stride,
                       const double* coef /* DEVICE [S, C] */, int accumulate, float* grad /* [S, seg_rows, C] */, int64_t grad_stride,
                       bsms_stream_t stream);

/* ---------------------------------------------------------------- batch assembly from resident trajectories ---
 * The level-0 node tensors of a batch (datasets/base.py:238-289, `proc_data`, plus the collate) built by ONE launch from
 * trajectories that live in HBM.  `samples` is a HOST table; sample s contributes n rows, rows of consecutive samples
 * are consecutive in the outputs (batch-global row r):
 *   node_in  [R, C+p+1] = [state_in(C) + noise | pos(p) | type(1)]
 *   node_tar [R, C]     = state_tar + g * noise,   g = fl32(1 - noise_gamma)   (1 - noise_gamma evaluated in fp64)
 *   node_mask[R]        = 1 if type equals one of the n_valid codes in `valid_types` (HOST), else 0
 *   noise_out[R, C]     = the noise that was added (nullable)
 * `noise_std` (HOST [C]) NULL: no noise, the state columns are copied bit for bit.  The table travels as a kernel argument,
 * 64 samples per launch (more samples: more launches, the row offset carried across); nothing is uploaded and nothing
 * synchronises.  Envelope: C in 1..8, p in 1..7, n_valid in 1..4 (BSMS_E_UNSUPPORTED otherwise), R < 2^32; null pointers
 * give BSMS_E_INVALID_ARG; n_samples == 0 returns BSMS_OK without a launch; all checked before any device call.
 *
 * NOISE CONTRACT (independent of launch shape and of the chunking).  For batch-global row r and channel c:
 *   (x0,x1,x2,x3) = Philox4x32-10( counter = (r, c / 4, draw_lo, draw_hi), key = (seed_lo, seed_hi) )
 *                   multipliers 0xD2511F53 (on counter word 0), 0xCD9E8D57 (on word 2); key increments 0x9E3779B9, 0xBB67AE85
 *   u_i = ((x_i >> 8) + 0.5) * 2^-24                                   (a real number in (0,1); see below)
 *   z0 = sqrt(-2 ln u0) cos(2 pi u1),  z1 = sqrt(-2 ln u0) sin(2 pi u1);  z2, z3 likewise from (u2, u3)
 *   noise(r,c) = fl32(noise_std[c]) * z[c % 4] in fp32, and exactly 0 where node_mask is 0
 *   node_in = fl32(state + noise),  node_tar = fl32(tar + fl32(g * noise))     (no fused multiply-add)
 * u_i has 25 significant bits when x_i >> 8 >= 2^23, so the kernel never rounds it: it forms w = min(u, 1 - u), which fp32
 * holds exactly, takes ln u as logf(w) or log1pf(-w) and the angle as fl32(fl32(2 pi) * w) with the sign of the sine
 * flipped in the upper half.  logf / log1pf / sqrtf / sincosf are the accurate library versions: z is within ~2.5e-6 of
 * the fp64 evaluation of the formulas above (|z| <= 5.9). */
typedef struct {
  const float *state_in, *state_tar, *pos, *type; /* DEVICE: [n,C], [n,C], [n,p], [n] */
  int64_t n;
} bsms_batch_sample;
int bsms_batch_assemble(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t p,
                        const float* noise_std /* HOST [C], nullable */, double noise_gamma,
                        const float* valid_types /* HOST */, int64_t n_valid, uint64_t seed, uint64_t draw, float* node_in,
                        float* node_tar, float* node_mask, float* noise_out /* nullable */, bsms_stream_t stream);
/* The LATER targets of an unrolled loss, from the same table: later [n_later, R, C] with
 *   later[j, r, :] = (state_tar + (j + 1) * n * C)[row of r inside its sample, :]        j = 0 .. n_later - 1
 * -- the resident state of a trajectory is [T, n, C], so the frames after `state_tar` follow it at a fixed stride; the CALLER
 * guarantees that n_later more frames exist behind every sample's state_tar.  Copied bit for bit, no noise.  One launch per 64
 * samples (the later frame is the grid's second axis), a block never straddles two samples.  n_later == 0 or n_samples == 0
 * returns BSMS_OK and touches nothing; C in 1..8 (BSMS_E_UNSUPPORTED), n_later <= 65535, null pointers give
 * BSMS_E_INVALID_ARG; all checked before any device call. */
int bsms_batch_targets(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t n_later, float* later,
                       bsms_stream_t stream);

/* ---------------------------------------------------------------- frame augmentation: rotated and reflected batches ---
 * bsms_batch_assemble with ONE RIGID TRANSFORM PER SAMPLE: `xf` is a HOST [n_samples, p, p] fp32 table (row-major), `vec_first`
 * a HOST [n_vec] int32 table with the first channel of every VECTOR GROUP, the p consecutive state channels [f, f+p).  For every
 * row of sample s, with Q = xf[s], a vector v = (v[0] .. v[p-1]) becomes
 *   y[a] = fl32( .. fl32( fl32(Q[a][0] * v[0]) + fl32(Q[a][1] * v[1]) ) .. )      b ascending, every product rounded, no FMA
 * -- applied to the position columns of node_in and, for every group, to those channels of state_in and of state_tar.  Scalar
 * channels, the node type and the mask are what bsms_batch_assemble writes.  The NOISE COMES AFTER THE TRANSFORM and is that
 * entry's in every respect (same Philox counter and key per batch-global row and channel, same noise_out, zero where the mask
 * is zero):  node_in = fl32(y_in + noise),  node_tar = fl32(y_tar + fl32(g * noise)).  noise_std NULL: the transformed columns
 * are exactly y and the others are bit copies.  The matrices are NOT checked for orthogonality: the kernel applies what it is
 * given (identity matrices reproduce bsms_batch_assemble up to the sign of a zero).
 * The matrices travel in the kernel-argument table (an entry is 88 B), 40 samples per launch; results do not depend on the
 * chunking, the row offset is carried across launches.  Nothing is uploaded and nothing synchronises.
 * Checked in this order, all before any device call:
 *   C in 1..8, p in 2..3, n_valid in 1..4, n_vec in 0..4          else BSMS_E_UNSUPPORTED
 *   n_samples >= 0                                                 else BSMS_E_INVALID_ARG
 *   vec_first non-null when n_vec > 0; every group inside [0, C); no two groups overlapping      else BSMS_E_INVALID_ARG
 *   n_samples == 0 returns BSMS_OK without a launch (nothing else is looked at)
 *   samples, xf, valid_types, node_in, node_tar, node_mask non-null       else BSMS_E_INVALID_ARG
 *   per sample: n in 0 .. 2^25 - 256 (BSMS_E_UNSUPPORTED), no null field where n > 0 (BSMS_E_INVALID_ARG). */
int bsms_batch_assemble_xf(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t p,
                           const float* xf /* HOST [n_samples,p,p] */, const int32_t* vec_first /* HOST [n_vec] */, int64_t n_vec,
                           const float* noise_std /* HOST [C], nullable */, double noise_gamma,
                           const float* valid_types /* HOST */, int64_t n_valid, uint64_t seed, uint64_t draw, float* node_in,
                           float* node_tar, float* node_mask, float* noise_out /* nullable */, bsms_stream_t stream);
/* The same transform on the rows of x [F, R, C] (DEVICE fp32): the later targets of an unrolled loss, predictions mapped back to
 * the data's frame, node_in itself (its position columns are one more group).  The first rows of EVERY frame are cut into
 * n_samples consecutive segments of rows[s] rows (HOST int64 table; a segment of 0 rows is legal anywhere) with one matrix each;
 * every vector group of every such row is replaced by Q v -- or by Q^T v when `transpose` is non-zero -- in the arithmetic and
 * order above; the other channels are copied.  Rows past the table (sum rows < R) are not touched.  out == x works in place: a
 * thread reads its row's groups completely before it writes; any other overlap of x and out is undefined.
 * One launch per 40 segments, the frame is the grid's second axis.  Checked in this order, all before any device call:
 *   C in 1..16 (node_in rows are C + p + 1 wide), p in 2..3, n_vec in 0..4, F <= 65535        else BSMS_E_UNSUPPORTED
 *   n_samples, F, R >= 0                                           else BSMS_E_INVALID_ARG
 *   vec_first / the groups as above, inside [0, C)                  else BSMS_E_INVALID_ARG
 *   n_samples == 0 or F == 0 returns BSMS_OK and touches nothing
 *   x, out, rows, xf non-null                                      else BSMS_E_INVALID_ARG
 *   per segment: rows[s] in 0 .. 2^25 - 256 (BSMS_E_UNSUPPORTED), running sum <= R (BSMS_E_INVALID_ARG). */
int bsms_rows_transform(const float* x, float* out, int64_t F, int64_t R, int64_t C, const int64_t* rows /* HOST [n_samples] */,
                        int64_t n_samples, int64_t p, const float* xf /* HOST [n_samples,p,p] */, int transpose,
                        const int32_t* vec_first /* HOST [n_vec] */, int64_t n_vec, bsms_stream_t stream);

/* ---------------------------------------------------------------- hierarchy builder (host) ---
 * BistrideMultiLayerGraph (graph_wrappers/bsms_graph_wrapper.py:8-154 + graph_wrapper.py:67-134): the
 * bi-stride multi-level hierarchy of a mesh, built natively on the HOST (no GPU needed, no SciPy/MKL).
 * Inputs are HOST pointers: coo int64 [2,E] (level-0 flat edges), pos [N,pos_dim] in fp64 (bsms_hierarchy_create) or
 * fp32 (bsms_hierarchy_create_f32).  The seed of a cluster is the node nearest its centroid
 * (bsms_graph_wrapper.py:118-124) and the reference evaluates that in the dtype of `pos_mesh` (datasets/base.py hands
 * it float32 mesh_pos): the two entries do the arithmetic in fp64 / fp32 respectively, in NumPy's evaluation order, so
 * the argmin -- hence m_ids -- is bit-exact for either dtype.  Level l has
 * level_nodes(l) nodes and level_edges(l) directed edges; copy_edges writes int64 [2,E_l] (level 0: the
 * caller's edges unchanged; coarser levels row-major with sorted columns), copy_ids writes the kept node
 * ids of level l (ascending, relative to level l; `m_ids[l]`), bit-exact w.r.t. the reference. */
typedef struct bsms_hierarchy bsms_hierarchy_t;
int bsms_hierarchy_create(const int64_t* coo_host, int64_t E, int64_t N, const double* pos_host,
                          int64_t pos_dim, int num_layers, bsms_hierarchy_t** out);
int bsms_hierarchy_create_f32(const int64_t* coo_host, int64_t E, int64_t N, const float* pos_host,
                              int64_t pos_dim, int num_layers, bsms_hierarchy_t** out);
int bsms_hierarchy_destroy(bsms_hierarchy_t* h);
int64_t bsms_hierarchy_level_nodes(const bsms_hierarchy_t* h, int level);
int64_t bsms_hierarchy_level_edges(const bsms_hierarchy_t* h, int level);
int bsms_hierarchy_copy_edges(const bsms_hierarchy_t* h, int level, int64_t* out);
int bsms_hierarchy_copy_ids(const bsms_hierarchy_t* h, int level, int64_t* out);

/* ---------------------------------------------------------------- optimizer step ------------
 * torch.nn.utils.clip_grad_norm_(params, max_grad_norm) + torch.optim.AdamW.step()
 * (trainer/trainer.py:150-152) fused over ONE flat fp32 array of all trainable parameters (the
 * data-parallel gradient buffer has the same layout).  `step` counts from 1 (bias correction);
 * max_grad_norm <= 0 disables clipping; grad_norm_out (device scalar, nullable) receives the
 * pre-clip global norm.  Decoupled weight decay and bias-corrected moments exactly as torch.optim.AdamW. */
size_t bsms_adamw_work_bytes(void);
int bsms_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                    float max_grad_norm, float* grad_norm_out, void* work, bsms_stream_t stream);
/* The general step: the same pass with parameter groups, an exponential moving average of the weights and a
 * non-finite guard.  bsms_adamw_step above is unchanged and stays the yardstick: with groups = ema = counters = NULL this entry
 * writes the same bits, and so does every group with lr_scale = 1 (against the old entry with that group's weight_decay) or
 * lr_scale = s (against the old entry with lr = the fp32 product lr * s).
 * GROUPS.  A table of segments of the flat array, each with a factor on the learning rate and its own weight decay.  The handle
 * owns one small device block, like a plan; bsms_optim_groups_create checks on the host, before any device call, that
 * 1 <= ngroups <= 4096 and that lr_scale / weight_decay are finite and >= 0 (BSMS_E_INVALID_ARG), that every count >= 1 and
 * that the groups are sorted by offset and tile [0, n) exactly -- no gap, no overlap, nothing short of or past n (BSMS_E_SHAPE);
 * *out is NULL after a refusal.  Offsets are arbitrary (no alignment is assumed).  Creation allocates and copies (blocking): it is
 * not for the data path.  A handle whose n differs from the call's is BSMS_E_SHAPE; with a handle the scalar weight_decay is
 * not read.  destroy(NULL) is BSMS_OK.
 * ARITHMETIC per element of group k: lr_k = lr * lr_scale_k (one fp32 product), then bsms_adamw_step's update with lr_k and
 * wd_k; then, if `ema`, ema = lerp(ema, p_new, 1 - ema_decay) as torch.lerp forms it in fp32: ema + (p_new - ema) * (1 - ema_decay)
 * when 1 - ema_decay < 0.5, p_new - (p_new - ema) * ema_decay otherwise (ema_decay = 0 copies the parameters and 1 keeps the
 * average, bit for bit).  ema_decay outside [0, 1] is BSMS_E_INVALID_ARG, also when ema is NULL.
 * GUARD (counters != NULL: device int64[2] {applied, skipped}).  The norm is always formed (`work` required, max_grad_norm may be
 * 0).  If it is not finite -- an inf or NaN gradient, or finite gradients whose sum of squares overflows fp32 -- no element of
 * params / exp_avg / exp_avg_sq / ema is written and counters[1] += 1; otherwise counters[0] += 1.  grad_norm_out receives the
 * norm either way.  The step number is the device's, t = counters[0] + 1 (bias corrections from t in fp64 on the device, rounded
 * once to fp32): `step` must be 0 (BSMS_E_INVALID_ARG otherwise).  The counters are updated once per call by a one-thread launch
 * behind the update.  Without counters: step >= 1 (BSMS_E_SHAPE), as bsms_adamw_step.
 * No atomics, no allocation, no synchronisation; every element is written by one thread (bit-identical from run to run); the
 * call captures into a HIP graph; elements past n are never touched; n == 0 launches nothing (and counts nothing).
 * `work`: bsms_optim_work_bytes() bytes, needed whenever a norm is (clipping, grad_norm_out or the guard). */
typedef struct bsms_optim_group { int64_t offset, count; float lr_scale, weight_decay; } bsms_optim_group_t;
typedef struct bsms_optim_groups bsms_optim_groups_t;
int bsms_optim_groups_create(const bsms_optim_group_t* host_groups, int ngroups, int64_t n, bsms_optim_groups_t** out);
int bsms_optim_groups_destroy(bsms_optim_groups_t* groups);
size_t bsms_optim_work_bytes(void);
int bsms_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const bsms_optim_groups_t* groups, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int64_t step, float max_grad_norm, float* ema, float ema_decay, int64_t* counters,
                    float* grad_norm_out, void* work, bsms_stream_t stream);
/* acc[i] = first ? g[i] : acc[i] + g[i] over a flat gradient buffer of n floats (first != 0 overwrites whatever acc held).
 * The weight-gradient kernels overwrite their slots, so every step of an unrolled loss writes a scratch buffer with the
 * layout of the real one and this entry folds it in; fp32 adds in a fixed order, one thread per element.  16-byte accesses
 * when both pointers are 16-byte aligned.  n == 0 returns BSMS_OK; n < 0 BSMS_E_SHAPE; null or identical pointers
 * BSMS_E_INVALID_ARG. */
int bsms_grad_accumulate(float* acc, const float* g, int64_t n, int first, bsms_stream_t stream);
/* Gradient accumulation over micro-batches: the coefficients of one fold, formed on the device from the sums the
 * step already has.  Micro-batch t (0-based) of a cycle, unroll step k < K; `sums` holds K entries `sums_stride` ELEMENTS apart:
 *   BSMS_ACCUM_SUMS_PAIR  float (S, M) of bsms_sim_epilogue:                 m = M, n = S
 *   BSMS_ACCUM_SUMS_ROW   double [M | SE[0..C) ...] of bsms_error_sums:      m = M, n = sum_c a_c SE[c] in channel order, a_c as
 *                         bsms_sim_objective_bwd forms it from `space`, `channel_weights` (nullable: ones) and the TARGET
 *                         normaliser's mean / meansq / std_eps (read with BSMS_LOSS_NORMALIZED only; the pair ignores all four)
 * (under data parallelism: after their all-reduce).  All fp64, no contraction:
 *   Q(m, n) = n / (m C),   loss(m, n) = Q (BSMS_LOSS_MSE) or sqrt(Q) (BSMS_LOSS_RMSE),   l = loss(m, n)
 *   running[k] = (Mc, Nc, Lc):  t == 0:  (m, n, l), whatever it held before (NaNs included)
 *                               t  > 0:  Mc = Mc' + m,  Nc = Nc' + n  (primes: the values read),  and
 *     BSMS_ACCUM_BATCH   Lc = loss(Mc, Nc);   mse:  a = Mc' / Mc,                 b = m / Mc
 *                                             rmse: a = (Lc' Mc') / (Lc Mc),      b = (l m) / (Lc Mc)
 *     BSMS_ACCUM_MEAN    Lc = (Lc' t + l) / (t + 1);   a = t / (t + 1),   b = 1 / (t + 1)
 *   loss_out[k] = fl32(Lc);   coef = (fl32(a), fl32(b)) of step k = 0, each rounded once;   t == 0 writes (0, 1).
 * After the call the gradient of Lc is  fl32(a) * (gradient of Lc') + fl32(b) * (gradient of l): what bsms_grad_fold forms.  m == 0,
 * and a zero loss under rmse, are not guarded: the non-finite coefficient shows.
 * One launch of one block; no atomics, no allocation, no synchronisation, nothing read back: the call can be captured into a HIP
 * graph.  Checked in this order, all before any device call: K in 1..4096, C in 1..8, t >= 0 (BSMS_E_UNSUPPORTED); layout, space,
 * kind and reduction in {0, 1} (BSMS_E_UNSUPPORTED); sums_stride >= 2 (pair) or 1 + C (row) (BSMS_E_SHAPE); null sums / running /
 * coef / loss_out, or a row with BSMS_LOSS_NORMALIZED and null statistics (BSMS_E_INVALID_ARG). */
enum { BSMS_ACCUM_SUMS_PAIR = 0, BSMS_ACCUM_SUMS_ROW = 1 };   /* layout */
enum { BSMS_ACCUM_BATCH = 0, BSMS_ACCUM_MEAN = 1 };           /* reduction */
int bsms_accum_coef(const void* sums, int layout, int64_t sums_stride, int64_t C, const double* mean /* nullable */,
                    const double* meansq /* nullable */, const double* std_eps /* nullable */,
                    const double* channel_weights /* nullable */, int space, int kind, int reduction, int64_t t, int64_t K,
                    double* running /* [K][3] */, float* coef /* [2] */, float* loss_out /* [K] */, bsms_stream_t stream);
/* acc[i] = fl32(fl32(a * acc[i]) + fl32(b * g[i])) over n floats, (a, b) = coef[0..1] read on the DEVICE (bsms_accum_coef's output):
 * three separately rounded fp32 operations per element, never fused, the same on the 16-byte path (both pointers 16-byte aligned)
 * and on the element path (anything else, and the tail), one thread per element: bit-identical from run to run.  The grid of
 * bsms_grad_accumulate.  Elements past n are never touched.  n == 0 returns BSMS_OK; n < 0 BSMS_E_SHAPE; null or identical
 * pointers (coef included) BSMS_E_INVALID_ARG; all before any device call.  No allocation, no synchronisation; can be captured. */
int bsms_grad_fold(float* acc, const float* g, int64_t n, const float* coef, bsms_stream_t stream);

/* ---------------------------------------------------------------- weight-gradient primitives ---
 * The batched weight gradient of D x D Linears, the launcher every MLP / GMP backward uses, as an entry of its own:
 *   job j:  dW[n * ldw + col0 + k] = sum_{r < R} G[r][n] * A[r][k]   (n, k < D),   db[n] = sum_{r < R} G[r][n]   (db nullable)
 * -- autograd's grad of nn.Linear.weight / .bias for y = A W^T + b with G = dL/dy (ops/basic.py:6-23); dW may be a column
 * block of a wider matrix (the first edge Linear: ldw = 2D + p + 1).  Outputs are OVERWRITTEN.  G [R, ldg] and A [R, lda] are
 * fp32, or bf16 when `bf16` != 0 (pitches in ELEMENTS, at least D, a multiple of 4 / 8 so that every row starts on 16 bytes).
 * Arithmetic, chosen per job (see "Arithmetic" at the top):
 *   bf16 != 0                     the stored bf16 values, one product, fp32 accumulation;
 *   g_bound and a_bound given     fp16 x 2 pieces, one power-of-two scale per operand TENSOR.  A bound slot is an array of
 *                                 bsms_wgrad_bound_width() floats (non-negative, 16-byte aligned); the operand's bound is
 *                                 max(slot) * mul and the caller guarantees bound >= max |value| (a larger value overflows fp16:
 *                                 the result is then inf / NaN).  An element within 2^-18 of the bound keeps 22 bits, below that
 *                                 one bit is lost per octave -- the envelope of the edge-level jobs;
 *   otherwise                     the range-free three-way bf16 split, six products: fp32-accurate over the whole fp32 range.
 * Jobs of the three kinds may be mixed; each kind is one launch + one reduction on `stream`, sharing `work`
 * (bsms_wgrad_work_bytes(D, njobs) bytes, 16-byte aligned).  `skip_mask` bit j: job j is not run and its outputs are not
 * touched (its pointers may be NULL), but its R still counts when the launch shape is chosen.
 * SPLIT-K CONTRACT: the rows of a job are cut into slabs whose length depends on D and on the row counts of ALL jobs of the
 * same kind in the call (skipped ones included); the slabs are summed in slab order by a second kernel, no atomics.  So
 * the result of a job is bit-identical from run to run for the same call (same D, same kinds, same R's), and may differ in
 * the last bits between calls that batch it with different jobs.  A job with R == 0 writes zeros.
 * Checked on the host before any launch: njobs in 0..20 (BSMS_E_INVALID_ARG; 0 returns BSMS_OK), D a multiple of 32 in
 * 32..256 (BSMS_E_UNSUPPORTED), null `jobs`, null or short `work` (BSMS_E_INVALID_ARG), R in 0..2^31-1 for every job and, for
 * the jobs that run, the pitches and col0 + D <= ldw (BSMS_E_SHAPE), null dW, null G / A with R > 0, pointers not aligned
 * for their 16-byte accesses (dW: 16 bytes when ldw and col0 are multiples of 4, else 4) and non-positive or non-finite
 * g_mul / a_mul of a bounded job (BSMS_E_INVALID_ARG). */
typedef struct {
  const void *G, *A;              /* DEVICE [R, ldg], [R, lda]: fp32, or bf16 when bf16 != 0 */
  float *dW, *db;                 /* DEVICE; db nullable */
  int64_t R;
  int ldg, lda, ldw, col0;
  int bf16;
  const float *g_bound, *a_bound; /* DEVICE, nullable: one bound slot each */
  float g_mul, a_mul;
} bsms_wgrad_job;
size_t bsms_wgrad_bound_width(void);
size_t bsms_wgrad_work_bytes(int64_t D, int njobs);   /* 0 outside the envelope */
int bsms_wgrad(const bsms_wgrad_job* jobs, int njobs, int64_t D, unsigned skip_mask, void* work, size_t work_bytes,
               bsms_stream_t stream);
/* The narrow side: out[s * os + f * of] = sum_{r < R} G[r][f] * S[r][s] for the s < S_cols <= 8 columns of a narrow matrix
 * S [R, S_ld] (S_ld = 0: S_cols) against G [R, D] (dense) -- the weight gradient of the encoder's first Linear (os = 1,
 * of = S_cols), of the decoder's last (os = D, of = 1) and of the fiber columns of the first edge Linear (os = 1,
 * of = 2D + p + 1, S_ld = 4 or 8).  `colsum` (nullable, [D]) receives sum_r G[r][:], `colsum_S` (nullable, [S_cols])
 * sum_r S[r][:].  fp32 fused multiply-adds: each of at most 512 workgroups sums a contiguous slab of rows in row order per
 * row lane, the partial blocks are added in a fixed order by a second kernel; no atomics, bit-identical from run to run.
 * A row pitch of S that is a multiple of 4 is read with 16-byte loads (S 16-byte aligned; columns past S_cols are read
 * and ignored).  `work`: bsms_small_wgrad_work_bytes(D) bytes.  Checked on the host before any launch: D as above and
 * S_cols in 1..8 (BSMS_E_UNSUPPORTED), R in 0..2^31-1, S_ld, os, of >= 1 (BSMS_E_SHAPE), null G / S / out / work, alignment,
 * short work (BSMS_E_INVALID_ARG).  R == 0 writes zeros. */
size_t bsms_small_wgrad_work_bytes(int64_t D);        /* 0 outside the envelope */
int bsms_small_wgrad(const float* G, const float* S, int64_t R, int64_t D, int S_cols, int S_ld, float* out, int64_t os,
                     int64_t of, float* colsum /* nullable */, float* colsum_S /* nullable */, void* work, size_t work_bytes,
                     bsms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_H */
