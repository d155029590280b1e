// The descriptor of one GMP block call, shared by gmp.hip (the block) and bsgmp.hip (the U-Net, which sequences blocks), and the
// entry points between the two.  Host code only: no kernel translation unit includes this header.
#pragma once
#include "host_orch.h"

namespace bsms {

// The shape of a block: every layout (carve_gmp_saved / carve_gmp_work), every pack table and every choice between two kernels is a
// function of these members -- so a size query and the call it serves cannot disagree.
struct GmpShape {
  int64_t B = 0, N = 0, E = 0, D = 0, p = 0;
  int H = 0;
  int precision = BSMS_F32;
  bool training = true;   // false: inference (`saved` == NULL at the ABI): only the messages, the aggregate and the forward packs exist

  // bf16 precisions: the edge activations and the messages are bf16 (half the floats; the sign bits keep their size) ...
  bool bf() const { return precision != BSMS_F32; }
  // ... and in BSMS_BF16_NODES the node MLP's saved activations likewise
  bool bfn() const { return precision == BSMS_BF16_NODES; }
  // The fused edge backward (efuse.hip; implies bf()): it recomputes the edge activations, so the layout keeps the two node
  // projections and the row images of the edge Linears instead of e_act and the transposed packs
  bool fused() const;
  // The edge forward with LDS-resident weights (efwd.hip): whenever no edge activation has to be saved, i.e. inference and the
  // training forward of the fused backward
  bool edge_fwd_resident() const;
  // every shape and precision requirement of a block, reported under the caller's name
  int check(const char* who) const;
};

// One call on a block: the shape, the level it acts on and its buffers.
struct GmpCall : GmpShape {
  const bsms_plan* plan = nullptr;
  const float* x = nullptr;               // [B, N, D] the block's input
  const float* pos = nullptr;             // [B, N, p], or [N, p] with pos_bstride == 0
  int64_t pos_bstride = 0;
  const float* const* params = nullptr;   // 4 (H + 1) pointers: mlp_node (W_l, b_l), then mlp_edge
  void* saved = nullptr;                  // the block's saved blob; null: inference
  void* work = nullptr;                   // one scratch set (bsms_gmp_work_bytes)
  void* packs_base = nullptr;             // inference only, nullable: the weight packs live there instead of behind the messages, so
                                          // that they can be filled ahead of the call and survive the scratch reuse of other blocks
  // the level and the buffers; `saved` decides between training and inference
  void bind(const bsms_plan* pl, void* saved_, void* work_, void* packs_) {
    plan = pl; N = pl ? pl->N : 0; E = pl ? pl->E : 0;
    saved = saved_; work = work_; packs_base = packs_; training = saved_ != nullptr;
  }
};

// `defer_slot` < 0: the side lanes are joined before returning (ABI semantics).  0/1: they are only MARKED in that slot;
// the caller joins later with side_wait_mark on both lanes and must not touch `work` or read `grads` before that.
// `grad_pos` (nullable): the position gradient, overwritten or -- `pos_accumulate` -- added to; `pos_work`: its edge scratch.
struct GmpBwdOpts {
  int defer_slot = -1;
  float* grad_pos = nullptr;
  void* pos_work = nullptr;
  bool pos_accumulate = false;
  bool frozen_bf16 = false;   // BSMS_BWD_FROZEN_BF16: null `grads` entries are accepted in the bf16 precisions
};

size_t gmp_pack_bytes(int64_t D, int hidden);   // inference packs of one block (upper bound)
size_t gmp_saved_bytes(const GmpShape& s);      // 0 outside the hidden range, like the ABI queries
// The block's prepack alone, for a forward that runs with `do_prepack` = false later in the same step
int gmp_prepack(const GmpCall& c, hipStream_t stream);
// One block's packs added to a pack group (`g` == null: the checks only, so that a caller can check every block before it adds the first)
int gmp_pack_group_add(PackGroup* g, const GmpCall& c);
// `resid2` (nullable): the skip connection added to the block's output (ops/BSMS.py:102)
int gmp_fwd_core(const GmpCall& c, float* out, const float* resid2, bool do_prepack, hipStream_t stream);
// The `grads` table of one block: 2 (H + 1) node-MLP entries, then 2 (H + 1) edge-MLP entries; each group
// all there or all null (the MLP is frozen), `grads` == NULL = both frozen.  BSMS_E_INVALID_ARG for a partly null group,
// BSMS_E_UNSUPPORTED for null entries in a bf16 precision unless `frozen_bf16` (BSMS_BWD_FROZEN_BF16).  A host check: nothing is launched.
int gmp_check_grads(float* const* grads, int hidden, int precision, const char* who, bool* node_live, bool* edge_live,
                    bool frozen_bf16 = false);
bool gmp_marks_chained();   // deferred-join mode: waiting for lane 1's mark of a slot is enough
int gmp_bwd_core(const GmpCall& c, const float* grad_out, float* grad_x, float* const* grads, const GmpBwdOpts& o, hipStream_t stream);

}  // namespace bsms
