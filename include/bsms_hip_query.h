/* bsms_hip_query.h -- C ABI of libbsms_hip_query.so, a companion of libbsms_hip.so (bsms_hip.h) for tests and tools.
 *
 * The surface of libbsms_hip.so is closed (bsms_hip_ext.h says why); this library links against it and adds one host-only entry.
 *
 * bsms_chain_launch_query: WHICH kernel, in which shape, does a chain launch (every MLP behind bsms_mlp_* / bsms_gmp_* / bsms_bsgmp_*)
 * take?  It answers from the functions the launch path itself calls (csrc/chain_launch.h: plan_fwd / plan_bwd) and
 * launches nothing.
 *   D: latent width.  backward = 0: (mode_a, mode_b) = (in_mode, out_mode); backward = 1: (gin, first).  The numbers of csrc/chain.h:
 *     in_mode   0 rows [R,D]   1 rows [x, x2]   2 narrow input (encoder)   3 edge rows gathered through the plan
 *     out_mode  0 LayerNorm    1 plain          2 narrow output (decoder)  3 two plain heads
 *     gin       0 rows through the LayerNorm backward   1 the same gathered by edge target   2 narrow output gradient (decoder)
 *     first     0 no input gradient   1 one input-gradient head   2 two ([x, x2])
 *     built pairs, forward: (0,1) (0,3) (1,1) (3,0) (1,0) (2,0) (0,2) (0,0); backward: (0,2) (1,0) (0,0) (2,1) (0,1).
 *   key: what the choice reads from a launch's arguments.  nstage: Linears on the matrix cores; nseq: weight packs the loader
 *     streams (forward: nstage, + 1 with in_mode 1; backward: nstage + the input-gradient heads).  The pointer sets are given as
 *     0 none / 1 all / 2 some set: act_stores = the activation stores behind the input stage and Linears 0 .. nstage-2;
 *     gstores = the layer gradients entering stages 0 .. nstage-1.  glast: the last gradient is stored; masks: every stage has its
 *     saved activation; resid: a residual is added to y.  Forward reads resid / act_stores, backward glast / gstores / masks.
 *   cus: CU count to decide for; 0 = the current device's.  With cus != 0 the entry touches no device (works without a GPU).
 *   info: family 0 feature-split (k_fs_*), 1 pipelined edge kernels (k_edge_*), 2 ring kernels (k_chain_*); the variant flags; the
 *     launch numbers (a tile = 16 * rb * cw rows; threads = 64 (cw + nload); lds = dynamic LDS in bytes); name e.g. "edge_fwd rb2 save lone".
 * Returns BSMS_E_INVALID_ARG for a null pointer, R < 1, cus < 0 or counts out of range, BSMS_E_UNSUPPORTED for a width, a mode pair
 * or a bf16 combination that is not built (the launch's own refusals); the message is behind bsms_last_error() of libbsms_hip.so. */
#ifndef BSMS_HIP_QUERY_H
#define BSMS_HIP_QUERY_H
#include "bsms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int64_t R;
  int nstage, nseq, bf16, store_mode, timing;
  int resid, act_stores;          /* forward */
  int glast, gstores, masks;      /* backward */
} bsms_chain_launch_key;
typedef struct {
  int family, rb, save, store, lone, bf16, timing;
  int cw, nload, nring, ntiles;
  int64_t grid, threads, lds, lds_max;
  char name[48];
} bsms_chain_launch_info;
int bsms_chain_launch_query(int D, int backward, int mode_a, int mode_b, const bsms_chain_launch_key* key, int cus,
                            bsms_chain_launch_info* out);

#ifdef __cplusplus
}
#endif
#endif /* BSMS_HIP_QUERY_H */
