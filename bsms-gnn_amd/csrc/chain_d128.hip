// The chain kernels and their launchers at D = 128 (NB = 8): a translation unit of its own, compiled in parallel with the other widths.
#pragma clang fp contract(off)   // before the kernel headers: chain_dev.h says why
#include "chain_launch.h"

namespace bsms {
template int launch_chain_fwd_nb<8>(int, int, const ChainFwdArgs&, hipStream_t);
template int launch_chain_bwd_nb<8>(int, int, const ChainBwdArgs&, hipStream_t);
template int chain_launch_query_nb<8>(int, int, int, const ChainLaunchKey&, int, ChainLaunch*);
}  // namespace bsms

// experiments only (not in bsms_hip.h): what residency does the runtime compute for the D = 128 edge chains?
#ifdef BSMS_EXPERIMENTS
extern "C" int bsms_debug_occupancy(int* fwd_blocks_per_cu, int* bwd_blocks_per_cu) {
  hipError_t e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(fwd_blocks_per_cu, k_chain_fwd<8, IN_EDGE, OUT_LN>,
                                                                kChainThreads, Ring<8>::lds_bytes(3));
  hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(bwd_blocks_per_cu, k_chain_bwd<8, G_EDGE_LN, F_NONE>,
                                                                kChainThreads, Ring<8>::lds_bytes(3));
  return (e1 == hipSuccess && e2 == hipSuccess) ? 0 : -4;
}
#endif
