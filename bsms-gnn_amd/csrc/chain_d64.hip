// The chain kernels and their launchers at D = 64 (NB = 4): a translation unit of its own, compiled in parallel with the other widths.
#pragma clang fp contract(off)   // before the kernel headers: chain_dev.h says why
#include "chain_launch.h"

namespace bsms {
template int launch_chain_fwd_nb<4>(int, int, const ChainFwdArgs&, hipStream_t);
template int launch_chain_bwd_nb<4>(int, int, const ChainBwdArgs&, hipStream_t);
template int chain_launch_query_nb<4>(int, int, int, const ChainLaunchKey&, int, ChainLaunch*);
}  // namespace bsms
