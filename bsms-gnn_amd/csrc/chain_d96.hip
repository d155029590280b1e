// The generic chain kernels at D = 96 (NB = 6) in a translation unit of their own: see chain.hip.
#define BSMS_CHAIN_NB 6
#include "chain.hip"
