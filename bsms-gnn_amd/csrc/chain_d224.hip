// The generic chain kernels at D = 224 (NB = 14) in a translation unit of their own: see chain.hip.
#define BSMS_CHAIN_NB 14
#include "chain.hip"
