// The generic chain kernels at D = 192 (NB = 12) in a translation unit of their own: see chain.hip.
#define BSMS_CHAIN_NB 12
#include "chain.hip"
