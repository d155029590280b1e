// The generic chain kernels at D = 160 (NB = 10) in a translation unit of their own: see chain.hip.
#define BSMS_CHAIN_NB 10
#include "chain.hip"
