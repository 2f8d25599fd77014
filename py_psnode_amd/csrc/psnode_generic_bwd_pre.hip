// K5 with the pre-activation family as well (psnode_act.h): psnode_generic_bwd.hip compiled a third time, with PSNODE_K5_ACT_BUILD and
// PSNODE_K5_PRE_BUILD.  The forward recomputation also keeps each hidden layer's pre-activation u in LDS, and the VJP takes the derivative of
// SiLU / GELU / GELU(tanh) / Mish from it.  A translation unit of its own, so that the kernels of psnode_generic_bwd.o and
// psnode_generic_bwd_act.o stay exactly what they are.
#define PSNODE_K5_ACT_BUILD 1
#define PSNODE_K5_PRE_BUILD 1
#include "psnode_generic_bwd.hip"
