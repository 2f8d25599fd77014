// K0 with the pre-activation family as well (psnode_act.h: SiLU, GELU, GELU(tanh), Mish next to the six kinds of the act build):
// psnode_generic.hip compiled a third time, with PSNODE_K0_ACT_BUILD and PSNODE_K0_PRE_BUILD.  A translation unit of its own, so that the
// kernels of psnode_generic.o and psnode_generic_act.o stay exactly what they are.
#define PSNODE_K0_ACT_BUILD 1
#define PSNODE_K0_PRE_BUILD 1
#include "psnode_generic.hip"
