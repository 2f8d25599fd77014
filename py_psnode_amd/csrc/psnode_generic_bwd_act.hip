// K5 with launch-time hidden-layer activations (psnode_act.h): psnode_generic_bwd.hip compiled a second time, with PSNODE_K5_ACT_BUILD.
// A translation unit of its own, so that the ELU(1) kernels of psnode_generic_bwd.o stay exactly what they are.
#define PSNODE_K5_ACT_BUILD 1
#include "psnode_generic_bwd.hip"
