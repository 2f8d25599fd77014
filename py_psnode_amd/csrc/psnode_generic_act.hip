// K0 with a launch-time hidden-layer activation (psnode_act.h): psnode_generic.hip compiled a second time, with PSNODE_K0_ACT_BUILD.
// A translation unit of its own, so that the ELU(1) kernels of psnode_generic.o stay exactly what they are.
#define PSNODE_K0_ACT_BUILD 1
#include "psnode_generic.hip"
