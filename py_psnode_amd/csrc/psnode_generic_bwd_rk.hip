// K5 with a launch-time Butcher tableau (psnode_rk_tableau_f32) and every activation kind: psnode_generic_bwd.hip compiled a fourth time, on
// top of the pre-activation build's macros (PSNODE_K5_ACT_BUILD, PSNODE_K5_PRE_BUILD), with PSNODE_K5_RK_BUILD.  A translation unit of its
// own, so that the kernels of psnode_generic_bwd.o, psnode_generic_bwd_act.o and psnode_generic_bwd_pre.o stay exactly what they are.
#define PSNODE_K5_ACT_BUILD 1
#define PSNODE_K5_PRE_BUILD 1
#define PSNODE_K5_RK_BUILD 1
#include "psnode_generic_bwd.hip"
