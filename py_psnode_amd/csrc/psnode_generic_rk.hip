// K0 with a launch-time Butcher tableau (psnode_rk_tableau_f32: any explicit Runge-Kutta method of up to four stages) and every activation
// kind: psnode_generic.hip compiled a fourth time, on top of the pre-activation build's macros, with PSNODE_K0_RK_BUILD.  A translation unit
// of its own, so that the kernels of psnode_generic.o, psnode_generic_act.o and psnode_generic_pre.o stay exactly what they are.
#define PSNODE_K0_ACT_BUILD 1
#define PSNODE_K0_PRE_BUILD 1
#define PSNODE_K0_RK_BUILD 1
#include "psnode_generic.hip"
