// K0 with stage-wise algebraic heads on the Lagrange-externals build (DAE instances only): the BuildLagSth object (psnode_generic_build.h).
#define PSNODE_BUILD BuildLagSth
#include "psnode_generic_impl.h"
