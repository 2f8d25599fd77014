// K5 with stage-wise algebraic heads on the linear-externals build (DAE instances only): the BuildLinSth object (psnode_generic_build.h).
#define PSNODE_BUILD BuildLinSth
#include "psnode_generic_bwd_impl.h"
