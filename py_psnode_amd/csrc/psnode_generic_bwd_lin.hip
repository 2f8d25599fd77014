// K5 with linearly interpolated externals on the sub-step build: the BuildLin object (psnode_generic_build.h).
#define PSNODE_BUILD BuildLin
#include "psnode_generic_bwd_impl.h"
