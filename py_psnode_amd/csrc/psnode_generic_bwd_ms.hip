// K5 with multiple-shooting restarts on the sub-step build: the BuildMs object (psnode_generic_build.h).
#define PSNODE_BUILD BuildMs
#include "psnode_generic_bwd_impl.h"
