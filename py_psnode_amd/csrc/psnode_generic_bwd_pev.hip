// K5 with per-trajectory events on the sub-step build: the BuildPev object (psnode_generic_build.h).
#define PSNODE_BUILD BuildPev
#include "psnode_generic_bwd_impl.h"
