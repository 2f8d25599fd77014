// K0 with two-step Adams-Bashforth on the per-trajectory build: the BuildAb object (psnode_generic_build.h).
#define PSNODE_BUILD BuildAb
#include "psnode_generic_impl.h"
