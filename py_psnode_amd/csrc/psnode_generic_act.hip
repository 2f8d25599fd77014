// K0 with a launch-time hidden-layer activation (psnode_act.h, six kinds): the BuildAct object (psnode_generic_build.h).
#define PSNODE_BUILD BuildAct
#include "psnode_generic_impl.h"
