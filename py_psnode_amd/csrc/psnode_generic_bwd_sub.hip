// K5 with sub-steps per grid interval on the tableau build: the BuildSub object (psnode_generic_build.h).
#define PSNODE_BUILD BuildSub
#include "psnode_generic_bwd_impl.h"
