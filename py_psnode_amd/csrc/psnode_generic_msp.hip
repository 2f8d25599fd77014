// K0 with the multiple-shooting segments spread over workgroups: the BuildMsp object (psnode_generic_build.h).
#define PSNODE_BUILD BuildMsp
#include "psnode_generic_impl.h"
