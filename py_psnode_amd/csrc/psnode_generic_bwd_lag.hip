// K5 with four-point Lagrange interpolation of the externals on the linear-externals build: the BuildLag object (psnode_generic_build.h).
#define PSNODE_BUILD BuildLag
#include "psnode_generic_bwd_impl.h"
