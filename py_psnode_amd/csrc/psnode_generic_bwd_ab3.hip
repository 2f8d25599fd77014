// K5 with three-step Adams-Bashforth and its predictor-corrector restart step: the BuildAb3 object (psnode_generic_build.h).
#define PSNODE_BUILD BuildAb3
#include "psnode_generic_bwd_impl.h"
