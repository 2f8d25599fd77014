// K0 with all ten activation kinds, the pre-activation family (SiLU / GELU / GELU(tanh) / Mish) among them: the BuildPre object (psnode_generic_build.h).
#define PSNODE_BUILD BuildPre
#include "psnode_generic_impl.h"
