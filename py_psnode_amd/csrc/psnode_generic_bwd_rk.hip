// K5 with a launch-time Butcher tableau (psnode_rk_tableau_f32, up to four stages) and every activation kind: the BuildRk object (psnode_generic_build.h).
#define PSNODE_BUILD BuildRk
#include "psnode_generic_bwd_impl.h"
