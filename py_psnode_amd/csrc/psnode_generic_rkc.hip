// K0 with one Runge-Kutta-Chebyshev step per grid interval on the sub-step build: the BuildRkc object (psnode_generic_build.h).
#define PSNODE_BUILD BuildRkc
#include "psnode_generic_impl.h"
