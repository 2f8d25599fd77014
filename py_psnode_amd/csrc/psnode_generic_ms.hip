// K0 with multiple-shooting restarts -- grid point k > 0 with k % every == 0 starts its step from the dataset row, a DAE's DE reads the
// head at that row -- on the sub-step build's policy (sub-steps per grid interval, every n >= 1; a launch-time Butcher tableau; every
// activation kind): the BuildMs object of psnode_generic_impl.h.  A translation unit of its own, so that the kernels of the other eight K0
// objects stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildMs; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_ms_kernel(const IntegrateDev a, const ActPair act, const psnode_rk_tableau_f32 rk, const MsDev sub) {
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_ms_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_ms(const IntegrateDev& a, bool dae, const ActPair& act, const psnode_rk_tableau_f32& rk, const MsDev& ms,
                             hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act, rk, ms);
}

}  // namespace psnode
