// K0 with linearly interpolated external inputs: the sub-step build (SubDev, any n >= 1; a launch-time Butcher tableau, every activation
// kind) whose stages read z | v at theta = (j + c_s) / n between the interval's two grid points -- the BuildLin object of
// psnode_generic_impl.h.  A translation unit of its own, so that the kernels of the other five K0 objects stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildLin; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_lin_kernel(const IntegrateDev a, const ActPair act, const psnode_rk_tableau_f32 rk, const SubDev sub) {
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_lin_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_lin(const IntegrateDev& a, bool dae, const ActPair& act, const psnode_rk_tableau_f32& rk, const SubDev& sub,
                              hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act, rk, sub);
}

}  // namespace psnode
