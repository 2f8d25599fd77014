// K5 with linearly interpolated external inputs: the sub-step build (SubDev, any n >= 1; a launch-time Butcher tableau, every activation
// kind) whose stages read z | v at theta = (j + c_s) / n between the interval's two grid points and whose external adjoints go to both
// -- the BuildLin object of psnode_generic_bwd_impl.h.  A translation unit of its own, so that the kernels of the other five K5 objects
// stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildLin; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_lin_kernel(const GBwd a, const ActPair act, const psnode_rk_tableau_f32 rk, const SubDev sub) {
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_lin_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
