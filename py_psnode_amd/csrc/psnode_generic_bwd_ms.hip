// K5 with multiple-shooting restarts -- the step that leaves grid point k > 0 with k % every == 0 started from the dataset row x_true[k]:
// its start adjoint and the x part of the restart head's VJP are dropped -- on the sub-step build's policy (sub-steps per grid interval,
// every n >= 1; a launch-time Butcher tableau; every activation kind): the BuildMs object of psnode_generic_bwd_impl.h.  A translation
// unit of its own, so that the kernels of the other eight K5 objects stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildMs; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_ms_kernel(const GBwd a, const ActPair act, const psnode_rk_tableau_f32 rk, const MsDev sub) {
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_ms_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
