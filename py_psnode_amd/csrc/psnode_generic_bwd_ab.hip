// K5 for two-step Adams-Bashforth -- the DE's VJP of step k takes phi_k = c0_k g_{k+1} + c1_{k+1} g_{k+2} where Euler's takes h g_{k+1}; the
// sweep keeps the two adjoints -- on the per-trajectory build's policy (a launch-time tableau, here always the one-stage one; every
// activation kind; a per-column event index): the BuildAb object of psnode_generic_bwd_impl.h.  A translation unit of its own, so that the
// kernels of the other seven K5 objects stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildAb; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_ab_kernel(const GBwd a, const ActPair act, const psnode_rk_tableau_f32 rk, const AbDev sub) {
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_ab_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
