// K5 with a launch-time Butcher tableau (psnode_rk_tableau_f32) and every activation kind: the BuildRk object of psnode_generic_bwd_impl.h.
// A translation unit of its own, so that the kernels of psnode_generic_bwd.o, psnode_generic_bwd_act.o and psnode_generic_bwd_pre.o stay
// exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildRk; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_rk_kernel(const GBwd a, const ActPair act, const psnode_rk_tableau_f32 rk) {
    const SubDev sub{};      // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_rk_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
