// K5 with launch-time hidden-layer activations (psnode_act.h): the BuildAct object of psnode_generic_bwd_impl.h.  A translation unit of its
// own, so that the ELU(1) kernels of psnode_generic_bwd.o stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildAct; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_act_kernel(const GBwd a, const ActPair act) {
    const psnode_rk_tableau_f32 rk{};      // never read: the tableau code is under `if constexpr (Bd::rk)`
    const SubDev sub{};                    // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_act_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
