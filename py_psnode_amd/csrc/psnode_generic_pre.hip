// K0 with the pre-activation family as well (psnode_act.h: SiLU, GELU, GELU(tanh), Mish next to the six kinds of the act build): the
// BuildPre object of psnode_generic_impl.h.  A translation unit of its own, so that the kernels of psnode_generic.o and
// psnode_generic_act.o stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildPre; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_pre_act_kernel(const IntegrateDev a, const ActPair act) {
    const psnode_rk_tableau_f32 rk{};      // never read: the tableau code is under `if constexpr (Bd::rk)`
    const SubDev sub{};                    // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_pre_act_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_pre(const IntegrateDev& a, bool dae, const ActPair& act, hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act);
}

}  // namespace psnode
