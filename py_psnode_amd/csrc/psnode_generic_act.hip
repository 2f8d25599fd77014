// K0 with a launch-time hidden-layer activation (psnode_act.h, six kinds): the BuildAct object of psnode_generic_impl.h.  A translation
// unit of its own, so that the ELU(1) kernels of psnode_generic.o stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildAct; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_act_kernel(const IntegrateDev a, const ActPair act) {
    const psnode_rk_tableau_f32 rk{};      // never read: the tableau code is under `if constexpr (Bd::rk)`
    const SubDev sub{};                    // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_act_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_act(const IntegrateDev& a, bool dae, const ActPair& act, hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act);
}

}  // namespace psnode
