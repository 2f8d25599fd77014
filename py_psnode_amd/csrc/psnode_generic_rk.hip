// K0 with a launch-time Butcher tableau (psnode_rk_tableau_f32: any explicit Runge-Kutta method of up to four stages) and every activation
// kind: the BuildRk object of psnode_generic_impl.h.  A translation unit of its own, so that the kernels of psnode_generic.o,
// psnode_generic_act.o and psnode_generic_pre.o stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildRk; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_rk_kernel(const IntegrateDev a, const ActPair act, const psnode_rk_tableau_f32 rk) {
    const SubDev sub{};      // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_rk_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_rk(const IntegrateDev& a, bool dae, const ActPair& act, const psnode_rk_tableau_f32& rk, hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act, rk);
}

}  // namespace psnode
