// K0 as two-step Adams-Bashforth -- x_{k+1} = x_k + c0 f_k + c1 f_{k-1}, one DE evaluation per step, an Euler restart at k = 0, at an event
// of the column and behind a zero step -- on the per-trajectory build's policy (a launch-time tableau, here always the one-stage one; every
// activation kind; a per-column event index): the BuildAb object of psnode_generic_impl.h.  A translation unit of its own, so that the
// kernels of the other seven K0 objects stay exactly what they are.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildAb; } }
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

template <bool DAE, int MODE, int ML, int QM = 4>
__global__ __launch_bounds__(NT) void generic_ab_kernel(const IntegrateDev a, const ActPair act, const psnode_rk_tableau_f32 rk, const AbDev sub) {
#include "psnode_generic_body.h"
}
template <> struct GenericKernels<Bd> {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_ab_kernel<DAE, MODE, ML, QM>; }
};

}  // namespace

hipError_t launch_generic_ab(const IntegrateDev& a, bool dae, const ActPair& act, const psnode_rk_tableau_f32& rk, const AbDev& ab,
                             hipStream_t stream) {
    return launch_generic_build<Bd>(a, dae, stream, act, rk, ab);
}

}  // namespace psnode
