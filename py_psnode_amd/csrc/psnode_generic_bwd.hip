// K5, the ELU(1) object (psnode_generic_bwd_impl.h): generic_backward_kernel, its launcher, and the exported host queries of all four builds.
#include "psnode_generic_build.h"
namespace psnode { namespace { using Bd = BuildElu1; } }
#include "psnode_generic_bwd_impl.h"

namespace psnode {
namespace {

template <bool gg, bool REG, bool ggA = gg, int STR = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_kernel(const GBwd a) {
    const NoActPair act;                   // no activation argument: ActCtx is empty
    const psnode_rk_tableau_f32 rk{};      // never read: the tableau code is under `if constexpr (Bd::rk)`
    const SubDev sub{};                    // never read: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_bwd_body.h"
}
template <> struct GenericBwdKernels<Bd> {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_kernel<gg, REG, ggA, STR>; }
};

}  // namespace

template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

// shared by the ODE and DAE entry points (psnode_backward.hip calls this for kernel = generic / unsupported MFMA shapes)
size_t generic_bwd_workspace_floats(const psnode_mlp_f32* de, const psnode_mlp_f32* ae, long long B) {
    GBwd a;
    memset(&a, 0, sizeof(a));
    fill_gmlp(*de, a.de);
    if (ae) fill_gmlp(*ae, a.ae);
    Arena A;
    return gbwd_layout(*de, ae, B, a, A), A.floats();
}

// (the pre fields, which this object's GBwd does not have, are written by a launch only: the fit reads none of them)
int generic_bwd_fits(const psnode_mlp_f32* de, const psnode_mlp_f32* ae, int xd, int zd, int vd, int id, bool pre, bool lin) {
    GBwd a;
    memset(&a, 0, sizeof(a));
    a.dae = ae != nullptr; a.xd = xd; a.zd = zd; a.vd = vd; a.id = id;
    int rows = fill_gmlp(*de, a.de);
    a.maxw = mlp_maxw(*de);
    if (ae) {
        const int r2 = fill_gmlp(*ae, a.ae);
        rows = r2 > rows ? r2 : rows;
        a.maxw = mlp_maxw(*ae) > a.maxw ? mlp_maxw(*ae) : a.maxw;
    }
    a.act_rows = rows;
    a.de_reg = de_reg_class(*de) ? 1 : 0;
    return gbwd_mode(a, pre, lin);
}

}  // namespace psnode
