// K5, the ELU(1) object (psnode_generic_bwd_impl.h), and the exported host queries of every build.
#define PSNODE_BUILD BuildElu1
#include "psnode_generic_bwd_impl.h"

namespace psnode {

// shared by the ODE and DAE entry points (psnode_backward.hip calls this for kernel = generic / unsupported MFMA shapes)
size_t generic_bwd_workspace_floats(const psnode_mlp_f32* de, const psnode_mlp_f32* ae, long long B) {
    GBwd a;
    memset(&a, 0, sizeof(a));
    fill_gmlp(*de, a.de);
    if (ae) fill_gmlp(*ae, a.ae);
    Arena A;
    return gbwd_layout(*de, ae, B, a, A), A.floats();
}

size_t generic_bwd_msp_workspace_floats(const psnode_mlp_f32* de, const psnode_mlp_f32* ae, long long B, int n, int nzv, long long chunks) {
    GBwd a;
    memset(&a, 0, sizeof(a));
    fill_gmlp(*de, a.de);
    if (ae) fill_gmlp(*ae, a.ae);
    Arena A;
    return gbwd_msp_layout(*de, ae, B, n, nzv, (size_t)chunks, a, A), A.floats();
}

// (the pre fields, which this object's GBwd does not have, are written by a launch only: the fit reads none of them)
int generic_bwd_fits(const psnode_mlp_f32* de, const psnode_mlp_f32* ae, int xd, int zd, int vd, int id, bool pre, int lin) {
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
