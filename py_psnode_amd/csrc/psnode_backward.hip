// C ABI of the backward passes (include/psnode_hip.h: psnode_ode_backward_*, psnode_dae_backward_*): argument validation and the
// dispatch among the backward kernel families --
//   K4x (psnode_backward_x.hip)          ODE, hidden 33..64 with saved rows, up to one wave per SIMD: one wave = 4 trajectories, no LDS (round 6)
//   K4f (psnode_backward_fused.hip)      ODE, in -> H -> H -> H -> x at hidden <= 128: one launch, saved-activation and recompute forms
//   K8f / K9 (psnode_latent_dpp.hip / psnode_latent64_bwd*.hip)   the latent integrators of the direct_encode models at hidden 16 / 64
//   K8 (psnode_latent_bwd.hip)           the latent DAE at hidden 16
//   K5 (psnode_generic_bwd_impl.h)       anything else that fits the LDS, with or without teacher forcing (its option families: psnode_generic_family.h)
// (the DAE's no_encode shapes go through psnode_dae_backward_wide_f32 -> K7f, psnode_dae_backward_fused.hip).
// Rounds 1-4 also carried K4 / K7, hidden-64 specialisations of the recompute form; K4f / K7f cover their shapes (round 5:
// profiles/scripts/variants/ keeps the sources).
#include <string.h>

#include <type_traits>

#include "psnode_generic_family.h"
#include "psnode_pack.h"

using namespace psnode;

namespace {
template <class Args>
bool method_ok(const Args* a) { return a && a->method >= PSNODE_EULER && a->method <= PSNODE_RK4_38; }
// the first three statuses of every backward entry point, in their order: NULL args, method, T / B
template <class Args>
int check_call(const Args* a) {
    if (!a) return PSNODE_ERR_NULL;
    if (!method_ok(a)) return PSNODE_ERR_METHOD;
    return a->T < 1 || a->B < 1 ? PSNODE_ERR_DIMS : PSNODE_OK;
}
bool mlp_ptrs_ok(const psnode_mlp_f32& m) {
    for (int l = 0; l < m.n_layers; ++l) if (!m.weight[l] || !m.bias[l]) return false;
    return true;
}
// the pointers every ODE / DAE backward kernel needs (PSNODE_ERR_NULL otherwise)
bool ptrs_ok(const psnode_ode_bwd_args_f32* a) {
    if (!mlp_ptrs_ok(a->de)) return false;
    if (!a->t.ptr || !a->all_initial || !a->xs || !a->grad_xs || !a->grad_x0 || !a->grad_all_initial || !a->grad_params) return false;
    if (a->z_dim > 0 && !a->z.ptr) return false;
    return !(a->event_idx && a->z_dim > 0 && !a->z_jump);
}
bool ptrs_ok(const psnode_dae_bwd_args_f32* a) {
    if (!mlp_ptrs_ok(a->de) || !mlp_ptrs_ok(a->ae)) return false;
    if (!a->t.ptr || !a->all_initial || !a->xs || !a->is || !a->grad_xs || !a->grad_x_init || !a->grad_all_initial || !a->grad_params_de ||
        !a->grad_params_ae)
        return false;
    if ((a->z_dim > 0 && !a->z.ptr) || (a->v_dim > 0 && !a->v.ptr)) return false;
    return !(a->event_idx && ((a->z_dim > 0 && !a->z_jump) || (a->v_dim > 0 && !a->v_jump)));
}

// ---- K5 (psnode_generic_bwd_impl.h): the recipe dims it takes, its call struct, the choice among its three builds
// pre: K5's builds that keep the pre-activations (their own LDS fit: psnode_generic_bwd_impl.h, pre_floats); lin: the linear-externals build's
bool ode_generic_ok(const psnode_ode_bwd_args_f32* a, bool pre = false, int lin = 0) {
    const psnode_mlp_f32& m = a->de;
    if (a->x_dim < 1 || a->z_dim < 0 || m.n_layers < 1 || m.n_layers > kMaxLayers) return false;
    if (m.in_dim != 3 * (a->x_dim + a->z_dim) || m.out_dim[m.n_layers - 1] != a->x_dim) return false;
    return generic_bwd_fits(&a->de, nullptr, a->x_dim, a->z_dim, 0, 0, pre, lin) != 0;
}
// (K5's mode for the shape, 0 = not taken: what psnode_dae_backward_supported returns)
int dae_generic_ok(const psnode_dae_bwd_args_f32* a, bool pre = false, int lin = 0) {
    if (a->x_dim < 1 || a->z_dim < 0 || a->v_dim < 0 || a->i_dim < 1) return 0;
    const int n = a->x_dim + a->z_dim + a->v_dim + a->i_dim;
    const psnode_mlp_f32 &d = a->de, &g = a->ae;
    if (d.n_layers < 1 || d.n_layers > kMaxLayers || g.n_layers < 1 || g.n_layers > kMaxLayers) return 0;
    if (d.in_dim != 3 * n || d.out_dim[d.n_layers - 1] != a->x_dim) return 0;
    if (g.in_dim != n + a->x_dim + a->z_dim + a->v_dim || g.out_dim[g.n_layers - 1] != a->i_dim) return 0;
    return generic_bwd_fits(&a->de, &a->ae, a->x_dim, a->z_dim, a->v_dim, a->i_dim, pre, lin);
}
GenericBwdCall generic_bwd_call(const psnode_ode_bwd_args_f32& a) {
    GenericBwdCall c{};
    c.method = a.method; c.xd = a.x_dim; c.zd = a.z_dim; c.T = a.T; c.B = a.B; c.de = &a.de;
    c.t = view(a.t); c.z = view(a.z); c.a0 = a.all_initial;
    c.ev = a.event_idx; c.n_events = a.n_events;
    bind_jumps(c, a);
    c.xs = a.xs; c.gxs = a.grad_xs; c.flags = a.flags;
    c.gx0 = a.grad_x0; c.gz = a.grad_z; c.gzj = a.grad_z_jump; c.ga0 = a.grad_all_initial; c.gparams_de = a.grad_params;
    return c;
}
GenericBwdCall generic_bwd_call(const psnode_dae_bwd_args_f32& a) {
    GenericBwdCall c{};
    c.method = a.method; c.xd = a.x_dim; c.zd = a.z_dim; c.vd = a.v_dim; c.id = a.i_dim; c.T = a.T; c.B = a.B; c.de = &a.de; c.ae = &a.ae;
    c.t = view(a.t); c.z = view(a.z); c.v = view(a.v); c.a0 = a.all_initial;
    c.ev = a.event_idx; c.n_events = a.n_events;
    bind_jumps(c, a);
    c.xs = a.xs; c.is_ = a.is; c.gxs = a.grad_xs; c.gis = a.grad_is;
    c.gx0 = a.grad_x_init; c.gz = a.grad_z; c.gv = a.grad_v; c.gzj = a.grad_z_jump; c.gvj = a.grad_v_jump; c.ga0 = a.grad_all_initial;
    c.gparams_de = a.grad_params_de; c.gparams_ae = a.grad_params_ae;
    return c;
}
// act: the activations of every build but kBuildElu1, which ignores them
int generic_backward(BuildId build, const GenericBwdCall& c, const ActPair* act, void* workspace, void* stream) {
    float* ws = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (build) {
        case kBuildElu1: return generic_backward_launch<BuildElu1>(c, act, ws, s);
        case kBuildAct: return generic_backward_launch<BuildAct>(c, act, ws, s);
        case kBuildPre: return generic_backward_launch<BuildPre>(c, act, ws, s);
        case kBuildRk: return generic_backward_launch<BuildRk>(c, act, ws, s);
        case kBuildSub: return generic_backward_launch<BuildSub>(c, act, ws, s);
        case kBuildLin: return generic_backward_launch<BuildLin>(c, act, ws, s);
        case kBuildPev: return generic_backward_launch<BuildPev>(c, act, ws, s);
        case kBuildAb: return generic_backward_launch<BuildAb>(c, act, ws, s);
        case kBuildMs: return generic_backward_launch<BuildMs>(c, act, ws, s);
        case kBuildMsp: return generic_backward_launch<BuildMsp>(c, act, ws, s);
        case kBuildAb3: return generic_backward_launch<BuildAb3>(c, act, ws, s);
        case kBuildLag: return generic_backward_launch<BuildLag>(c, act, ws, s);
        case kBuildRkc: return generic_backward_launch<BuildRkc>(c, act, ws, s);
        case kBuildLinSth: return generic_backward_launch<BuildLinSth>(c, act, ws, s);
        case kBuildLagSth: return generic_backward_launch<BuildLagSth>(c, act, ws, s);
    }
    return PSNODE_ERR_UNSUPPORTED;      // (no such build)
}
// K4f: every width <= 128 (z_dim up to 8), saved-activation and recompute forms
bool use_fused_bwd(const psnode_ode_bwd_args_f32* a) { return a->kernel != PSNODE_KERNEL_GENERIC && fused_bwd_shape_ok(a); }
// K8 needs 16-byte aligned rows; with pointers not yet known (dims-only queries) the shape decides
bool use_latent_bwd(const psnode_ode_bwd_args_f32* a) {
    return a->kernel != PSNODE_KERNEL_GENERIC && latent_bwd_shape_ok(a) && (!a->xs || latent_bwd_ptrs_ok(a));
}
bool use_latent64_bwd(const psnode_ode_bwd_args_f32* a) {   // K9: the only fused backward for this shape (K5's LDS budget is too small)
    return a->kernel != PSNODE_KERNEL_GENERIC && latent64_ode_bwd_shape_ok(a) && (!a->xs || latent64_ode_bwd_ptrs_ok(a));
}
}  // namespace

extern "C" int32_t psnode_ode_backward_supported(const psnode_ode_bwd_args_f32* a) {
    if (!method_ok(a)) return 0;
    if (a->kernel == PSNODE_KERNEL_MFMA_WIDE || a->kernel == PSNODE_KERNEL_MFMA_TILE) return fused_bwd_shape_ok(a);
    if (a->kernel == PSNODE_KERNEL_MFMA_WAVE) return bwd_x_shape_ok(a);       // K4x (needs the saved rows at launch)
    if (a->kernel == PSNODE_KERNEL_MFMA) return fused_bwd_shape_ok(a) || use_latent_bwd(a) || use_latent64_bwd(a);
    return use_fused_bwd(a) || use_latent_bwd(a) || use_latent64_bwd(a) || ode_generic_ok(a);
}

extern "C" int64_t psnode_ode_backward_param_count(const psnode_ode_bwd_args_f32* a) {
    return a && a->de.n_layers >= 1 && a->de.n_layers <= kMaxLayers ? mlp_np(a->de) : 0;
}

extern "C" size_t psnode_ode_backward_workspace_bytes(const psnode_ode_bwd_args_f32* a) {
    if (!a || !psnode_ode_backward_supported(a)) return 0;
    size_t floats = ode_generic_ok(a) ? generic_bwd_workspace_floats(&a->de, nullptr, a->B) : 0;
    if (latent_bwd_shape_ok(a)) floats = latent_bwd_workspace_floats(a->B) > floats ? latent_bwd_workspace_floats(a->B) : floats;
    if (latent64_ode_bwd_shape_ok(a)) floats = latent64_ode_bwd_workspace_floats(a->B) > floats ? latent64_ode_bwd_workspace_floats(a->B) : floats;
    if (fused_bwd_shape_ok(a)) { const size_t f3 = fused_bwd_workspace_floats(a); floats = f3 > floats ? f3 : floats; }
    if (bwd_x_shape_ok(a)) { const size_t f4 = bwd_x_workspace_floats(a); floats = f4 > floats ? f4 : floats; }
    return floats * sizeof(float);
}

extern "C" int32_t psnode_ode_backward_f32(const psnode_ode_bwd_args_f32* a, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_call(a);
    if (rc) return rc;
    if (!psnode_ode_backward_supported(a)) return PSNODE_ERR_UNSUPPORTED;
    if (!ptrs_ok(a)) return PSNODE_ERR_NULL;
    if (!workspace_ok(workspace, workspace_bytes, psnode_ode_backward_workspace_bytes(a))) return PSNODE_ERR_WORKSPACE;
    if ((a->saved_act != nullptr) != (a->saved_xstage != nullptr)) return PSNODE_ERR_NULL;
    if (a->kernel == PSNODE_KERNEL_MFMA_WAVE && !bwd_x_preferred(a)) return PSNODE_ERR_UNSUPPORTED;   // K4x: saved rows, no teacher forcing
    if (a->kernel == PSNODE_KERNEL_MFMA_TILE && !fused_bwd_shape_ok(a)) return PSNODE_ERR_UNSUPPORTED;
    if (a->saved_act && !use_fused_bwd(a) && !use_latent64_bwd(a)) return PSNODE_ERR_UNSUPPORTED;      // only K4x, K4f and K9 read them
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->flags & ~PSNODE_FLAG_INPUT_TRUE_X) return PSNODE_ERR_UNSUPPORTED;
    if (a->flags & PSNODE_FLAG_INPUT_TRUE_X) {      // teacher-forced backward: K4f (recompute form) where the shape is its, else K5
        if (a->saved_act || a->kernel == PSNODE_KERNEL_MFMA_WAVE) return PSNODE_ERR_UNSUPPORTED;
        if (use_fused_bwd(a)) return fused_bwd_launch(a, static_cast<float*>(workspace), s);
        if ((a->kernel != PSNODE_KERNEL_AUTO && a->kernel != PSNODE_KERNEL_GENERIC) || !ode_generic_ok(a)) return PSNODE_ERR_UNSUPPORTED;
        return generic_backward(kBuildElu1, generic_bwd_call(*a), nullptr, workspace, stream);
    }
    if (bwd_x_preferred(a)) return bwd_x_launch(a, static_cast<float*>(workspace), s);      // K4x: up to one wave per SIMD at hidden 33..64
    if (use_latent_bwd(a)) return latent_bwd_launch(a, static_cast<float*>(workspace), s);
    if (use_latent64_bwd(a)) return latent64_ode_bwd_launch(a, static_cast<float*>(workspace), s);
    if (use_fused_bwd(a)) return fused_bwd_launch(a, static_cast<float*>(workspace), s);
    if (a->kernel == PSNODE_KERNEL_MFMA) return PSNODE_ERR_UNSUPPORTED;   // latent shape, unaligned views
    return generic_backward(kBuildElu1, generic_bwd_call(*a), nullptr, workspace, stream);
}

namespace {
bool use_latent16_dae_bwd(const psnode_dae_bwd_args_f32* a) {
    return a->kernel != PSNODE_KERNEL_GENERIC && latent16_dae_bwd_shape_ok(a) && (!a->xs || latent16_dae_bwd_ptrs_ok(a));
}
bool use_latent64_dae_bwd(const psnode_dae_bwd_args_f32* a) {
    return a->kernel != PSNODE_KERNEL_GENERIC && latent64_dae_bwd_shape_ok(a) && (!a->xs || latent64_dae_bwd_ptrs_ok(a));
}
}  // namespace

extern "C" int32_t psnode_dae_backward_supported(const psnode_dae_bwd_args_f32* a) {
    if (!method_ok(a)) return 0;
    if (a->x_dim < 1 || a->z_dim < 0 || a->v_dim < 0 || a->i_dim < 1) return 0;
    if (a->kernel == PSNODE_KERNEL_MFMA) return use_latent64_dae_bwd(a) || use_latent16_dae_bwd(a);
    if (use_latent64_dae_bwd(a) || use_latent16_dae_bwd(a)) return 1;
    return dae_generic_ok(a);
}

extern "C" size_t psnode_dae_backward_workspace_bytes(const psnode_dae_bwd_args_f32* a) {
    if (!a || !psnode_dae_backward_supported(a)) return 0;
    if (latent64_dae_bwd_shape_ok(a) && a->kernel != PSNODE_KERNEL_GENERIC) {
        // sized for every kernel this launch can end up on: K9, or K5 when the pointers turn out unaligned and K5 fits the shape
        size_t f = latent64_dae_bwd_workspace_floats(a);
        if (generic_bwd_fits(&a->de, &a->ae, a->x_dim, a->z_dim, a->v_dim, a->i_dim, false)) {
            const size_t k5 = generic_bwd_workspace_floats(&a->de, &a->ae, a->B);
            f = k5 > f ? k5 : f;
        }
        return f * sizeof(float);
    }
    if (latent16_dae_bwd_shape_ok(a)) {      // K8 (DAE) or, for unaligned views / kernel = generic, K5: the larger of the two
        const size_t k8 = latent16_dae_bwd_workspace_floats(a), k5 = generic_bwd_workspace_floats(&a->de, &a->ae, a->B);
        return (k8 > k5 ? k8 : k5) * sizeof(float);
    }
    return generic_bwd_workspace_floats(&a->de, &a->ae, a->B) * sizeof(float);
}

extern "C" int32_t psnode_dae_backward_f32(const psnode_dae_bwd_args_f32* a, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_call(a);
    if (rc) return rc;
    if (!psnode_dae_backward_supported(a)) return PSNODE_ERR_UNSUPPORTED;
    if (!ptrs_ok(a)) return PSNODE_ERR_NULL;
    if (!workspace_ok(workspace, workspace_bytes, psnode_dae_backward_workspace_bytes(a))) return PSNODE_ERR_WORKSPACE;
    {
        const bool sv = a->saved_act != nullptr;
        if ((a->saved_xstage != nullptr) != sv || (a->saved_ae_act != nullptr) != sv) return PSNODE_ERR_NULL;
        if (sv && a->event_idx && (!a->saved_ev_act || !a->saved_ev_i)) return PSNODE_ERR_NULL;
        if (sv && !use_latent64_dae_bwd(a)) return PSNODE_ERR_UNSUPPORTED;      // only K9 reads them here
    }
    if (use_latent64_dae_bwd(a)) return latent64_dae_bwd_launch(a, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
    if (use_latent16_dae_bwd(a)) return latent16_dae_bwd_launch(a, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
    if (a->kernel == PSNODE_KERNEL_MFMA) return PSNODE_ERR_UNSUPPORTED;
    return generic_backward(kBuildElu1, generic_bwd_call(*a), nullptr, workspace, stream);
}

// ---- The K5 entry-point families psnode_dae_backward_tf_* and psnode_{ode,dae}_backward_{act,rk,sub,lin,lag,pev,ab,ab3,ms,msp,rkc}_*: one checked call path
// (k5_backward), one query (k5_supported) over the family table of psnode_generic_family.h, which also holds the order of the checks per family.
namespace {
constexpr uint32_t kTfFlags = PSNODE_FLAG_INPUT_TRUE_X | PSNODE_FLAG_INPUT_TRUE_I;

// the difference between the three args structs: the base call, the flags and the ones the struct knows, the AE, the plain entry points
const psnode_ode_bwd_args_f32& base(const psnode_ode_bwd_args_f32& a) { return a; }
const psnode_dae_bwd_args_f32& base(const psnode_dae_bwd_args_f32& a) { return a; }
const psnode_dae_bwd_args_f32& base(const psnode_dae_bwd_tf_args_f32& a) { return a.base; }
uint32_t tf_flags(const psnode_ode_bwd_args_f32& a) { return a.flags; }
uint32_t tf_flags(const psnode_dae_bwd_args_f32&) { return 0; }
uint32_t tf_flags(const psnode_dae_bwd_tf_args_f32& a) { return a.flags; }
uint32_t tf_mask(const psnode_ode_bwd_args_f32&) { return PSNODE_FLAG_INPUT_TRUE_X; }
uint32_t tf_mask(const psnode_dae_bwd_args_f32&) { return 0; }
uint32_t tf_mask(const psnode_dae_bwd_tf_args_f32&) { return kTfFlags; }
const psnode_mlp_f32* ae_of(const psnode_ode_bwd_args_f32&) { return nullptr; }
const psnode_mlp_f32* ae_of(const psnode_dae_bwd_args_f32& a) { return &a.ae; }
int generic_ok(const psnode_ode_bwd_args_f32* a, bool pre, int lin) { return ode_generic_ok(a, pre, lin); }
int generic_ok(const psnode_dae_bwd_args_f32* a, bool pre, int lin) { return dae_generic_ok(a, pre, lin); }
int backward_elu1(const psnode_ode_bwd_args_f32* a, void* ws, size_t bytes, void* stream) { return psnode_ode_backward_f32(a, ws, bytes, stream); }
int backward_elu1(const psnode_dae_bwd_args_f32* a, void* ws, size_t bytes, void* stream) { return psnode_dae_backward_f32(a, ws, bytes, stream); }
int backward_elu1(const psnode_dae_bwd_tf_args_f32* a, void* ws, size_t bytes, void* stream) { return psnode_dae_backward_tf_f32(a, ws, bytes, stream); }
int supported_elu1(const psnode_ode_bwd_args_f32* a) { return psnode_ode_backward_supported(a); }
int supported_elu1(const psnode_dae_bwd_args_f32* a) { return psnode_dae_backward_supported(a); }
int supported_elu1(const psnode_dae_bwd_tf_args_f32* a) { return psnode_dae_backward_tf_supported(a); }
// the saved_* rows a family refuses: every one, but the _act family's call only the ones below kSavedAll and its query saved_act alone
enum Saved { kSavedAct, kSavedActCall, kSavedAll };
bool saved_rows(const psnode_ode_bwd_args_f32& a, Saved s) { return a.saved_act || (s != kSavedAct && a.saved_xstage); }
bool saved_rows(const psnode_dae_bwd_args_f32& a, Saved s) {
    return a.saved_act || (s != kSavedAct && (a.saved_xstage || a.saved_ae_act)) || (s == kSavedAll && (a.saved_ev_act || a.saved_ev_i));
}
// the dataset rows of the flags set, next to the pointers of the base call; the call struct with them
bool ptrs_ok(const psnode_dae_bwd_tf_args_f32* a) {
    if (((a->flags & PSNODE_FLAG_INPUT_TRUE_X) && !a->x_true) || ((a->flags & PSNODE_FLAG_INPUT_TRUE_I) && !a->i_true)) return false;
    return ptrs_ok(&a->base);
}
GenericBwdCall generic_bwd_call(const psnode_dae_bwd_tf_args_f32& a) {
    GenericBwdCall c = generic_bwd_call(a.base);
    c.flags = a.flags; c.xt = a.x_true; c.it = a.i_true;
    return c;
}

template <class Args>
bool k5_route_ok(const FamilyRow& f, const Args& a, const ActPair& p, bool elu1, bool query) {
    const auto& b = base(a);
    const uint32_t flags = tf_flags(a);
    if (b.kernel != PSNODE_KERNEL_AUTO && b.kernel != PSNODE_KERNEL_GENERIC) return false;
    if ((flags & ~tf_mask(a)) || (flags && !elu1)) return false;      // (teacher forcing: ELU(1) only)
    if (f.no_tf && flags) return false;
    if (saved_rows(b, f.saved_all ? kSavedAll : query ? kSavedAct : kSavedActCall)) return false;
    return generic_ok(&b, f.pre || family_build(f, act_pair_keeps_u(p)) == kBuildPre, f.lin) != 0;      // (the fit of the build)
}
// K5's workspace for the family's call: gbwd_layout, or the segment-parallel build's own layout for the call's chunks
template <class Base>
size_t k5_workspace_floats(const FamilyRow& f, const Base& b, const CallOpts& o) {
    if (!f.par) return generic_bwd_workspace_floats(&b.de, ae_of(b), b.B);
    const psnode_mlp_f32* ae = ae_of(b);
    const int n = b.de.in_dim / 3;      // (the recipe: 3 n input columns, checked by the route)
    return generic_bwd_msp_workspace_floats(&b.de, ae, b.B, n, ae ? ae->in_dim - n - b.x_dim : 0, family_chunks(f, o, b.T));
}

template <class Args>
int k5_backward(Family fam, const Args* a, const CallOpts& o, void* workspace, size_t workspace_bytes, void* stream) {
    constexpr bool tf_struct = std::is_same<Args, psnode_dae_bwd_tf_args_f32>::value;
    ActPair p;
    psnode_rk_tableau_f32 t;
    bool elu1 = true;
    int rc = family_front(fam, o, p, elu1);
    if (rc) return rc;
    const FamilyRow& f = kFamilies[fam];
    if (f.elu1_plain && elu1) return backward_elu1(a, workspace, workspace_bytes, stream);
    if constexpr (tf_struct) {
        if (fam == kFamAct) {      // (_sub, substeps == 1, no tableau: the _act family takes the base args)
            if (!a) return PSNODE_ERR_NULL;
            if (a->flags) return PSNODE_ERR_UNSUPPORTED;
            return k5_backward(kFamAct, &a->base, {o.de_act, o.ae_act}, workspace, workspace_bytes, stream);
        }
    }
    rc = family_tableau(f, o.tab, a ? &base(*a).method : nullptr, t);
    if (rc) return rc;
    const auto& b = base(*a);
    if (b.T < 1 || b.B < 1 || (tf_struct && tf_flags(*a) && b.T < 2)) return PSNODE_ERR_DIMS;
    if (!k5_route_ok(f, *a, p, elu1, false) || family_chunks(f, o, b.T) > kMaxChunks) return PSNODE_ERR_UNSUPPORTED;
    const int nsub = family_substeps(f, o);
    if (!ptrs_ok(a) || (nsub > 1 && b.T >= 2 && !o.sub->x_sub) || (f.needs_events && !b.event_idx)) return PSNODE_ERR_NULL;
    if (f.seg && b.T - 1 > o.every() && !o.x_true()) return PSNODE_ERR_NULL;
    if (!workspace_ok(workspace, workspace_bytes, k5_workspace_floats(f, b, o) * sizeof(float))) return PSNODE_ERR_WORKSPACE;
    GenericBwdCall c = generic_bwd_call(*a);
    if (f.tab != kTabNone) c.rk = &t;
    c.substeps = nsub;
    c.x_sub = o.sub ? o.sub->x_sub : nullptr;
    c.stencil = o.stencil;
    c.rkc = o.rkc;
    c.ab_pt = o.per_trajectory != 0;
    if (f.seg) { c.ms_every = o.every(); c.ms_x_true = o.x_true(); c.ms_per_group = o.per_group(); }
    return generic_backward(family_build(f, act_pair_keeps_u(p)), c, &p, workspace, stream);
}

template <class Args>
int k5_supported(Family fam, const Args* a, const CallOpts& o) {
    ActPair p;
    psnode_rk_tableau_f32 t;
    bool elu1 = true;
    if (!a || family_front(fam, o, p, elu1)) return 0;
    const FamilyRow& f = kFamilies[fam];
    if (f.elu1_plain && elu1) return supported_elu1(a);
    if constexpr (std::is_same<Args, psnode_dae_bwd_tf_args_f32>::value) {
        if (fam == kFamAct) return a->flags == 0 && k5_supported(kFamAct, &a->base, {o.de_act, o.ae_act});      // (as k5_backward's)
    }
    if (family_tableau(f, o.tab, &base(*a).method, t)) return 0;
    return k5_route_ok(f, *a, p, elu1, true) && family_chunks(f, o, base(*a).T) <= kMaxChunks;
}

// (DAE: the ODE's sizes come from psnode_ode_backward_workspace_bytes)
size_t k5_workspace_bytes(Family fam, const psnode_dae_bwd_tf_args_f32* a, const CallOpts& o) {
    if (!k5_supported(fam, a, o)) return 0;
    if (kFamilies[fam].demotes && o.sub->substeps == 1 && !o.tab) {      // the entry point that call goes to
        ActPair p;
        bool elu1 = true;
        act_pair(o.de_act, o.ae_act, p, elu1);
        return elu1 ? psnode_dae_backward_tf_workspace_bytes(a) : psnode_dae_backward_workspace_bytes(&a->base);
    }
    return k5_workspace_floats(kFamilies[fam], a->base, o) * sizeof(float);
}
}  // namespace

// ---- the K5 families (their table and the order of their checks: psnode_generic_family.h).  Each wrapper names its family and what it
// takes; flags == 0 on _tf is the plain call.
extern "C" int32_t psnode_dae_backward_tf_supported(const psnode_dae_bwd_tf_args_f32* a) {
    if (a && a->flags == 0) return psnode_dae_backward_supported(&a->base);
    return k5_supported(kFamTf, a, {});
}
extern "C" size_t psnode_dae_backward_tf_workspace_bytes(const psnode_dae_bwd_tf_args_f32* a) {
    if (a && a->flags == 0) return psnode_dae_backward_workspace_bytes(&a->base);
    return k5_workspace_bytes(kFamTf, a, {});
}
extern "C" int32_t psnode_dae_backward_tf_f32(const psnode_dae_bwd_tf_args_f32* a, void* workspace, size_t workspace_bytes, void* stream) {
    if (a && a->flags == 0) return psnode_dae_backward_f32(&a->base, workspace, workspace_bytes, stream);
    return k5_backward(kFamTf, a, {}, workspace, workspace_bytes, stream);
}

extern "C" int32_t psnode_ode_backward_act_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act) {
    return k5_supported(kFamAct, a, {de_act});
}
extern "C" int32_t psnode_ode_backward_act_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamAct, a, {de_act}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_act_supported(const psnode_dae_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act) {
    return k5_supported(kFamAct, a, {de_act, ae_act});
}
extern "C" int32_t psnode_dae_backward_act_f32(const psnode_dae_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act, void* ws,
                                               size_t bytes, void* stream) {
    return k5_backward(kFamAct, a, {de_act, ae_act}, ws, bytes, stream);
}

extern "C" int32_t psnode_ode_backward_rk_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_rk_tableau_f32* tab) {
    return k5_supported(kFamRk, a, {de_act, nullptr, tab});
}
extern "C" int32_t psnode_ode_backward_rk_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                              void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamRk, a, {de_act, nullptr, tab}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_rk_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab) {
    return k5_supported(kFamRk, a, {de_act, ae_act, tab});
}
extern "C" size_t psnode_dae_backward_rk_workspace_bytes(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                         const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab) {
    return k5_workspace_bytes(kFamRk, a, {de_act, ae_act, tab});
}
extern "C" int32_t psnode_dae_backward_rk_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                              const psnode_rk_tableau_f32* tab, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamRk, a, {de_act, ae_act, tab}, ws, bytes, stream);
}

extern "C" int32_t psnode_ode_backward_sub_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k5_supported(kFamSub, a, {de_act, nullptr, tab, sub});
}
extern "C" int32_t psnode_ode_backward_sub_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamSub, a, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_sub_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub) {
    return k5_supported(kFamSub, a, {de_act, ae_act, tab, sub});
}
extern "C" size_t psnode_dae_backward_sub_workspace_bytes(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                          const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                          const psnode_substeps_f32* sub) {
    return k5_workspace_bytes(kFamSub, a, {de_act, ae_act, tab, sub});
}
extern "C" int32_t psnode_dae_backward_sub_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes,
                                               void* stream) {
    return k5_backward(kFamSub, a, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

extern "C" int32_t psnode_ode_backward_lin_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k5_supported(kFamLin, a, {de_act, nullptr, tab, sub});
}
extern "C" int32_t psnode_ode_backward_lin_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamLin, a, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_lin_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub) {
    return k5_supported(kFamLin, a, {de_act, ae_act, tab, sub});
}
extern "C" size_t psnode_dae_backward_lin_workspace_bytes(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                          const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                          const psnode_substeps_f32* sub) {
    return k5_workspace_bytes(kFamLin, a, {de_act, ae_act, tab, sub});
}
extern "C" int32_t psnode_dae_backward_lin_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes,
                                               void* stream) {
    return k5_backward(kFamLin, a, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

// (per-trajectory events: the args' event_idx is the [T-1, B] table of psnode_event_table_pt_f32)
extern "C" int32_t psnode_ode_backward_pev_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k5_supported(kFamPev, a, {de_act, nullptr, tab, sub});
}
extern "C" int32_t psnode_ode_backward_pev_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamPev, a, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_pev_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub) {
    return k5_supported(kFamPev, a, {de_act, ae_act, tab, sub});
}
extern "C" int32_t psnode_dae_backward_pev_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes,
                                               void* stream) {
    return k5_backward(kFamPev, a, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

// (two-step Adams-Bashforth: per_trajectory says whether a non-NULL event_idx is the [T-1, B] table or the shared [T-1])
extern "C" int32_t psnode_ode_backward_ab_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act) {
    return k5_supported(kFamAb, a, {de_act});
}
extern "C" int32_t psnode_ode_backward_ab_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, int32_t per_trajectory, void* ws,
                                              size_t bytes, void* stream) {
    return k5_backward(kFamAb, a, {de_act, nullptr, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_ab_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_act_f32* ae_act) {
    return k5_supported(kFamAb, a, {de_act, ae_act});
}
extern "C" int32_t psnode_dae_backward_ab_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                              int32_t per_trajectory, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamAb, a, {de_act, ae_act, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}

// (four-point Lagrange externals: the _lin family's prototypes and order of checks, plus the stencil table -- NULL: one piece 0 .. T - 1)
extern "C" int32_t psnode_ode_backward_lag_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st) {
    return k5_supported(kFamLag, a, {de_act, nullptr, tab, sub, nullptr, 0, nullptr, st});
}
extern "C" int32_t psnode_ode_backward_lag_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamLag, a, {de_act, nullptr, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_lag_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st) {
    return k5_supported(kFamLag, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st});
}
extern "C" size_t psnode_dae_backward_lag_workspace_size(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                         const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                         const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st) {
    return k5_workspace_bytes(kFamLag, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st});
}
// (stage-wise algebraic heads, DAE only: the _lag family's prototypes and order of checks plus `interp`, which picks the interpolant)
extern "C" int32_t psnode_dae_backward_sth_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st, int32_t interp) {
    Family fam;
    return sth_family(interp, fam) ? k5_supported(fam, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}) : 0;
}
extern "C" size_t psnode_dae_backward_sth_workspace_size(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                          const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                          const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st, int32_t interp) {
    Family fam;
    return sth_family(interp, fam) ? k5_workspace_bytes(fam, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}) : 0;
}
extern "C" int32_t psnode_dae_backward_sth_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st,
                                               int32_t interp, void* ws, size_t bytes, void* stream) {
    Family fam;
    if (!sth_family(interp, fam)) return PSNODE_ERR_METHOD;
    return k5_backward(fam, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_lag_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st,
                                               void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamLag, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}

// (Runge-Kutta-Chebyshev: the adjoint of the recurrence, stage by stage; the _sub family's checks with the stage count in the sub-steps' place)
extern "C" int32_t psnode_ode_backward_rkc_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc) {
    psnode_substeps_f32 s;
    return k5_supported(kFamRkc, a, {de_act, nullptr, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc});
}
extern "C" int32_t psnode_ode_backward_rkc_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc, void* ws,
                                               size_t bytes, void* stream) {
    psnode_substeps_f32 s;
    return k5_backward(kFamRkc, a, {de_act, nullptr, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_rkc_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rkc_f32* rkc) {
    psnode_substeps_f32 s;
    return k5_supported(kFamRkc, a, {de_act, ae_act, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc});
}
extern "C" size_t psnode_dae_backward_rkc_workspace_size(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                         const psnode_act_f32* ae_act, const psnode_rkc_f32* rkc) {
    psnode_substeps_f32 s;
    return k5_workspace_bytes(kFamRkc, a, {de_act, ae_act, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc});
}
extern "C" int32_t psnode_dae_backward_rkc_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rkc_f32* rkc, void* ws, size_t bytes, void* stream) {
    psnode_substeps_f32 s;
    return k5_backward(kFamRkc, a, {de_act, ae_act, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc}, ws, bytes, stream);
}

// (three-step Adams-Bashforth with the Heun restart step: the _ab family's prototypes and order of checks)
extern "C" int32_t psnode_ode_backward_ab3_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act) {
    return k5_supported(kFamAb3, a, {de_act});
}
extern "C" int32_t psnode_ode_backward_ab3_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, int32_t per_trajectory, void* ws,
                                              size_t bytes, void* stream) {
    return k5_backward(kFamAb3, a, {de_act, nullptr, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_ab3_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_act_f32* ae_act) {
    return k5_supported(kFamAb3, a, {de_act, ae_act});
}
extern "C" int32_t psnode_dae_backward_ab3_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                              int32_t per_trajectory, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamAb3, a, {de_act, ae_act, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}

// (multiple shooting: the step that leaves grid point k > 0 with k % seg->every == 0 started from seg->x_true[k])
extern "C" int32_t psnode_ode_backward_ms_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                                    const psnode_segments_f32* seg) {
    return k5_supported(kFamMs, a, {de_act, nullptr, tab, sub, seg});
}
extern "C" int32_t psnode_ode_backward_ms_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                              const psnode_substeps_f32* sub, const psnode_segments_f32* seg, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamMs, a, {de_act, nullptr, tab, sub, seg}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_ms_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                    const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                    const psnode_substeps_f32* sub, const psnode_segments_f32* seg) {
    return k5_supported(kFamMs, a, {de_act, ae_act, tab, sub, seg});
}
extern "C" int32_t psnode_dae_backward_ms_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                              const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg,
                                              void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamMs, a, {de_act, ae_act, tab, sub, seg}, ws, bytes, stream);
}

// (segments in parallel: the _ms call swept by a tiles x chunks grid; its workspace is its own -- one parameter partial per workgroup, and
//  what crosses a chunk border)
extern "C" int32_t psnode_ode_backward_msp_supported(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                                     const psnode_segment_groups_f32* grp) {
    return k5_supported(kFamMsp, a, {de_act, nullptr, tab, sub, nullptr, 0, grp});
}
extern "C" size_t psnode_ode_backward_msp_workspace_size(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act,
                                                         const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                                         const psnode_segment_groups_f32* grp) {
    const CallOpts o{de_act, nullptr, tab, sub, nullptr, 0, grp};
    return k5_supported(kFamMsp, a, o) ? k5_workspace_floats(kFamilies[kFamMsp], *a, o) * sizeof(float) : 0;
}
extern "C" int32_t psnode_ode_backward_msp_f32(const psnode_ode_bwd_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp, void* ws, size_t bytes,
                                               void* stream) {
    return k5_backward(kFamMsp, a, {de_act, nullptr, tab, sub, nullptr, 0, grp}, ws, bytes, stream);
}
extern "C" int32_t psnode_dae_backward_msp_supported(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                     const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                     const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp) {
    return k5_supported(kFamMsp, a, {de_act, ae_act, tab, sub, nullptr, 0, grp});
}
extern "C" size_t psnode_dae_backward_msp_workspace_size(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act,
                                                         const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                                         const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp) {
    return k5_workspace_bytes(kFamMsp, a, {de_act, ae_act, tab, sub, nullptr, 0, grp});
}
extern "C" int32_t psnode_dae_backward_msp_f32(const psnode_dae_bwd_tf_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                               const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                               const psnode_segment_groups_f32* grp, void* ws, size_t bytes, void* stream) {
    return k5_backward(kFamMsp, a, {de_act, ae_act, tab, sub, nullptr, 0, grp}, ws, bytes, stream);
}
