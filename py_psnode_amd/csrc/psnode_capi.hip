// C ABI of libpsnode_hip.so (see include/psnode_hip.h): argument validation, the forward workspace's layout (psnode_workspace.h),
// weight packing and kernel dispatch.  Everything is enqueued on the caller's stream.  (K0's option families: psnode_generic_family.h.)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "psnode_generic_family.h"

namespace psnode {
namespace {

constexpr size_t kAlignFloats = 64;   // 256-byte alignment of every workspace segment

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the widths alone (the dims-only queries); `ptrs`: also every layer's weight and bias, in check_mlp's order of statuses
int check_mlp_dims(const psnode_mlp_f32& m, int want_in, int want_out, bool ptrs = false) {
    if (m.n_layers < 1 || m.n_layers > kMaxLayers) return PSNODE_ERR_DIMS;
    if (m.in_dim != want_in || m.in_dim < 1) return PSNODE_ERR_DIMS;
    if (m.in_dim > PSNODE_MAX_IN_WIDTH) return PSNODE_ERR_UNSUPPORTED;    // consistent, but wider than any kernel takes
    for (int l = 0; l < m.n_layers; ++l) {
        if (m.out_dim[l] < 1) return PSNODE_ERR_DIMS;
        if (m.out_dim[l] > PSNODE_MAX_WIDTH) return PSNODE_ERR_UNSUPPORTED;
        if (ptrs && (!m.weight[l] || !m.bias[l])) return PSNODE_ERR_NULL;
    }
    if (m.out_dim[m.n_layers - 1] != want_out) return PSNODE_ERR_DIMS;
    return PSNODE_OK;
}
int check_mlp(const psnode_mlp_f32& m, int want_in, int want_out) { return check_mlp_dims(m, want_in, want_out, true); }

// takes the MLP's image segments (K0's MFMA images, one per layer)
void take_images(MlpDev& d, Arena& A) {
    int k = d.in_dim;
    for (int l = 0; l < d.n_layers; ++l) {
        d.wt[l] = A.take(round_up(generic_image_floats(k, d.out_dim[l]), kAlignFloats));
        k = d.out_dim[l];
    }
}
// The forward workspace: K0's images of the DE | of the AE | the pack of the MFMA family that takes the shape (sized for the largest of
// them: psnode_mfma.hip).  Returns the pack.
float* forward_layout(const psnode_mlp_f32& de, const psnode_mlp_f32* ae, MlpDev& dde, MlpDev& dae, Arena& A) {
    bind_mlp(de, dde);
    take_images(dde, A);
    if (ae) { bind_mlp(*ae, dae); take_images(dae, A); }
    float* pack = A.take(mfma_pack_floats(&de, ae));
    A.slack(kAlignFloats);      // kept from the parent, purpose not established (every segment in front of it is a multiple of 64 floats)
    return pack;
}

int max_width(const psnode_mlp_f32& m) {
    int w = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) w = m.out_dim[l] > w ? m.out_dim[l] : w;
    return w;
}
// widest layer OUTPUT of the call's MLPs (IntegrateDev::maxo)
int max_out_width(const psnode_mlp_f32& de, const psnode_mlp_f32* ae) {
    int w = 1;
    for (int l = 0; l < de.n_layers; ++l) w = de.out_dim[l] > w ? de.out_dim[l] : w;
    if (ae) for (int l = 0; l < ae->n_layers; ++l) w = ae->out_dim[l] > w ? ae->out_dim[l] : w;
    return w;
}

__global__ void event_table_kernel(long long n_steps, const float* clock, long long stride_k, const float* ev_times,
                                   long long stride_e, int n_events, int* event_idx, int* dup_flag) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_steps) return;
    const float tk = clock[k * stride_k];
    int hit = -1, cnt = 0;
    for (int e = 0; e < n_events; ++e) {
        if (ev_times[e * stride_e] == tk) {   // exact equality, like Tensor.__contains__ (neural_base.py:54)
            if (hit < 0) hit = e;
            ++cnt;
        }
    }
    event_idx[k] = hit;
    if (cnt > 1 && dup_flag) *dup_flag = 1;
}

// (call: psnode_act.h, K0Call -- the plain entry points pass K0Call{})
int dispatch(IntegrateDev& d, bool dae, int kernel, const psnode_mlp_f32* de, const psnode_mlp_f32* ae, void* workspace,
             size_t workspace_bytes, hipStream_t stream, const K0Call& call) {
    if (!workspace_ok(workspace, workspace_bytes, psnode_workspace_bytes(de, ae))) return PSNODE_ERR_WORKSPACE;
    Arena A{static_cast<float*>(workspace)};
    float* pack = forward_layout(*de, dae ? ae : nullptr, d.de, d.ae, A);
    d.maxw = max_width(*de);
    if (dae && max_width(*ae) > d.maxw) d.maxw = max_width(*ae);
    d.maxo = max_out_width(*de, dae ? ae : nullptr);

    const bool has_mfma = call.build == kBuildElu1 && (dae ? mfma_dae_supported(d) : mfma_ode_supported(d));
    const bool want_mfma = kernel == PSNODE_KERNEL_MFMA || kernel == PSNODE_KERNEL_MFMA_TILE || kernel == PSNODE_KERNEL_MFMA_WAVE;
    if (want_mfma && !has_mfma) return PSNODE_ERR_UNSUPPORTED;
    if (kernel == PSNODE_KERNEL_MFMA_WAVE && !(dae ? mfma_x_dae_supported(d) : mfma_x_ode_supported(d))) return PSNODE_ERR_UNSUPPORTED;
    d.kern = kernel;
    const bool use_mfma = has_mfma && kernel != PSNODE_KERNEL_GENERIC;
    if (d.T < 1 || d.B < 1) return PSNODE_ERR_DIMS;
    if (use_mfma) return ok_or_hip(launch_mfma(d, dae, pack, stream));

    if (generic_lds_bytes(d, dae, (call.build == kBuildLag || call.build == kBuildLagSth) ? 2 : ((call.build == kBuildLin || call.build == kBuildLinSth) ? 1 : 0)) > 160 * 1024) return PSNODE_ERR_UNSUPPORTED;
    hipError_t e = launch_pack_image(d.de, dae ? &d.ae : nullptr, d.xd, d.xd + d.zd + (dae ? d.vd + d.id : 0), d.zd + (dae ? d.vd : 0), stream);
    if (e != hipSuccess) return PSNODE_ERR_HIP;
    switch (call.build) {
        case kBuildElu1: e = launch_generic<BuildElu1>(d, dae, call, stream); break;
        case kBuildAct: e = launch_generic<BuildAct>(d, dae, call, stream); break;
        case kBuildPre: e = launch_generic<BuildPre>(d, dae, call, stream); break;
        case kBuildRk: e = launch_generic<BuildRk>(d, dae, call, stream); break;
        case kBuildSub: e = launch_generic<BuildSub>(d, dae, call, stream); break;
        case kBuildLin: e = launch_generic<BuildLin>(d, dae, call, stream); break;
        case kBuildPev: e = launch_generic<BuildPev>(d, dae, call, stream); break;
        case kBuildAb: e = launch_generic<BuildAb>(d, dae, call, stream); break;
        case kBuildMs: e = launch_generic<BuildMs>(d, dae, call, stream); break;
        case kBuildMsp: e = launch_generic<BuildMsp>(d, dae, call, stream); break;
        case kBuildAb3: e = launch_generic<BuildAb3>(d, dae, call, stream); break;
        case kBuildLag: e = launch_generic<BuildLag>(d, dae, call, stream); break;
        case kBuildRkc: e = launch_generic<BuildRkc>(d, dae, call, stream); break;
        case kBuildLinSth: e = launch_generic<BuildLinSth>(d, dae, call, stream); break;
        case kBuildLagSth: e = launch_generic<BuildLagSth>(d, dae, call, stream); break;
    }
    return ok_or_hip(e);
}

// dims-only view of the args: what the *_save_hidden / *_kernel_for / *_act_supported queries ask the kernel families with (no pointers),
// and what fill_ode / fill_dae start from
IntegrateDev dims_only(const psnode_ode_args_f32& a) {
    IntegrateDev d;
    memset(&d, 0, sizeof(d));
    d.method = a.method; d.flags = a.flags; d.xd = a.x_dim; d.zd = a.z_dim; d.T = a.T; d.B = a.B;
    bind_dims(a.de, d.de);
    d.kern = a.kernel;      // a forced _TILE / _WAVE / GENERIC is what the call would run
    return d;
}
IntegrateDev dims_only(const psnode_dae_args_f32& a) {
    IntegrateDev d;
    memset(&d, 0, sizeof(d));
    d.method = a.method; d.flags = a.flags; d.xd = a.x_dim; d.zd = a.z_dim; d.vd = a.v_dim; d.id = a.i_dim; d.T = a.T; d.B = a.B;
    bind_dims(a.de, d.de);
    bind_dims(a.ae, d.ae);
    d.kern = a.kernel;
    return d;
}

int fill_ode(const psnode_ode_args_f32* a, IntegrateDev& d) {
    if (!a) return PSNODE_ERR_NULL;
    if (a->method < PSNODE_EULER || a->method > PSNODE_RK4_38) return PSNODE_ERR_METHOD;
    if (a->x_dim < 1 || a->z_dim < 0 || a->T < 1 || a->B < 1) return PSNODE_ERR_DIMS;
    const int n = a->x_dim + a->z_dim;
    int rc = check_mlp(a->de, 3 * n, a->x_dim);
    if (rc) return rc;
    if (!a->t.ptr || !a->x.ptr || !a->all_initial || !a->x_out) return PSNODE_ERR_NULL;
    if (a->z_dim > 0 && !a->z.ptr) return PSNODE_ERR_NULL;
    if (a->event_idx && a->z_dim > 0 && !a->z_jump) return PSNODE_ERR_NULL;
    d = dims_only(*a);
    d.flags &= PSNODE_FLAG_INPUT_TRUE_X;
    d.t = view(a->t);
    d.x = view(a->x);
    d.z = view(a->z);
    d.a0 = a->all_initial;
    d.ev = a->event_idx;
    bind_jumps(d, *a);
    d.xo = a->x_out;
    if ((a->save_act != nullptr) != (a->save_xstage != nullptr)) return PSNODE_ERR_NULL;
    d.sact = a->save_act;
    d.sxst = a->save_xstage;
    return PSNODE_OK;
}

int fill_dae(const psnode_dae_args_f32* a, IntegrateDev& d) {
    if (!a) return PSNODE_ERR_NULL;
    if (a->method < PSNODE_EULER || a->method > PSNODE_RK4_38) return PSNODE_ERR_METHOD;
    if (a->x_dim < 1 || a->z_dim < 0 || a->v_dim < 0 || a->i_dim < 1 || a->T < 1 || a->B < 1) return PSNODE_ERR_DIMS;
    const int n = a->x_dim + a->z_dim + a->v_dim + a->i_dim;
    int rc = check_mlp(a->de, 3 * n, a->x_dim);
    if (rc) return rc;
    rc = check_mlp(a->ae, n + a->x_dim + a->z_dim + a->v_dim, a->i_dim);
    if (rc) return rc;
    if (!a->t.ptr || !a->x_init || !a->all_initial || !a->x_out || !a->i_out) return PSNODE_ERR_NULL;
    if ((a->z_dim > 0 && !a->z.ptr) || (a->v_dim > 0 && !a->v.ptr)) return PSNODE_ERR_NULL;
    if ((a->flags & PSNODE_FLAG_INPUT_TRUE_X) && !a->x.ptr) return PSNODE_ERR_NULL;
    if ((a->flags & PSNODE_FLAG_INPUT_TRUE_I) && !a->i.ptr) return PSNODE_ERR_NULL;
    if (a->event_idx && ((a->z_dim > 0 && !a->z_jump) || (a->v_dim > 0 && !a->v_jump))) return PSNODE_ERR_NULL;
    d = dims_only(*a);
    d.flags &= PSNODE_FLAG_INPUT_TRUE_X | PSNODE_FLAG_INPUT_TRUE_I;
    d.t = view(a->t);
    d.x = view(a->x);
    d.z = view(a->z);
    d.v = view(a->v);
    d.i = view(a->i);
    d.x_init = a->x_init;
    d.a0 = a->all_initial;
    d.ev = a->event_idx;
    bind_jumps(d, *a);
    d.xo = a->x_out;
    d.io = a->i_out;
    const bool sv = a->save_act != nullptr;
    if ((a->save_xstage != nullptr) != sv || (a->save_ae_act != nullptr) != sv) return PSNODE_ERR_NULL;
    if (sv && a->event_idx && (!a->save_ev_act || !a->save_ev_i)) return PSNODE_ERR_NULL;
    d.sact = a->save_act;
    d.sxst = a->save_xstage;
    d.saeact = a->save_ae_act;
    d.sevact = a->save_ev_act;
    d.sevi = a->save_ev_i;
    return PSNODE_OK;
}

// ---- The K0 entry-point families psnode_{ode,dae}_integrate_{act,rk,sub,lin,lag,pev,ab,ab3,ms,msp,rkc}_* and psnode_dae_integrate_sth_*: one checked call path (k0_integrate) and one query
// (k0_supported) over the family table of psnode_generic_family.h, which also holds the order of the checks per family.
// the ODE / DAE difference: the side outputs, the recipe widths, fill_*, the AE, the plain entry point
bool side_outputs(const psnode_ode_args_f32& a) { return a.save_act || a.save_xstage; }
bool side_outputs(const psnode_dae_args_f32& a) { return a.save_act || a.save_xstage || a.save_ae_act || a.save_ev_act || a.save_ev_i; }
bool recipe_ok(const psnode_ode_args_f32& a) {
    return a.x_dim >= 1 && a.z_dim >= 0 && !check_mlp_dims(a.de, 3 * (a.x_dim + a.z_dim), a.x_dim);
}
bool recipe_ok(const psnode_dae_args_f32& a) {
    if (a.x_dim < 1 || a.z_dim < 0 || a.v_dim < 0 || a.i_dim < 1) return false;
    const int n = a.x_dim + a.z_dim + a.v_dim + a.i_dim;
    return !check_mlp_dims(a.de, 3 * n, a.x_dim) && !check_mlp_dims(a.ae, n + a.x_dim + a.z_dim + a.v_dim, a.i_dim);
}
int fill(const psnode_ode_args_f32* a, IntegrateDev& d) { return fill_ode(a, d); }
int fill(const psnode_dae_args_f32* a, IntegrateDev& d) { return fill_dae(a, d); }
const psnode_mlp_f32* ae_of(const psnode_ode_args_f32&) { return nullptr; }
const psnode_mlp_f32* ae_of(const psnode_dae_args_f32& a) { return &a.ae; }
bool has_dataset_x(const psnode_ode_args_f32&) { return true; }      // (fill_ode requires the pointer)
bool has_dataset_x(const psnode_dae_args_f32& a) { return a.x.ptr != nullptr; }
int integrate_elu1(const psnode_ode_args_f32* a, void* ws, size_t bytes, void* stream) { return psnode_ode_integrate_f32(a, ws, bytes, stream); }
int integrate_elu1(const psnode_dae_args_f32* a, void* ws, size_t bytes, void* stream) { return psnode_dae_integrate_f32(a, ws, bytes, stream); }

// K0 only (AUTO / GENERIC) and no training side outputs; the _act family looks at save_act alone (a lone save_xstage is fill_*'s status)
template <class Args>
bool k0_route_ok(const FamilyRow& f, const Args& a) {
    if (a.kernel != PSNODE_KERNEL_AUTO && a.kernel != PSNODE_KERNEL_GENERIC) return false;
    if (f.no_tf && (a.flags & (PSNODE_FLAG_INPUT_TRUE_X | PSNODE_FLAG_INPUT_TRUE_I))) return false;
    if (f.seg && !has_dataset_x(a)) return false;      // (the restarts read x)
    return f.saved_all ? !side_outputs(a) : !a.save_act;
}

template <class Args>
int k0_integrate(Family fam, const Args* args, const CallOpts& o, void* workspace, size_t workspace_bytes, void* stream) {
    K0Call call{};
    bool elu1 = true;
    int rc = family_front(fam, o, call.act, elu1);
    if (rc) return rc;
    const FamilyRow& f = kFamilies[fam];
    if (f.elu1_plain && elu1) return integrate_elu1(args, workspace, workspace_bytes, stream);
    rc = family_tableau(f, o.tab, args ? &args->method : nullptr, call.rk);
    if (rc && !(f.tab == kTabNone && rc == PSNODE_ERR_METHOD)) return rc;      // (a call without a tableau leaves a bad method to fill_*, behind the route; its query refuses it in front)
    Args c = *args;
    if (f.tab != kTabNone) c.method = PSNODE_EULER;      // (not read by the build; fill_* checks it)
    if (!k0_route_ok(f, c) || family_chunks(f, o, c.T) > kMaxChunks) return PSNODE_ERR_UNSUPPORTED;
    IntegrateDev d;
    rc = fill(&c, d);
    if (rc) return rc;
    if (f.needs_events && !d.ev) return PSNODE_ERR_NULL;
    call.build = family_build(f, act_pair_pre(call.act));      // (K0 keeps no u)
    call.ev_pt = o.per_trajectory ? 1 : 0;
    call.ms_every = o.has_seg() ? o.every() : 0;
    call.per_group = o.per_group();
    call.sub = SubDev{family_substeps(f, o), o.sub ? o.sub->x_sub : nullptr};
    call.stencil = o.stencil;
    call.rkc = o.rkc;
    return dispatch(d, ae_of(c) != nullptr, c.kernel, &c.de, ae_of(c), workspace, workspace_bytes, static_cast<hipStream_t>(stream), call);
}

// the same checks from the dims alone, and the LDS fit of the family's build
template <class Args>
int k0_supported(Family fam, const Args* a, const CallOpts& o) {
    ActPair p;
    psnode_rk_tableau_f32 t;
    bool elu1 = true;
    if (!a || family_front(fam, o, p, elu1)) return 0;
    const FamilyRow& f = kFamilies[fam];
    if (family_tableau(f, o.tab, &a->method, t) || !recipe_ok(*a)) return 0;
    if (f.elu1_plain && elu1) return 1;
    if (!k0_route_ok(f, *a) || family_chunks(f, o, a->T) > kMaxChunks) return 0;
    IntegrateDev d = dims_only(*a);
    d.maxo = max_out_width(a->de, ae_of(*a));
    return generic_lds_bytes(d, ae_of(*a) != nullptr, f.lin) <= 160 * 1024;
}

}  // namespace

int rk_tableau_check(const psnode_rk_tableau_f32* tab) {
    if (!tab) return PSNODE_ERR_NULL;
    if (tab->stages < 1 || tab->stages > 4) return PSNODE_ERR_METHOD;
    for (int s = 0; s < 4; ++s) {
        if (!isfinite(tab->b[s]) || (s >= tab->stages && tab->b[s] != 0.0f)) return PSNODE_ERR_METHOD;
        for (int j = 0; j < 4; ++j) {
            if (!isfinite(tab->a[s][j])) return PSNODE_ERR_METHOD;
            if ((j >= s || s >= tab->stages) && tab->a[s][j] != 0.0f) return PSNODE_ERR_METHOD;
        }
    }
    return PSNODE_OK;
}

int sub_tableau(const psnode_rk_tableau_f32* tab, int method, psnode_rk_tableau_f32& out) {
    if (tab) {
        out = *tab;
        return rk_tableau_check(tab);
    }
    if (method < PSNODE_EULER || method > PSNODE_RK4_38) return PSNODE_ERR_METHOD;
    memset(&out, 0, sizeof(out));
    out.stages = rk_stages(method);
    for (int s = 0; s < out.stages; ++s) {
        out.b[s] = rk_b(method, s);
        for (int j = 0; j < s; ++j) out.a[s][j] = rk_a(method, s, j);
    }
    return PSNODE_OK;
}

int substeps_check(const psnode_substeps_f32* sub) {
    if (!sub) return PSNODE_ERR_NULL;
    return sub->substeps < 1 || sub->substeps > 1024 ? PSNODE_ERR_DIMS : PSNODE_OK;
}

int act_from_abi(const psnode_act_f32* in, ActDev& out, bool& is_elu1) {
    out = ActDev{PSNODE_ACT_ELU, 1.0f, 1.0f, 20.0f, 1.0f};
    is_elu1 = true;
    if (!in) return PSNODE_OK;
    const bool pre = in->kind >= PSNODE_ACT_SILU && in->kind <= PSNODE_ACT_MISH;      // (no parameters: alpha / beta / threshold ignored)
    if ((in->kind < PSNODE_ACT_ELU || in->kind > PSNODE_ACT_SOFTPLUS) && !pre) return PSNODE_ERR_METHOD;
    out.kind = in->kind;
    out.alpha = 0.0f;
    switch (in->kind) {
        case PSNODE_ACT_ELU:
            if (!isfinite(in->alpha) || !(in->alpha > 0.0f)) return PSNODE_ERR_DIMS;
            out.alpha = in->alpha;
            break;
        case PSNODE_ACT_LEAKY_RELU:
            if (!isfinite(in->alpha) || !(in->alpha >= 0.0f)) return PSNODE_ERR_DIMS;
            out.alpha = in->alpha;
            break;
        case PSNODE_ACT_SOFTPLUS:
            if (!isfinite(in->beta) || !(in->beta > 0.0f) || !isfinite(in->threshold)) return PSNODE_ERR_DIMS;
            out.beta = in->beta;
            out.thr = in->threshold;
            out.ibeta = 1.0f / in->beta;
            break;
        default: break;
    }
    is_elu1 = in->kind == PSNODE_ACT_ELU && in->alpha == 1.0f;
    return PSNODE_OK;
}

}  // namespace psnode

using namespace psnode;

extern "C" {

int32_t psnode_abi_version(void) { return PSNODE_ABI_VERSION; }

const char* psnode_build_info(void) { return "psnode_hip abi " PSNODE_STR(PSNODE_ABI_VERSION) " gfx950 (generic + mfma kernels), built " __DATE__; }

const char* psnode_status_string(int32_t s) {
    switch (s) {
        case PSNODE_OK: return "ok";
        case PSNODE_ERR_NULL: return "required pointer is NULL";
        case PSNODE_ERR_DIMS: return "bad or inconsistent dimensions";
        case PSNODE_ERR_METHOD: return "unknown integration method";
        case PSNODE_ERR_WORKSPACE: return "workspace missing, misaligned (256 B) or too small";
        case PSNODE_ERR_UNSUPPORTED: return "shape not supported by the requested kernel";
        case PSNODE_ERR_HIP: return "HIP runtime error";
        default: return "unknown status";
    }
}

size_t psnode_workspace_bytes(const psnode_mlp_f32* de, const psnode_mlp_f32* ae) {
    if (!de || de->n_layers > kMaxLayers || (ae && ae->n_layers > kMaxLayers)) return 0;      // (the layout fills an MlpDev per MLP)
    MlpDev dde, dae;
    Arena A;
    return forward_layout(*de, ae, dde, dae, A), A.bytes();
}

int32_t psnode_event_table_f32(int64_t n_steps, const float* clock, int64_t stride_k, const float* event_times,
                               int64_t stride_e, int32_t n_events, int32_t* event_idx, int32_t* dup_flag, void* stream) {
    if (n_steps <= 0) return PSNODE_OK;
    if (!clock || !event_idx || (n_events > 0 && !event_times)) return PSNODE_ERR_NULL;
    if (n_events < 0) return PSNODE_ERR_DIMS;
    const unsigned grid = (unsigned)((n_steps + 255) / 256);
    hipLaunchKernelGGL(event_table_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)n_steps, clock,
                       (long long)stride_k, event_times, (long long)stride_e, (int)n_events, event_idx, dup_flag);
    return ok_or_hip(hipGetLastError());
}

int32_t psnode_ode_save_hidden(const psnode_ode_args_f32* a) {
    return !a || a->kernel == PSNODE_KERNEL_GENERIC ? 0 : mfma_ode_save_hidden(dims_only(*a));
}

int32_t psnode_ode_integrate_f32(const psnode_ode_args_f32* args, void* workspace, size_t workspace_bytes, void* stream) {
    IntegrateDev d;
    const int rc = fill_ode(args, d);
    if (rc) return rc;
    // only K1 proper / K3c write the training side outputs (checked with the pointers in place: alignment counts)
    if (d.sact && (args->kernel == PSNODE_KERNEL_GENERIC || !mfma_ode_save_hidden(d))) return PSNODE_ERR_UNSUPPORTED;
    return dispatch(d, false, args->kernel, &args->de, nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), K0Call{});
}

int32_t psnode_dae_save_hidden(const psnode_dae_args_f32* a) {
    return !a || a->kernel == PSNODE_KERNEL_GENERIC ? 0 : mfma_dae_save_hidden(dims_only(*a));
}

int32_t psnode_dae_integrate_f32(const psnode_dae_args_f32* args, void* workspace, size_t workspace_bytes, void* stream) {
    IntegrateDev d;
    const int rc = fill_dae(args, d);
    if (rc) return rc;
    // only K2 proper writes the training side outputs
    if (d.sact && (args->kernel == PSNODE_KERNEL_GENERIC || !mfma_dae_save_hidden(d))) return PSNODE_ERR_UNSUPPORTED;
    return dispatch(d, true, args->kernel, &args->de, &args->ae, workspace, workspace_bytes, static_cast<hipStream_t>(stream), K0Call{});
}

// ---- the K0 families (their table and the order of their checks: psnode_generic_family.h).  Each wrapper names its family and what it takes.
int32_t psnode_ode_integrate_act_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act) {
    return k0_supported(kFamAct, a, {de_act});
}
int32_t psnode_ode_integrate_act_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamAct, args, {de_act}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_act_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act) {
    return k0_supported(kFamAct, a, {de_act, ae_act});
}
int32_t psnode_dae_integrate_act_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act, void* ws,
                                     size_t bytes, void* stream) {
    return k0_integrate(kFamAct, args, {de_act, ae_act}, ws, bytes, stream);
}

int32_t psnode_ode_integrate_rk_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab) {
    return k0_supported(kFamRk, a, {de_act, nullptr, tab});
}
int32_t psnode_ode_integrate_rk_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab, void* ws,
                                    size_t bytes, void* stream) {
    return k0_integrate(kFamRk, args, {de_act, nullptr, tab}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_rk_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab) {
    return k0_supported(kFamRk, a, {de_act, ae_act, tab});
}
int32_t psnode_dae_integrate_rk_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamRk, args, {de_act, ae_act, tab}, ws, bytes, stream);
}

int32_t psnode_ode_integrate_sub_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub) {
    return k0_supported(kFamSub, a, {de_act, nullptr, tab, sub});
}
int32_t psnode_ode_integrate_sub_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamSub, args, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_sub_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k0_supported(kFamSub, a, {de_act, ae_act, tab, sub});
}
int32_t psnode_dae_integrate_sub_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamSub, args, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

int32_t psnode_ode_integrate_lin_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub) {
    return k0_supported(kFamLin, a, {de_act, nullptr, tab, sub});
}
int32_t psnode_ode_integrate_lin_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamLin, args, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_lin_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k0_supported(kFamLin, a, {de_act, ae_act, tab, sub});
}
int32_t psnode_dae_integrate_lin_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamLin, args, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

// (per-trajectory events: the args' event_idx is the [T-1, B] table of psnode_event_table_pt_f32)
int32_t psnode_ode_integrate_pev_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub) {
    return k0_supported(kFamPev, a, {de_act, nullptr, tab, sub});
}
int32_t psnode_ode_integrate_pev_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamPev, args, {de_act, nullptr, tab, sub}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_pev_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub) {
    return k0_supported(kFamPev, a, {de_act, ae_act, tab, sub});
}
int32_t psnode_dae_integrate_pev_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamPev, args, {de_act, ae_act, tab, sub}, ws, bytes, stream);
}

// (two-step Adams-Bashforth: per_trajectory says whether a non-NULL event_idx is the [T-1, B] table or the shared [T-1])
int32_t psnode_ode_integrate_ab_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act) {
    return k0_supported(kFamAb, a, {de_act});
}
int32_t psnode_ode_integrate_ab_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* ws, size_t bytes,
                                    void* stream) {
    return k0_integrate(kFamAb, args, {de_act, nullptr, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_ab_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act) {
    return k0_supported(kFamAb, a, {de_act, ae_act});
}
int32_t psnode_dae_integrate_ab_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    int32_t per_trajectory, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamAb, args, {de_act, ae_act, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}

// (four-point Lagrange externals: the _lin family's prototypes and order of checks, plus the stencil table -- NULL: one piece 0 .. T - 1)
int32_t psnode_ode_integrate_lag_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st) {
    return k0_supported(kFamLag, a, {de_act, nullptr, tab, sub, nullptr, 0, nullptr, st});
}
int32_t psnode_ode_integrate_lag_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamLag, args, {de_act, nullptr, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_lag_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st) {
    return k0_supported(kFamLag, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st});
}
// (stage-wise algebraic heads, DAE only: the _lag family's prototypes and order of checks plus `interp`, which picks the interpolant and
//  with it the _lin or the _lag row on the stage-heads builds; the table is read under PSNODE_EXT_LAGRANGE alone)
int32_t psnode_dae_integrate_sth_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st,
                                           int32_t interp) {
    Family fam;
    return sth_family(interp, fam) ? k0_supported(fam, a, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}) : 0;
}
int32_t psnode_dae_integrate_sth_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st,
                                     int32_t interp, void* ws, size_t bytes, void* stream) {
    Family fam;
    if (!sth_family(interp, fam)) return PSNODE_ERR_METHOD;
    return k0_integrate(fam, args, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_lag_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* st, void* ws,
                                     size_t bytes, void* stream) {
    return k0_integrate(kFamLag, args, {de_act, ae_act, tab, sub, nullptr, 0, nullptr, st}, ws, bytes, stream);
}

// (three-step Adams-Bashforth with the Heun restart step: the _ab family's prototypes and order of checks)
int32_t psnode_ode_integrate_ab3_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act) {
    return k0_supported(kFamAb3, a, {de_act});
}
int32_t psnode_ode_integrate_ab3_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* ws, size_t bytes,
                                    void* stream) {
    return k0_integrate(kFamAb3, args, {de_act, nullptr, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_ab3_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act) {
    return k0_supported(kFamAb3, a, {de_act, ae_act});
}
int32_t psnode_dae_integrate_ab3_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    int32_t per_trajectory, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamAb3, args, {de_act, ae_act, nullptr, nullptr, nullptr, per_trajectory}, ws, bytes, stream);
}

// (Runge-Kutta-Chebyshev: one s-stage step per grid interval; the _sub family's checks with the stage count in the sub-steps' place)
int32_t psnode_ode_integrate_rkc_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc) {
    psnode_substeps_f32 s;
    return k0_supported(kFamRkc, a, {de_act, nullptr, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc});
}
int32_t psnode_ode_integrate_rkc_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc, void* ws, size_t bytes,
                                     void* stream) {
    psnode_substeps_f32 s;
    return k0_integrate(kFamRkc, args, {de_act, nullptr, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_rkc_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rkc_f32* rkc) {
    psnode_substeps_f32 s;
    return k0_supported(kFamRkc, a, {de_act, ae_act, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc});
}
int32_t psnode_dae_integrate_rkc_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rkc_f32* rkc, void* ws, size_t bytes, void* stream) {
    psnode_substeps_f32 s;
    return k0_integrate(kFamRkc, args, {de_act, ae_act, nullptr, rkc_as_sub(rkc, s), nullptr, 0, nullptr, nullptr, rkc}, ws, bytes, stream);
}

// (multiple shooting: grid point k > 0 with k % seg->every == 0 restarts from row k of the args' x, which then holds all T rows)
int32_t psnode_ode_integrate_ms_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub, const psnode_segments_f32* seg) {
    return k0_supported(kFamMs, a, {de_act, nullptr, tab, sub, seg});
}
int32_t psnode_ode_integrate_ms_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, const psnode_segments_f32* seg, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamMs, args, {de_act, nullptr, tab, sub, seg}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_ms_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg) {
    return k0_supported(kFamMs, a, {de_act, ae_act, tab, sub, seg});
}
int32_t psnode_dae_integrate_ms_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg, void* ws,
                                    size_t bytes, void* stream) {
    return k0_integrate(kFamMs, args, {de_act, ae_act, tab, sub, seg}, ws, bytes, stream);
}

// (segments in parallel: the _ms call over a tiles x chunks grid, chunk c the grp->per_group consecutive segments from c per_group every on)
int32_t psnode_ode_integrate_msp_supported(const psnode_ode_args_f32* a, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp) {
    return k0_supported(kFamMsp, a, {de_act, nullptr, tab, sub, nullptr, 0, grp});
}
int32_t psnode_ode_integrate_msp_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp, void* ws, size_t bytes, void* stream) {
    return k0_integrate(kFamMsp, args, {de_act, nullptr, tab, sub, nullptr, 0, grp}, ws, bytes, stream);
}
int32_t psnode_dae_integrate_msp_supported(const psnode_dae_args_f32* a, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp) {
    return k0_supported(kFamMsp, a, {de_act, ae_act, tab, sub, nullptr, 0, grp});
}
int32_t psnode_dae_integrate_msp_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp, void* ws,
                                     size_t bytes, void* stream) {
    return k0_integrate(kFamMsp, args, {de_act, ae_act, tab, sub, nullptr, 0, grp}, ws, bytes, stream);
}

int32_t psnode_ode_kernel_for(const psnode_ode_args_f32* a) {
    if (!a) return PSNODE_ERR_NULL;
    IntegrateDev d = dims_only(*a);
    if (a->kernel == PSNODE_KERNEL_GENERIC || !mfma_ode_supported(d)) return PSNODE_KERNEL_GENERIC;
    d.sact = a->save_act;
    return mfma_x_ode_preferred(d) ? PSNODE_KERNEL_MFMA_WAVE : PSNODE_KERNEL_MFMA;      // (_WAVE: K1x -- the one-wave-per-4-trajectories integrator)
}

int32_t psnode_dae_kernel_for(const psnode_dae_args_f32* a) {
    if (!a) return PSNODE_ERR_NULL;
    IntegrateDev d = dims_only(*a);
    if (a->kernel == PSNODE_KERNEL_GENERIC || !mfma_dae_supported(d)) return PSNODE_KERNEL_GENERIC;
    d.sact = a->save_act;
    return mfma_x_dae_preferred(d) ? PSNODE_KERNEL_MFMA_WAVE : PSNODE_KERNEL_MFMA;      // (_WAVE: K2x)
}

}  // extern "C"

// ---- shared by every backward kernel: out[p] = sum over the per-workgroup partial vectors, in a fixed order (deterministic).
//      The first np_a entries go to out_a, the remaining np_b to out_b (out_b may be null when np_b == 0).
namespace psnode {
namespace {
// Two launches when there are many partial vectors (K8f: 1024 per-wave vectors of 1824 parameters = 44 us in one launch): the first sums
// each of kPartSlices slices INTO the slice's own first vector (in place -- the partials are the caller's scratch, exactly nparts vectors
// long, and a thread reads only its own column of its own slice), the second sums the slices' first vectors.
constexpr int kPartSlices = 16;
__device__ __forceinline__ float sum_parts(const float* __restrict__ part, const int np, const int pidx, const int q0, const int q1, const int qs) {
    // eight independent chains: one chain is (q1 - q0) / qs DEPENDENT loads; the order of the sum stays fixed
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int q = q0;
    for (; q + 8 * qs <= q1; q += 8 * qs) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += part[(size_t)(q + j * qs) * np + pidx];
    }
    for (int j = 0; q < q1; q += qs, ++j) acc[j] += part[(size_t)q * np + pidx];
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}
__global__ void reduce_partials_slices_kernel(float* __restrict__ part, int np, int nparts, int per) {
    const int pidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= np) return;
    const int q0 = blockIdx.y * per, q1 = q0 + per < nparts ? q0 + per : nparts;
    if (q0 >= nparts) return;
    part[(size_t)q0 * np + pidx] = sum_parts(part, np, pidx, q0, q1, 1);
}
__global__ void reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out_a, float* __restrict__ out_b, int np_a,
                                       int np_b, int nparts, int stride) {
    const int pidx = blockIdx.x * blockDim.x + threadIdx.x, np = np_a + np_b;
    if (pidx >= np) return;
    const float total = sum_parts(part, np, pidx, 0, nparts, stride);
    if (pidx < np_a) out_a[pidx] = total;
    else out_b[pidx - np_a] = total;
}
}  // namespace
hipError_t launch_reduce_partials(float* part, float* out_a, float* out_b, int np_a, int np_b, int nparts, hipStream_t s) {
    const int np = np_a + np_b;
    int stride = 1;
    if (nparts >= 8 * kPartSlices) {       // many vectors: sum kPartSlices slices in place first (the partials are scratch: nothing reads them again)
        stride = (nparts + kPartSlices - 1) / kPartSlices;
        hipLaunchKernelGGL(reduce_partials_slices_kernel, dim3((np + 63) / 64, kPartSlices), dim3(64), 0, s, part, np, nparts, stride);
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((np + 63) / 64), dim3(64), 0, s, part, out_a, out_b, np_a, np_b, nparts, stride);   // 64-wide: more CUs
    return hipGetLastError();
}
}  // namespace psnode
