// K6 with a pointwise loss other than the squared error -- L1, SmoothL1(beta), Huber(delta) -- and the per-sample evaluation form of all
// four kinds: instances of the tile walk of psnode_loss_tile.h (the squared-error training kernels are psnode_loss.hip's).
//   training form    out[d] = scale * inv_norm * col_weight[d] * sum_{t,b} mask * rho(pred - target), the t = 0 term, the total, and
//                    grad_pred; K6's partial rows and K6's double-precision finish (launch_loss_finish)
//   per-sample form  out[b,d] = sum_t rho(pred * m - target * m): evalute_model's
//                    `torch.sum(Loss_func(x_pred * mask, x * mask, reduction='none'), dim=1)` (neural_00_ODE_01_no_encode.py:123)
// The kind is a template parameter of the kernel, beta / delta a launch-uniform float of the device struct.
#include <cmath>

#include "psnode_loss_tile.h"

namespace psnode {
namespace {

template <class P, bool PS>
using KindKernels = LossKernels<P, LossDevP, PS>;

// f(policy{}) for the kind of a checked fn.  MSE: the per-sample form has a squared-error instance here, the training form does not (its
// squared-error kernels are psnode_loss.hip's, and the entry point forwards to them).
template <bool MSE, class F>
auto with_kind(int kind, F&& f) {
    switch (kind) {
        case PSNODE_LOSS_L1: return f(RhoL1{});
        case PSNODE_LOSS_SMOOTH_L1: return f(RhoSmoothL1{});
        default:
            if constexpr (MSE) {
                if (kind == PSNODE_LOSS_MSE) return f(RhoMse{});
            }
            return f(RhoHuber{});
    }
}

bool has_param(int kind) { return kind == PSNODE_LOSS_SMOOTH_L1 || kind == PSNODE_LOSS_HUBER; }

// kind 0..3; beta / delta of kinds 2 and 3 finite and > 0
bool fn_ok(const psnode_loss_fn_f32* fn) {
    if (fn->kind < PSNODE_LOSS_MSE || fn->kind > PSNODE_LOSS_HUBER) return false;
    return !has_param(fn->kind) || (std::isfinite(fn->param) && fn->param > 0.0f);
}

void bind_fn(LossDevP& d, const psnode_loss_fn_f32* fn) {
    const bool p = fn && has_param(fn->kind);
    d.prm = p ? fn->param : 1.0f;
    d.iprm = p ? (float)(1.0 / (double)fn->param) : 1.0f;
}

// the per-sample form has no weights, no normalisation, no t = 0 term and no gradient
bool plain_args(const psnode_loss_args_f32* a) {
    return !a->col_weight && !a->inv_norm && a->scale == 1.0f && a->t0_coef == 0.0f && !a->grad_pred;
}

}  // namespace
}  // namespace psnode

using namespace psnode;

// Order of the checks of the three entry points, all before any launch:
//   | args == NULL                                                      | PSNODE_ERR_NULL        |
//   | fn != NULL: kind outside 0..3; kinds 2, 3: param <= 0, NaN, inf   | PSNODE_ERR_UNSUPPORTED |
//   | per-sample only: col_weight / inv_norm / grad_pred set,           | PSNODE_ERR_UNSUPPORTED |
//   |                  scale != 1, t0_coef != 0                         |                        |
//   | K6's own, in K6's order (loss_call_dev): T, B, D < 1, mask_width  | PSNODE_ERR_DIMS        |
//   |   D > 64                                                          | PSNODE_ERR_UNSUPPORTED |
//   |   pred / target / out (/ mask) pointer NULL                       | PSNODE_ERR_NULL        |
//   |   more than 2^31 - 1 tiles                                        | PSNODE_ERR_UNSUPPORTED |
//   | training form only: workspace NULL, short or not 16-B aligned     | PSNODE_ERR_WORKSPACE   |
// fn == NULL is the squared error.  psnode_masked_loss_supported answers 1 exactly where psnode_masked_loss_f32 gets past the pointer and
// tile rows, i.e. where a call with a workspace of psnode_masked_mse_workspace_bytes(args) launches.
static int32_t loss_args_status(const psnode_loss_args_f32* a, const psnode_loss_fn_f32* fn, bool per_sample, LossDevP& d) {
    if (!a) return PSNODE_ERR_NULL;
    if (fn && !fn_ok(fn)) return PSNODE_ERR_UNSUPPORTED;
    if (per_sample && !plain_args(a)) return PSNODE_ERR_UNSUPPORTED;
    const int st = loss_call_dev(a, d);
    if (st != PSNODE_OK) return st;
    bind_fn(d, fn);
    return PSNODE_OK;
}

extern "C" int32_t psnode_masked_loss_supported(const psnode_loss_args_f32* a, const psnode_loss_fn_f32* fn) {
    LossDevP d;
    return loss_args_status(a, fn, false, d) == PSNODE_OK ? 1 : 0;
}

extern "C" int32_t psnode_masked_loss_f32(const psnode_loss_args_f32* a, const psnode_loss_fn_f32* fn, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    LossDevP d;
    const int32_t st = loss_args_status(a, fn, false, d);
    if (st != PSNODE_OK) return st;
    if (!fn || fn->kind == PSNODE_LOSS_MSE) return psnode_masked_mse_f32(a, workspace, workspace_bytes, stream);   // K6 itself, bit for bit
    if (!loss_workspace_ok(workspace, workspace_bytes, loss_partial_bytes(a, d))) return PSNODE_ERR_WORKSPACE;
    d.partial = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long rows = 0;
    const hipError_t e = with_kind<false>(fn->kind, [&](auto p) { return launch_loss_tiles<KindKernels<decltype(p), false>>(a, d, s, &rows); });
    if (e != hipSuccess) return PSNODE_ERR_HIP;
    return ok_or_hip(launch_loss_finish(d.partial, rows, a->D, a->out, s));
}

extern "C" int32_t psnode_loss_per_sample_f32(const psnode_loss_args_f32* a, const psnode_loss_fn_f32* fn, void* stream) {
    LossDevP d;
    const int32_t st = loss_args_status(a, fn, true, d);
    if (st != PSNODE_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long rows = 0;
    return ok_or_hip(with_kind<true>(fn ? fn->kind : PSNODE_LOSS_MSE,
                               [&](auto p) { return launch_loss_tiles<KindKernels<decltype(p), true>>(a, d, s, &rows); }));
}
