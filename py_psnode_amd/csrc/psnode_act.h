// Hidden-layer activations other than ELU(1) for the generic kernels K0 (psnode_generic_impl.h) and K5 (psnode_generic_bwd_impl.h).
//
// The ELU(1) kernels of both files do not see any of this: they keep elu_quad / elu_grad_quad (psnode_common.h).  The activation kernels
// (the same sources compiled a second time under the BuildAct policy, psnode_generic_act.hip / psnode_generic_bwd_act.hip) take an
// ActDev per MLP as a kernel argument and switch on its kind, which is uniform over the launch (scalar branches, no divergence).
//
// Every listed activation but one has a derivative that is a function of the layer OUTPUT h (K5 rebuilds and keeps layer outputs, not
// pre-activations):
//   ELU(alpha)              x > 0 ? x : alpha (e^x - 1)                          h > 0 ? 1 : h + alpha
//   Tanh                    tanh x                                               1 - h^2
//   Sigmoid                 1 / (1 + e^-x)                                       h (1 - h)
//   ReLU                    max(x, 0)                                            h > 0 ? 1 : 0        (torch's rule at 0)
//   LeakyReLU(s), s >= 0    x > 0 ? x : s x                                      h > 0 ? 1 : s
//   Softplus(beta, thr)     beta x > thr ? x : log(1 + e^(beta x)) / beta        beta h > thr ? 1 : 1 - e^(-beta h)     (thr >= 24 ln 2 only)
// Softplus is the exception.  Torch decides its derivative on the INPUT (beta x > thr ? 1 : sigmoid(beta x)), and the forward jumps at
// beta x = thr from log1p(e^thr) down to thr, so h is not monotonic in x: for beta x in (log(e^thr - 1), thr] the rule on h above returns 1
// where torch returns sigmoid(beta x), an error of up to e^-thr (0.37 at thr = 1; every x <= 0 at thr <= 0).  That is below fp32
// resolution (2^-24) only from thr >= 24 ln 2 = 16.64 (kSoftplusCut): a Softplus with such a threshold (torch's default 20) keeps the rule
// on h in the act build, any other runs K5's pre build (act_keeps_u), which keeps u and takes beta u > thr ? 1 : 1 / (1 + e^(-beta u))
// (softplus_grad_u: free of cancellation on both sides; e^(-beta u) = inf gives 0).  The builds that keep u for every kind (tableau,
// sub-steps, linear externals) take that form for every threshold.
// Accuracy (DESIGN.md "Activations"): the exponentials go through v_exp_f32 (exp2, 1 ulp), the reciprocals through v_rcp_f32 (1 ulp),
// the logarithm through v_log_f32.  Each value carries an ABSOLUTE error of about 1e-7, the same budget as the round-3 ELU form that the
// ELU(1) kernels ship (psnode_common.h).
#pragma once
#include "psnode_common.h"
#include "psnode_generic_build.h"

namespace psnode {

struct ActDev {
    int kind;          // psnode_act_kind
    float alpha;       // ELU: alpha, LeakyReLU: negative slope
    float beta, thr;   // Softplus
    float ibeta;       // Softplus: 1 / beta
};
struct ActPair {
    ActDev de, ae;
};

constexpr float kLn2 = 0.693147180559945309f;

__device__ __forceinline__ float act_exp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// one value; `a.kind` is uniform
__device__ __forceinline__ float act1(float x, const ActDev& a) {
    switch (a.kind) {
        case PSNODE_ACT_ELU: {
            // max(x, 0) + alpha (clamp(e^x, 0, 1) - 1): for x > 0 the exponential side is alpha (1 - 1) = 0 exactly (as elu_quad)
            const float t = __builtin_amdgcn_fmed3f(act_exp(x), 0.0f, 1.0f);
            return fmaxf(x, 0.0f) + a.alpha * (t - 1.0f);
        }
        case PSNODE_ACT_TANH: {
            // tanh |x| = (1 - t) / (1 + t), t = e^(-2|x|) in (0, 1]: 1 - t is exact for t >= 0.5 (Sterbenz), no overflow for any x
            const float t = __builtin_amdgcn_exp2f(-2.0f * kLog2e * fabsf(x));
            return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
        }
        case PSNODE_ACT_SIGMOID:
            return __builtin_amdgcn_rcpf(1.0f + act_exp(-x));      // e^-x = inf -> rcp(inf) = 0
        case PSNODE_ACT_RELU:
            return fmaxf(x, 0.0f);
        case PSNODE_ACT_LEAKY_RELU:
            return x > 0.0f ? x : x * a.alpha;
        default: {      // PSNODE_ACT_SOFTPLUS
            const float y = x * a.beta;
            // log1p(t) = log(u) t / (u - 1), u = 1 + t (exact where u rounds to 1: then log1p(t) = t to fp32 precision)
            const float t = act_exp(y), u = 1.0f + t;
            const float l1p = u == 1.0f ? t : __builtin_amdgcn_logf(u) * kLn2 * (t * __builtin_amdgcn_rcpf(u - 1.0f));
            return (y > a.thr || y > 80.0f) ? x : l1p * a.ibeta;     // (y > 80: e^y overflows; the limit is x)
        }
    }
}

typedef float act_f4 __attribute__((ext_vector_type(4)));
// the quad forms branch ONCE on the kind (K0 runs one wave per SIMD: nothing hides a taken branch, DESIGN.md "Activations")
template <int KIND>
__device__ __forceinline__ act_f4 act_quad_k(const act_f4 v, const ActDev& a) {
    ActDev k = a;
    k.kind = KIND;
    return act_f4{act1(v[0], k), act1(v[1], k), act1(v[2], k), act1(v[3], k)};
}
__device__ __forceinline__ act_f4 act_quad(const act_f4 v, const ActDev& a) {
    switch (a.kind) {
        case PSNODE_ACT_ELU: return act_quad_k<PSNODE_ACT_ELU>(v, a);
        case PSNODE_ACT_TANH: return act_quad_k<PSNODE_ACT_TANH>(v, a);
        case PSNODE_ACT_SIGMOID: return act_quad_k<PSNODE_ACT_SIGMOID>(v, a);
        case PSNODE_ACT_RELU: return act_quad_k<PSNODE_ACT_RELU>(v, a);
        case PSNODE_ACT_LEAKY_RELU: return act_quad_k<PSNODE_ACT_LEAKY_RELU>(v, a);
        default: return act_quad_k<PSNODE_ACT_SOFTPLUS>(v, a);
    }
}

// d act / d pre-activation, from the output h
__device__ __forceinline__ float act_grad1(float h, const ActDev& a) {
    switch (a.kind) {
        case PSNODE_ACT_ELU: return h > 0.0f ? 1.0f : h + a.alpha;
        case PSNODE_ACT_TANH: return 1.0f - h * h;
        case PSNODE_ACT_SIGMOID: return h * (1.0f - h);
        case PSNODE_ACT_RELU: return h > 0.0f ? 1.0f : 0.0f;
        case PSNODE_ACT_LEAKY_RELU: return h > 0.0f ? 1.0f : a.alpha;
        default: {      // PSNODE_ACT_SOFTPLUS
            const float y = h * a.beta;
            return y > a.thr ? 1.0f : 1.0f - act_exp(-y);
        }
    }
}
template <int KIND>
__device__ __forceinline__ act_f4 act_grad_quad_k(const act_f4 h, const ActDev& a) {
    ActDev k = a;
    k.kind = KIND;
    return act_f4{act_grad1(h[0], k), act_grad1(h[1], k), act_grad1(h[2], k), act_grad1(h[3], k)};
}
__device__ __forceinline__ act_f4 act_grad_quad(const act_f4 h, const ActDev& a) {
    switch (a.kind) {
        case PSNODE_ACT_ELU: return act_grad_quad_k<PSNODE_ACT_ELU>(h, a);
        case PSNODE_ACT_TANH: return act_grad_quad_k<PSNODE_ACT_TANH>(h, a);
        case PSNODE_ACT_SIGMOID: return act_grad_quad_k<PSNODE_ACT_SIGMOID>(h, a);
        case PSNODE_ACT_RELU: return act_grad_quad_k<PSNODE_ACT_RELU>(h, a);
        case PSNODE_ACT_LEAKY_RELU: return act_grad_quad_k<PSNODE_ACT_LEAKY_RELU>(h, a);
        default: return act_grad_quad_k<PSNODE_ACT_SOFTPLUS>(h, a);
    }
}

// Softplus' from the pre-activation u (torch's rule): the pre build's form, and the only correct one below kSoftplusCut (head of this file)
constexpr float kSoftplusCut = 16.6355323f;      // 24 ln 2: from here e^-thr < 2^-24 and the rule on h is torch's to fp32 precision
__device__ __forceinline__ float softplus_grad_u(float u, const ActDev& a) {
    const float y = u * a.beta;
    return y > a.thr ? 1.0f : __builtin_amdgcn_rcpf(1.0f + act_exp(-y));
}
__device__ __forceinline__ act_f4 softplus_grad_u_quad(const act_f4 u, const ActDev& a) {
    return act_f4{softplus_grad_u(u[0], a), softplus_grad_u(u[1], a), softplus_grad_u(u[2], a), softplus_grad_u(u[3], a)};
}

// wave-uniform copy (the kind drives scalar branches; selects between the DE's and the AE's act stay scalar)
__device__ __forceinline__ ActDev act_pick(bool first, const ActDev& x, const ActDev& y) {
    auto u = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    ActDev r;
    r.kind = __builtin_amdgcn_readfirstlane(first ? x.kind : y.kind);
    r.alpha = u(first ? x.alpha : y.alpha);
    r.beta = u(first ? x.beta : y.beta);
    r.thr = u(first ? x.thr : y.thr);
    r.ibeta = u(first ? x.ibeta : y.ibeta);
    return r;
}

// ---- the pre-activation family (kind >= PSNODE_ACT_PRE_FAMILY): SiLU, GELU (erf / tanh form), Mish.  Their derivatives are functions of the
// PRE-activation u, not of h, so K5 keeps u for them (its pre build: psnode_generic_bwd_pre.hip).  New functions, kept out of act_quad /
// act_grad_quad, so that the six-kind kernels keep their instruction stream.  Every form below is finite for every finite u (|u| up to the
// fp32 range: each exponential that can overflow is taken of a non-positive argument or guarded, and GELU(tanh)' clamps u^2 at 1e4 --
// e^(-2|z|) is exactly 0 from |u| = 11 up, so the clamp changes no value and keeps 0 * (1 + 3 k u^2) from becoming 0 * inf beyond
// |u| = 1.8e19) and keeps the ~1e-7 absolute budget:
//   SiLU        u s,  s = 1 / (1 + e^-u)                          s (1 + u (1 - s)),  1 - s = e^-u s for u >= 0 (no cancellation)
//   GELU        u Phi(u),  Phi(u) = erfc(-u / sqrt 2) / 2          Phi(u) + u phi(u)   (erfc: no cancellation of 1 + erf for u < 0)
//   GELU(tanh)  u (1 + t) / 2,  t = tanh z,  z = c (u + k u^3)    (1 + t) / 2 + u (1 - t^2) c (1 + 3 k u^2) / 2
//               with e = e^(-2|z|), r = 1 / (1 + e):  (1 + t) / 2 = r (z < 0 ? e : 1),  1 - t^2 = 4 e r^2   (both free of cancellation)
//   Mish        u T,  T = tanh(softplus u) = n / (n + 2),  n = w (w + 2),  w = e^u     (T = 1 above u = 20, where n / (n + 2) rounds to 1)
//               T + u (1 - T^2) sigma(u),  1 - T^2 = 4 (n + 1) / (n + 2)^2,  sigma(u) = w / (1 + w)
//               (the closed form of tanh(log1p(e^u)): the log1p form loses 1 - e^(-2 sp) to cancellation where sp is small, ~1e-6 at u = -20)
constexpr float kSqrtHalf = 0.707106781186547524f, kInvSqrt2Pi = 0.398942280401432678f;
constexpr float kGeluC = 0.797884560802865355f, kGeluK = 0.044715f;     // sqrt(2 / pi), the cubic coefficient of GELU(tanh)

template <int KIND>
__device__ __forceinline__ float pre_act1_k(float u) {
    if constexpr (KIND == PSNODE_ACT_SILU) {
        return u * __builtin_amdgcn_rcpf(1.0f + act_exp(-u));           // e^-u = inf -> u * 0
    } else if constexpr (KIND == PSNODE_ACT_GELU) {
        return u * (0.5f * erfcf(-u * kSqrtHalf));
    } else if constexpr (KIND == PSNODE_ACT_GELU_TANH) {
        const float z = kGeluC * (u + kGeluK * u * u * u);
        const float e = __builtin_amdgcn_exp2f(-2.0f * kLog2e * fabsf(z)), r = __builtin_amdgcn_rcpf(1.0f + e);
        return u * (r * (z < 0.0f ? e : 1.0f));
    } else {    // PSNODE_ACT_MISH
        const float w = act_exp(fminf(u, 20.0f)), n = w * (w + 2.0f);
        return u * (u > 20.0f ? 1.0f : n * __builtin_amdgcn_rcpf(n + 2.0f));
    }
}
template <int KIND>
__device__ __forceinline__ float pre_grad1_k(float u) {
    if constexpr (KIND == PSNODE_ACT_SILU) {
        const float e = act_exp(-u), s = __builtin_amdgcn_rcpf(1.0f + e);
        const float oms = u >= 0.0f ? e * s : 1.0f - s;                 // 1 - s (e * s would be inf * 0 where e^-u overflows)
        return s * (1.0f + u * oms);
    } else if constexpr (KIND == PSNODE_ACT_GELU) {
        return 0.5f * erfcf(-u * kSqrtHalf) + u * (kInvSqrt2Pi * act_exp(-0.5f * u * u));
    } else if constexpr (KIND == PSNODE_ACT_GELU_TANH) {
        const float u2 = fminf(u * u, 1e4f), z = kGeluC * (u + kGeluK * u2 * u);      // (|u| > 100: z stays beyond +-3.5e4, e = 0)
        const float e = __builtin_amdgcn_exp2f(-2.0f * kLog2e * fabsf(z)), r = __builtin_amdgcn_rcpf(1.0f + e);
        return r * (z < 0.0f ? e : 1.0f) + (u * (2.0f * e * r * r)) * (kGeluC * (1.0f + 3.0f * kGeluK * u2));
    } else {    // PSNODE_ACT_MISH
        const float w = act_exp(fminf(u, 20.0f)), n = w * (w + 2.0f), q = __builtin_amdgcn_rcpf(n + 2.0f);
        const float sech2 = 4.0f * (n + 1.0f) * q * q, sg = w * __builtin_amdgcn_rcpf(1.0f + w);
        return u > 20.0f ? 1.0f : n * q + u * sech2 * sg;
    }
}
template <int KIND>
__device__ __forceinline__ act_f4 pre_act_quad_k(const act_f4 v) {
    return act_f4{pre_act1_k<KIND>(v[0]), pre_act1_k<KIND>(v[1]), pre_act1_k<KIND>(v[2]), pre_act1_k<KIND>(v[3])};
}
template <int KIND>
__device__ __forceinline__ act_f4 pre_grad_quad_k(const act_f4 u) {
    return act_f4{pre_grad1_k<KIND>(u[0]), pre_grad1_k<KIND>(u[1]), pre_grad1_k<KIND>(u[2]), pre_grad1_k<KIND>(u[3])};
}
// the pre build's forms over all ten kinds (an ActPair may mix the families): kinds < 32 are act1 / act_quad and take their derivative
// from h (the forms of act_grad1, the numbers of the act build) -- but Softplus, which takes it from u (softplus_grad_u) --, the family >= 32
// from u.  One branch per quad, as act_quad: pre_grad_quad switches over the six low kinds itself, Softplus in the default arm (a test for
// Softplus in front of act_grad_quad made the tableau build copy a VGPR to an AGPR under partial EXEC, which the ISA lint refuses).
__device__ __forceinline__ act_f4 pre_act_quad(const act_f4 v, const ActDev& a) {
    if (a.kind < PSNODE_ACT_PRE_FAMILY) return act_quad(v, a);
    switch (a.kind) {
        case PSNODE_ACT_SILU: return pre_act_quad_k<PSNODE_ACT_SILU>(v);
        case PSNODE_ACT_GELU: return pre_act_quad_k<PSNODE_ACT_GELU>(v);
        case PSNODE_ACT_GELU_TANH: return pre_act_quad_k<PSNODE_ACT_GELU_TANH>(v);
        default: return pre_act_quad_k<PSNODE_ACT_MISH>(v);
    }
}
__device__ __forceinline__ act_f4 pre_grad_quad(const act_f4 h, const act_f4 u, const ActDev& a) {
    if (a.kind < PSNODE_ACT_PRE_FAMILY) {
        switch (a.kind) {
            case PSNODE_ACT_ELU: return act_grad_quad_k<PSNODE_ACT_ELU>(h, a);
            case PSNODE_ACT_TANH: return act_grad_quad_k<PSNODE_ACT_TANH>(h, a);
            case PSNODE_ACT_SIGMOID: return act_grad_quad_k<PSNODE_ACT_SIGMOID>(h, a);
            case PSNODE_ACT_RELU: return act_grad_quad_k<PSNODE_ACT_RELU>(h, a);
            case PSNODE_ACT_LEAKY_RELU: return act_grad_quad_k<PSNODE_ACT_LEAKY_RELU>(h, a);
            default: return softplus_grad_u_quad(u, a);
        }
    }
    switch (a.kind) {
        case PSNODE_ACT_SILU: return pre_grad_quad_k<PSNODE_ACT_SILU>(u);
        case PSNODE_ACT_GELU: return pre_grad_quad_k<PSNODE_ACT_GELU>(u);
        case PSNODE_ACT_GELU_TANH: return pre_grad_quad_k<PSNODE_ACT_GELU_TANH>(u);
        default: return pre_grad_quad_k<PSNODE_ACT_MISH>(u);
    }
}
__device__ __forceinline__ float pre_act1(float x, const ActDev& a) {
    if (a.kind < PSNODE_ACT_PRE_FAMILY) return act1(x, a);
    switch (a.kind) {
        case PSNODE_ACT_SILU: return pre_act1_k<PSNODE_ACT_SILU>(x);
        case PSNODE_ACT_GELU: return pre_act1_k<PSNODE_ACT_GELU>(x);
        case PSNODE_ACT_GELU_TANH: return pre_act1_k<PSNODE_ACT_GELU_TANH>(x);
        default: return pre_act1_k<PSNODE_ACT_MISH>(x);
    }
}
__device__ __forceinline__ float pre_grad1(float h, float u, const ActDev& a) {
    if (a.kind < PSNODE_ACT_PRE_FAMILY) return a.kind == PSNODE_ACT_SOFTPLUS ? softplus_grad_u(u, a) : act_grad1(h, a);
    switch (a.kind) {
        case PSNODE_ACT_SILU: return pre_grad1_k<PSNODE_ACT_SILU>(u);
        case PSNODE_ACT_GELU: return pre_grad1_k<PSNODE_ACT_GELU>(u);
        case PSNODE_ACT_GELU_TANH: return pre_grad1_k<PSNODE_ACT_GELU_TANH>(u);
        default: return pre_grad1_k<PSNODE_ACT_MISH>(u);
    }
}
// a call with an activation of the pre-activation family on either MLP runs the pre build
inline bool act_pair_pre(const ActPair& p) { return p.de.kind >= PSNODE_ACT_PRE_FAMILY || p.ae.kind >= PSNODE_ACT_PRE_FAMILY; }
// K5 needs u for the derivative: the pre-activation family, and a Softplus whose threshold is below kSoftplusCut (head of this file).  Such a
// call runs K5's pre build; K0 keeps no u and asks act_pair_pre alone.
inline bool act_keeps_u(const ActDev& a) { return a.kind >= PSNODE_ACT_PRE_FAMILY || (a.kind == PSNODE_ACT_SOFTPLUS && !(a.thr >= kSoftplusCut)); }
inline bool act_pair_keeps_u(const ActPair& p) { return act_keeps_u(p.de) || act_keeps_u(p.ae); }

// psnode_capi.hip: validates a psnode_act_f32 and converts it (NULL = ELU(1)).  Returns PSNODE_OK / PSNODE_ERR_*; `is_elu1` = the
// existing ELU(1) routes apply.
int act_from_abi(const psnode_act_f32* in, ActDev& out, bool& is_elu1);
// the two activations of an _act call (the ODE's has ae = NULL); `elu1`: both are ELU(1), the call takes the entry point without _act
inline int act_pair(const psnode_act_f32* de, const psnode_act_f32* ae, ActPair& p, bool& elu1) {
    bool e_de = true, e_ae = true;
    int rc = act_from_abi(de, p.de, e_de);
    if (rc == PSNODE_OK) rc = act_from_abi(ae, p.ae, e_ae);
    elu1 = e_de && e_ae;
    return rc;
}

// psnode_generic.hip: K0's launch planning, shared by both builds
size_t generic_plan(const IntegrateDev& a, bool dae, unsigned& mask, int lin = 0);      // lin: 1 the linear-externals build's layout, 2 the Lagrange build's
int generic_reg_mode(const IntegrateDev& a, bool dae);
bool generic_wide_mode(const IntegrateDev& a, bool dae);
// What a K0 call carries beyond its args: the build of the generic kernel that runs it and that build's kernel arguments.  The plain entry
// points pass K0Call{}: ELU(1), the args' method, one step per interval -- the only call the MFMA kernels take.
struct K0Call {
    BuildId build;
    ActPair act;                   // every build but kBuildElu1
    psnode_rk_tableau_f32 rk;      // the builds with a tableau: given, or the args' method written as one (family_tableau)
    SubDev sub;                    // kBuildSub, kBuildLin, kBuildPev, kBuildMs: sub-steps per grid interval and x_sub
    int ev_pt, ms_every;           // kBuildAb: the event table is [T-1, B]; kBuildMs: grid point k > 0 with k % ms_every == 0 restarts from row k of x
    int per_group;                 // kBuildMsp: segments per time chunk (the grid is tiles x msp_chunks(T, ms_every, per_group))
    const signed char* stencil;    // kBuildLag: the stencil table int8 [T-1, B], or null (one piece 0 .. T - 1)
    const psnode_rkc_f32* rkc;     // kBuildRkc: the recurrence's coefficients (sub.n is its stage count, sub.x_sub its stage buffer)
};
// K0's launcher (psnode_generic_impl.h), instantiated once per build policy in that policy's object, as K5's generic_backward_launch<B>
// (psnode_common.h) is: reads of `call` what B's kernels take.  BuildPev: a.ev is the [T-1, B] table and not null; BuildMs, BuildMsp: a.x has all T rows.
template <class B>
hipError_t launch_generic(const IntegrateDev& a, bool dae, const K0Call& call, hipStream_t stream);

}  // namespace psnode
