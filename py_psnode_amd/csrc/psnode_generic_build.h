// The build policy of the generic kernels K0 (psnode_generic_impl.h) and K5 (psnode_generic_bwd_impl.h): what separates the objects each
// is compiled into, as constants the language can see.  Each object is one file that names its policy and includes the impl header:
//   #define PSNODE_BUILD BuildAct
//   #include "psnode_generic_impl.h"
// The kernel, its instance table and the launcher are written once, in the impl header; what a policy's kernels take behind their args struct
// follows from the policy (n_extra, Sub).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "psnode_hip.h"

namespace psnode {

// Sub-steps per grid interval (psnode_substeps_f32, include/psnode_hip.h), as the sub-step builds of K0 / K5 take them: one further kernel
// argument behind the tableau.  Every grid interval [t[k], t[k + 1]] runs n equal sub-steps; x_sub [T-1, n-1, B, xd] keeps the start state
// of sub-steps 1 .. n-1 of every interval (row (k, j - 1): sub-step j) -- written by K0 when the pointer is not null, read by K5.
struct SubDev {
    int n;
    float* x_sub;
};
// What the Adams-Bashforth builds of K0 / K5 take in SubDev's place (the bodies read it under the same name): one sub-step, no x_sub, and
// the shape of the event table -- ev_pt != 0: int32 [T-1, B], every trajectory its own column; 0: the shared int32 [T-1], which every
// column reads through a column stride of 0.  The table may be null (no events).
struct AbDev {
    int n;
    float* x_sub;
    int ev_pt;
};
// (the bodies ask through an overload: a discarded `if constexpr` arm of a non-dependent SubDev is still type-checked)
__host__ __device__ inline int ev_table_pt(const SubDev&) { return 0; }
__host__ __device__ inline int ev_table_pt(const AbDev& s) { return s.ev_pt; }
// What the multiple-shooting builds of K0 / K5 take in SubDev's place (psnode_segments_f32, include/psnode_hip.h): the sub-step build's
// argument plus `every` >= 1 -- grid point k > 0 with k % every == 0 restarts from the dataset row -- and, for K5, those rows x_true
// [T, B, xd] (K0 reads IntegrateDev::x, psnode_common.h; null where no step restarts).
struct MsDev {
    int n;
    float* x_sub;
    int every;
    const float* x_true;
};
__host__ __device__ inline int ev_table_pt(const MsDev&) { return 0; }
// What the Lagrange-externals builds of K0 / K5 take in SubDev's place: the sub-step build's argument plus the stencil table
// (psnode_ext_stencil_f32, include/psnode_hip.h) -- int8 [T-1, B], one code byte per grid interval and trajectory; null: one piece
// 0 .. T - 1 for every trajectory.
struct LagDev {
    int n;
    float* x_sub;
    const signed char* stencil;
};
__host__ __device__ inline int ev_table_pt(const LagDev&) { return 0; }
// What the Runge-Kutta-Chebyshev builds of K0 / K5 take in SubDev's place (psnode_rkc_f32, include/psnode_hip.h): n is the stage count of the
// ONE step every grid interval takes, x_sub [T-1, n-1, B, xd] keeps Y_1 .. Y_{n-1} of every interval (row (k, j - 1): Y_j), and the five
// coefficient arrays of the recurrence (entry j - 1: stage j) travel with the argument -- a stage pass reads its row through rkc_coef.
constexpr int kRkcMaxStages = 32;
struct RkcDev {
    int n;
    float* x_sub;
    float kap[kRkcMaxStages], mu[kRkcMaxStages], nu[kRkcMaxStages], mut[kRkcMaxStages], gam[kRkcMaxStages];
};
__host__ __device__ inline int ev_table_pt(const RkcDev&) { return 0; }
template <class S> __host__ __device__ inline const signed char* lag_table(const S&) { return nullptr; }
__host__ __device__ inline const signed char* lag_table(const LagDev& s) { return s.stencil; }
// (asked through overloads for the reason above)
template <class S> __host__ __device__ inline int ms_every(const S&) { return 0; }
__host__ __device__ inline int ms_every(const MsDev& s) { return s.every; }
template <class S> __host__ __device__ inline const float* ms_x_true(const S&) { return nullptr; }
__host__ __device__ inline const float* ms_x_true(const MsDev& s) { return s.x_true; }
// What the segment-parallel builds of K0 / K5 take in MsDev's place (psnode_segment_groups_f32, include/psnode_hip.h): the multiple-shooting
// argument plus `per_group` >= 1 -- workgroup (tile, c = blockIdx.y) runs the steps of the per_group consecutive segments
// c per_group every .. min((c + 1) per_group every, T - 1) alone -- and, for K5, what crosses a chunk border (folded by the launch behind
// the sweep; workspace segments, gbwd_msp_layout): ga0_part [C - 1, B, n], the grad_all_initial partial of every chunk c > 0, and border
// [C - 1, B, zd + vd], the z | v part of the head VJP at grid point k_hi of every chunk c < C - 1 (a DAE's; that row is chunk c + 1's).
struct MspDev {
    int n;
    float* x_sub;
    int every;
    const float* x_true;
    int per_group;
    float* ga0_part;
    float* border;
};
__host__ __device__ inline int ev_table_pt(const MspDev&) { return 0; }
__host__ __device__ inline int ms_every(const MspDev& s) { return s.every; }
__host__ __device__ inline const float* ms_x_true(const MspDev& s) { return s.x_true; }
// the chunk of the calling workgroup: steps k_lo .. k_hi - 1 of a record of T grid points (k_lo < k_hi <= T - 1: the launcher's grid)
// (host) the chunks of a record: n_seg = ceil((T - 1) / every) segments in groups of per_group, at least one (a record without a step)
inline long long msp_chunks(long long T, long long every, long long per_group) {
    const long long n_seg = T > 1 ? (T - 1 + every - 1) / every : 0, C = (n_seg + per_group - 1) / per_group;
    return C > 1 ? C : 1;
}
struct MspChunk { long long k_lo, k_hi; };
template <class S> __device__ inline MspChunk msp_chunk(const S&, long long T) { return MspChunk{0, T - 1}; }
__device__ inline MspChunk msp_chunk(const MspDev& s, long long T) {
    const long long span = (long long)s.per_group * s.every, lo = (long long)blockIdx.y * span, hi = lo + span;
    return MspChunk{lo, hi < T - 1 ? hi : T - 1};
}
template <class S> __device__ inline float* msp_ga0_part(const S&) { return nullptr; }
__device__ inline float* msp_ga0_part(const MspDev& s) { return s.ga0_part; }
template <class S> __device__ inline float* msp_border(const S&) { return nullptr; }
__device__ inline float* msp_border(const MspDev& s) { return s.border; }


// The coefficients of step k of the Adams-Bashforth 3 builds (Bd::ab3) for one trajectory column, from h0, h1, h2 = h_k, h_{k-1}, h_{k-2},
// the step's restart flag R_k and `shallow` = R_{k-1} || h_{k-1} + h_{k-2} == 0 (depth 1).  One function for K0 and K5: the same
// expressions on the same values, so K5's coefficients are K0's bit for bit (the objects are built without contraction).  The order of
// operations is neural_dae.AB3._ab3_step's.  A restart step's c0 is h: the Euler predictor of its corrector.
struct Ab3Coef { float c0, c1, c2; };
__device__ __forceinline__ Ab3Coef ab3_coef(float h0, float h1, float h2, bool restart, bool shallow) {
    const float half_rho = (h0 / h1) / 2.0f;                       // depth 1: AB2's step
    const float g1 = h0 * h0 / 2.0f, g2 = h0 * h0 * h0 / 3.0f + h1 * g1, D = g2 / (h1 + h2);      // depth 2
    const float p = g1 / h1, q = D / h1, u = D / h2;
    Ab3Coef cf;
    cf.c0 = restart ? h0 : (shallow ? h0 * (1.0f + half_rho) : h0 + p + q);
    cf.c1 = restart ? 0.0f : (shallow ? -(h0 * half_rho) : -p - q - u);
    cf.c2 = (restart || shallow) ? 0.0f : u;
    return cf;
}

// The stencil of grid interval k of one trajectory column in the Lagrange-externals builds (Bd::lag): q = 2 .. 4 consecutive nodes from
// row s on, off = k - s; the value at theta is sum_m l_m(off + theta) node_{s+m}.  Decoded from the column's code byte (off in bits 0-1, q in
// bits 2-4), or, without a table, from k and T alone (one piece 0 .. T - 1).  Clamped so that no byte makes a kernel read outside rows
// 0 .. T - 1 (T >= 2 wherever an interval exists): 2 <= q <= min(4, T), 0 <= s <= T - q.
struct LagStencil { long long s; int q, off; };
// the column's code byte of interval k (a kernel loads it one interval ahead); without a table: q = 4 from k - 1 on, which lag_decode clamps
__device__ __forceinline__ int lag_code(const signed char* tab, long long k, long long B, long long b) {
    return tab ? (int)tab[k * B + b] : ((k > 0 ? 1 : 0) | (4 << 2));
}
__device__ __forceinline__ LagStencil lag_decode(int code, long long k, long long T) {
    int off = code & 3, q = (code >> 2) & 7;
    q = q < 2 ? 2 : (q > 4 ? 4 : q);
    if (q > T) q = (int)T;
    long long s = k - off;
    if (s + q > T) s = T - q;
    if (s < 0) s = 0;
    return LagStencil{s, q, (int)(k - s)};
}
__device__ __forceinline__ LagStencil lag_stencil(const signed char* tab, long long k, long long T, long long B, long long b) {
    return lag_decode(lag_code(tab, k, B, b), k, T);
}
// The weights l_m(u) = (prod_{r != m} (u - r)) / (prod_{r != m} (m - r)), u = off + theta, of the q nodes (0 beyond them): numerator and
// denominator each a product in increasing r from 1 -- the denominator a small integer --, one division per weight.  At theta = 0 and
// theta = 1 u is an integer, so the numerator is the denominator or 0 and the weights are exactly 1 / 0.  One function for K0 and K5:
// K5's weights are K0's bit for bit (the objects are built without contraction).  lag_eval: the sum in increasing m.
struct LagW { float w[4]; };
__device__ __forceinline__ LagW lag_weights(int off, int q, float theta) {
    const float u = (float)off + theta;
    LagW o;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float num = 1.0f;
        int den = 1;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r != m && r < q) { num = num * (u - (float)r); den = den * (m - r); }
        o.w[m] = m < q ? num / (float)den : 0.0f;
    }
    return o;
}
__device__ __forceinline__ float lag_eval(const LagW& w, int q, float n0, float n1, float n2, float n3) {
    float acc = w.w[0] * n0;
    acc = acc + w.w[1] * n1;
    if (q > 2) acc = acc + w.w[2] * n2;
    if (q > 3) acc = acc + w.w[3] * n3;
    return acc;
}

// The coefficients of stage j = j0 + 1 of the Runge-Kutta-Chebyshev builds (Bd::rkc), wave-uniform: Y_j = kap Y_0 + mu Y_{j-1} + nu Y_{j-2} +
// (mut h) F(Y_{j-1}) + (gam h) F_0; stage 1 reads mut alone.  One function for K0 and K5: the same values, read the same way.  j0 is
// launch-uniform (the stage loop's counter), so the reads are scalar loads from the kernel's argument segment.
struct RkcCoef { float kap, mu, nu, mut, gam; };
template <class S> __device__ __forceinline__ RkcCoef rkc_coef(const S&, int) { return RkcCoef{0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
__device__ __forceinline__ RkcCoef rkc_coef(const RkcDev& s, int j0) {
    auto u = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const int j = __builtin_amdgcn_readfirstlane(j0) & (kRkcMaxStages - 1);      // (the host checks the stage count; the mask keeps any index inside the arrays)
    return RkcCoef{u(s.kap[j]), u(s.mu[j]), u(s.nu[j]), u(s.mut[j]), u(s.gam[j])};
}

template <bool ACT, bool PRE, bool RK, bool SUB = false, bool LIN = false, bool PEV = false, bool AB = false, bool MS = false, bool PAR = false,
          bool AB3 = false, bool LAG = false, bool RKC = false, bool STH = false>
struct GenericBuild {
    static constexpr bool act = ACT;      // the hidden-layer activation is a kernel argument (ActPair, psnode_act.h), not ELU(1)
    static constexpr bool pre = PRE;      // the hidden layers' pre-activations u are kept next to h (SiLU / GELU / Mish differentiate from u)
    static constexpr bool rk = RK;        // the stage loops read a psnode_rk_tableau_f32 kernel argument instead of a.method
    static constexpr bool sub = SUB;      // every grid interval runs SubDev::n equal sub-steps (a further kernel argument, above)
    static constexpr bool lin = LIN;      // every stage reads z | v interpolated linearly between the interval's two grid points (needs sub)
    static constexpr bool pev = PEV;      // the event table is [T-1, B]: every trajectory jumps at its own steps (needs sub; not with lin)
    static constexpr bool ab = AB;        // two-step Adams-Bashforth: one DE evaluation per step, the previous slope and per-column c0 / c1 (AbDev;
                                          // needs pev, whose per-column event index also serves a shared table through a column stride of 0)
    static constexpr bool ms = MS;        // multiple shooting: every MsDev::every-th grid point restarts from the dataset row (MsDev;
                                          // needs sub; not with lin, pev or ab)
    static constexpr bool ab3 = AB3;      // three-step Adams-Bashforth with a predictor-corrector restart step: two previous slopes, per-column c0 / c1 / c2,
                                          // and on restart steps a second DE stage (a DAE: behind a head evaluation of its own) on the rows of grid
                                          // point k + 1 (AbDev; needs ab)
    static constexpr bool lag = LAG;      // the interpolant of lin is the polynomial through the up to four neighbouring dataset rows of the interval's
                                          // piece, by the stencil table (LagDev; needs lin)
    static constexpr bool rkc = RKC;      // every grid interval is one s-stage Runge-Kutta-Chebyshev step: the sub-step loop with one evaluation per pass, the
                                          // three-term recurrence in the sub-step update's place, h undivided (RkcDev; needs sub, a one-stage tableau)
    static constexpr bool sth = STH;      // stage-wise algebraic heads: a DAE's head i = g(X_s; z | v at theta_s) is evaluated in front of every stage s >= 1 of a
                                          // (sub-)step instead of being frozen over the stages (needs lin; DAE instances only; the layouts are lin's / lag's)
    static constexpr int lin_layout = LAG ? 2 : (LIN ? 1 : 0);      // the LDS layout the fit queries count: none, lin's regions, lag's
    static constexpr bool par = PAR;      // segments in parallel: the launch grid is tiles x chunks, workgroup (tile, c) runs the segments of time chunk c
                                          // alone (MspDev; needs ms)
    // The kernels' arguments behind the args struct, each a by-value parameter of its own: ActPair (act) | psnode_rk_tableau_f32 (rk) | Sub (sub).
    // A kernel without one of them names the never-read default of kernel_arg in its place.
    static constexpr int n_extra = SUB ? 3 : (RK ? 2 : (ACT ? 1 : 0));
    using Sub = std::conditional_t<RKC, RkcDev, std::conditional_t<LAG, LagDev, std::conditional_t<AB, AbDev, std::conditional_t<PAR, MspDev, std::conditional_t<MS, MsDev, SubDev>>>>>;
    // K5's waves per SIMD: the fully streamed instances (STR 2) that fitted 256 registers keep two workgroups per CU -- every one of the
    // act build, the ELU(1) build's with the accumulators in LDS, none of the builds that keep u
    static constexpr int two_waves(bool gg, int str) { return PRE ? 1 : (str == 2 && (ACT || !gg) ? 2 : 1); }
};
// The sub-step loop of both kernel bodies: `do { ... } while (si.more())` around what a step does per sub-step.  Without sub-steps it is one
// pass whose every question is a constant, so that the builds without them compile to the code they had before the loop existed.
template <bool SUB> struct SubIter {
    int n, i;
    __host__ __device__ explicit SubIter(int n_) : n(n_), i(0) {}
    __host__ __device__ bool first() const { return i == 0; }
    __host__ __device__ bool last() const { return i + 1 == n; }
    __host__ __device__ bool more() { return ++i < n; }
};
template <> struct SubIter<false> {
    static constexpr int i = 0;
    __host__ __device__ explicit constexpr SubIter(int) {}
    static constexpr bool first() { return true; }
    static constexpr bool last() { return true; }
    static constexpr bool more() { return false; }
};

// Kernel argument I behind the args struct: the I-th of `extra`, or -- the build takes fewer -- a local default that is never read
template <int I, class D> __host__ __device__ constexpr D kernel_arg(const D& dflt) { return dflt; }
template <int I, class D, class E0, class... E>
__host__ __device__ constexpr decltype(auto) kernel_arg(const D& dflt, const E0& e0, const E&... e) {
    if constexpr (I == 0) return (e0); else return kernel_arg<I - 1>(dflt, e...);
}
// The policy's Sub argument from what a call carries, for both directions (K0 writes x_sub and has no x_true; K5 reads both)
template <class B>
typename B::Sub build_sub(int n, float* x_sub, int ev_pt, int ms_every, const float* x_true, int per_group = 1, float* ga0_part = nullptr,
                          float* border = nullptr, const signed char* stencil = nullptr, const psnode_rkc_f32* rkc = nullptr) {
    if constexpr (B::rkc) {
        RkcDev r{};
        r.n = n;
        r.x_sub = x_sub;
        if (rkc)
            for (int j = 0; j < kRkcMaxStages; ++j) { r.kap[j] = rkc->kappa[j]; r.mu[j] = rkc->mu[j]; r.nu[j] = rkc->nu[j]; r.mut[j] = rkc->mu_t[j]; r.gam[j] = rkc->gamma_t[j]; }
        return r;
    } else
    if constexpr (B::lag) return LagDev{n, x_sub, stencil};
    else if constexpr (B::ab) return AbDev{1, nullptr, ev_pt};
    else if constexpr (B::par) return MspDev{n, x_sub, ms_every, x_true, per_group, ga0_part, border};
    else if constexpr (B::ms) return MsDev{n, x_sub, ms_every, x_true};
    else return SubDev{n, x_sub};
}

using BuildElu1 = GenericBuild<false, false, false>;
using BuildAct = GenericBuild<true, false, false>;
using BuildPre = GenericBuild<true, true, false>;
using BuildRk = GenericBuild<true, true, true>;
using BuildSub = GenericBuild<true, true, true, true>;      // BuildRk's policy with sub-steps: all ten activation kinds, the tableau
using BuildLin = GenericBuild<true, true, true, true, true>;      // BuildSub's policy with linearly interpolated externals; every substeps >= 1
using BuildPev = GenericBuild<true, true, true, true, false, true>;      // BuildSub's policy with per-trajectory events; every substeps >= 1
using BuildAb = GenericBuild<true, true, true, true, false, true, true>;      // BuildPev's policy as Adams-Bashforth 2; one sub-step, a one-stage tableau
using BuildMs = GenericBuild<true, true, true, true, false, false, false, true>;      // BuildSub's policy with multiple-shooting restarts; every substeps >= 1
using BuildMsp = GenericBuild<true, true, true, true, false, false, false, true, true>;      // BuildMs's policy with the segments spread over workgroups: a tiles x chunks grid
using BuildAb3 = GenericBuild<true, true, true, true, false, true, true, false, false, true>;      // BuildAb's policy as Adams-Bashforth 3 with the Heun restart step
using BuildLag = GenericBuild<true, true, true, true, true, false, false, false, false, false, true>;      // BuildLin's policy with the four-point Lagrange interpolant of the stencil table
using BuildRkc = GenericBuild<true, true, true, true, false, false, false, false, false, false, false, true>;      // BuildSub's policy as one Runge-Kutta-Chebyshev step per interval: the stage count in the sub-steps' place
using BuildLinSth = GenericBuild<true, true, true, true, true, false, false, false, false, false, false, false, true>;      // BuildLin's policy with a head evaluation in front of every stage s >= 1
using BuildLagSth = GenericBuild<true, true, true, true, true, false, false, false, false, false, true, false, true>;      // BuildLag's policy with the same
enum BuildId { kBuildElu1, kBuildAct, kBuildPre, kBuildRk, kBuildSub, kBuildLin, kBuildPev, kBuildAb, kBuildMs, kBuildMsp, kBuildAb3, kBuildLag, kBuildRkc, kBuildLinSth, kBuildLagSth };      // what a call names its build with

}  // namespace psnode
