// K5 -- generic fused backward pass (discretise-then-optimise) for ODE and DAE, any layer count / widths that fit LDS.
// The always-available HIP path for training, as psnode_generic.hip is for the forward: shapes with an MFMA backward
// (K4, psnode_backward.hip) use that one.
//
// One workgroup = 16 trajectories walked from the last grid point to the first, everything in LDS:
//   * activations of ONE MLP evaluation for all layers, [unit][TP] with a padded row stride TP = 20 floats: 16 lanes
//     reading 16 consecutive rows with ds_read_b128 then hit 16 disjoint bank quads (stride 16 would be 4..16-way);
//   * parameter-gradient accumulators for every weight and bias (each element owned by one thread: no atomics),
//     written once at the end as a per-workgroup partial and summed in a fixed order by reduce_partials (deterministic);
//   * the RK adjoint state (stage inputs, k_s, g_k[s], carries) and the external-input gradients.
// Per step: stage forwards (to rebuild the stage inputs), then for each stage in reverse a forward with stored
// activations followed by the VJP:  delta_in = W^T delta_out * ELU'(.) (weights read row-major, coalesced over the input
// index) and dW += delta (x) act in 4x4 register blocks.  DAE: the AE head's VJP is chained in through the algebraic
// variable (i_{k+1} = g(x_{k+1}; z,v) feeds the DE of step k+1; at event steps i0 = g(x_k; jumps) instead).
// Teacher forcing (GBwd::flags) changes the outer sweep only: which rows a step starts from and which adjoints travel to the step before.
#include <string.h>

// One object per build policy is compiled from this header (psnode_generic_build.h: each alias with its one-line description).  A policy's
// file psnode_generic_bwd_<fam>.hip names it as PSNODE_BUILD in front of the include; the kernel (generic_backward_kernel, around
// psnode_generic_bwd_body.h) and the launcher (generic_backward_launch<Bd>) are written below, once.
// The policy decides in the language: the kernel-argument structs (GMlpT / GBwdT: the pre fields are a base that is empty elsewhere), the
// activation context ActCtx every device function takes, the stage coefficients (coef_a, coef_b) and
// `if constexpr` in the kernel body and the launcher.  The host's fit and layout functions take `pre` at run time.
#pragma once
#include "psnode_act.h"
#include "psnode_generic_tile.h"
#include "psnode_launch.h"

namespace psnode {
namespace {

using Bd = PSNODE_BUILD;

constexpr int TP = 20;    // padded row stride (floats)

// Kernel-argument structs.  The pre and tableau builds carry two more fields, at the end of each struct: they are a base class that is empty
// in the other builds, so that the ELU(1) and act kernels' argument layout has no trace of them.
struct GMlpBase {
    int L, in_dim;
    int out_dim[kMaxLayers];
    const float* w[kMaxLayers];    // row-major [out][in] (caller's nn.Linear weight)
    const float* wt[kMaxLayers];   // transposed [in][out] (workspace)
    const float* b[kMaxLayers];
    int gw[kMaxLayers], gb[kMaxLayers];   // offsets of dW, db in the flat gradient vector (nn.Linear order)
    int act[kMaxLayers + 1];              // row offsets of the layer activations (act[0] = input) in the acts buffer
    int np;
};
template <bool PRE> struct GMlpPre { int pre[kMaxLayers]; };      // float offsets of the hidden layers' pre-activations in the u region (set_pre_layout)
template <> struct GMlpPre<false> {};
template <bool PRE> struct GMlpT : GMlpBase, GMlpPre<PRE> {};
using GMlp = GMlpT<Bd::pre>;
static_assert(sizeof(GMlpT<false>) == sizeof(GMlpBase) && sizeof(GMlpT<true>) == sizeof(GMlpBase) + sizeof(int) * kMaxLayers, "pre[] follows np directly");

template <bool PRE> struct GBwdBody {
    int method, dae;
    int xd, zd, vd, id;
    long long T, B;
    GMlpT<PRE> de, ae;
    ViewDev t, z, v;
    const float* a0;
    const int* ev;
    const float* zj; long long zjb, zje;
    const float* vj; long long vjb, vje;
    int n_events;
    const float *xs, *is_, *gxs, *gis;
    // teacher forcing (include/psnode_hip.h, PSNODE_FLAG_INPUT_TRUE_X / _I): launch-uniform, tested at sweep level only.  xt / it: the dataset
    // rows x_true / i_true [T,B,.] (an ODE call hands the dataset in as xs: its launcher sets xt = xs)
    unsigned flags;
    const float *xt, *it;
    float *gx0, *gz, *gv, *gzj, *gvj, *ga0, *wpart;
    int maxw, act_rows;
    int gacc_global;   // parameter-gradient accumulators in this workgroup's slice of wpart (global, L2) instead of LDS: 0 = none,
                       // 1 = both MLPs', 2 = the AE's only (register path of a DAE: the DE's tile-major accumulators stay in LDS)
    // register path of the DE (round 6): <= 4 layers of <= 64 units, 3 n <= 128 input columns.  Plain and transposed MFMA images (workspace;
    // psnode_generic.hip: launch_pack_plain_images); the wave's A operands of both stay in VGPRs for the launch.
    int de_reg;
    const float* fimg[kMaxLayers];
    const float* timg[kMaxLayers];
    // streamed path (round 6): the MLPs that are not on the register path -- str 1: the AE head of a DAE whose DE is, 2: both MLPs -- read
    // their MFMA A operands from the same kind of images (L2-resident), one chunk ahead; no staging through LDS
    int str;
    float* tmpart;     // per-workgroup TILE-MAJOR global accumulators of the MLPs off the staged path (gacc_global != 0): tm_total(de) + tm_total(ae)
    const float* fimgA[kMaxLayers];
    const float* timgA[kMaxLayers];
};
template <bool PRE> struct UpreOff { int upre_off; };      // float offset of the u region in LDS (behind everything else)
template <> struct UpreOff<false> {};
template <bool PRE> struct GBwdT : GBwdBody<PRE>, UpreOff<PRE> {};
struct GBwd : GBwdT<Bd::pre> {};       // (a name of its own: it is part of the kernels' mangled names)
static_assert(sizeof(GBwdT<false>) == sizeof(GBwdBody<false>) && sizeof(GBwdT<true>) == sizeof(GBwdBody<true>) + 8, "upre_off follows timgA directly");
// the u region of this workgroup (nullptr in the builds that keep none)
template <bool PRE> __device__ __forceinline__ float* u_region(float* lds, const UpreOff<PRE>& o) {
    if constexpr (PRE) return lds + o.upre_off; else return nullptr;
}

__device__ __forceinline__ float delu(float h) { return elu_grad(h); }   // ELU'(pre) from h = ELU(pre)

// The hidden-layer activation of one MLP as the device functions below see it: one ordinary parameter, shaped by the build policy.
// act1 / actq: the activation of a value / of four.  keep1 / keepq: store a hidden layer's pre-activation u at [row][c] of its [unit][TP]
// rows / at quad idx of its quad-row image (layer l's region, GMlp::pre[l]).  dact1 / dactq: the derivative, from h and -- where the build
// keeps it -- the u stored there.
template <bool ACT, bool PRE> struct ActCtxT;
template <> struct ActCtxT<false, false> {      // ELU(1): nothing to carry, nothing kept
    __device__ __forceinline__ ActCtxT(NoAct, float*) {}
    __device__ __forceinline__ float act1(float v) const { return elu1(v); }
    __device__ __forceinline__ f4 actq(f4 v) const { return elu_quad(v); }
    __device__ __forceinline__ void keep1(const GMlpBase&, int, int, int, float) const {}
    __device__ __forceinline__ void keepq(const GMlpBase&, int, int, f4) const {}
    __device__ __forceinline__ float dact1(float h, const GMlpBase&, int, int, int) const { return delu(h); }
    __device__ __forceinline__ f4 dactq(f4 h, const GMlpBase&, int, int) const { return elu_grad_quad(h); }
};
template <> struct ActCtxT<true, false> {       // the MLP's ActDev; the derivative from h
    const ActDev& ac;
    __device__ __forceinline__ ActCtxT(const ActDev& a, float*) : ac(a) {}
    __device__ __forceinline__ float act1(float v) const { return psnode::act1(v, ac); }
    __device__ __forceinline__ f4 actq(f4 v) const { return act_quad(v, ac); }
    __device__ __forceinline__ void keep1(const GMlpBase&, int, int, int, float) const {}
    __device__ __forceinline__ void keepq(const GMlpBase&, int, int, f4) const {}
    __device__ __forceinline__ float dact1(float h, const GMlpBase&, int, int, int) const { return act_grad1(h, ac); }
    __device__ __forceinline__ f4 dactq(f4 h, const GMlpBase&, int, int) const { return act_grad_quad(h, ac); }
};
template <> struct ActCtxT<true, true> {        // the ActDev and the u region in LDS
    const ActDev& ac;
    float* upre;
    __device__ __forceinline__ ActCtxT(const ActDev& a, float* u) : ac(a), upre(u) {}
    __device__ __forceinline__ float act1(float v) const { return pre_act1(v, ac); }
    __device__ __forceinline__ f4 actq(f4 v) const { return pre_act_quad(v, ac); }
    __device__ __forceinline__ void keep1(const GMlpT<true>& m, int l, int row, int c, float u) const { upre[m.pre[l] + row * TP + c] = u; }
    __device__ __forceinline__ void keepq(const GMlpT<true>& m, int l, int idx, f4 u) const { reinterpret_cast<f4*>(upre + m.pre[l])[idx] = u; }
    __device__ __forceinline__ float dact1(float h, const GMlpT<true>& m, int l, int row, int c) const {
        return pre_grad1(h, upre[m.pre[l] + row * TP + c], ac);
    }
    __device__ __forceinline__ f4 dactq(f4 h, const GMlpT<true>& m, int l, int idx) const {
        return pre_grad_quad(h, reinterpret_cast<const f4*>(upre + m.pre[l])[idx], ac);
    }
};
using ActCtx = ActCtxT<Bd::act, Bd::pre>;

// The stage loops' forms.  The tableau build reads the stage count and the coefficients of its psnode_rk_tableau_f32: the coefficients go to
// LDS once (kernel body) -- a[4][4] | b[4] in the fourth slot of `ks`, which holds k_0 .. k_{S - 2} only (nx >= 20 floats) -- and come back as
// broadcast reads (indexed as kernel arguments they are scalar loads, and their waits, inside the stage loops); a coefficient that is
// exactly 0 is skipped (kernel body).  The other builds use rk_stages / rk_a / rk_b of a.method.
__device__ __forceinline__ float rk_u(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float coef_a(int method, const float* ks, int nx, int s, int j) {
    if constexpr (Bd::rk) return rk_u(ks[3 * nx + 4 * s + j]); else return rk_a(method, s, j);
}
__device__ __forceinline__ float coef_b(int method, const float* ks, int nx, int s) {
    if constexpr (Bd::rk) return rk_u(ks[3 * nx + 16 + s]); else return rk_b(method, s);
}

typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4v gm(float a, float b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// All three matrix products below run on v_mfma_f32_16x16x4_f32 with operands read straight from LDS (lane l:
// i = j = l&15, k-slot g = l>>4).  Output tiles of 16 rows are dealt round-robin to the four waves.

// forward with stored activations: acts[act[0]] = input rows; writes acts[act[l+1]].
// out[u][traj] = sum_k W[u][k] in[k][traj]:  A[i][g] = W^T staged in `wbuf` as [k][N] (chunks of input rows, partial sums
// of multi-chunk layers live in `out`), B[g][j] = in[k = 4q+g][traj j].  Barrier after every chunk.
// (forceinline: as separate functions the buffers arrive as GENERIC pointers and every LDS access becomes a flat_load / flat_store)
__device__ __forceinline__ void g_forward(const GMlp& m, float* acts, float* wbuf, const ActCtx& cx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
    int K = m.in_dim;
    for (int l = 0; l < m.L; ++l) {
        const int N = m.out_dim[l];
        const float* __restrict__ wt = m.wt[l];
        const float* __restrict__ bias = m.b[l];
        const float* in = acts + m.act[l] * TP;
        float* out = acts + m.act[l + 1] * TP;
        const bool last = (l + 1 == m.L);
        const int KC = (kWBuf / N) & ~3;   // input rows per chunk: a multiple of 4, >= 4 because N <= PSNODE_MAX_WIDTH = kWBuf / 4
        for (int k0 = 0; k0 < K; k0 += KC) {
            const int kc = K - k0 < KC ? K - k0 : KC;
            stage_weights(wt + (size_t)k0 * N, wbuf, kc * N);
            const bool first = k0 == 0, final = k0 + kc >= K;
            for (int mt = wave; mt * 16 < N; mt += 4) {
                const int u = 16 * mt + i;
                f4v accA, accB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int uu = 16 * mt + 4 * g + r, uc = uu < N ? uu : N - 1;
                    const float bv = bias[uc], ov = out[uc * TP + i];      // two address spaces: load both, select the value
                    accA[r] = uu < N ? (first ? bv : ov) : 0.0f;
                }
                for (int kq = 0; kq < kc; kq += 8) {
                    const int ka = kq + g, kb = kq + 4 + g;
                    // clamped addresses, unconditional loads, selects: a predicated LDS load is an exec-masked branch around every operand
                    const int kac = ka < kc ? ka : kc - 1, kbc = kb < kc ? kb : kc - 1, uc = u < N ? u : N - 1;
                    const float wa = wbuf[kac * N + uc], ia = in[(k0 + kac) * TP + i], wb = wbuf[kbc * N + uc], ib = in[(k0 + kbc) * TP + i];
                    const float a0 = (ka < kc && u < N) ? wa : 0.0f, b0 = ka < kc ? ia : 0.0f;
                    const float a1 = (kb < kc && u < N) ? wb : 0.0f, b1 = kb < kc ? ib : 0.0f;
                    accA = gm(a0, b0, accA);
                    accB = gm(a1, b1, accB);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int uu = 16 * mt + 4 * g + r;
                    if (uu < N) {
                        float v = accA[r] + accB[r];
                        if (final && !last) cx.keep1(m, l, uu, i, v);
                        if (final && !last) v = cx.act1(v);
                        out[uu * TP + i] = v;
                    }
                }
            }
            __syncthreads();
        }
        K = N;
    }
}

// VJP of the MLP: `din` holds delta of the output [N_L][TP]; returns the buffer with the input gradient [in_dim][TP].
// Accumulates dW, db into gacc.  Ends with a barrier.
// gacc_l / gacc_g: the parameter-gradient accumulators in LDS or in this workgroup's global slice (gg, a template parameter: a runtime
// choice between the two pointers makes every access a flat one)
template <bool gg>
__device__ __forceinline__ float* g_vjp(const GMlp& m, const float* acts, float* din, float* dout, float* gacc_l, float* gacc_g, float* wbuf, const ActCtx& cx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    for (int l = m.L - 1; l >= 0; --l) {
        const int N = m.out_dim[l], K = l == 0 ? m.in_dim : m.out_dim[l - 1];
        const float* a_in = acts + m.act[l] * TP;
        // ---- dW[j][k] += sum_tr delta[j][tr] * a_in[k][tr]: 16x16 tiles, contraction over the 16 trajectories
        //      A[i][g] = delta[16 mt + i][tr = 4q+g], B[g][j] = a_in[16 kt + j][tr]; each tile is owned by one wave
        float* gw_l = gacc_l + m.gw[l];
        float* gw_g = gacc_g + m.gw[l];
        const int ntk = (K + 15) / 16, ntiles = ((N + 15) / 16) * ntk;
        for (int tile = wave; tile < ntiles; tile += 4) {
            const int mt = tile / ntk, kt = tile % ntk;
            const int ju = 16 * mt + i, ku = 16 * kt + i;
            f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int tr = 4 * q + g;
                const float dv = din[(ju < N ? ju : N - 1) * TP + tr], av = a_in[(ku < K ? ku : K - 1) * TP + tr];
                acc = gm(ju < N ? dv : 0.0f, ku < K ? av : 0.0f, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jr = 16 * mt + 4 * g + r;
                if (jr < N && ku < K) { if constexpr (gg) gw_g[jr * K + ku] += acc[r]; else gw_l[jr * K + ku] += acc[r]; }
            }
        }
        // ---- db[j] += sum_tr delta[j][tr]
        for (int j = tid; j < N; j += NT) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < TB; ++c) s += din[j * TP + c];
            if constexpr (gg) gacc_g[m.gb[l] + j] += s; else gacc_l[m.gb[l] + j] += s;
        }
        // ---- delta_in[k] = sum_j W[j][k] delta[j]  (* ELU'(a_in[k]) for hidden layers): A[i][g] = W[j = 4q+g][16 kt + i] from the
        //      row-major weights staged in chunks of output rows, B[g][j] = delta[4q+g][traj]; partial sums in dout
        __syncthreads();
        const float* __restrict__ w = m.w[l];
        const int JC = (kWBuf / K) & ~3;
        for (int j0 = 0; j0 < N; j0 += JC) {
            const int jc = N - j0 < JC ? N - j0 : JC;
            stage_weights(w + (size_t)j0 * K, wbuf, jc * K);
            const bool first = j0 == 0, final = j0 + jc >= N;
            for (int kt = wave; kt * 16 < K; kt += 4) {
                const int ku = 16 * kt + i;
                f4v accA, accB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kr = 16 * kt + 4 * g + r;
                    const float dv = dout[(kr < K ? kr : K - 1) * TP + i];
                    accA[r] = (!first && kr < K) ? dv : 0.0f;
                }
                for (int jq = 0; jq < jc; jq += 8) {
                    const int ja = jq + g, jb = jq + 4 + g;
                    const int jac = ja < jc ? ja : jc - 1, jbc = jb < jc ? jb : jc - 1, kc_ = ku < K ? ku : K - 1;
                    const float wa = wbuf[jac * K + kc_], da = din[(j0 + jac) * TP + i], wb = wbuf[jbc * K + kc_], db_ = din[(j0 + jbc) * TP + i];
                    const float a0 = (ja < jc && ku < K) ? wa : 0.0f, b0 = ja < jc ? da : 0.0f;
                    const float a1 = (jb < jc && ku < K) ? wb : 0.0f, b1 = jb < jc ? db_ : 0.0f;
                    accA = gm(a0, b0, accA);
                    accB = gm(a1, b1, accB);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kr = 16 * kt + 4 * g + r;
                    if (kr < K) {
                        float v = accA[r] + accB[r];
                        if (final && l > 0) v *= cx.dact1(a_in[kr * TP + i], m, l - 1, kr, i);
                        dout[kr * TP + i] = v;
                    }
                }
            }
            __syncthreads();
        }
        float* tmp = din; din = dout; dout = tmp;
    }
    return din;
}

// ---- register path of the DE (the forward recomputation and the delta propagation of g_vjp): what K0's register form is for the forward
// pass (psnode_generic.hip).  Activations and deltas additionally live in QUAD-ROW buffers (float index ((col / 4) * 16 + traj) * 4 + col % 4:
// the B operands of four MFMA steps are one lane-linear ds_read_b128, a D tile one ds_write_b128); the [unit][TP] copies stay, they are what
// the weight-gradient MFMAs (contraction over the trajectories) and the step's glue read.
// (up16, qi, mfma_quad, tile_reg, tile_reg_any: psnode_generic_tile.h)

struct RegFwd { f4 first[8]; f4 rest[3][4]; };          // layer 0: <= 128 input columns; layers 1..3: <= 64
struct RegBwd { f4 first[2][4]; f4 rest[3][4]; };       // transposed: layer 0 has <= 8 tiles over its inputs (two per wave), the others <= 4

__device__ __forceinline__ void load_reg_images(const GBwd& a, RegFwd& fw, RegBwd& bw) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const bool on = l < a.de.L;
        const int K = on ? (l ? a.de.out_dim[l - 1] : a.de.in_dim) : 0, N = on ? a.de.out_dim[l] : 0;
        const int SK = (K + 15) >> 4, SN = (N + 15) >> 4;           // quads of the forward contraction / of the transposed one
        const f4* __restrict__ F = reinterpret_cast<const f4*>(a.fimg[on ? l : 0]) + lane;
        const f4* __restrict__ Tm = reinterpret_cast<const f4*>(a.timg[on ? l : 0]) + lane;
#pragma unroll
        for (int q = 0; q < (l ? 4 : 8); ++q) {
            const f4 v = (w < SN && q < SK) ? F[((size_t)(w < SN ? w : 0) * SK + (q < SK ? q : 0)) * 64] : zero;
            if (l == 0) fw.first[q] = v; else fw.rest[l - 1][q] = v;
        }
#pragma unroll
        for (int j = 0; j < (l ? 1 : 2); ++j) {
            const int kt = w + 4 * j;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f4 v = (kt < SK && q < SN) ? Tm[((size_t)(kt < SK ? kt : 0) * SN + (q < SN ? q : 0)) * 64] : zero;
                if (l == 0) bw.first[j][q] = v; else bw.rest[l - 1][q] = v;
            }
        }
    }
}

// quad-row buffers of the register path (float offsets from qb): the DE input, the hidden activations, two delta buffers
struct QOff { int in, act[kMaxLayers - 1], d0, d1, total; };
__host__ __device__ inline QOff q_offsets(const GMlp& m) {
    QOff q;
    int o = 0;
    q.in = o; o += up16(m.in_dim) * TB;
    int mx = 16;
    for (int l = 0; l < kMaxLayers - 1; ++l) {
        q.act[l] = o;
        if (l + 1 < m.L) o += up16(m.out_dim[l]) * TB;
    }
    for (int l = 0; l < m.L; ++l) mx = up16(m.out_dim[l]) > mx ? up16(m.out_dim[l]) : mx;
    q.d0 = o; o += mx * TB;
    q.d1 = o; o += mx * TB;
    q.total = o;
    return q;
}

// Register path with the accumulators in LDS: the DE's weight gradients are kept TILE-MAJOR -- [tile = mt * ntk + kt][lane][4], the MFMA D layout:
// one ds_read_b128 + one ds_write_b128 per tile instead of four predicated b32 read-modify-writes (13 of 77 ms at x_dim 20, hidden 64) -- and
// un-permuted into nn.Linear order once, when the workgroup's partial is written out.  Per layer: 16 x 16 tiles padded, then all the biases.
__host__ __device__ inline int tm_dw_off(const GMlp& m, int l) {
    int o = 0, k = m.in_dim;
    for (int q = 0; q < l; ++q) { o += up16(m.out_dim[q]) * up16(k); k = m.out_dim[q]; }
    return o;
}
__host__ __device__ inline int tm_db_off(const GMlp& m, int l) {
    int o = tm_dw_off(m, m.L);
    for (int q = 0; q < l; ++q) o += m.out_dim[q];
    return o;
}
__host__ __device__ inline int tm_total(const GMlp& m) { return (tm_db_off(m, m.L) + 3) & ~3; }

// forward with stored activations, the DE in registers: acts[act[0]] = input rows; writes acts[act[l + 1]] and the quad-row copies
__device__ __forceinline__ void g_forward_reg(const GBwd& a, float* acts, float* qb, const QOff& qo, const RegFwd& fw, const ActCtx& cx) {
    const GMlp& m = a.de;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, j = lane & 15;
    {   // the input rows -> quad-row, pad columns zero
        const float* u = acts + m.act[0] * TP;
        for (int idx = tid; idx < up16(m.in_dim) * TB; idx += NT)
            qb[qo.in + qi(idx / TB, idx % TB)] = idx / TB < m.in_dim ? u[(idx / TB) * TP + idx % TB] : 0.0f;
        __syncthreads();
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (l >= m.L) break;
        const int K = l ? m.out_dim[l - 1] : m.in_dim, N = m.out_dim[l];
        const int S4 = (K + 15) >> 4, NTL = (N + 15) >> 4;
        const bool last = (l + 1 == m.L);
        if (w < NTL) {
            const f4* bq = reinterpret_cast<const f4*>(qb + (l ? qo.act[l - 1 < 3 ? l - 1 : 0] : qo.in)) + lane;
            const f4 bias = *reinterpret_cast<const f4*>(a.fimg[l] + (size_t)NTL * S4 * 256 + 16 * w + 4 * g);
            f4 acc;
            if (l == 0) acc = tile_reg_any<8>(S4, bq, fw.first);
            else acc = tile_reg_any<4>(S4, bq, fw.rest[l - 1 < 3 ? l - 1 : 0]);
            acc = acc + bias;
            const f4 e = last ? acc : cx.actq(acc);
            float* out = acts + m.act[l + 1] * TP;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int uu = 16 * w + 4 * g + r;
                if (uu < N) out[uu * TP + j] = e[r];
            }
            if (!last) reinterpret_cast<f4*>(qb + qo.act[l < 3 ? l : 0])[w * 64 + lane] = e;
            if (!last) cx.keepq(m, l < 3 ? l : 0, w * 64 + lane, acc);
        }
        __syncthreads();
    }
}

// VJP of the DE with the delta propagation in registers (the weight-gradient part is g_vjp's)
template <bool gg>
__device__ __forceinline__ float* g_vjp_reg(const GBwd& a, const float* acts, float* din, float* dout, float* gacc_l, float* gacc_g, float* qb,
                                            const QOff& qo, const RegBwd& bw, const ActCtx& cx) {
    const GMlp& m = a.de;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(wave);
    int qd = qo.d0, qn = qo.d1;
    {   // the output gradient -> quad-row, pad columns zero
        const int N = m.out_dim[m.L - 1];
        for (int idx = tid; idx < up16(N) * TB; idx += NT) qb[qd + qi(idx / TB, idx % TB)] = idx / TB < N ? din[(idx / TB) * TP + idx % TB] : 0.0f;
        __syncthreads();
    }
#pragma unroll
    for (int l = 3; l >= 0; --l) {
        if (l >= m.L) continue;
        const int N = m.out_dim[l], K = l == 0 ? m.in_dim : m.out_dim[l - 1];
        const float* a_in = acts + m.act[l] * TP;
        // ---- dW[j][k] += sum_tr delta[j][tr] * a_in[k][tr],  db[j] += sum_tr delta[j][tr]      (as g_vjp)
        const int ntk = (K + 15) / 16, ntiles = ((N + 15) / 16) * ntk;
#ifndef PSNODE_K5_ABL
#define PSNODE_K5_ABL 0      // timing-only builds: 1 = no accumulation into gacc, 2 = no weight-gradient tiles at all, 3 = no forward recomputation
#endif
        // weight-gradient tiles.  Global accumulators (gg) are tile-major like the LDS ones -- one 16-byte read-modify-write per lane and tile
        // -- and the NEXT tile's old value is requested before this tile's MFMAs: four predicated b32 read-modify-writes per tile with the
        // L2 round trip exposed cost 56 of 95 ms at hidden 128.
        f4* T4 = reinterpret_cast<f4*>(gg ? gacc_g + tm_dw_off(m, l) : gacc_l + tm_dw_off(m, l)) + lane;
        f4 oldn = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (gg) { if (wave < ntiles) oldn = T4[wave * 64]; }
        for (int tile = wave; tile < (PSNODE_K5_ABL == 2 ? 0 : ntiles); tile += 4) {
            const int mt = tile / ntk, kt = tile % ntk;
            const int ju = 16 * mt + i, ku = 16 * kt + i;
            // MFMA step q contracts the trajectories 4 g + q (slot g): a lane's four operands are ONE 16-byte read of its row (TP = 20 floats:
            // 80-byte rows, 16-byte aligned)
            const f4 dv = *reinterpret_cast<const f4*>(din + (ju < N ? ju : N - 1) * TP + 4 * g);
            const f4 av = *reinterpret_cast<const f4*>(a_in + (ku < K ? ku : K - 1) * TP + 4 * g);
            f4 old = oldn;
            if constexpr (gg) oldn = T4[(tile + 4 < ntiles ? tile + 4 : tile) * 64];
            else old = T4[tile * 64];
            f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = gm(ju < N ? dv[q] : 0.0f, ku < K ? av[q] : 0.0f, acc);
            if (PSNODE_K5_ABL == 1) { if (acc[0] == 123.456f) T4[0] = acc; continue; }
            T4[tile * 64] = old + acc;                   // rows / columns beyond the matrix accumulate zeros
        }
        for (int jj = tid; jj < N; jj += NT) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < TB; ++c) s += din[jj * TP + c];
            if constexpr (gg) gacc_g[tm_db_off(m, l) + jj] += s; else gacc_l[tm_db_off(m, l) + jj] += s;
        }
        // ---- delta_in[k] = sum_j W[j][k] delta[j]  (* ELU'(a_in[k]) for hidden layers): tiles over k, A operands (W^T) in registers
        const int SN = (N + 15) >> 4, NTK = (K + 15) >> 4;
        const f4* bq = reinterpret_cast<const f4*>(qb + qd) + lane;
#pragma unroll
        for (int jt = 0; jt < (l ? 1 : 2); ++jt) {
            const int kt = w + 4 * jt;
            if (kt < NTK) {
                f4 acc = l == 0 ? tile_reg_any<4>(SN, bq, bw.first[jt]) : tile_reg_any<4>(SN, bq, bw.rest[l > 0 ? l - 1 : 0]);
                // layer 0 stores the accumulator as it is: on the taken edge of the switch's exit branch the compiler's hazard count is one
                // wait state short of the MFMA's write (ISA lint check B); the tied nop puts the distance on every path
                asm volatile("s_nop 3" : "+v"(acc));
                if (l > 0) {
                    const f4 h = reinterpret_cast<const f4*>(qb + qo.act[l - 1 >= 0 ? l - 1 : 0])[kt * 64 + lane];
                    acc = acc * cx.dactq(h, m, l - 1 >= 0 ? l - 1 : 0, kt * 64 + lane);
                    reinterpret_cast<f4*>(qb + qn)[kt * 64 + lane] = acc;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kr = 16 * kt + 4 * g + r;
                    if (kr < K) dout[kr * TP + i] = acc[r];
                }
            }
        }
        __syncthreads();
        { float* tmp = din; din = dout; dout = tmp; }
        { const int t_ = qd; qd = qn; qn = t_; }
    }
    return din;
}

// ---- streamed path: one output tile with its A operands read from the image (L2), one chunk of four quads ahead of the MFMAs that use
// them; B operands from the quad-row buffer.  (The loads are unconditional on clamped addresses: see psnode_generic.hip, mlp_eval.)
__device__ __forceinline__ f4 tile_stream(const f4* __restrict__ A, const int S4, const f4* bq) {
    f4 acc = f4{0.f, 0.f, 0.f, 0.f}, acc2 = acc;
    f4 nxt[4];
    auto fetch4 = [&](int q0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) nxt[c] = A[(q0 + c < S4 ? q0 + c : S4 - 1) * 64];
    };
    fetch4(0);
    for (int q0 = 0; q0 < S4; q0 += 4) {
        f4 cur[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[c] = nxt[c];
        fetch4(q0 + 4 < S4 ? q0 + 4 : S4 - 1);
        if (q0 + 4 <= S4) {
            f4 bv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[c] = bq[(q0 + c) * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 4; ++c) mfma_quad(cur[c], bv[c], (c & 1) ? acc2 : acc);
        } else {
            for (int c = 0; q0 + c < S4; ++c) mfma_quad(c == 0 ? cur[0] : (c == 1 ? cur[1] : cur[2]), bq[(q0 + c) * 64], acc);
        }
    }
    return acc + acc2;
}

// forward with stored activations, streamed: acts[act[0]] = input rows; writes acts[act[l + 1]] and the quad-row copies
__device__ __forceinline__ void g_forward_str(const GMlp& m, const float* const* fimg, float* acts, float* qb, const QOff& qo, const ActCtx& cx) {
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, j = lane & 15;
    {
        const float* u = acts + m.act[0] * TP;
        for (int idx = tid; idx < up16(m.in_dim) * TB; idx += NT)
            qb[qo.in + qi(idx / TB, idx % TB)] = idx / TB < m.in_dim ? u[(idx / TB) * TP + idx % TB] : 0.0f;
        __syncthreads();
    }
    for (int l = 0; l < m.L; ++l) {
        const int K = l ? m.out_dim[l - 1] : m.in_dim, N = m.out_dim[l];
        const int S4 = (K + 15) >> 4, NTL = (N + 15) >> 4;
        const bool last = (l + 1 == m.L);
        const f4* bq = reinterpret_cast<const f4*>(qb + (l ? qo.act[l - 1] : qo.in)) + lane;
        float* out = acts + m.act[l + 1] * TP;
        for (int nt = w; nt < NTL; nt += 4) {
            const f4 bias = *reinterpret_cast<const f4*>(fimg[l] + (size_t)NTL * S4 * 256 + 16 * nt + 4 * g);
            f4 acc = tile_stream(reinterpret_cast<const f4*>(fimg[l]) + (size_t)nt * S4 * 64 + lane, S4, bq) + bias;
            const f4 e = last ? acc : cx.actq(acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int uu = 16 * nt + 4 * g + r;
                if (uu < N) out[uu * TP + j] = e[r];
            }
            if (!last) reinterpret_cast<f4*>(qb + qo.act[l])[nt * 64 + lane] = e;
            if (!last) cx.keepq(m, l, nt * 64 + lane, acc);
        }
        __syncthreads();
    }
}

// VJP, streamed: weight gradients as on the register path (tile-major LDS accumulators at gacc_l when !gg), delta propagation on the
// transposed images
template <bool gg>
__device__ __forceinline__ float* g_vjp_str(const GMlp& m, const float* const* timg, const float* acts, float* din, float* dout, float* gacc_l,
                                            float* gacc_g, float* qb, const QOff& qo, const ActCtx& cx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(wave);
    int qd = qo.d0, qn = qo.d1;
    {
        const int N = m.out_dim[m.L - 1];
        for (int idx = tid; idx < up16(N) * TB; idx += NT) qb[qd + qi(idx / TB, idx % TB)] = idx / TB < N ? din[(idx / TB) * TP + idx % TB] : 0.0f;
        __syncthreads();
    }
    for (int l = m.L - 1; l >= 0; --l) {
        const int N = m.out_dim[l], K = l == 0 ? m.in_dim : m.out_dim[l - 1];
        const float* a_in = acts + m.act[l] * TP;
        const int ntk = (K + 15) / 16, ntiles = ((N + 15) / 16) * ntk;
        // weight-gradient tiles.  Global accumulators (gg) are tile-major like the LDS ones -- one 16-byte read-modify-write per lane and tile
        // -- and the NEXT tile's old value is requested before this tile's MFMAs: four predicated b32 read-modify-writes per tile with the
        // L2 round trip exposed cost 56 of 95 ms at hidden 128.
        f4* T4 = reinterpret_cast<f4*>(gg ? gacc_g + tm_dw_off(m, l) : gacc_l + tm_dw_off(m, l)) + lane;
        f4 oldn = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (gg) { if (wave < ntiles) oldn = T4[wave * 64]; }
        for (int tile = wave; tile < (PSNODE_K5_ABL == 2 ? 0 : ntiles); tile += 4) {
            const int mt = tile / ntk, kt = tile % ntk;
            const int ju = 16 * mt + i, ku = 16 * kt + i;
            // MFMA step q contracts the trajectories 4 g + q (slot g): a lane's four operands are ONE 16-byte read of its row (TP = 20 floats:
            // 80-byte rows, 16-byte aligned)
            const f4 dv = *reinterpret_cast<const f4*>(din + (ju < N ? ju : N - 1) * TP + 4 * g);
            const f4 av = *reinterpret_cast<const f4*>(a_in + (ku < K ? ku : K - 1) * TP + 4 * g);
            f4 old = oldn;
            if constexpr (gg) oldn = T4[(tile + 4 < ntiles ? tile + 4 : tile) * 64];
            else old = T4[tile * 64];
            f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = gm(ju < N ? dv[q] : 0.0f, ku < K ? av[q] : 0.0f, acc);
            if (PSNODE_K5_ABL == 1) { if (acc[0] == 123.456f) T4[0] = acc; continue; }
            T4[tile * 64] = old + acc;                   // rows / columns beyond the matrix accumulate zeros
        }
        for (int jj = tid; jj < N; jj += NT) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < TB; ++c) s += din[jj * TP + c];
            if constexpr (gg) gacc_g[tm_db_off(m, l) + jj] += s; else gacc_l[tm_db_off(m, l) + jj] += s;
        }
        const int SN = (N + 15) >> 4, NTK = (K + 15) >> 4;
        const f4* bq = reinterpret_cast<const f4*>(qb + qd) + lane;
        for (int kt = w; kt < NTK; kt += 4) {
            f4 acc = tile_stream(reinterpret_cast<const f4*>(timg[l]) + (size_t)kt * SN * 64 + lane, SN, bq);
            asm volatile("s_nop 3" : "+v"(acc));       // (as on the register path: the store below may sit on a taken branch edge)
            if (l > 0) {
                const f4 h = reinterpret_cast<const f4*>(qb + qo.act[l - 1])[kt * 64 + lane];
                acc = acc * cx.dactq(h, m, l - 1, kt * 64 + lane);
                reinterpret_cast<f4*>(qb + qn)[kt * 64 + lane] = acc;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kr = 16 * kt + 4 * g + r;
                if (kr < K) dout[kr * TP + i] = acc[r];
            }
        }
        __syncthreads();
        { float* tmp = din; din = dout; dout = tmp; }
        { const int t_ = qd; qd = qn; qn = t_; }
    }
    return din;
}

// gg / ggA: the DE's / the AE's accumulators live in the workgroup's global slice.  REG: the DE on the register path.  STR: 1 = the AE
// head streamed, 2 = both MLPs streamed (0: whatever is not on the register path stages its weights through LDS).
// (waves per SIMD, Bd::two_waves: the fully streamed instances that fitted 256 registers -- two workgroups per CU where their LDS allows
//  it -- keep that budget: the sweep-level flag values must not cost them the second workgroup)
// Extra: Bd::n_extra by-value arguments behind `a`, in the order act | rk | sub; the body sees all three names.  (B = Bd, named in the template
// for the kernel's symbol alone.)
template <class B, bool gg, bool REG, bool ggA, int STR, class... Extra>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(Bd::two_waves(gg, STR), 8))) void generic_backward_kernel(const GBwd a, const Extra... extra) {
    static_assert(std::is_same_v<B, Bd> && sizeof...(Extra) == B::n_extra, "the policy's argument list");
    const auto& act = kernel_arg<0>(NoActPair{}, extra...);                // ELU(1): no activation argument, ActCtx is empty
    const auto& rk = kernel_arg<1>(psnode_rk_tableau_f32{}, extra...);     // never read without one: the tableau code is under `if constexpr (Bd::rk)`
    const auto& sub = kernel_arg<2>(SubDev{}, extra...);                   // never read without one: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_bwd_body.h"
}
template <class B, class... Extra> struct GenericBwdKernels {
    template <bool gg, bool REG, bool ggA, int STR> static constexpr auto get() { return &generic_backward_kernel<B, gg, REG, ggA, STR, Extra...>; }
};

// (g.wt, the transposed weights of the forward recomputation, are workspace segments: gbwd_layout)
int fill_gmlp(const psnode_mlp_f32& m, GMlp& g) {
    g.L = m.n_layers;
    g.in_dim = m.in_dim;
    int k = m.in_dim, off = 0, rows = 0;
    g.act[0] = 0;
    rows = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) {
        g.out_dim[l] = m.out_dim[l];
        g.w[l] = m.weight[l];
        g.b[l] = m.bias[l];
        g.gw[l] = off; off += m.out_dim[l] * k;
        g.gb[l] = off; off += m.out_dim[l];
        g.act[l + 1] = rows;
        rows += m.out_dim[l];
        k = m.out_dim[l];
    }
    g.np = off;
    return rows;
}

// the u region of one MLP: per hidden layer [unit][TP] rows on the staged path (`quad` false), a quad-row image (as its h in qb) on the
// register / streamed paths.  Returns the floats; m.pre gets each layer's offset in the builds that have the field.
template <bool PRE> int pre_layout(GMlpT<PRE>& m, bool quad) {
    int o = 0;
    for (int l = 0; l + 1 < m.L; ++l) {
        if constexpr (PRE) m.pre[l] = o;
        o += quad ? up16(m.out_dim[l]) * TB : m.out_dim[l] * TP;
    }
    return o;
}
size_t pre_floats(const GBwd& a) {      // both MLPs share the region (their evaluations never overlap in time)
    GBwd c = a;
    const int de = pre_layout(c.de, a.de_reg || a.str == 2), ae = a.dae ? pre_layout(c.ae, a.str >= 1) : 0;
    return (size_t)(de > ae ? de : ae);
}
// a launch of a build that keeps u: both MLPs' layer offsets, and the region behind everything else
template <bool PRE> void place_u_region(GBwdT<PRE>& a, size_t lds_floats, size_t u_floats) {
    if constexpr (PRE) {
        pre_layout(a.de, a.de_reg || a.str == 2);
        if (a.dae) pre_layout(a.ae, a.str >= 1);
        a.upre_off = (int)(lds_floats - u_floats);
    }
}

// pre (here and below): count the u region, as the builds that keep the pre-activations lay LDS out (Bd::pre at a launch); lin: count the
// linear-externals build's three z | v regions (both ends of the interval, the right end's adjoint; 2: the Lagrange build's eight -- four node rows, their adjoints)
size_t gbwd_lds_floats(const GBwd& a, bool pre, int lin = 0) {
    const int vd = a.dae ? a.vd : 0, id = a.dae ? a.id : 0, ne = a.zd + vd + id, n = a.xd + ne;
    const bool de_tm = a.de_reg || a.str == 2, ae_tm = a.str >= 1;
    const size_t de_acc = a.gacc_global == 1 ? 0 : (size_t)(de_tm ? tm_total(a.de) : a.de.np);
    const size_t np_all = de_acc + ((a.dae && a.gacc_global == 0) ? (size_t)(ae_tm ? tm_total(a.ae) : a.ae.np) : 0);
    const bool stages = (!a.de_reg && a.str != 2) || (a.dae && a.str == 0);
    size_t q = 0;
    if (de_tm) q = (size_t)q_offsets(a.de).total;
    if (a.dae && ae_tm && (size_t)q_offsets(a.ae).total > q) q = (size_t)q_offsets(a.ae).total;
    return (size_t)a.act_rows * TP + 2 * (size_t)a.maxw * TP + 2 * (size_t)n * TP + 2 * (size_t)ne * TP + (size_t)a.xd * TP * (1 + 12 + 2) +
           (size_t)id * TP + TP + (lin == 2 ? 8 : (lin ? 3 : 0)) * (size_t)(a.zd + vd) * TP + (stages ? kWBuf : 0) + ((np_all + 3) & ~(size_t)3) + q + (pre ? pre_floats(a) : 0);
}
// the DE's shape class of the register path
bool de_reg_class(const psnode_mlp_f32& de) {
    if (de.n_layers > 4 || de.in_dim > 128) return false;
    for (int l = 0; l < de.n_layers; ++l)
        if (de.out_dim[l] > 64) return false;
    return true;
}
// K5's workspace, per MLP m (0 the DE, 1 the AE) and layer: the transposed weights of both MLPs | the plain and the transposed MFMA images
// of both (register / streamed paths) | one natural-order partial vector per workgroup (both MLPs) | one tile-major accumulator slice per
// workgroup (tm_total of both MLPs: the paths with global accumulators).  `a` (filled: fill_gmlp) gets the segments it carries.
struct GBwdLayout { float *img[2][kMaxLayers], *imgT[2][kMaxLayers]; };
inline size_t up64(size_t v) { return (v + 63) / 64 * 64; }
// (chunks: 1, or the time chunks of the segment-parallel build -- one partial and one slice per workgroup of its tiles x chunks grid)
GBwdLayout gbwd_layout(const psnode_mlp_f32& de, const psnode_mlp_f32* ae, long long B, GBwd& a, Arena& A, size_t chunks = 1) {
    const size_t nwg = (size_t)((B + TB - 1) / TB) * chunks;
    const psnode_mlp_f32* mlp[2] = {&de, ae};
    GMlp* g[2] = {&a.de, &a.ae};
    GBwdLayout L{};
    for (int m = 0; m < (ae ? 2 : 1); ++m)
        for (int l = 0, k = mlp[m]->in_dim; l < mlp[m]->n_layers; k = mlp[m]->out_dim[l++])
            g[m]->wt[l] = A.take(up64((size_t)k * mlp[m]->out_dim[l]));
    for (int m = 0; m < (ae ? 2 : 1); ++m)
        for (int l = 0, k = mlp[m]->in_dim; l < mlp[m]->n_layers; k = mlp[m]->out_dim[l++]) {
            L.img[m][l] = A.take(up64(generic_image_floats(k, mlp[m]->out_dim[l])), 64);
            L.imgT[m][l] = A.take(up64(generic_image_floats(mlp[m]->out_dim[l], k)));
        }
    a.wpart = A.take(nwg * (size_t)(a.de.np + (ae ? a.ae.np : 0)));
    // The parent's size paid a whole 64 floats for each of its pointer round-ups (in front of the images -- which consumes nothing, the
    // segments before it being multiples of 64 -- and in front of the tile-major slices) and one more per MLP's images; bytes are kept, so
    // what the one real round-up leaves of them is stated as the remainder.  Beyond the round-ups: kept from the parent, purpose not established.
    const size_t tm_pad = A.pad(64);
    a.tmpart = A.take(nwg * (size_t)(tm_total(a.de) + (ae ? tm_total(a.ae) : 0)), 64);
    A.slack((ae ? 4 : 3) * 64 - tm_pad);
    return L;
}
// The segment-parallel build's workspace: gbwd_layout with one partial per workgroup of the tiles x chunks grid | the grad_all_initial
// partials of the chunks c > 0, [chunks - 1][B][n] | (DAE) the border slots of the chunks c < chunks - 1, [chunks - 1][B][zd + vd]: the
// z | v part of the head VJP at the chunk's last grid point, which is the next chunk's row (msp_fold_kernel adds both where they belong).
struct GBwdMspLayout { GBwdLayout base; float *ga0_part, *border; };
GBwdMspLayout gbwd_msp_layout(const psnode_mlp_f32& de, const psnode_mlp_f32* ae, long long B, int n, int nzv, size_t chunks, GBwd& a, Arena& A) {
    GBwdMspLayout L{};
    L.base = gbwd_layout(de, ae, B, a, A, chunks);
    L.ga0_part = A.take((chunks - 1) * (size_t)B * n);
    L.border = A.take(ae ? (chunks - 1) * (size_t)B * nzv : 0);
    return L;
}
// Behind the sweep of the segment-parallel build, on its stream: grad_all_initial (chunk 0's) += the partials of chunks 1 .. chunks - 1 in
// ascending order, and row (c + 1) span of grad_z / grad_v += chunk c's border slot (span = per_group every grid steps per chunk).  One
// thread per element, each the only writer of its element: bitwise repeatable.  (B_ = the policy: instantiated in its object alone.)
template <class B_>
__global__ void msp_fold_kernel(float* __restrict__ ga0, const float* __restrict__ ga0_part, float* __restrict__ gz, float* __restrict__ gv,
                                const float* __restrict__ border, long long B, int n, int zd, int vd, long long span, int chunks) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x, n_a0 = B * n, nzv = zd + vd;
    if (e < n_a0) {
        float acc = ga0[e];
        for (int c = 1; c < chunks; ++c) acc += ga0_part[(size_t)(c - 1) * n_a0 + e];
        ga0[e] = acc;
        return;
    }
    if (!border || e >= n_a0 + (long long)(chunks - 1) * B * nzv) return;
    const long long q = e - n_a0, c = q / (B * nzv), b = (q / nzv) % B;
    const int r = (int)(q % nzv);
    const bool isz = r < zd;
    float* dst = isz ? gz : gv;
    if (dst) dst[((c + 1) * span * B + b) * (isz ? zd : vd) + (isz ? r : r - zd)] += border[q];
}

// 1: everything in LDS; 2: only with the parameter-gradient accumulators in global memory; 0: does not fit.  a.de_reg (the DE's class
// allows the register path) is kept when its quad-row buffers fit next to the LDS accumulators, else dropped.
int gbwd_mode(GBwd& a, bool pre, int lin = 0) {
    const int want_reg = a.de_reg;
    // paths in order of preference: register DE (+ streamed AE head), everything streamed, then the staged paths; for each, the accumulators
    // in LDS, the AE's in the global slice, both there
    const int cand[4][2] = {{want_reg, a.dae ? 1 : 0}, {0, 2}, {want_reg, 0}, {0, 0}};      // {de_reg, str}
    for (int c = 0; c < 4; ++c) {
        if (c == 0 && !want_reg) continue;
        if (c == 2 && (!want_reg || !a.dae)) continue;
        a.de_reg = cand[c][0]; a.str = cand[c][1];
        a.gacc_global = 0;
        if (gbwd_lds_floats(a, pre, lin) * sizeof(float) <= 160 * 1024) return 1;
        if (a.dae && (a.de_reg || a.str == 2)) {
            a.gacc_global = 2;
            if (gbwd_lds_floats(a, pre, lin) * sizeof(float) <= 160 * 1024) return 2;
        }
        a.gacc_global = 1;
        if (gbwd_lds_floats(a, pre, lin) * sizeof(float) <= 160 * 1024) return 2;
    }
    return 0;
}

int mlp_maxw(const psnode_mlp_f32& m) {
    int w = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) w = m.out_dim[l] > w ? m.out_dim[l] : w;
    return w;
}
bool mlp_ok(const psnode_mlp_f32& m, int in_dim, int out_dim) {
    if (m.n_layers < 1 || m.n_layers > kMaxLayers || m.in_dim != in_dim || m.out_dim[m.n_layers - 1] != out_dim) return false;
    for (int l = 0; l < m.n_layers; ++l)
        if (m.out_dim[l] < 1 || m.out_dim[l] > PSNODE_MAX_WIDTH || !m.weight[l] || !m.bias[l]) return false;
    return true;
}

}  // namespace


// launches pack (transpose), the backward kernel and the partial reduction (`act`: read by the activation builds only)
template <class Pol>
int generic_backward_launch(const GenericBwdCall& c, const ActPair* act, float* workspace, hipStream_t stream) {
    const psnode_mlp_f32 *de = c.de, *ae = c.ae;
    const bool dae = ae != nullptr;
    const long long B = c.B;
    const int n = c.xd + c.zd + (dae ? c.vd + c.id : 0);
    if (!mlp_ok(*de, 3 * n, c.xd)) return PSNODE_ERR_DIMS;
    if (dae && !mlp_ok(*ae, n + c.xd + c.zd + c.vd, c.id)) return PSNODE_ERR_DIMS;
    GBwd a;
    memset(&a, 0, sizeof(a));
    a.method = c.method; a.dae = dae; a.xd = c.xd; a.zd = c.zd; a.vd = c.vd; a.id = c.id; a.T = c.T; a.B = B;
    int rows = fill_gmlp(*de, a.de);
    a.maxw = mlp_maxw(*de);
    if (dae) {
        const int r2 = fill_gmlp(*ae, a.ae);
        rows = r2 > rows ? r2 : rows;
        a.maxw = mlp_maxw(*ae) > a.maxw ? mlp_maxw(*ae) : a.maxw;
    }
    a.act_rows = rows;
    a.t = c.t; a.z = c.z; a.v = c.v; a.a0 = c.a0; a.ev = c.ev; a.zj = c.zj; a.zjb = c.zjb; a.zje = c.zje; a.vj = c.vj; a.vjb = c.vjb;
    a.vje = c.vje; a.n_events = c.n_events; a.xs = c.xs; a.is_ = c.is_; a.gxs = c.gxs; a.gis = c.gis; a.gx0 = c.gx0; a.gz = c.gz; a.gv = c.gv;
    a.gzj = c.gzj; a.gvj = c.gvj; a.ga0 = c.ga0;
    a.flags = c.flags; a.xt = dae ? c.xt : c.xs; a.it = c.it;
    a.de_reg = de_reg_class(*de) ? 1 : 0;
    Arena A{workspace};
    // (the segment-parallel build: a tiles x chunks grid, one partial per workgroup and what crosses a chunk border behind them)
    [[maybe_unused]] unsigned chunks = 1;
    [[maybe_unused]] float *ga0_part = nullptr, *border = nullptr;
    GBwdLayout L;
    if constexpr (Pol::par) {
        chunks = (unsigned)msp_chunks(c.T, c.ms_every, c.ms_per_group);
        const GBwdMspLayout M = gbwd_msp_layout(*de, ae, B, n, c.zd + (dae ? c.vd : 0), chunks, a, A);
        L = M.base; ga0_part = M.ga0_part; border = M.border;
    } else {
        L = gbwd_layout(*de, ae, B, a, A);
    }
    for (int l = 0; l < kMaxLayers; ++l) { a.fimg[l] = L.img[0][l]; a.timg[l] = L.imgT[0][l]; a.fimgA[l] = L.img[1][l]; a.timgA[l] = L.imgT[1][l]; }
    if (!gbwd_mode(a, Pol::pre, Pol::lin_layout)) return PSNODE_ERR_UNSUPPORTED;
    const size_t lds = gbwd_lds_floats(a, Pol::pre, Pol::lin_layout) * sizeof(float);
    place_u_region<Pol::pre>(a, gbwd_lds_floats(a, Pol::pre, Pol::lin_layout), pre_floats(a));
    // transposed weights for the forward recomputation
    MlpDev mde, mae;
    memset(&mde, 0, sizeof(mde));
    memset(&mae, 0, sizeof(mae));
    auto to_dev = [](const GMlp& g, MlpDev& m) {
        m.n_layers = g.L; m.in_dim = g.in_dim;
        for (int l = 0; l < g.L; ++l) { m.out_dim[l] = g.out_dim[l]; m.w[l] = g.w[l]; m.wt[l] = g.wt[l]; m.bias[l] = g.b[l]; }
    };
    to_dev(a.de, mde);
    if (dae) to_dev(a.ae, mae);
    if (launch_pack_transpose(mde, dae ? &mae : nullptr, stream) != hipSuccess) return PSNODE_ERR_HIP;
    if ((a.de_reg || a.str == 2) && launch_pack_plain_images(mde, L.img[0], L.imgT[0], stream) != hipSuccess) return PSNODE_ERR_HIP;
    if (dae && a.str >= 1 && launch_pack_plain_images(mae, L.img[1], L.imgT[1], stream) != hipSuccess) return PSNODE_ERR_HIP;
    // <DE accumulators global, DE on the register path, AE accumulators global, streamed MLPs>
    const unsigned nwg = (unsigned)((B + TB - 1) / TB);
    auto go = [&](const auto&... extra) {
        using K = GenericBwdKernels<Pol, std::decay_t<decltype(extra)>...>;
        auto kern = K::template get<false, false, false, 0>();
        const int g = a.gacc_global;
        if (a.de_reg && a.str == 1) kern = g == 1 ? K::template get<true, true, true, 1>() : (g == 2 ? K::template get<false, true, true, 1>() : K::template get<false, true, false, 1>());
        else if (a.de_reg) kern = g == 1 ? K::template get<true, true, true, 0>() : (g == 2 ? K::template get<false, true, true, 0>() : K::template get<false, true, false, 0>());
        else if (a.str == 2) kern = g == 1 ? K::template get<true, false, true, 2>() : (g == 2 ? K::template get<false, false, true, 2>() : K::template get<false, false, false, 2>());
        else kern = g ? K::template get<true, false, true, 0>() : K::template get<false, false, false, 0>();
        return launch_attr(true, kern, dim3(nwg, Pol::par ? chunks : 1u), dim3(NT), lds, stream, a, extra...);
    };
    hipError_t e;
    if constexpr (Pol::par) e = go(*act, *c.rk, build_sub<Pol>(c.substeps, const_cast<float*>(c.x_sub), 0, c.ms_every, c.ms_x_true, c.ms_per_group, ga0_part, border));
    else if constexpr (Pol::sub) e = go(*act, *c.rk, build_sub<Pol>(c.substeps, const_cast<float*>(c.x_sub), c.ab_pt ? 1 : 0, c.ms_every, c.ms_x_true, 1, nullptr, nullptr, c.stencil, c.rkc));
    else if constexpr (Pol::rk) e = go(*act, *c.rk);
    else if constexpr (Pol::act) e = go(*act);
    else e = go();
    if (e != hipSuccess) return PSNODE_ERR_HIP;
    if constexpr (Pol::par) {
        if (chunks > 1) {
            const int nzv = c.zd + (dae ? c.vd : 0);
            const long long items = B * n + (dae ? (long long)(chunks - 1) * B * nzv : 0);
            hipLaunchKernelGGL(msp_fold_kernel<Pol>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, c.ga0, ga0_part, c.gz, c.gv,
                               dae ? border : nullptr, B, n, c.zd, dae ? c.vd : 0, (long long)c.ms_per_group * c.ms_every, (int)chunks);
            if (hipGetLastError() != hipSuccess) return PSNODE_ERR_HIP;
        }
    }
    return ok_or_hip(launch_reduce_partials(a.wpart, c.gparams_de, c.gparams_ae, a.de.np, dae ? a.ae.np : 0, (int)(nwg * (Pol::par ? chunks : 1u)), stream));
}
template int generic_backward_launch<Bd>(const GenericBwdCall&, const ActPair*, float*, hipStream_t);

}  // namespace psnode
