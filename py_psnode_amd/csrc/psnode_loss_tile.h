// K6's tile walk, written once: the fast tile kernel (D a power of two, float4 streams), the scalar tile kernel (any D <= 64, any strides),
// their host plan, and the pointwise policies.  psnode_loss.hip instantiates it with the squared error (the kernels it always had, the same
// code object: DESIGN.md "K6: loss kinds"); psnode_loss_kinds.hip with L1 / SmoothL1 / Huber and with the per-sample evaluation form.
//
// A policy P gives rho(e) and rho'(e) of one error e = pred - target; the kinds with a parameter (beta / delta) read it, launch-uniform, from
// the device struct LossDevP.
// PS (per-sample form): out[b,d] = sum_t rho(pred * m - target * m), one workgroup per strip of TB trajectories walking that strip's time
// tiles in order -- the SAME tile loop launched with tiles_b workgroups (tile += gridDim.x then steps through one strip's time tiles) --
// one writer and one summation order per out[b,d], no partial rows, no second launch.
#pragma once
#include "psnode_launch.h"

namespace psnode {

// the double-precision, fixed-order sum of the partial rows (psnode_loss.hip): out[c] = sum_rows partial[row][c], out[D+1] = total
hipError_t launch_loss_finish(const float* partial, long long rows, int D, float* out, hipStream_t stream);

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;        // threads per workgroup
constexpr int TT = 16;         // grid points per tile
constexpr int kMaxLossD = 64;  // widest row
constexpr int kMaxBlocks = 2048;

struct LossDev {
    long long T, B;
    int D, mask_w, TB, pitch, mpitch;   // scalar kernel: TB = trajectories per tile; LDS pitches per trajectory (floats)
    ViewDev pred, target, mask;
    const float* col_w;
    const float* inv_norm;
    float scale, t0_coef;
    float* grad;
    float* partial;    // [n_blocks][D+1]
    float* out;
    long long tiles_b, n_tiles;
};
// ... and the parameter of a kind that has one (beta / delta) with its reciprocal
struct LossDevP : LossDev {
    float prm, iprm;
};
// ---- pointwise policies: rho(e) and rho'(e) of one error, p = beta / delta and ip = 1 / p the launch-uniform parameter.  `squared`: the
// training kernels write K6's own products in K6's own order (`wm * er * er`, `2.0f * norm * wm * er`) instead of calling the policy --
// a call, even an inlined one, changes the schedule the compiler gives the wide-row instances, and K6's code object is to stay what it was.
struct RhoMse {
    static constexpr bool squared = true;
    static __device__ __forceinline__ float rho(float e, float, float) { return e * e; }
    static __device__ __forceinline__ float drho(float e, float, float) { return 2.0f * e; }
};
struct RhoL1 {       // rho' = sign(e), 0 at e == 0 (torch's rule)
    static constexpr bool squared = false;
    static __device__ __forceinline__ float rho(float e, float, float) { return fabsf(e); }
    static __device__ __forceinline__ float drho(float e, float, float) { return e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f); }
};
struct RhoSmoothL1 {  // p = beta
    static constexpr bool squared = false;
    static __device__ __forceinline__ float rho(float e, float p, float ip) {
        const float ae = fabsf(e);
        return ae < p ? 0.5f * e * e * ip : ae - 0.5f * p;
    }
    static __device__ __forceinline__ float drho(float e, float p, float ip) { return e <= -p ? -1.0f : (e >= p ? 1.0f : e * ip); }
};
struct RhoHuber {     // p = delta
    static constexpr bool squared = false;
    static __device__ __forceinline__ float rho(float e, float p, float) {
        const float ae = fabsf(e);
        return ae < p ? 0.5f * e * e : p * (ae - 0.5f * p);
    }
    static __device__ __forceinline__ float drho(float e, float p, float) { return fminf(fmaxf(e, -p), p); }
};

// the evaluation expression's error: the mask multiplies both operands, two products and one subtraction, each rounded
__device__ __forceinline__ float masked_err(float p, float t, float m) { return __fsub_rn(__fmul_rn(p, m), __fmul_rn(t, m)); }

// ---------------------------------------------------------------------------------------------------------------
// fast path: D in {1,2,4,...,64}; pred dense time-major (stride_b == D, 16-B aligned rows); target (and a width-D mask)
// dense along time (stride_t == D).  VT: target/mask rows are 16-B aligned, stage them with float4 loads.
template <class P, class Dev, int D, bool VT, bool PS>
__global__ __launch_bounds__(NT) void loss_fast_kernel(const Dev a) {
    constexpr int TB = NT / D;                      // trajectories per tile: one tile row = 256 floats
    constexpr int PK = NT + (D > 4 ? D : 4);        // LDS pitch of one grid point (floats)
    constexpr int MPK = TB + 4;                     // pitch of the width-1 mask tile
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tg = lds;                                // [TT][PK]
    float* mk = lds + TT * PK;                      // [TT][PK] (mask width D) or [TT][MPK] (width 1)

    const int tid = threadIdx.x, kq = tid >> 6, c = tid & 63;
    const int mw = a.mask_w;
    const float norm = PS ? 1.0f : a.scale * (a.inv_norm ? a.inv_norm[0] : 1.0f);
    const float t0c = a.t0_coef;
    float cw[4], acc[4] = {0.f, 0.f, 0.f, 0.f}, acc0 = 0.0f;
    if constexpr (!PS) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cw[e] = a.col_w ? a.col_w[(4 * c + e) % D] : 1.0f;
    }

    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long b0 = (tile % a.tiles_b) * TB, k0 = (tile / a.tiles_b) * TT;
        const int nb = (int)(a.B - b0 < TB ? a.B - b0 : TB), nk = (int)(a.T - k0 < TT ? a.T - k0 : TT);

        // ---- pred: issue the tile's loads first (4 grid points per thread, floats 4c..4c+3 of the 256-float tile row)
        const bool colv = (4 * c) / D < nb;
        f4 p4[TT / 4];
#pragma unroll
        for (int it = 0; it < TT / 4; ++it) {
            const int kk = kq + 4 * it;
            p4[it] = (colv && kk < nk) ? *reinterpret_cast<const f4*>(a.pred.p + (k0 + kk) * a.pred.st + b0 * D + 4 * c)
                                       : f4{0.f, 0.f, 0.f, 0.f};
        }
        // ---- target (and width-D mask): contiguous along time per trajectory -> time-major LDS tile
        auto stage = [&](const ViewDev& v, float* dst) {
            if constexpr (VT) {
                constexpr int V = TT * D / 4, PER = TB * V / NT;   // float4 per trajectory; per thread
                f4 r[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + NT * i, bl = idx / V, q = idx % V, kk = (4 * q) / D, d0 = (4 * q) % D;
                    r[i] = (bl < nb && kk < nk) ? *reinterpret_cast<const f4*>(v.p + (b0 + bl) * v.sb + (k0 + kk) * D + d0)
                                                : f4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + NT * i, bl = idx / V, q = idx % V, kk = (4 * q) / D, d0 = (4 * q) % D;
                    *reinterpret_cast<f4*>(dst + kk * PK + bl * D + d0) = r[i];
                }
            } else {
                constexpr int R = TT * D, PER = TB * R / NT;       // floats per trajectory; per thread (= TT)
                float r[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + NT * i, bl = idx / R, q = idx % R;
                    r[i] = (bl < nb && q / D < nk) ? v.p[(b0 + bl) * v.sb + k0 * D + q] : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + NT * i, bl = idx / R, q = idx % R;
                    dst[(q / D) * PK + bl * D + (q % D)] = r[i];
                }
            }
        };
        stage(a.target, tg);
        if (mw == D && D > 1) stage(a.mask, mk);
        else if (mw == 1) {
            for (int idx = tid; idx < TB * TT; idx += NT) {
                const int bl = idx / TT, kk = idx % TT;
                mk[kk * MPK + bl] = (bl < nb && kk < nk) ? a.mask.p[(b0 + bl) * a.mask.sb + (k0 + kk) * a.mask.st] : 0.0f;
            }
        }
        __syncthreads();

        // ---- stream against the tile
#pragma unroll
        for (int it = 0; it < TT / 4; ++it) {
            const int kk = kq + 4 * it;
            const long long k = k0 + kk;
            const f4 t4 = *reinterpret_cast<const f4*>(tg + kk * PK + 4 * c);
            f4 m4 = f4{1.f, 1.f, 1.f, 1.f};
            if (mw == D && D > 1) m4 = *reinterpret_cast<const f4*>(mk + kk * PK + 4 * c);
            else if (mw == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) m4[e] = mk[kk * MPK + (4 * c + e) / D];
            }
            if constexpr (PS) {     // rows past the tile's edge hold zeros in both operands: rho(0) = 0
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += P::rho(masked_err(p4[it][e], t4[e], m4[e]), a.prm, a.iprm);
            } else {
                f4 g4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float er = p4[it][e] - t4[e];
                    const float wm = cw[e] * m4[e];
                    if constexpr (P::squared) {
                        acc[e] += wm * er * er;
                        g4[e] = 2.0f * norm * wm * er;
                        if (k == 0) { acc0 += er * er; g4[e] += 2.0f * t0c * er; }
                    } else {
                        acc[e] += wm * P::rho(er, a.prm, a.iprm);
                        g4[e] = norm * wm * P::drho(er, a.prm, a.iprm);
                        if (k == 0) { acc0 += P::rho(er, a.prm, a.iprm); g4[e] += t0c * P::drho(er, a.prm, a.iprm); }
                    }
                }
                if (a.grad && colv && kk < nk) *reinterpret_cast<f4*>(a.grad + (k * a.B + b0) * D + 4 * c) = g4;
            }
        }
        __syncthreads();
    }

    if constexpr (PS) {
        // ---- this strip's table rows: the four waves hold grid points kk = kq (mod 4) of the same 256 (trajectory, column) slots
        float* red = lds;                           // [4 waves][NT]  (tiles are done: the last loop ended on a barrier)
        *reinterpret_cast<f4*>(red + kq * NT + 4 * c) = f4{acc[0], acc[1], acc[2], acc[3]};
        __syncthreads();
        const long long b0 = (long long)blockIdx.x * TB;
        const int nb = (int)(a.B - b0 < TB ? a.B - b0 : TB);
        if (tid < nb * D) a.out[b0 * D + tid] = (red[tid] + red[NT + tid]) + (red[2 * NT + tid] + red[3 * NT + tid]);
    } else {
        // ---- workgroup sums, fixed order.  Column of acc[e] = (4c+e) % D: lanes that differ only in bits >= log2(D/4)
        //      of c hold the same columns -> xor butterflies over those bits.
        constexpr int LOW = D >= 4 ? D / 4 : 1;
#pragma unroll
        for (int m = 32; m >= LOW; m >>= 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], m, 64);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc0 += __shfl_xor(acc0, m, 64);
        float* red = lds;                               // [4 waves][D + 1]  (tiles are done: the last loop ended on a barrier)
        if (c < LOW) {
            if constexpr (D >= 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) red[kq * (D + 1) + 4 * c + e] = acc[e];
            } else if constexpr (D == 2) {
                red[kq * 3 + 0] = acc[0] + acc[2];
                red[kq * 3 + 1] = acc[1] + acc[3];
            } else {
                red[kq * 2] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            }
            if (c == 0) red[kq * (D + 1) + D] = acc0;
        }
        __syncthreads();
        if (tid <= D) {
            const float s = (red[tid] + red[(D + 1) + tid]) + (red[2 * (D + 1) + tid] + red[3 * (D + 1) + tid]);
            a.partial[(long long)blockIdx.x * (D + 1) + tid] = s * (tid < D ? norm : t0c);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// scalar path: any D <= 64, any strides.  Thread = (trajectory, column); the training form runs one tile per workgroup, the per-sample
// form one strip of TB trajectories per workgroup (its time tiles in order).
template <class P, class Dev, bool PS>
__global__ __launch_bounds__(NT) void loss_scalar_kernel(const Dev a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tg = lds;                                   // [TB][pitch]   target tile  (b, k, d)
    float* mk = tg + (size_t)a.TB * a.pitch;           // [TB][mpitch]  mask tile
    float* red = mk + (size_t)a.TB * a.mpitch;         // [2][NT]       block reduction

    const int tid = threadIdx.x, D = a.D, TB = a.TB;
    long long tile = blockIdx.x;
    float acc = 0.0f, acc0 = 0.0f;
    // the training form leaves this loop after its one tile; the per-sample form walks its strip's time tiles (tile += tiles_b)
    for (;;) {
        const long long b0 = (tile % a.tiles_b) * TB, k0 = (tile / a.tiles_b) * TT;
        const int nb = (int)(a.B - b0 < TB ? a.B - b0 : TB), nk = (int)(a.T - k0 < TT ? a.T - k0 : TT);

        // target / mask tile -> LDS, walked in the operand's own contiguous order
        const bool b_major = a.target.st <= a.target.sb;   // [B,T,D] memory: time is the inner run
        const int row = TT * D;
        for (int idx = tid; idx < TB * row; idx += NT) {
            int bl, kk, d;
            if (b_major) { bl = idx / row; kk = (idx % row) / D; d = idx % D; }
            else { kk = idx / (TB * D); bl = (idx % (TB * D)) / D; d = idx % D; }
            if (bl < nb && kk < nk) tg[bl * a.pitch + kk * D + d] = a.target.p[(k0 + kk) * a.target.st + (b0 + bl) * a.target.sb + d];
        }
        if (a.mask_w > 0) {
            const int mw = a.mask_w, mrow = TT * mw;
            const bool mb_major = a.mask.st <= a.mask.sb;
            for (int idx = tid; idx < TB * mrow; idx += NT) {
                int bl, kk, d;
                if (mb_major) { bl = idx / mrow; kk = (idx % mrow) / mw; d = idx % mw; }
                else { kk = idx / (TB * mw); bl = (idx % (TB * mw)) / mw; d = idx % mw; }
                if (bl < nb && kk < nk) mk[bl * a.mpitch + kk * mw + d] = a.mask.p[(k0 + kk) * a.mask.st + (b0 + bl) * a.mask.sb + d];
            }
        }
        __syncthreads();

        const int bl = tid / D, d = tid % D;
        if constexpr (PS) {
            if (bl < nb) {
                const float* pp = a.pred.p + (b0 + bl) * a.pred.sb + d;
                const float* tl = tg + bl * a.pitch + d;
                const float* ml = mk + bl * a.mpitch + (a.mask_w == D ? d : 0);
                const int mw = a.mask_w;
#pragma unroll 4
                for (int kk = 0; kk < nk; ++kk)
                    acc += P::rho(masked_err(pp[(k0 + kk) * a.pred.st], tl[kk * D], mw > 0 ? ml[kk * mw] : 1.0f), a.prm, a.iprm);
            }
            __syncthreads();                           // the next tile overwrites tg / mk
            tile += gridDim.x;
            if (tile >= a.n_tiles) {
                if (bl < nb) a.out[b0 * D + tid] = acc;    // tid = bl * D + d: one writer per out[b,d]
                break;
            }
        } else {
            const float norm = a.scale * (a.inv_norm ? a.inv_norm[0] : 1.0f);
            if (bl < nb) {
                const float cw = a.col_w ? a.col_w[d] : 1.0f;
                const float* pp = a.pred.p + (b0 + bl) * a.pred.sb + d;
                float* gp = a.grad ? a.grad + (b0 + bl) * D + d : nullptr;
                const float* tl = tg + bl * a.pitch + d;
                const float* ml = mk + bl * a.mpitch + (a.mask_w == D ? d : 0);
                const int mw = a.mask_w;
#pragma unroll 4
                for (int kk = 0; kk < nk; ++kk) {
                    const long long k = k0 + kk;
                    const float e = pp[k * a.pred.st] - tl[kk * D];
                    const float wm = cw * (mw > 0 ? ml[kk * mw] : 1.0f);
                    float g;
                    if constexpr (P::squared) {      // K6's expressions in K6's order, written out (see the fast kernel)
                        acc += wm * e * e;
                        g = 2.0f * norm * wm * e;
                        if (k == 0) { acc0 = e * e; g += 2.0f * a.t0_coef * e; }
                    } else {
                        acc += wm * P::rho(e, a.prm, a.iprm);
                        g = norm * wm * P::drho(e, a.prm, a.iprm);
                        if (k == 0) { acc0 = P::rho(e, a.prm, a.iprm); g += a.t0_coef * P::drho(e, a.prm, a.iprm); }
                    }
                    if (gp) gp[k * a.B * D] = g;
                }
            }
            red[tid] = acc;
            red[NT + tid] = acc0;
            __syncthreads();
            if (tid <= D) {
                float s = 0.0f;
                if (tid < D) { for (int q = 0; q < nb; ++q) s += red[q * D + tid]; s *= norm; }
                else { for (int q = 0; q < nb * D; ++q) s += red[NT + q]; s *= a.t0_coef; }
                a.partial[tile * (D + 1) + tid] = s;
            }
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host: plan, path selection, the checks of a call
bool plan(const psnode_loss_args_f32* a, LossDev& d) {
    if (a->T < 1 || a->B < 1 || a->D < 1 || a->D > kMaxLossD) return false;
    if (a->mask_width != 0 && a->mask_width != 1 && a->mask_width != a->D) return false;
    d.T = a->T; d.B = a->B; d.D = a->D; d.mask_w = a->mask_width;
    d.TB = NT / a->D;
    // pitch == D (mod 64): lanes (bl, d) of one wave hit 64 distinct LDS banks
    auto pitch_for = [&](int w) { return w > 0 ? ((TT * w - w + 63) / 64) * 64 + w : 0; };
    d.pitch = pitch_for(a->D);
    d.mpitch = pitch_for(a->mask_width);
    d.tiles_b = (a->B + d.TB - 1) / d.TB;
    d.n_tiles = d.tiles_b * ((a->T + TT - 1) / TT);
    return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 0: scalar kernel; 1: fast kernel, scalar staging; 2: fast kernel, float4 staging
int fast_mode(const psnode_loss_args_f32* a) {
    const int D = a->D;
    if (D & (D - 1)) return 0;
    if (a->pred.stride_b != D || (a->pred.stride_t & 3) || !aligned16(a->pred.ptr) || ((a->B * D) & 3)) return 0;
    if (a->grad_pred && !aligned16(a->grad_pred)) return 0;
    if (a->target.stride_t != D) return 0;
    if (a->mask_width == D && D > 1 && a->mask.stride_t != D) return 0;
    bool vt = D >= 4 && !(a->target.stride_b & 3) && aligned16(a->target.ptr);
    if (a->mask_width == D && D > 1) vt = vt && !(a->mask.stride_b & 3) && aligned16(a->mask.ptr);
    return vt ? 2 : 1;
}

long long block_rows(const psnode_loss_args_f32* a, const LossDev& d) {
    if (!fast_mode(a)) return d.n_tiles;
    return d.n_tiles < kMaxBlocks ? d.n_tiles : kMaxBlocks;
}

// K6's checks of a non-NULL args, in K6's order, and the device struct of a call that passes them:
//   dims (T, B, D >= 1; mask_width 0 | 1 | D) -> DIMS;  D > 64 -> UNSUPPORTED;  pred / target / out / mask pointers -> NULL;
//   more than 2^31 - 1 tiles -> UNSUPPORTED
int loss_call_dev(const psnode_loss_args_f32* a, LossDev& d) {
    if (a->T < 1 || a->B < 1 || a->D < 1) return PSNODE_ERR_DIMS;
    if (a->mask_width != 0 && a->mask_width != 1 && a->mask_width != a->D) return PSNODE_ERR_DIMS;
    if (!plan(a, d)) return PSNODE_ERR_UNSUPPORTED;
    if (!a->pred.ptr || !a->target.ptr || !a->out || (a->mask_width > 0 && !a->mask.ptr)) return PSNODE_ERR_NULL;
    if (d.n_tiles > 0x7fffffffLL) return PSNODE_ERR_UNSUPPORTED;
    d.pred = {a->pred.ptr, a->pred.stride_t, a->pred.stride_b};
    d.target = {a->target.ptr, a->target.stride_t, a->target.stride_b};
    d.mask = {a->mask.ptr, a->mask.stride_t, a->mask.stride_b};
    d.col_w = a->col_weight; d.inv_norm = a->inv_norm; d.scale = a->scale; d.t0_coef = a->t0_coef;
    d.grad = a->grad_pred; d.partial = nullptr; d.out = a->out;
    return PSNODE_OK;
}
// ... then the partial rows [n_tiles][D+1] (sized for the scalar kernel, so that the same workspace serves either kernel)
size_t loss_partial_bytes(const psnode_loss_args_f32* a, const LossDev& d) { return (size_t)d.n_tiles * (a->D + 1) * sizeof(float); }
bool loss_workspace_ok(const void* ws, size_t bytes, size_t need) { return ws && bytes >= need && !((uintptr_t)ws & 15); }

// LDS of the two kernels (bytes)
template <int D>
size_t loss_fast_lds(const LossDev& d, bool per_sample) {
    constexpr int PK = NT + (D > 4 ? D : 4), MPK = NT / D + 4;
    size_t fl = (size_t)TT * PK + (d.mask_w == D && D > 1 ? (size_t)TT * PK : (d.mask_w == 1 ? (size_t)TT * MPK : 0));
    if (fl < 4 * (D + 1)) fl = 4 * (D + 1);
    if (per_sample && fl < 4 * NT) fl = 4 * NT;
    return fl * sizeof(float);
}
size_t loss_scalar_lds(const LossDev& d) { return ((size_t)d.TB * (d.pitch + d.mpitch) + 2 * NT) * sizeof(float); }

// ---- launch of the tile kernels of one policy P on its device struct Dev.  Training form: one workgroup per tile, at most kMaxBlocks on
// the fast path (*rows = partial rows written); per-sample form (PS): one workgroup per strip of trajectories.
template <class P, class DevT, bool PS>
struct LossKernels {
    static constexpr bool per_sample = PS;
    template <int D, bool VT>
    static auto fast() { return &loss_fast_kernel<P, DevT, D, VT, PS>; }
    static auto scalar() { return &loss_scalar_kernel<P, DevT, PS>; }
};
template <class K, int D, class Dev>
hipError_t launch_loss_fast(const Dev& d, int mode, unsigned blocks, hipStream_t s) {
    const size_t lds = loss_fast_lds<D>(d, K::per_sample);
    if constexpr (D >= 4) {
        if (mode == 2) {
            hipLaunchKernelGGL((K::template fast<D, true>()), dim3(blocks), dim3(NT), lds, s, d);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((K::template fast<D, false>()), dim3(blocks), dim3(NT), lds, s, d);
    return hipGetLastError();
}

template <class K, class Dev>
hipError_t launch_loss_tiles(const psnode_loss_args_f32* a, const Dev& d, hipStream_t s, long long* rows) {
    const int mode = fast_mode(a);
    *rows = K::per_sample ? d.tiles_b : block_rows(a, d);
    if (mode)
        return pick<1, 2, 4, 8, 16, 32, 64>(a->D, [&](auto tag) { return launch_loss_fast<K, decltype(tag)::value>(d, mode, (unsigned)*rows, s); });
    hipLaunchKernelGGL(K::scalar(), dim3((unsigned)*rows), dim3(NT), loss_scalar_lds(d), s, d);
    return hipGetLastError();
}

}  // namespace
}  // namespace psnode
