// Generic fused fixed-grid integrator for gfx950 (K0), the part all four builds share: any layer count, layer widths and state dims within the ABI limits.
//
// One launch integrates ALL T-1 steps: a workgroup of four waves owns TB = 16 trajectories (they never interact, my_solvers.py:66 is
// row-wise over the batch) and walks the time grid with its state in LDS.  This is the always-available HIP path: the shapes outside
// the specialised integrators' classes (x_dim > 16, z + v + i > 8, depth != 3 hidden layers, mixed or very wide layers -- all of them
// data- or user-defined upstream, neural_00_ODE_01_no_encode.py:293) run here.
//
// Round 6: the Linear layers run on v_mfma_f32_16x16x4_f32 (before: one fp32 fmaf chain per (unit, 4 trajectories) item with the
// weights re-staged through LDS for every layer of every evaluation).  D[i = unit][j = trajectory] += A[i][k] * B[k][j]:
//   * activations live in LDS in QUAD-ROW order, float index ((col / 4) * 16 + traj) * 4 + col % 4: MFMA step (q, c) -- c = 0..3 -- takes
//     the columns 16 q + 4 k + c in its k-slot k, so lane (k, j)'s B operands of four consecutive steps are ONE lane-linear ds_read_b128
//     (f4 index 64 q + lane), and a D tile (lane (g, j), register r = unit 16 nt + 4 g + r) goes back as ONE lane-linear ds_write_b128
//     (f4 index 64 nt + lane): no transposes, no bank conflicts;
//   * the weights come from an image in the workspace (pack_image_kernel), [tile nt][q][lane] f4 with the same column order, zero-padded
//     to 16 rows x 16 columns.  Layers whose images fit the LDS left over (greedy in layer order, DE first: generic_plan) are copied there
//     once per launch and read like the activations; the others are STREAMED: one coalesced 1 KB global load per four MFMAs, L2-resident
//     (every workgroup reads the same image every evaluation), issued one chunk of 16 MFMAs ahead and in flight across the layer barrier
//     (lds_barrier waits for LDS traffic only);
//   * output tile nt of a layer belongs to wave nt % 4; bias (padded, in LDS) added behind the MFMAs; ELU on the
//     accumulator; one barrier per layer.
// The two MLP inputs (DE: a0 | s - a0 | s, AE: a0 | x | z | v) have their own buffers and keep their constant columns between evaluations:
// a0 is written once, the externals once per step, and per stage only the state's columns -- by the same pass that applies the stage's
// update, so an evaluation costs its layers' barriers plus one.  The next grid point's clocks, event index and z | v rows are loaded a
// step ahead (registers), the AE head's input of the end-of-step evaluation is written by the last stage's update.
// Padded columns: the image holds zeros there and the input builders write zeros into the pad columns of the first layer's input; a
// hidden layer's pad units come out of the MFMA as ELU(0 + 0) = 0.
//
// One object per build policy is compiled from this header (psnode_generic_build.h: each alias with its one-line description).  A policy's
// file psnode_generic_<fam>.hip names it as PSNODE_BUILD in front of the include; the kernel (generic_kernel, around psnode_generic_body.h)
// and the launcher (launch_generic<Bd>) are written below, once.
// The device functions take the activation as one ordinary parameter, ActCtx; the kernel body chooses the tableau code with
// `if constexpr (Bd::rk)`, the sub-step code with `if constexpr (Bd::sub)`.  The host's plan / fit / pack code is compiled once, in
// psnode_generic.hip.
#pragma once
#include "psnode_act.h"
#include "psnode_generic_tile.h"
#include "psnode_launch.h"

namespace psnode {

namespace {

using Bd = PSNODE_BUILD;

// The hidden-layer activation of one MLP as mlp_eval / mlp_reg / mlp_regw see it: ELU(1) carries nothing, the act build the MLP's ActDev
// (six kinds, act_quad), the pre and tableau builds the same for all ten kinds (pre_act_quad; the forward needs no pre-activation)
__device__ __forceinline__ NoAct act_pick(bool, NoAct, NoAct) { return {}; }
template <bool ACT, bool PRE> struct ActCtxT;
template <> struct ActCtxT<false, false> {
    __device__ __forceinline__ ActCtxT(NoAct) {}
    __device__ __forceinline__ f4 actq(f4 v) const { return elu_quad(v); }
};
template <> struct ActCtxT<true, false> {
    const ActDev& ac;
    __device__ __forceinline__ f4 actq(f4 v) const { return act_quad(v, ac); }
};
template <> struct ActCtxT<true, true> {
    const ActDev& ac;
    __device__ __forceinline__ f4 actq(f4 v) const { return pre_act_quad(v, ac); }
};
using ActCtx = ActCtxT<Bd::act, Bd::pre>;

// Column order of the two MLP inputs (the first layers' images use the same one): the columns that change most often come first and end on
// a quad boundary, so that the register forms can fold everything behind them into a per-step (DE) / per-trajectory (AE) constant.
//   DE  cat(a0, s - a0, s) (DE_Func.forward):   [ (s - a0)_x | s_x | pad to SX ] [ a0 | (s - a0)_ext | s_ext | pad ]    ext = z | v | i
//   AE  cat(a0, x, z, v)   (AE_Func.forward):   [ x | z | v | pad to SA ] [ a0 | pad ]
__host__ __device__ constexpr int de_sx(int xd) { return up16(2 * xd); }
__host__ __device__ constexpr int de_k16(int xd, int n) { return de_sx(xd) + up16(n + 2 * (n - xd)); }
__host__ __device__ inline int de_orig_col(int k, int xd, int n) {      // -> column of the nn.Linear weight, -1: pad
    const int ne = n - xd;
    if (k < xd) return n + k;
    if (k < 2 * xd) return 2 * n + (k - xd);
    if (k < de_sx(xd)) return -1;
    k -= de_sx(xd);
    if (k < n) return k;
    if (k < n + ne) return n + xd + (k - n);
    if (k < n + 2 * ne) return 2 * n + xd + (k - n - ne);
    return -1;
}
__host__ __device__ constexpr int ae_sa(int xd, int nzv) { return up16(xd + nzv); }
__host__ __device__ constexpr int ae_k16(int xd, int nzv, int n) { return ae_sa(xd, nzv) + up16(n); }
__host__ __device__ inline int ae_orig_col(int k, int xd, int nzv, int n) {
    if (k < xd + nzv) return n + k;
    if (k < ae_sa(xd, nzv)) return -1;
    k -= ae_sa(xd, nzv);
    return k < n ? k : -1;
}

// floats of one layer's image: N16 x K16 weights + N16 biases
// (+ 16 columns: the two padded blocks of a first layer)
__host__ __device__ constexpr size_t image_floats(int K, int N) { return (size_t)up16(N) * (up16(K) + 16) + up16(N); }
// floats of the padded biases of every layer (LDS region behind the kernel's state)
__host__ __device__ inline int generic_bias_floats(const IntegrateDev& a, bool dae) {
    int tot = 0;
    for (int l = 0; l < a.de.n_layers; ++l) tot += up16(a.de.out_dim[l]);
    if (dae) for (int l = 0; l < a.ae.n_layers; ++l) tot += up16(a.ae.out_dim[l]);
    return tot;
}

// One MLP as the time loop sees it: wave-uniform scalars, built once per launch so that no kernel-argument load (a scalar-cache round trip,
// and an lgkmcnt wait that also drains the LDS queue) sits between two chunks.  The layer loop of mlp_eval is fully unrolled over
// ML (4 or kMaxLayers: the kernel is instantiated for both), which makes every index below a constant.
template <int ML>
struct Tab {
    int L;
    unsigned dims[ML];     // resident << 31 | quads of the contraction (ceil(K / 16)) << 16 | output tiles (ceil(N / 16))
    unsigned off[ML];      // streamed layer: f4 offset of its image from `base`; resident layer: FLOAT offset of its copy in LDS
    unsigned boff[ML];     // float offset of the padded bias in LDS
    const f4* base;                // image of layer 0 (workspace)
    int qx;                        // quads of layer 0's leading block (DE: the state's columns, AE: x | z | v)
    unsigned first_off;            // this wave's first STREAMED chunk of an evaluation: f4 offset ...
    int first_q;                   // ... and the quads of that tile (0: the wave owns no tile in a streamed layer of this MLP)
};
__device__ __forceinline__ int tab_tiles(unsigned d) { return (int)(d & 0xffffu); }
__device__ __forceinline__ int tab_quads(unsigned d) { return (int)((d >> 16) & 0x7fffu); }
__device__ __forceinline__ bool tab_res(unsigned d) { return (d >> 31) != 0; }

// `res`: bit l = layer l's image is resident in LDS; `bias_at` / `img_at`: running float offsets of the LDS regions (advanced)
// k0 / qx: layer 0's padded contraction length (de_k16 / ae_k16) and the quads of its leading block
template <int ML>
__device__ __forceinline__ Tab<ML> make_tab(const MlpDev& m, int w, unsigned res, unsigned& bias_at, unsigned& img_at, int k0, int qx) {
    Tab<ML> t;
    t.L = m.n_layers;
    t.qx = qx;
    t.base = reinterpret_cast<const f4*>(m.wt[0]);
    t.first_off = 0; t.first_q = 0;
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        const int K = l ? m.out_dim[l - 1] : k0, N = m.out_dim[l];
        const unsigned S4 = (K + 15) >> 4, NTL = (N + 15) >> 4;
        const bool on = l < m.n_layers, r = on && ((res >> l) & 1u);
        t.dims[l] = on ? ((r ? 1u << 31 : 0u) | S4 << 16 | NTL) : 0u;
        t.off[l] = !on ? 0u : (r ? img_at : (unsigned)((m.wt[l] - m.wt[0]) >> 2));
        t.boff[l] = bias_at;
        if (on) bias_at += 16u * NTL;
        if (r) img_at += 256u * NTL * S4;
    }
#pragma unroll
    for (int l = ML - 1; l >= 0; --l)
        if (l < m.n_layers && !tab_res(t.dims[l]) && tab_tiles(t.dims[l]) > w) {
            t.first_off = t.off[l] + (unsigned)w * tab_quads(t.dims[l]) * 64u;
            t.first_q = tab_quads(t.dims[l]);
        }
    return t;
}

// field-by-field select (a ternary on the structs goes through a stack copy: scratch)
template <int ML>
__device__ __forceinline__ Tab<ML> pick_tab(bool first, const Tab<ML>& x, const Tab<ML>& y) {
    // readfirstlane: the results are wave-uniform and have to stay scalar -- kept in VGPRs (the compiler does that under SGPR pressure)
    // every loop bound of mlp_eval turns into exec-mask control flow
    auto u = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
    Tab<ML> t;
    t.L = (int)u(first ? x.L : y.L);
    t.qx = (int)u(first ? x.qx : y.qx);
    const unsigned long long pb = reinterpret_cast<unsigned long long>(first ? x.base : y.base);
    t.base = reinterpret_cast<const f4*>((unsigned long long)u((unsigned)(pb >> 32)) << 32 | u((unsigned)pb));
    t.first_off = u(first ? x.first_off : y.first_off);
    t.first_q = (int)u(first ? x.first_q : y.first_q);
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        t.dims[l] = u(first ? x.dims[l] : y.dims[l]);
        t.off[l] = u(first ? x.off[l] : y.off[l]);
        t.boff[l] = u(first ? x.boff[l] : y.boff[l]);
    }
    return t;
}

// copies the biases (always) and the resident images into LDS; no barrier
template <int ML>
__device__ __forceinline__ void load_resident(const MlpDev& m, const Tab<ML>& t, float* lds) {
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l >= t.L) break;
        const int NTL = tab_tiles(t.dims[l]), S4 = tab_quads(t.dims[l]);
        const float* __restrict__ src = m.wt[l];
        for (int i = threadIdx.x; i < 16 * NTL; i += NT) lds[t.boff[l] + i] = src[(size_t)NTL * S4 * 256 + i];
        if (tab_res(t.dims[l]))
            for (int i = threadIdx.x; i < NTL * S4 * 64; i += NT) reinterpret_cast<f4*>(lds + t.off[l])[i] = reinterpret_cast<const f4*>(src)[i];
    }
}

// A-operand look-ahead carried from one layer / MLP evaluation into the next: one chunk (up to four f4 = 16 MFMA steps).
//   STREAM kernels: the wave's next chunk among the STREAMED layers, from the workspace image (hides the L2 latency);
//   all-resident kernels: chunk 0 of the wave's first tile of the next layer, read from LDS in front of the layer barrier, so that only
//   the activations are read behind it.
// `tag`: the MLP (its workspace image) whose first chunk `a` holds at the start of an evaluation; a wrong guess costs one more read.
struct Pref {
    f4 a[4];
    const f4* tag;
};

// (PSNODE_K0_ABL, psnode_generic_tile.h: ablation builds, timing only, wrong results -- 1 = a quarter of the MFMAs, 2 = no ELU, 3 = no layer barrier,
//  4 = no MLP at all, 5 = no operand reads / MFMAs, 6 = no look-ahead read)
// One output tile with both operands in LDS, Q quads, straight-line: every read in flight before the first MFMA, two accumulator chains.
// PA: the A operands of quads 0 .. 3 come from `pa` (read in front of the layer barrier).  With one wave per SIMD nothing hides a taken
// branch (an instruction-cache round trip each): a loop over the quads with its guards and tails cost more than the MFMAs it issued
// (profiles/r06_k0_generic_mfma.txt), so the contraction lengths up to 128 columns get a body each and the layer picks one with a switch.
template <int Q, bool PA>
__device__ __forceinline__ f4 tile_body(const f4* at, const f4* bq, const f4 (&pa)[4]) {
    f4 av[Q], bv[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) {
        bv[c] = bq[c * 64];
        if (PA && c < 4) av[c] = pa[c]; else av[c] = at[c * 64];
    }
    __builtin_amdgcn_sched_barrier(0);
    f4 acc = f4{0.f, 0.f, 0.f, 0.f}, acc2 = acc;
#pragma unroll
    for (int c = 0; c < Q; ++c) mfma_quad(av[c], bv[c], (c & 1) ? acc2 : acc);
    return Q > 1 ? acc + acc2 : acc;
}
template <bool PA>
__device__ __forceinline__ f4 tile_any(int S4, const f4* at, const f4* bq, const f4 (&pa)[4]) {
    switch (S4) {
        case 1: return tile_body<1, PA>(at, bq, pa);
        case 2: return tile_body<2, PA>(at, bq, pa);
        case 3: return tile_body<3, PA>(at, bq, pa);
        case 4: return tile_body<4, PA>(at, bq, pa);
        case 5: return tile_body<5, PA>(at, bq, pa);
        case 6: return tile_body<6, PA>(at, bq, pa);
        case 7: return tile_body<7, PA>(at, bq, pa);
        case 8: return tile_body<8, PA>(at, bq, pa);
        default: break;
    }
    // longer contractions: eight quads straight, then chunks of four and single quads
    f4 acc = tile_body<8, PA>(at, bq, pa), acc2 = f4{0.f, 0.f, 0.f, 0.f};
    int q0 = 8;
    for (; q0 + 4 <= S4; q0 += 4) {
        f4 av[4], bv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { av[c] = at[(q0 + c) * 64]; bv[c] = bq[(q0 + c) * 64]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) mfma_quad(av[c], bv[c], (c & 1) ? acc2 : acc);
    }
    for (; q0 < S4; ++q0) mfma_quad(at[q0 * 64], bq[q0 * 64], acc);
    return acc + acc2;
}

// MLP over the TB columns: layer 0 reads the quad-row buffer at float offset `in`, the layers write `ping` / `pong` alternately; returns
// the offset of the last layer's output.  Ends with a barrier.  `nx`: the MLP evaluated after this one.
template <bool STREAM, int ML>
__device__ __forceinline__ int mlp_eval(const Tab<ML>& T, float* lds, int in, const int ping, const int pong, Pref& pf, const Tab<ML>& nx, const ActCtx& cx) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // STREAM: chunk = quads q0 .. q0 + 3 of one tile, clamped inside the tile's run of the image (in bounds, unused beyond the tile's quads).
    // The address comes out of scalar selects and the four loads are unconditional straight-line code: a load inside a conditional block
    // gets its result copied (and waited for) at the end of that block, in front of the MFMAs it should overlap.
    auto fetch = [&](const f4* base, unsigned off, int rem, f4 (&a)[4]) {
        const f4* __restrict__ A = base + off + lane;
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = A[(c < rem ? c : rem - 1) * 64];
    };
    // all-resident: chunk 0 of tile w of layer l of t, from LDS (nothing if the wave has no tile there)
    auto peek = [&](const Tab<ML>& t, int l, f4 (&a)[4]) {
        const int S4 = tab_quads(t.dims[l]);
        if (w < tab_tiles(t.dims[l])) {
            const f4* at = reinterpret_cast<const f4*>(lds + t.off[l]) + w * S4 * 64 + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] = at[(c < S4 ? c : S4 - 1) * 64];
        }
    };
    if constexpr (STREAM) {
        if (pf.tag != T.base && T.first_q > 0) fetch(T.base, T.first_off, T.first_q, pf.a);
    } else {
        if (pf.tag != T.base) peek(T, 0, pf.a);
    }
    int out = ping;
    if (PSNODE_K0_ABL == 4) { lds_barrier(); return out; }
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l >= T.L) break;
        out = (l & 1) ? pong : ping;
        const int S4 = tab_quads(T.dims[l]), NTL = tab_tiles(T.dims[l]);
        const bool last = (l + 1 == T.L);
        const f4* bq = reinterpret_cast<const f4*>(lds + in) + lane;
        const f4* b16 = reinterpret_cast<const f4*>(lds + T.boff[l]) + (lane >> 4);
        f4* oq = reinterpret_cast<f4*>(lds + out) + lane;
        auto finish = [&](f4 acc, const f4 bias, int nt) {
            acc = acc + bias;
            const f4 e = PSNODE_K0_ABL != 2 ? cx.actq(acc) : acc;
            oq[nt * 64] = last ? acc : e;         // a select, not a branch
        };
        if (!STREAM || tab_res(T.dims[l])) {
            const f4* aq = reinterpret_cast<const f4*>(lds + T.off[l]) + lane;
            int nt = w;
            if constexpr (!STREAM) {
                if (nt < NTL) {                              // first tile: the A operands of its first four quads were read in front of the barrier
                    const f4 bias = b16[4 * nt];
                    finish(PSNODE_K0_ABL == 5 ? bias : tile_any<true>(S4, aq + nt * S4 * 64, bq, pf.a), bias, nt);
                    nt += 4;
                }
            }
            for (; nt < NTL; nt += 4) {
                const f4 bias = b16[4 * nt];
                finish(tile_any<false>(S4, aq + nt * S4 * 64, bq, pf.a), bias, nt);
            }
        } else {
            // where this wave's A stream continues behind its last chunk of layer l: its first tile of a later streamed layer, else of the
            // next evaluation
            const f4* tbase = nx.base;
            unsigned toff = nx.first_off;
            int tq = nx.first_q > 0 ? nx.first_q : 1;
#pragma unroll
            for (int nl = ML - 1; nl > l; --nl)
                if (nl < T.L && !tab_res(T.dims[nl]) && tab_tiles(T.dims[nl]) > w) {
                    tbase = T.base; toff = T.off[nl] + (unsigned)w * tab_quads(T.dims[nl]) * 64u; tq = tab_quads(T.dims[nl]);
                }
            for (int nt = w; nt < NTL; nt += 4) {
                const f4 bias = b16[4 * nt];
                f4 acc = f4{0.f, 0.f, 0.f, 0.f};
                const unsigned coff = T.off[l] + (unsigned)(nt * S4) * 64u;
                for (int q0 = 0; q0 < S4; q0 += 4) {
                    f4 cur[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) cur[c] = pf.a[c];
                    // ---- the next chunk: same tile, the wave's next tile, or the continuation behind this layer
                    const bool same = q0 + 4 < S4, more = nt + 4 < NTL;
                    const f4* nb = (same || more) ? T.base : tbase;
                    const unsigned no = same ? coff + (unsigned)(q0 + 4) * 64u : (more ? coff + (unsigned)(4 * S4) * 64u : toff);
                    const int nr = same ? S4 - q0 - 4 : (more ? S4 : tq);
                    fetch(nb, no, nr, pf.a);
                    if (q0 + 4 <= S4) {
                        f4 bv[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) bv[c] = bq[(q0 + c) * 64];
                        __builtin_amdgcn_sched_barrier(0);      // all four reads in flight before the first MFMA
#pragma unroll
                        for (int c = 0; c < 4; ++c) mfma_quad(cur[c], bv[c], acc);
                    } else {
                        for (int c = 0; q0 + c < S4; ++c) mfma_quad(c == 0 ? cur[0] : (c == 1 ? cur[1] : cur[2]), bq[(q0 + c) * 64], acc);
                    }
                }
                finish(acc, bias, nt);
            }
        }
        if constexpr (!STREAM && PSNODE_K0_ABL != 6) {       // the next layer's first A operands, in front of the barrier
            if (!last) peek(T, l + 1 < ML ? l + 1 : l, pf.a);
            else peek(nx, 0, pf.a);
        }
        if (PSNODE_K0_ABL != 3) lds_barrier();
        in = out;
    }
    if constexpr (STREAM) { if (T.first_q > 0) pf.tag = nx.base; }      // a wave without a streamed tile in T has fetched nothing
    else pf.tag = nx.base;
    return out;
}

// ---- register mode: every layer has at most four output tiles (one per wave), the first contraction at most 16 QM columns (QM = 4 or 8),
// the others at most 64.  The wave's A operands of the WHOLE MLP stay in registers for the launch (wr[l][q]: quad q of its tile of layer l, zero where
// the wave has no tile or the tile is shorter), as in the specialised tile integrators: a layer then reads only the activations from LDS
// (tile_reg / tile_reg_any: psnode_generic_tile.h).
// the wave's operand registers of one MLP: layer 0 (the only one whose contraction can exceed 64 columns: the other layers read a layer
// output of at most 64 units) holds QM quads, the others four
template <int ML, int QM>
struct WReg {
    f4 first[QM];
    f4 rest[ML - 1][4];
};

// Layer 0 behind its leading block: bias + the products of quads qx .. of tile nt with the input columns that are constant over a step
// (DE: a0 and the externals) or a trajectory (AE: a0).  Once per step / launch: the A operands come from the workspace image (L2), one
// chunk ahead.  The register forms start layer 0's accumulator from this value and multiply only the leading block per evaluation.
template <int ML>
__device__ __forceinline__ f4 fold0(const Tab<ML>& T, const float* lds, int in, int nt) {
    const int lane = threadIdx.x & 63;
    const int S4 = tab_quads(T.dims[0]);
    const f4* __restrict__ A = T.base + T.off[0] + (unsigned)(nt * S4) * 64u + lane;
    const f4* bq = reinterpret_cast<const f4*>(lds + in) + lane;
    f4 acc = reinterpret_cast<const f4*>(lds + T.boff[0])[4 * nt + (lane >> 4)];
    f4 nxt[4];
    auto fetch4 = [&](int q0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) nxt[c] = A[(q0 + c < S4 ? q0 + c : S4 - 1) * 64];
    };
    fetch4(T.qx < S4 ? T.qx : S4 - 1);
    for (int q0 = T.qx; q0 < S4; q0 += 4) {
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
            for (int c = 0; c < 4; ++c) mfma_quad(cur[c], bv[c], acc);
        } else {
            for (int c = 0; q0 + c < S4; ++c) mfma_quad(c == 0 ? cur[0] : (c == 1 ? cur[1] : cur[2]), bq[(q0 + c) * 64], acc);
        }
    }
    return acc;
}

template <int ML, int QM>
__device__ __forceinline__ void load_regs(const MlpDev& m, const Tab<ML>& t, WReg<ML, QM>& wr) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        const int S4 = l < t.L ? tab_quads(t.dims[l]) : 0, NTL = l < t.L ? tab_tiles(t.dims[l]) : 0;
        const f4* __restrict__ A = reinterpret_cast<const f4*>(m.wt[l < t.L ? l : 0]) + (size_t)(w < NTL ? w : 0) * S4 * 64 + lane;
#pragma unroll
        for (int q = 0; q < (l ? 4 : QM); ++q) {
            const f4 v = (w < NTL && q < (l ? S4 : t.qx)) ? A[q * 64] : f4{0.f, 0.f, 0.f, 0.f};      // layer 0: its leading block only
            if (l == 0) wr.first[q] = v; else wr.rest[l - 1][q] = v;
        }
    }
}

// c0: fold0 of this wave's tile of layer 0 (bias included)
template <int ML, int QM>
__device__ __forceinline__ int mlp_reg(const Tab<ML>& T, float* lds, int in, const int ping, const int pong, const WReg<ML, QM>& wr, const f4 c0, const ActCtx& cx) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int out = ping;
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l >= T.L) break;
        out = (l & 1) ? pong : ping;
        const int S4 = tab_quads(T.dims[l]);
        const bool last = (l + 1 == T.L);
        if (w < tab_tiles(T.dims[l])) {
            const f4* bq = reinterpret_cast<const f4*>(lds + in) + lane;
            const f4 bias = reinterpret_cast<const f4*>(lds + T.boff[l])[4 * w + (lane >> 4)];
            f4 acc;
            if (l == 0) acc = tile_reg_any<QM>(T.qx, bq, wr.first) + c0;
            else acc = tile_reg_any<4>(S4, bq, wr.rest[l ? l - 1 : 0]) + bias;
            const f4 e = cx.actq(acc);
            reinterpret_cast<f4*>(lds + out)[w * 64 + lane] = last ? acc : e;
        }
        lds_barrier();
        in = out;
    }
    return out;
}

// ---- wide register form: hidden layers of up to 128 units = up to EIGHT tiles, two per wave (nt = w and w + 4), contractions up to 128
// columns; the last layer at most four tiles.  2 .. 4 layers.  The wave's two tiles share the activation reads: half the LDS traffic per
// MFMA of the one-tile form.  224 operand registers at four layers (the compiler parks part of them in AGPRs).
template <int ML>
struct WRegW {
    f4 first[2][8];
    f4 mid[ML - 2][2][8];
    f4 last[8];
};

template <int ML>
__device__ __forceinline__ void load_regs_wide(const MlpDev& m, const Tab<ML>& t, WRegW<ML>& wr) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        const bool on = l < t.L, is_last = l + 1 == t.L;
        const int S4 = on ? tab_quads(t.dims[l]) : 0, NTL = on ? tab_tiles(t.dims[l]) : 0;
        const f4* __restrict__ A = reinterpret_cast<const f4*>(m.wt[on ? l : 0]) + lane;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nt = w + 4 * j;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int QL = l ? S4 : t.qx;               // layer 0: its leading block only
                const f4 v = (nt < NTL && q < QL) ? A[((size_t)(nt < NTL ? nt : 0) * S4 + (q < QL ? q : 0)) * 64] : zero;
                if (is_last) { if (j == 0) wr.last[q] = v; }
                else if (l == 0) wr.first[j][q] = v;
                else if (l < ML - 1) wr.mid[l - 1 < ML - 2 ? l - 1 : 0][j][q] = v;
            }
        }
    }
}

// Q quads, one or two tiles on the same activation reads
template <int Q, bool TWO>
__device__ __forceinline__ void tile2_reg(const f4* bq, const f4 (&wa)[8], const f4 (&wb)[8], f4& ra, f4& rb) {
    f4 bv[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) bv[c] = bq[c * 64];
    __builtin_amdgcn_sched_barrier(0);
    f4 a0 = f4{0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
#pragma unroll
    for (int c = 0; c < Q; ++c) {
        mfma_quad(wa[c], bv[c], (c & 1) ? a1 : a0);
        if (TWO) mfma_quad(wb[c], bv[c], (c & 1) ? b1 : b0);
    }
    ra = Q > 1 ? a0 + a1 : a0;
    rb = Q > 1 ? b0 + b1 : b0;
}
template <bool TWO>
__device__ __forceinline__ void tile2_any(int S4, const f4* bq, const f4 (&wa)[8], const f4 (&wb)[8], f4& ra, f4& rb) {
    switch (S4) {
        case 1: tile2_reg<1, TWO>(bq, wa, wb, ra, rb); break;
        case 2: tile2_reg<2, TWO>(bq, wa, wb, ra, rb); break;
        case 3: tile2_reg<3, TWO>(bq, wa, wb, ra, rb); break;
        case 4: tile2_reg<4, TWO>(bq, wa, wb, ra, rb); break;
        case 5: tile2_reg<5, TWO>(bq, wa, wb, ra, rb); break;
        case 6: tile2_reg<6, TWO>(bq, wa, wb, ra, rb); break;
        case 7: tile2_reg<7, TWO>(bq, wa, wb, ra, rb); break;
        default: tile2_reg<8, TWO>(bq, wa, wb, ra, rb); break;
    }
}

// c0a / c0b: fold0 of the wave's two tiles of layer 0 (bias included)
template <int ML>
__device__ __forceinline__ int mlp_regw(const Tab<ML>& T, float* lds, int in, const int ping, const int pong, const WRegW<ML>& wr, const f4 c0a,
                                        const f4 c0b, const ActCtx& cx) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int out = ping;
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l >= T.L) break;
        out = (l & 1) ? pong : ping;
        const int S4 = tab_quads(T.dims[l]), NTL = tab_tiles(T.dims[l]);
        const bool last = (l + 1 == T.L);
        if (w < NTL) {
            const f4* bq = reinterpret_cast<const f4*>(lds + in) + lane;
            const f4* b16 = reinterpret_cast<const f4*>(lds + T.boff[l]) + (lane >> 4);
            f4* oq = reinterpret_cast<f4*>(lds + out) + lane;
            const bool two = !last && w + 4 < NTL;
            const f4 bias0 = b16[4 * w], bias1 = b16[4 * (two ? w + 4 : w)];
            f4 ra, rb;
            const int QL = l ? S4 : T.qx;
            if (last && l) tile2_any<false>(QL, bq, wr.last, wr.last, ra, rb);
            else if (l == 0) { if (two) tile2_any<true>(QL, bq, wr.first[0], wr.first[1], ra, rb); else tile2_any<false>(QL, bq, wr.first[0], wr.first[0], ra, rb); }
            else {
                constexpr int MI = ML - 2;
                const int mi = l - 1 < MI ? l - 1 : 0;
                if (two) tile2_any<true>(S4, bq, wr.mid[mi][0], wr.mid[mi][1], ra, rb); else tile2_any<false>(S4, bq, wr.mid[mi][0], wr.mid[mi][0], ra, rb);
            }
            ra = ra + (l ? bias0 : c0a);
            oq[w * 64] = last ? ra : cx.actq(ra);
            if (two) { rb = rb + (l ? bias1 : c0b); oq[(w + 4) * 64] = cx.actq(rb); }
        }
        lds_barrier();
        in = out;
    }
    return out;
}

// a launch-uniform 64-bit value, pinned in scalar registers (two readfirstlane halves)
__device__ __forceinline__ long long uniform64(long long v) {
    const unsigned long long u = (unsigned long long)v;
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u));
}

// PF: z | v values a thread keeps in flight for the next grid point (items tid + 256 j); rows beyond 16 PF are loaded where they are used
constexpr int PF = 4;

// The kernel of policy B = Bd (named in the template for the kernel's symbol alone: the body reads Bd).  Extra: B::n_extra by-value arguments
// behind `a`, in the order act | rk | sub; the body sees all three names.  MODE 0: weights in registers (mlp_reg; QM = 4 or 8 quads per
// tile), 1: every image resident in LDS, 2: some layers streamed, 3: the DE in the wide register form (mlp_regw)
template <class B, bool DAE, int MODE, int ML, int QM, class... Extra>
__global__ __launch_bounds__(NT) void generic_kernel(const IntegrateDev a, const Extra... extra) {
    static_assert(std::is_same_v<B, Bd> && sizeof...(Extra) == B::n_extra, "the policy's argument list");
    const auto& act = kernel_arg<0>(NoActPair{}, extra...);                // ELU(1): no activation argument, ActCtx is empty
    const auto& rk = kernel_arg<1>(psnode_rk_tableau_f32{}, extra...);     // never read without one: the tableau code is under `if constexpr (Bd::rk)`
    const auto& sub = kernel_arg<2>(SubDev{}, extra...);                   // never read without one: the sub-step code is under `if constexpr (Bd::sub)`
#include "psnode_generic_body.h"
}
template <class B, class... Extra> struct GenericKernels {
    template <bool DAE, int MODE, int ML, int QM = 4> static constexpr auto get() { return &generic_kernel<B, DAE, MODE, ML, QM, Extra...>; }
};

}  // namespace

// plans, sets the dynamic-LDS limit and launches the instance of policy B for this call; extra: the kernel's arguments behind `a`
template <class B, class... Extra>
hipError_t launch_generic_build(const IntegrateDev& a_in, bool dae, unsigned chunks, hipStream_t stream_, const Extra&... extra) {
    using K = GenericKernels<B, Extra...>;
    IntegrateDev a = a_in;
    const size_t lds = generic_plan(a, dae, a.k0_res, B::lin_layout);
    const unsigned grid = (unsigned)((a.B + TB - 1) / TB);
    unsigned all = (1u << a.de.n_layers) - 1u;
    if (dae) all |= ((1u << a.ae.n_layers) - 1u) << 8;
    const bool stream = a.k0_res != all;          // some layer's image does not fit LDS
    // Up to one workgroup per CU in the launch: ask for more than half a CU's LDS, so that the dispatcher cannot put two workgroups on one CU
    // (two waves per SIMD sharing the MFMA pipe) while other CUs stay empty.
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    // (chunks: 1, or the time chunks of the segment-parallel build -- the grid's second dimension; the workgroups of all of them share the CUs)
    const size_t lds_launch = ((unsigned long long)grid * chunks <= (unsigned long long)cus && lds < 81 * 1024) ? 81 * 1024 : lds;
    auto go = [&](auto kern) { return launch_attr(true, kern, dim3(grid, chunks), dim3(NT), lds_launch, stream_, a, extra...); };
    const int qm = generic_reg_mode(a, dae);
    const bool deep = a.de.n_layers > 4 || (dae && a.ae.n_layers > 4);      // the layer loop is unrolled 4 or kMaxLayers times
    if constexpr (B::sth) {      // stage heads exist in a DAE alone: its instances only (register QM 4 / 8, resident, streamed, each deep form)
        if (!dae) return hipErrorInvalidValue;
        if (qm == 4) return go(K::template get<true, 0, 4, 4>());
        if (qm == 8) return go(K::template get<true, 0, 4, 8>());
        if (deep) return stream ? go(K::template get<true, 2, kMaxLayers>()) : go(K::template get<true, 1, kMaxLayers>());
        return stream ? go(K::template get<true, 2, 4>()) : go(K::template get<true, 1, 4>());
    } else {
    if (qm && deep) return qm == 4 ? go(K::template get<false, 0, kMaxLayers, 4>()) : go(K::template get<false, 0, kMaxLayers, 8>());
    if (qm == 4) return dae ? go(K::template get<true, 0, 4, 4>()) : go(K::template get<false, 0, 4, 4>());
    if (qm == 8) return dae ? go(K::template get<true, 0, 4, 8>()) : go(K::template get<false, 0, 4, 8>());
    if (generic_wide_mode(a, dae)) return go(K::template get<false, 3, 4>());
    if (deep) {
        if (dae) return stream ? go(K::template get<true, 2, kMaxLayers>()) : go(K::template get<true, 1, kMaxLayers>());
        return stream ? go(K::template get<false, 2, kMaxLayers>()) : go(K::template get<false, 1, kMaxLayers>());
    }
    if (dae) return stream ? go(K::template get<true, 2, 4>()) : go(K::template get<true, 1, 4>());
    return stream ? go(K::template get<false, 2, 4>()) : go(K::template get<false, 1, 4>());
    }
}

template <class B>
hipError_t launch_generic(const IntegrateDev& a, bool dae, const K0Call& call, hipStream_t stream) {
    if constexpr (B::par) {
        return launch_generic_build<B>(a, dae, (unsigned)msp_chunks(a.T, call.ms_every, call.per_group), stream, call.act, call.rk,
                                       build_sub<B>(call.sub.n, call.sub.x_sub, call.ev_pt, call.ms_every, nullptr, call.per_group));
    } else if constexpr (B::sub) {
        return launch_generic_build<B>(a, dae, 1u, stream, call.act, call.rk,
                                       build_sub<B>(call.sub.n, call.sub.x_sub, call.ev_pt, call.ms_every, nullptr, 1, nullptr, nullptr, call.stencil, call.rkc));
    } else if constexpr (B::rk) return launch_generic_build<B>(a, dae, 1u, stream, call.act, call.rk);
    else if constexpr (B::act) return launch_generic_build<B>(a, dae, 1u, stream, call.act);
    else return launch_generic_build<B>(a, dae, 1u, stream);
}
template hipError_t launch_generic<Bd>(const IntegrateDev&, bool, const K0Call&, hipStream_t);

}  // namespace psnode
