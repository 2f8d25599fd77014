// Micro-benchmark behind DESIGN.md "K1 at B = 4096: the exchange-free 4x4x1 tile" (round 5).
//   hipcc --offload-arch=gfx950 -O3 profiles/scripts/ubench_4x4.hip -o /tmp/ub4 && /tmp/ub4
// The candidate decomposition: ONE wave owns 4 trajectories and ALL 64 hidden units -- no LDS, no barrier.  One H -> H layer is
//   D[traj r][unit 4b+c] += act[k][traj r] * W[unit 4b+c][k]      64 x v_mfma_f32_4x4x1_16B_f32 (16 blocks of 4x4x1),
// A = activations (lane (b,t) register c holds act[k = 4b+c][traj t]; CBSZ = 4 / ABID = b broadcasts block b's four rows to all 16 blocks),
// B = weights (lane (b',c') holds W[4b'+c'][k]: one VGPR per k, 64 per layer), D lane (b,c) register r = out[unit 4b+c][traj r].  The
// layer-to-layer re-layout (D -> A) is a 4 x 4 transpose inside every lane quad: 8 v_cndmask_b32_dpp (quad_perm), no LDS.
// Compared against profiles/scripts/ubench_exchange.hip (today's 4-wave tile: 16 x v_mfma_f32_16x16x4_f32 + one LDS exchange per layer;
// 343.8 ns bare, 391.0 ns with 24 VALU instructions of ELU).  Modes:
//   0  64 MFMA (2 accumulator chains) only                                   : the issue floor of the 4x4x1 form
//   1  + the in-quad transpose (8 v_cndmask_b32_dpp)
//   2  + the ELU of the wave's 4 values per lane (elu_quad of psnode_common.h: the same values per lane as today)
//   3  as 2 with FOUR accumulator chains (3 packed adds more)
//   4  as 2 with the round-5 ELU (the clamp of the negative side rides on v_exp_f32's output modifier: 3 instead of 4 issue slots per value)
//   5  64 MFMA without the A broadcast (CBSZ = 0): is the 10-cycle issue interval a property of the broadcast?
//   6  the whole layer with the scaled-domain ELU;  7 / 8  64 MFMA with one / two SALU instructions behind each: are they free?
//   11  64 MFMA on ONE accumulator chain as the compiler emits it (it places the s_nop 1 of a dependent SrcC itself);  12  the same as asm
//       blocks of 4 k with an explicit s_nop 1 behind every MFMA;  13  the whole layer (scaled-domain ELU + transpose) on one chain;
//   14  as 13 with the transpose's two butterfly stages in alternating order from layer to layer (vcc is handed on: 3 mask moves, not 4)
//   20 / 21  the waist of K1x's stage, 64 -> 8 -> 64: the output layer (8 MFMAs) -> block fold -> one RK stage input -> L1 (8 MFMAs), as ticks
//       per pass.  20 = the 16-block form (two dim-tiles, permlane32 + permlane16 folds, the RK operations on two scalars); 21 = the
//       8-block form (B-operand lane-group broadcast BLGP 1 / 2, two chains merged by packed adds, permlane16 fold, packed RK operations).
//       The 8-block form also gets a mapping check against a double-precision matvec (does BLGP broadcast what the ISA text says?).
//   30 / 31  the seam behind K1x's first layer (`ubench_4x4 l1` runs these two alone): 30 = mapping check of BLGP 4 .. 7 (the B operand's row
//       broadcast) and of the whole first layer with the roles swapped (A = weights, B = state), against double precision and, as raw words,
//       against today's form; 31 = the stage head (L1 -> merge -> ELU [-> transpose]) in both forms, as ticks per head.
// It also checks, bit for bit over 2^24 inputs, that the round-5 ELU form equals round 3's.
// Grid: 1024 single-wave workgroups (= B 4096: one wave per SIMD), and 2048 (two per SIMD) for reference.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

template <int ABID, bool BC = true>
__device__ __forceinline__ f4 mf(float a, float b, f4 c) {
    if constexpr (BC) return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0);
    else return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f4 elu_quad(f4 v) {
    const float L2E = 1.44269504088896340736f;
    f4 o;
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        f2 xn = f2{fminf(v[i], 0.f), fminf(v[i + 1], 0.f)};
        f2 y = xn * L2E;
        f2 t = f2{__builtin_amdgcn_exp2f(y[0]), __builtin_amdgcn_exp2f(y[1])};
        f2 u = t - 1.0f;
        o[i] = fmaxf(v[i], u[0]); o[i + 1] = fmaxf(v[i + 1], u[1]);
    }
    return o;
}

// round 5: exp2(min(y, 0)) == clamp(exp2(y)) to [0, 1] -- the VOP3 output modifier of v_exp_f32 replaces the v_min_f32
__device__ __forceinline__ f4 elu_quad_clamp(f4 v) {
    const float L2E = 1.44269504088896340736f;
    f4 o;
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        f2 y = f2{v[i], v[i + 1]} * L2E;
        f2 t = f2{__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(y[0]), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(y[1]), 0.f, 1.f)};
        f2 u = t - 1.0f;
        o[i] = fmaxf(v[i], u[0]); o[i + 1] = fmaxf(v[i + 1], u[1]);
    }
    return o;
}
__device__ __forceinline__ f4 elu_quad_scaled(f4 v) {
    const f2 c = f2{1.44269504088896340736f, 1.44269504088896340736f}, nc = -c;
    const f2 ea = f2{__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[0]), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[1]), 0.f, 1.f)};
    const f2 eb = f2{__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[2]), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[3]), 0.f, 1.f)};
    const f2 ua = __builtin_elementwise_fma(c, ea, nc), ub = __builtin_elementwise_fma(c, eb, nc);
    return f4{fmaxf(v[0], ua[0]), fmaxf(v[1], ua[1]), fmaxf(v[2], ub[0]), fmaxf(v[3], ub[1])};
}
// the same on an accumulator as the MFMA left it (one chain: no sum in front): fmaxf would cost a canonicalising v_max_f32 more per
// element, the NaN-propagating maximum (v_maximum3_f32) does not
__device__ __forceinline__ f4 elu_quad_scaled_acc(f4 v) {
    const f2 c = f2{1.44269504088896340736f, 1.44269504088896340736f}, nc = -c;
    const f2 ea = f2{__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[0]), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[1]), 0.f, 1.f)};
    const f2 eb = f2{__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[2]), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(v[3]), 0.f, 1.f)};
    const f2 ua = __builtin_elementwise_fma(c, ea, nc), ub = __builtin_elementwise_fma(c, eb, nc);
    return f4{__builtin_elementwise_maximum(v[0], ua[0]), __builtin_elementwise_maximum(v[1], ua[1]),
              __builtin_elementwise_maximum(v[2], ub[0]), __builtin_elementwise_maximum(v[3], ub[1])};
}
__global__ void elu_forms(unsigned* ndiff) {
    // every float whose low 8 mantissa bits are a fixed pattern: 2^24 values over the whole exponent range, both signs
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned d = 0;
#pragma unroll 1
    for (unsigned lo = 0; lo < 256; lo += 85) {
        const float x = __uint_as_float((i << 8) | lo);
        if (x != x) continue;
        const f4 a = elu_quad(f4{x, x, x, x}), b = elu_quad_clamp(f4{x, x, x, x});
        d += __float_as_uint(a[0]) != __float_as_uint(b[0]);
    }
    if (d) atomicAdd(ndiff, d);
}

// 4x4 transpose of (r0..r3) x (lanes 4q..4q+3): two butterfly stages of 4 v_cndmask_b32_dpp each (D = vcc ? src1 : dpp(src0)).
// One asm block: the hazard recognizer does not look inside, so it carries its own wait states (VALU write -> DPP read: 2).
__device__ __forceinline__ f4 quad_transpose(f4 v, const int) {
    float a0, a1, a2, a3, o0, o1, o2, o3;
    const unsigned long long EVEN = 0x5555555555555555ull, LO = 0x3333333333333333ull;
    asm volatile(
        "s_nop 1\n\t"
        "s_mov_b64 vcc, %12\n\t"
        "v_cndmask_b32_dpp %0, %9, %8, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %2, %11, %10, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_not_b64 vcc, vcc\n\t"
        "v_cndmask_b32_dpp %1, %8, %9, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %3, %10, %11, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 vcc, %13\n\t"
        "v_cndmask_b32_dpp %4, %2, %0, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %5, %3, %1, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_not_b64 vcc, vcc\n\t"
        "v_cndmask_b32_dpp %6, %0, %2, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %7, %1, %3, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(EVEN), "s"(LO)
        : "vcc", "scc");
    return f4{o0, o1, o2, o3};
}

// The same transpose with a compile-time stage order and the mask handed from seam to seam in vcc.  The two butterfly stages (lane bit 0 <->
// register bit 0, lane bit 1 <-> register bit 1) commute.  ORD 0: enters with vcc = EVEN lanes, leaves with vcc = HI lanes (bit 1 set);
// ORD 1: enters with HI, leaves with EVEN -- so alternating seams need 3 mask moves each instead of 4.
template <int ORD>
__device__ __forceinline__ f4 quad_transpose_seq(f4 v, unsigned long long& m) {
    float a0, a1, a2, a3, o0, o1, o2, o3;
    const unsigned long long ODD = 0xAAAAAAAAAAAAAAAAull, LO = 0x3333333333333333ull;
    // the asm's mask operands ARE vcc's halves: what one seam leaves is what the next one reads, the compiler has no move to emit
    // (a 64-bit register variable on vcc crashes this compiler's backend)
    register unsigned mlo asm("vcc_lo") = (unsigned)m;
    register unsigned mhi asm("vcc_hi") = (unsigned)(m >> 32);
    if constexpr (ORD == 0) {
        asm volatile(
            "s_nop 1\n\t"
            "v_cndmask_b32_dpp %0, %11, %10, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %2, %13, %12, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "s_not_b64 vcc, vcc\n\t"
            "v_cndmask_b32_dpp %1, %10, %11, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %3, %12, %13, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "s_mov_b64 vcc, %14\n\t"
            "v_cndmask_b32_dpp %4, %2, %0, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %5, %3, %1, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "s_not_b64 vcc, vcc\n\t"
            "v_cndmask_b32_dpp %6, %0, %2, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %7, %1, %3, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
            : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "+s"(mlo), "+s"(mhi)
            : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(LO)
            : "scc");
    } else {
        asm volatile(
            "s_nop 1\n\t"
            "v_cndmask_b32_dpp %2, %10, %12, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %3, %11, %13, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "s_not_b64 vcc, vcc\n\t"
            "v_cndmask_b32_dpp %0, %12, %10, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %1, %13, %11, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "s_mov_b64 vcc, %14\n\t"
            "v_cndmask_b32_dpp %5, %0, %1, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %7, %2, %3, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "s_not_b64 vcc, vcc\n\t"
            "v_cndmask_b32_dpp %4, %1, %0, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %6, %3, %2, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
            : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "+s"(mlo), "+s"(mhi)
            : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(ODD)
            : "scc");
    }
    m = (unsigned long long)mhi << 32 | mlo;
    return f4{o0, o1, o2, o3};
}

template <int C, int B0, int NACC, bool BC = true, int FILL = 0>
__device__ __forceinline__ void quarter(const float (&wreg)[64], const float hc, f4 (&acc)[4], unsigned& g_sfill) {
    // the 16 k's that register c of the A operand carries: k = 4b + c, ABID = b
#define STEP(B) acc[(B) % NACC] = mf<B, BC>(hc, wreg[4 * (B) + C], acc[(B) % NACC]); \
    if constexpr (FILL == 1) { asm volatile("s_add_u32 %0, %0, 1" : "+s"(g_sfill)); } \
    if constexpr (FILL == 2) { asm volatile("s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 3" : "+s"(g_sfill)); }
    STEP(0) STEP(1) STEP(2) STEP(3) STEP(4) STEP(5) STEP(6) STEP(7) STEP(8) STEP(9) STEP(10) STEP(11) STEP(12) STEP(13) STEP(14) STEP(15)
#undef STEP
}

// mode 9: the 64 MFMAs of a layer with the B operands READ FROM AccVGPRs (inline asm, `a` constraint -- K2x's hh_layer_acc): is an AGPR source slower?
template <int BB>
__device__ __forceinline__ void block_acc(const float (&wk)[64], const f4 hA, f4& accA, f4& accB) {
    asm volatile(
        "v_mfma_f32_4x4x1_16b_f32 %0, %2, %6, %0 cbsz:4 abid:%10\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %1, %3, %7, %1 cbsz:4 abid:%10\n\t"
        "s_nop 0\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %0, %4, %8, %0 cbsz:4 abid:%10\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %1, %5, %9, %1 cbsz:4 abid:%10\n\t"
        "s_nop 0"
        : "+v"(accA), "+v"(accB)
        : "v"(hA[0]), "v"(hA[1]), "v"(hA[2]), "v"(hA[3]), "a"(wk[4 * BB + 0]), "a"(wk[4 * BB + 1]), "a"(wk[4 * BB + 2]), "a"(wk[4 * BB + 3]), "n"(BB));
}
// mode 10: the same asm with the B operands in VGPRs (`v` constraint): the asm form's own cost
template <int BB>
__device__ __forceinline__ void block_vgpr(const float (&wk)[64], const f4 hA, f4& accA, f4& accB) {
    asm volatile(
        "v_mfma_f32_4x4x1_16b_f32 %0, %2, %6, %0 cbsz:4 abid:%10\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %1, %3, %7, %1 cbsz:4 abid:%10\n\t"
        "s_nop 0\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %0, %4, %8, %0 cbsz:4 abid:%10\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %1, %5, %9, %1 cbsz:4 abid:%10\n\t"
        "s_nop 0"
        : "+v"(accA), "+v"(accB)
        : "v"(hA[0]), "v"(hA[1]), "v"(hA[2]), "v"(hA[3]), "v"(wk[4 * BB + 0]), "v"(wk[4 * BB + 1]), "v"(wk[4 * BB + 2]), "v"(wk[4 * BB + 3]), "n"(BB));
}
// mode 12: ONE accumulator chain, asm, an explicit s_nop 1 behind every MFMA (a dependent SrcC of a 2-pass MFMA needs 2 wait states)
template <int BB>
__device__ __forceinline__ void block_one(const float (&wk)[64], const f4 hA, f4& acc) {
    asm volatile(
        "v_mfma_f32_4x4x1_16b_f32 %0, %1, %5, %0 cbsz:4 abid:%9\n\t"
        "s_nop 1\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %0, %2, %6, %0 cbsz:4 abid:%9\n\t"
        "s_nop 1\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %0, %3, %7, %0 cbsz:4 abid:%9\n\t"
        "s_nop 1\n\t"
        "v_mfma_f32_4x4x1_16b_f32 %0, %4, %8, %0 cbsz:4 abid:%9\n\t"
        "s_nop 1"
        : "+v"(acc)
        : "v"(hA[0]), "v"(hA[1]), "v"(hA[2]), "v"(hA[3]), "v"(wk[4 * BB + 0]), "v"(wk[4 * BB + 1]), "v"(wk[4 * BB + 2]), "v"(wk[4 * BB + 3]), "n"(BB));
}
__global__ __launch_bounds__(64) void bench_asm_one(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    const int l = threadIdx.x;
    float wreg[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) wreg[i] = wsrc[i * 64 + l];
    f4 h = f4{0.1f + 0.001f * l, 0.2f, 0.3f, 0.4f};
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; ++it) {
        f4 a0 = f4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_nop 1" : "+v"(a0));          // VALU write -> MFMA SrcC read
#define BLK(B_) block_one<B_>(wreg, h, a0);
        BLK(0) BLK(1) BLK(2) BLK(3) BLK(4) BLK(5) BLK(6) BLK(7) BLK(8) BLK(9) BLK(10) BLK(11) BLK(12) BLK(13) BLK(14) BLK(15)
#undef BLK
        asm volatile("s_nop 1" : "+v"(a0));          // (with the block's own s_nop 1: MFMA write, 2 passes -> VALU read)
        h = a0 * 1e-3f;
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 64 + l] = h[0] + h[1] + h[2] + h[3];
    if (blockIdx.x == 0 && l == 0) *cyc = t1 - t0;
}
void run_asm_one(const char* name, int nwg, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench_asm_one<<<nwg, 64>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench_asm_one<<<nwg, 64>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long c; hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-58s waves/SIMD=%d : %7.1f ns per layer (wall), s_memtime %.2f ticks\n", name, nwg / 1024, ms * 1e6 / niter, (double)c / niter);
}
template <bool ACC>
__global__ __launch_bounds__(64) void bench_asm(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    const int l = threadIdx.x;
    float wreg[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) wreg[i] = wsrc[i * 64 + l];
    f4 h = f4{0.1f + 0.001f * l, 0.2f, 0.3f, 0.4f};
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; ++it) {
        f4 a0 = f4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#define BLK(B_) if constexpr (ACC) block_acc<B_>(wreg, h, a0, a1); else block_vgpr<B_>(wreg, h, a0, a1);
        BLK(0) BLK(1) BLK(2) BLK(3) BLK(4) BLK(5) BLK(6) BLK(7) BLK(8) BLK(9) BLK(10) BLK(11) BLK(12) BLK(13) BLK(14) BLK(15)
#undef BLK
        asm volatile("s_nop 3" : "+v"(a0), "+v"(a1));
        h = (a0 + a1) * 1e-3f;
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 64 + l] = h[0] + h[1] + h[2] + h[3];
    if (blockIdx.x == 0 && l == 0) *cyc = t1 - t0;
}
template <bool ACC>
void run_asm(const char* name, int nwg, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench_asm<ACC><<<nwg, 64>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench_asm<ACC><<<nwg, 64>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long c; hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-58s waves/SIMD=%d : %7.1f ns per layer (wall), s_memtime %.2f ticks\n", name, nwg / 1024, ms * 1e6 / niter, (double)c / niter);
}

template <int MODE>
__global__ __launch_bounds__(64) void bench(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    const int l = threadIdx.x;
    float wreg[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) wreg[i] = wsrc[i * 64 + l];
    f4 h = f4{0.1f + 0.001f * l, 0.2f, 0.3f, 0.4f};
    constexpr int NACC = MODE == 3 ? 4 : (MODE == 11 || MODE == 13 || MODE == 14 ? 1 : 2);
    constexpr int NLAYER = MODE == 14 ? 2 : 1;                         // layers per iteration (mode 14: one of each transpose order)
    unsigned sfill = 0;
    unsigned long long vmask = 0x5555555555555555ull;                  // mode 14: the mask the next seam starts with (EVEN lanes)
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; it += NLAYER) {
#pragma unroll
      for (int ly = 0; ly < NLAYER; ++ly) {
        f4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
        constexpr int FILL = MODE == 7 ? 1 : (MODE == 8 ? 2 : 0);      // modes 7 / 8: one / two SALU instructions behind every MFMA
        quarter<0, 0, NACC, MODE != 5, FILL>(wreg, h[0], acc, sfill);
        quarter<1, 0, NACC, MODE != 5, FILL>(wreg, h[1], acc, sfill);
        quarter<2, 0, NACC, MODE != 5, FILL>(wreg, h[2], acc, sfill);
        quarter<3, 0, NACC, MODE != 5, FILL>(wreg, h[3], acc, sfill);
        __builtin_amdgcn_sched_barrier(0);
        f4 s = acc[0];
        if constexpr (NACC >= 2) s += acc[1];
        if constexpr (NACC == 4) s += acc[2] + acc[3];
        if constexpr (MODE == 6) s = elu_quad_scaled(s);
        else if constexpr (MODE == 13 || MODE == 14) s = elu_quad_scaled_acc(s);
        else if constexpr (MODE == 4) s = elu_quad_clamp(s);
        else if constexpr (MODE >= 2 && MODE < 5) s = elu_quad(s);
        if constexpr ((MODE >= 1 && MODE != 5 && MODE < 7) || MODE == 13) s = quad_transpose(s, l);
        if constexpr (MODE == 14) { if (ly == 0) s = quad_transpose_seq<0>(s, vmask); else s = quad_transpose_seq<1>(s, vmask); }
        h = s * 1e-3f;      // keep the chain finite (one packed multiply pair; K1 has the accumulator sum in its place)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 64 + l] = h[0] + h[1] + h[2] + h[3] + (float)sfill + (float)(vmask & 1);
    if (blockIdx.x == 0 && l == 0) *cyc = t1 - t0;
}

// Today's decomposition with the SAME ELU, for a like-for-like figure: the H -> H layer of K1 at hidden 64 as the kernel runs it (4 waves
// per 16-trajectory tile, v_mfma_f32_16x16x4_f32, ds_write_b128 -> 3 own-quarter MFMAs -> s_barrier -> 3 ds_read_b128 -> 13 MFMAs,
// accumulator sum, ELU).  ELUF: 0 = round 3's (min + mul + exp + add + max), 1 = round 5's clamp form, 2 = the scaled-domain form.
__device__ __forceinline__ f4 mf16(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
template <int ELUF, bool XCH>
__global__ __launch_bounds__(256) void bench16(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    __shared__ f4 xb[2][4][64];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    float wm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wm[i] = wsrc[(16 * w + i) * 64 + l];
    f4 h = f4{0.1f + 0.001f * l, 0.2f, 0.3f, 0.4f};
    int p = 0;
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; ++it) {
        if constexpr (XCH) xb[p][w][l] = h;
        f4 accA = f4{0.f, 0.f, 0.f, 0.f}, accB = accA;
        accA = mf16(wm[0], h[0], accA); accB = mf16(wm[1], h[1], accB); accA = mf16(wm[2], h[2], accA);
        asm volatile("" : "+v"(accA), "+v"(accB));
        __builtin_amdgcn_sched_barrier(0);
        f4 vq[4];
        if constexpr (XCH) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#pragma unroll
            for (int c = 1; c < 4; ++c) vq[c] = xb[p][(w + c) & 3][l];
        } else {
#pragma unroll
            for (int c = 1; c < 4; ++c) vq[c] = h;
        }
        asm volatile("" : "+v"(accA), "+v"(accB));
        __builtin_amdgcn_sched_barrier(0);
        accB = mf16(wm[3], h[3], accB);
#pragma unroll
        for (int c = 1; c < 4; ++c) {
            accA = mf16(wm[4 * c + 0], vq[c][0], accA); accB = mf16(wm[4 * c + 1], vq[c][1], accB);
            accA = mf16(wm[4 * c + 2], vq[c][2], accA); accB = mf16(wm[4 * c + 3], vq[c][3], accB);
        }
        f4 s = accA + accB;
        s = ELUF == 0 ? elu_quad(s) : (ELUF == 1 ? elu_quad_clamp(s) : elu_quad_scaled(s));
        h = s * 1e-3f;
        p ^= 1;
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 256 + threadIdx.x] = h[0] + h[1] + h[2] + h[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) *cyc = t1 - t0;
}
template <int ELUF, bool XCH>
void run16(const char* name, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench16<ELUF, XCH><<<256, 256>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench16<ELUF, XCH><<<256, 256>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-58s 4-wave tile   : %7.1f ns per layer (wall)\n", name, ms * 1e6 / niter);
}

// functional check of the mapping on one wave: out[unit][traj] = sum_k W[unit][k] act[k][traj], then transposed back into A layout
__global__ void check(const float* __restrict__ W, const float* __restrict__ act, float* __restrict__ res) {
    const int l = threadIdx.x, b = l >> 2, t = l & 3;
    float wreg[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) wreg[k] = W[l * 64 + k];                 // B operand of k: lane (b',c') = W[unit 4b'+c' = lane][k]
    f4 h;
#pragma unroll
    for (int c = 0; c < 4; ++c) h[c] = act[(4 * b + c) * 4 + t];          // A layout: lane (b,t) register c = act[k = 4b+c][t]
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    unsigned sf = 0;
    quarter<0, 0, 2>(wreg, h[0], acc, sf);
    quarter<1, 0, 2>(wreg, h[1], acc, sf);
    quarter<2, 0, 2>(wreg, h[2], acc, sf);
    quarter<3, 0, 2>(wreg, h[3], acc, sf);
    f4 s = acc[0] + acc[1];                                               // D: lane (b,c) register r = out[unit 4b+c][traj r]
    s = quad_transpose(s, l);                                             // A layout again: lane (b,t) register c = out[unit 4b+c][traj t]
#pragma unroll
    for (int c = 0; c < 4; ++c) res[(4 * b + c) * 4 + t] = s[c];
}

// the ordered transposes against the plain one, bit for bit, on one wave of distinct values (both orders, vcc handed on)
__global__ void check_seq(unsigned* nbad) {
    const int l = threadIdx.x;
    const f4 v = f4{(float)(4 * l), (float)(4 * l + 1), (float)(4 * l + 2), (float)(4 * l + 3)};
    const f4 ref = quad_transpose(v, l);
    unsigned long long m = 0x5555555555555555ull;
    const f4 t0 = quad_transpose_seq<0>(v, m);
    const bool hi_ok = m == 0xCCCCCCCCCCCCCCCCull;
    const f4 t1 = quad_transpose_seq<1>(v, m);
    const bool even_ok = m == 0x5555555555555555ull;
    unsigned bad = !hi_ok + !even_ok;
#pragma unroll
    for (int i = 0; i < 4; ++i) bad += (t0[i] != ref[i]) + (t1[i] != ref[i]);
    if (bad) atomicAdd(nbad, bad);
}

// ---- the waist (modes 20 / 21).  The image functions are copies of psnode_mfma_x.h's (this file stands alone).
constexpr int l4_k(int m, int lane) { return 32 * (m >> 2) + 4 * ((lane >> 2) & 7) + (m & 3); }
constexpr int l4_dim(int lane) { return 4 * (lane >> 5) + (lane & 3); }
constexpr int l4_bias_dim(int r, int lane) { return ((lane >> 2) & 7) == 0 ? 4 * (lane >> 5) + r : -1; }
template <int BLGP>
__device__ __forceinline__ f4 mfl(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, BLGP); }
__device__ __forceinline__ void row_sum2(float& a, float& b) {
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf"
        : "+v"(a), "+v"(b));
}
__device__ __forceinline__ f2 row_sum2(const f2 k) {
    float a, b;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf"
        : "=&v"(a), "=&v"(b)
        : "v"(k[0]), "v"(k[1]));
    return f2{a, b};
}
__device__ __forceinline__ float fold32(const float a, const float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float fold16(const float a, const float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// 16-block form: A register 4 j + cc, lane (b, r) = W4[4 j + r][4 b + cc]; C tile j register r, block 0 = bias of dim 4 j + r
__device__ __forceinline__ f2 l4_16(const float (&w4a)[8], const f4 (&b4c)[2], const f4 hA) {
    f4 p0 = b4c[0], p1 = b4c[1];
    p0 = mf<0, false>(w4a[0], hA[0], p0); p1 = mf<0, false>(w4a[4], hA[0], p1);
    p0 = mf<0, false>(w4a[1], hA[1], p0); p1 = mf<0, false>(w4a[5], hA[1], p1);
    p0 = mf<0, false>(w4a[2], hA[2], p0); p1 = mf<0, false>(w4a[6], hA[2], p1);
    p0 = mf<0, false>(w4a[3], hA[3], p0); p1 = mf<0, false>(w4a[7], hA[3], p1);
    const float q0 = fold32(p0[0], p1[0]), q1 = fold32(p0[1], p1[1]), q2 = fold32(p0[2], p1[2]), q3 = fold32(p0[3], p1[3]);
    float k01 = fold16(q0, q2), k23 = fold16(q1, q3);
    row_sum2(k01, k23);
    return f2{k01, k23};
}
// 8-block form: A register m = 4 half + cc, lane = W4[l4_dim(lane)][l4_k(m, lane)]; C register r = bias of l4_bias_dim(r, lane)
__device__ __forceinline__ f2 l4_8(const float (&w4a)[8], const f4 b4c, const f4 hA) {
    f4 lo = b4c, hi = f4{0.f, 0.f, 0.f, 0.f};
    lo = mfl<1>(w4a[0], hA[0], lo); hi = mfl<2>(w4a[4], hA[0], hi);
    lo = mfl<1>(w4a[1], hA[1], lo); hi = mfl<2>(w4a[5], hA[1], hi);
    lo = mfl<1>(w4a[2], hA[2], lo); hi = mfl<2>(w4a[6], hA[2], hi);
    lo = mfl<1>(w4a[3], hA[3], lo); hi = mfl<2>(w4a[7], hA[3], hi);
    const f4 q = lo + hi;
    const auto e = __builtin_amdgcn_permlane16_swap(__float_as_uint(q[0]), __float_as_uint(q[2]), false, false);
    const auto o = __builtin_amdgcn_permlane16_swap(__float_as_uint(q[1]), __float_as_uint(q[3]), false, false);
    return row_sum2(f2{__uint_as_float(e[0]), __uint_as_float(o[0])} + f2{__uint_as_float(e[1]), __uint_as_float(o[1])});
}
// out[dim][traj] = b4[dim] + sum_k W4[dim][k] act[k][traj] through either form; img = the form's 8 A registers + its C registers, [reg][lane]
template <bool NEW>
__global__ void check_l4(const float* __restrict__ img, const float* __restrict__ act, float* __restrict__ res) {
    const int l = threadIdx.x, b = l >> 2, t = l & 3;
    float w4a[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) w4a[m] = img[m * 64 + l];
    f4 h;
#pragma unroll
    for (int c = 0; c < 4; ++c) h[c] = act[(4 * b + c) * 4 + t];
    f2 k;
    if constexpr (NEW) {
        f4 b4c;
#pragma unroll
        for (int r = 0; r < 4; ++r) b4c[r] = img[(8 + r) * 64 + l];
        k = l4_8(w4a, b4c, h);
    } else {
        f4 b4c[2];
#pragma unroll
        for (int r = 0; r < 8; ++r) b4c[r >> 2][r & 3] = img[(8 + r) * 64 + l];
        k = l4_16(w4a, b4c, h);
    }
    res[l * 2 + 0] = k[0];                                     // every lane reports, [lane][2]: the state layout holds a row's two dims in EVERY block
    res[l * 2 + 1] = k[1];                                     // of the row (the host works out a lane's dims and trajectory)
}
template <bool NEW>
__global__ __launch_bounds__(64) void bench_waist(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    const int l = threadIdx.x;
    float w4a[8], w1x[8];
    f4 b4c[2];
#pragma unroll
    for (int m = 0; m < 8; ++m) { w4a[m] = wsrc[m * 64 + l]; w1x[m] = wsrc[(8 + m) * 64 + l]; b4c[m >> 2][m & 3] = wsrc[(16 + m) * 64 + l]; }
    f4 h = f4{0.1f + 0.001f * l, 0.2f, 0.3f, 0.4f};
    const f4 c0 = f4{0.01f, 0.02f, 0.03f, 0.04f};
    f2 X = f2{0.1f, 0.2f};
    const float hs = 1e-3f + 1e-6f * (float)niter;             // (a run-time value: the step)
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; ++it) {
        f2 s;
        if constexpr (NEW) {
            const f2 k = l4_8(w4a, b4c[0], h);
            s = X + hs * k;                                    // one stage input: two packed operations
        } else {
            const f2 k = l4_16(w4a, b4c, h);
            const float s01 = X[0] + hs * k[0], s23 = X[1] + hs * k[1];      // ... four scalar ones
            s = f2{s01, s23};
        }
        f4 accA = c0, accB = f4{0.f, 0.f, 0.f, 0.f};
        accA = mf<0>(s[0], w1x[0], accA);  accB = mf<4>(s[0], w1x[1], accB);
        accA = mf<8>(s[0], w1x[2], accA);  accB = mf<12>(s[0], w1x[3], accB);
        accA = mf<0>(s[1], w1x[4], accA);  accB = mf<4>(s[1], w1x[5], accB);
        accA = mf<8>(s[1], w1x[6], accA);  accB = mf<12>(s[1], w1x[7], accB);
        h = (accA + accB) * 1e-3f;
        __builtin_amdgcn_sched_barrier(0);
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 64 + l] = h[0] + h[1] + h[2] + h[3];
    if (blockIdx.x == 0 && l == 0) *cyc = t1 - t0;
}
template <bool NEW>
void run_waist(const char* name, int nwg, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench_waist<NEW><<<nwg, 64>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench_waist<NEW><<<nwg, 64>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long c; hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-58s waves/SIMD=%d : %7.1f ns per pass (wall), s_memtime %.2f ticks\n", name, nwg / 1024, ms * 1e6 / niter, (double)c / niter);
}
// both forms of the output layer against a double-precision matvec, every (dim, k) of a dense W4 and the bias
bool check_waist() {
    float W4[8 * 64], b4[8], ha[64 * 4], img[16 * 64], hr[64 * 2];
    for (int i = 0; i < 8 * 64; ++i) W4[i] = (float)((i * 7919 + 13) % 1000) * 1e-3f - 0.5f;
    for (int i = 0; i < 8; ++i) b4[i] = 0.25f * (float)(i + 1);
    for (int i = 0; i < 64 * 4; ++i) ha[i] = (float)((i * 104729 + 7) % 1000) * 1e-3f - 0.5f;
    float *dimg, *dact, *dres;
    hipMalloc(&dimg, sizeof(img)); hipMalloc(&dact, sizeof(ha)); hipMalloc(&dres, sizeof(hr));
    hipMemcpy(dact, ha, sizeof(ha), hipMemcpyHostToDevice);
    bool all_ok = true;
    for (int form = 0; form < 2; ++form) {
        for (int i = 0; i < 16 * 64; ++i) img[i] = 0.f;
        for (int lane = 0; lane < 64; ++lane) {
            const int b = lane >> 2, r = lane & 3;
            for (int m = 0; m < 8; ++m)
                img[m * 64 + lane] = form ? W4[l4_dim(lane) * 64 + l4_k(m, lane)] : W4[(4 * (m >> 2) + r) * 64 + 4 * b + (m & 3)];
            if (form) { for (int q = 0; q < 4; ++q) if (l4_bias_dim(q, lane) >= 0) img[(8 + q) * 64 + lane] = b4[l4_bias_dim(q, lane)]; }
            else if (b == 0) { for (int q = 0; q < 8; ++q) img[(8 + q) * 64 + lane] = b4[q]; }
        }
        hipMemcpy(dimg, img, sizeof(img), hipMemcpyHostToDevice);
        hipMemset(dres, 0, sizeof(hr));
        if (form) check_l4<true><<<1, 64>>>(dimg, dact, dres); else check_l4<false><<<1, 64>>>(dimg, dact, dres);
        hipMemcpy(hr, dres, sizeof(hr), hipMemcpyDeviceToHost);
        double worst = 0;
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 2; ++e) {
                const int rho = lane >> 4, t = lane & 3, d = 4 * (rho >> 1) + 2 * (rho & 1) + e;
                double ref = b4[d];
                for (int k = 0; k < 64; ++k) ref += (double)W4[d * 64 + k] * ha[k * 4 + t];
                const double df = fabs(ref - hr[lane * 2 + e]);
                if (df > worst) worst = df;
            }
        printf("output layer mapping check, %s + fold, all 64 lanes x 2 dims vs a double-precision matvec: max abs diff %.3g %s\n",
               form ? "8-block form (BLGP 1 / 2 broadcast, two chains)" : "16-block form (two dim-tiles)", worst, worst < 1e-4 ? "OK" : "WRONG");
        all_ok = all_ok && worst < 1e-4;
    }
    hipFree(dimg); hipFree(dact); hipFree(dres);
    return all_ok;
}

// ---- the seam behind the first layer (modes 30 / 31; profiles/k1x_l1_seam_ab.txt).  The state sits replicated over the four blocks of a
// 16-lane row; BLGP 4 + rho hands row rho of the B operand to all four rows, so with A = weights and B = state L1's accumulator comes out
// with register <-> unit-in-quad, lane <-> (block, trajectory): the A layout of the next layer, no transpose behind the ELU.
//   30  mapping check: BLGP 4..7 alone (one MFMA of distinct values per lane) and the whole swapped first layer, against double precision
//   31  the stage head, ticks per pass: L1 with CBSZ = 4 / ABID = 4 rho, merge, ELU, transpose   against   L1 with BLGP 4 + rho, merge, ELU
constexpr int l1_dim(int m) { return 4 * ((m & 3) >> 1) + 2 * ((m & 3) & 1) + (m >= 4 ? 1 : 0); }
template <int BLGP>
__global__ void check_blgp(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ res) {
    const int l = threadIdx.x;
    const f4 d = mfl<BLGP>(a[l], b[l], f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int r = 0; r < 4; ++r) res[r * 64 + l] = d[r];
}
// L1 in the swapped form: chain A starts from the constant and takes m = 0, 2, 4, 6, chain B m = 1, 3, 5, 7 (the order of today's form)
__device__ __forceinline__ f4 l1_swapped(const float (&w1x)[8], const f2 s, const f4 cz) {
    f4 accA = cz, accB = f4{0.f, 0.f, 0.f, 0.f};
    accA = mfl<4>(w1x[0], s[0], accA);  accB = mfl<5>(w1x[1], s[0], accB);
    accA = mfl<6>(w1x[2], s[0], accA);  accB = mfl<7>(w1x[3], s[0], accB);
    accA = mfl<4>(w1x[4], s[1], accA);  accB = mfl<5>(w1x[5], s[1], accB);
    accA = mfl<6>(w1x[6], s[1], accA);  accB = mfl<7>(w1x[7], s[1], accB);
    return accA + accB;
}
__device__ __forceinline__ f4 l1_today(const float (&w1x)[8], const f2 s, const f4 cz) {
    f4 accA = cz, accB = f4{0.f, 0.f, 0.f, 0.f};
    accA = mf<0>(s[0], w1x[0], accA);  accB = mf<4>(s[0], w1x[1], accB);
    accA = mf<8>(s[0], w1x[2], accA);  accB = mf<12>(s[0], w1x[3], accB);
    accA = mf<0>(s[1], w1x[4], accA);  accB = mf<4>(s[1], w1x[5], accB);
    accA = mf<8>(s[1], w1x[6], accA);  accB = mf<12>(s[1], w1x[7], accB);
    return accA + accB;
}
// out[unit][traj] = sum_d W1[unit][d] x[d][traj], reported in the A layout (lane (b, t) register cc = unit 4b + cc): the swapped form as it
// is, today's form through the in-quad transpose.  img = the 8 weight registers [m][lane = unit]; x = [8 dims][4 trajectories]
template <bool SWAPPED>
__global__ void check_l1(const float* __restrict__ img, const float* __restrict__ x, float* __restrict__ res) {
    const int l = threadIdx.x, b = l >> 2, t = l & 3, rho = l >> 4, d01 = 4 * (rho >> 1) + 2 * (rho & 1);
    float w1x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) w1x[m] = img[m * 64 + l];
    const f2 s = f2{x[d01 * 4 + t], x[(d01 + 1) * 4 + t]};     // the state layout: a row's two adjacent dims, in every block of the row
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    const f4 h = SWAPPED ? l1_swapped(w1x, s, z) : quad_transpose(l1_today(w1x, s, z), l);
#pragma unroll
    for (int c = 0; c < 4; ++c) res[(4 * b + c) * 4 + t] = h[c];
}
bool check_l1_seam() {
    bool all_ok = true;
    float ha[64], hb[64], hd[4 * 64], *da, *db, *dd;
    for (int i = 0; i < 64; ++i) { ha[i] = 1.0f + (float)i; hb[i] = 0.5f + 0.25f * (float)((i * 37) % 64); }     // (exact products)
    hipMalloc(&da, sizeof(ha)); hipMalloc(&db, sizeof(hb)); hipMalloc(&dd, sizeof(hd));
    hipMemcpy(da, ha, sizeof(ha), hipMemcpyHostToDevice); hipMemcpy(db, hb, sizeof(hb), hipMemcpyHostToDevice);
    for (int blgp = 4; blgp < 8; ++blgp) {
        hipMemset(dd, 0, sizeof(hd));
        if (blgp == 4) check_blgp<4><<<1, 64>>>(da, db, dd); else if (blgp == 5) check_blgp<5><<<1, 64>>>(da, db, dd);
        else if (blgp == 6) check_blgp<6><<<1, 64>>>(da, db, dd); else check_blgp<7><<<1, 64>>>(da, db, dd);
        hipMemcpy(hd, dd, sizeof(hd), hipMemcpyDeviceToHost);
        int bad = 0;
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int blk = lane >> 2, c = lane & 3;
                // D_b[r][c] = A_b[r] B_src[c]: A from the block's own lanes, B from block (blk & 3) of row blgp - 4
                const double ref = (double)ha[4 * blk + r] * (double)hb[16 * (blgp - 4) + 4 * (blk & 3) + c];
                bad += ref != (double)hd[r * 64 + lane];
            }
        printf("BLGP %d on v_mfma_f32_4x4x1_16b_f32 (B row %d to all four rows), 64 lanes x 4 registers vs a double-precision product: %d mismatches %s\n",
               blgp, blgp - 4, bad, bad ? "WRONG" : "OK");
        all_ok = all_ok && !bad;
    }
    float W1[64 * 8], x[8 * 4], img[8 * 64], hr[64 * 4], *dimg, *dx, *dres;
    for (int i = 0; i < 64 * 8; ++i) W1[i] = (float)((i * 7919 + 13) % 1000) * 1e-3f - 0.5f;
    for (int i = 0; i < 8 * 4; ++i) x[i] = (float)((i * 104729 + 7) % 1000) * 1e-3f - 0.5f;
    for (int m = 0; m < 8; ++m) for (int u = 0; u < 64; ++u) img[m * 64 + u] = W1[u * 8 + l1_dim(m)];
    hipMalloc(&dimg, sizeof(img)); hipMalloc(&dx, sizeof(x)); hipMalloc(&dres, sizeof(hr));
    hipMemcpy(dimg, img, sizeof(img), hipMemcpyHostToDevice); hipMemcpy(dx, x, sizeof(x), hipMemcpyHostToDevice);
    float first[64 * 4];
    for (int form = 0; form < 2; ++form) {
        hipMemset(dres, 0, sizeof(hr));
        if (form) check_l1<true><<<1, 64>>>(dimg, dx, dres); else check_l1<false><<<1, 64>>>(dimg, dx, dres);
        hipMemcpy(hr, dres, sizeof(hr), hipMemcpyDeviceToHost);
        double worst = 0;
        for (int u = 0; u < 64; ++u)
            for (int t = 0; t < 4; ++t) {
                double ref = 0;
                for (int d = 0; d < 8; ++d) ref += (double)W1[u * 8 + d] * x[d * 4 + t];
                const double df = fabs(ref - hr[u * 4 + t]);
                if (df > worst) worst = df;
            }
        printf("first layer mapping check, %s, 64 units x 4 trajectories vs a double-precision matvec: max abs diff %.3g %s\n",
               form ? "swapped (A = weights, B = state on BLGP 4 + rho), no transpose" : "today's (A = state on CBSZ 4 / ABID 4 rho) + in-quad transpose",
               worst, worst < 1e-5 ? "OK" : "WRONG");
        all_ok = all_ok && worst < 1e-5;
        if (form == 0) { for (int i = 0; i < 64 * 4; ++i) first[i] = hr[i]; }
        else {
            int nd = 0;
            for (int i = 0; i < 64 * 4; ++i) { unsigned p, q; memcpy(&p, &first[i], 4); memcpy(&q, &hr[i], 4); nd += p != q; }
            printf("first layer, swapped against today's form as raw 32-bit words: %d of 256 differ %s\n", nd, nd ? "(NOT bit-exact)" : "(bit-exact)");
            all_ok = all_ok && nd == 0;
        }
    }
    hipFree(da); hipFree(db); hipFree(dd); hipFree(dimg); hipFree(dx); hipFree(dres);
    return all_ok;
}
// the stage head as K1x runs it: L1 (8 MFMAs, two chains) -> merge -> scaled-domain ELU -> (today: in-quad transpose, the order alternating as
// in a sequence of seams) -> hA.  Two heads per iteration; what closes the loop (hA -> the next stage input) is the same in both forms.
template <bool SWAPPED>
__global__ __launch_bounds__(64) void bench_head(float* out, long long* cyc, int niter, const float* __restrict__ wsrc) {
    const int l = threadIdx.x;
    float w1x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) w1x[m] = wsrc[m * 64 + l];
    const f4 cz = f4{0.01f, 0.02f, 0.03f, 0.04f};
    f2 s = f2{0.1f + 0.001f * l, 0.2f};
    unsigned long long vmask = 0x5555555555555555ull;
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < niter; it += 2) {
#pragma unroll
        for (int ly = 0; ly < 2; ++ly) {
            f4 h;
            if constexpr (SWAPPED) {
                h = elu_quad_scaled(l1_swapped(w1x, s, cz));
            } else {
                h = elu_quad_scaled(l1_today(w1x, s, cz));
                if (ly == 0) h = quad_transpose_seq<0>(h, vmask); else h = quad_transpose_seq<1>(h, vmask);
            }
            s = f2{h[0], h[1]} * 1e-3f + f2{h[2], h[3]};       // (two packed operations: stands in for the layers behind)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const long long t1 = __builtin_readcyclecounter();
    out[blockIdx.x * 64 + l] = s[0] + s[1] + (float)(vmask & 1);
    if (blockIdx.x == 0 && l == 0) *cyc = t1 - t0;
}
template <bool SWAPPED>
void run_head(const char* name, int nwg, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench_head<SWAPPED><<<nwg, 64>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench_head<SWAPPED><<<nwg, 64>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long c; hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-58s waves/SIMD=%d : %7.1f ns per head (wall), s_memtime %.2f ticks\n", name, nwg / 1024, ms * 1e6 / niter, (double)c / niter);
}
// the gate of the first-layer seam: mapping, then three alternating runs of each form of the head.  `ubench_4x4 l1` runs this alone.
bool l1_seam_gate(float* out, long long* cyc, const float* w) {
    const bool ok = check_l1_seam();
    run_head<false>("stage head, L1 on CBSZ 4 / ABID, ELU, transpose", 1024, out, cyc, w);
    run_head<true>("stage head, L1 swapped on BLGP 4 + rho, ELU", 1024, out, cyc, w);
    run_head<false>("stage head, today's (again)", 1024, out, cyc, w);
    run_head<true>("stage head, swapped (again)", 1024, out, cyc, w);
    run_head<false>("stage head, today's (third)", 1024, out, cyc, w);
    run_head<true>("stage head, swapped (third)", 1024, out, cyc, w);
    return ok;
}

template <int MODE>
void run(const char* name, int nwg, float* out, long long* cyc, const float* w) {
    const int niter = 4000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    bench<MODE><<<nwg, 64>>>(out, cyc, 10, w);
    hipEventRecord(e0);
    bench<MODE><<<nwg, 64>>>(out, cyc, niter, w);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long c; hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-58s waves/SIMD=%d : %7.1f ns per layer (wall), s_memtime %.2f ticks\n", name, nwg / 1024, ms * 1e6 / niter, (double)c / niter);
}

int main(int argc, char** argv) {
    float *out, *w, *act, *res; long long* cyc;
    hipMalloc(&out, 2048 * 64 * sizeof(float)); hipMalloc(&cyc, 8);
    hipMalloc(&w, 64 * 64 * 4); hipMalloc(&act, 64 * 4 * 4); hipMalloc(&res, 64 * 4 * 4);
    float hw[64 * 64], ha[64 * 4], hr[64 * 4];
    for (int i = 0; i < 64 * 64; ++i) hw[i] = (float)((i * 7919) % 1000) * 1e-3f - 0.5f;
    for (int i = 0; i < 64 * 4; ++i) ha[i] = (float)((i * 104729) % 1000) * 1e-3f - 0.5f;
    hipMemcpy(w, hw, sizeof(hw), hipMemcpyHostToDevice);
    hipMemcpy(act, ha, sizeof(ha), hipMemcpyHostToDevice);
    if (argc > 1 && !strcmp(argv[1], "l1")) return l1_seam_gate(out, cyc, w) ? 0 : 1;
    check<<<1, 64>>>(w, act, res);
    hipMemcpy(hr, res, sizeof(hr), hipMemcpyDeviceToHost);
    double worst = 0;
    for (int u = 0; u < 64; ++u)
        for (int t = 0; t < 4; ++t) {
            double ref = 0;
            for (int k = 0; k < 64; ++k) ref += (double)hw[u * 64 + k] * ha[k * 4 + t];
            const double d = fabs(ref - hr[u * 4 + t]);
            if (d > worst) worst = d;
        }
    printf("mapping check (64 x 4x4x1 CBSZ=4/ABID=b + in-quad transpose vs a double-precision matvec): max abs diff %.3g %s\n", worst,
           worst < 1e-4 ? "OK" : "WRONG");
    {
        unsigned* nb; hipMalloc(&nb, 4); hipMemset(nb, 0, 4);
        check_seq<<<1, 64>>>(nb);
        unsigned hnb; hipMemcpy(&hnb, nb, 4, hipMemcpyDeviceToHost);
        printf("ordered in-quad transposes (stage order 0 / 1, mask handed on in vcc) vs the plain one: %u mismatches %s\n", hnb, hnb ? "WRONG" : "OK");
        hipFree(nb);
    }
    check_waist();
    l1_seam_gate(out, cyc, w);
    run_waist<false>("waist 64 -> 8 -> 64, 16-block fold, scalar RK", 1024, out, cyc, w);
    run_waist<true>("waist 64 -> 8 -> 64, 8-block fold (BLGP), packed RK", 1024, out, cyc, w);
    run_waist<false>("waist, 16-block fold, scalar RK (again)", 1024, out, cyc, w);
    run_waist<true>("waist, 8-block fold (BLGP), packed RK (again)", 1024, out, cyc, w);
    run_waist<false>("waist, 16-block fold, scalar RK (third)", 1024, out, cyc, w);
    run_waist<true>("waist, 8-block fold (BLGP), packed RK (third)", 1024, out, cyc, w);
    run<0>("64 x 4x4x1 (2 chains), nothing else", 1024, out, cyc, w);
    run<11>("64 x 4x4x1 on ONE chain (compiler form), nothing else", 1024, out, cyc, w);
    run_asm_one("64 x 4x4x1 on ONE chain, asm with s_nop 1", 1024, out, cyc, w);
    run<6>("the whole layer with the scaled-domain ELU (2 chains)", 1024, out, cyc, w);
    run<13>("the whole layer, scaled ELU, ONE chain", 1024, out, cyc, w);
    run<14>("the whole layer, ONE chain, alternating transpose order", 1024, out, cyc, w);
    run<0>("64 x 4x4x1 (2 chains), nothing else (again)", 1024, out, cyc, w);
    run<11>("64 x 4x4x1 on ONE chain (compiler form) (again)", 1024, out, cyc, w);
    run<6>("the whole layer, scaled ELU, 2 chains (again)", 1024, out, cyc, w);
    run<13>("the whole layer, scaled ELU, ONE chain (again)", 1024, out, cyc, w);
    run<14>("the whole layer, ONE chain, alternating order (again)", 1024, out, cyc, w);
    run_asm<false>("64 x 4x4x1 as ONE asm block per 4 k, B in VGPRs", 1024, out, cyc, w);
    run_asm<true>("64 x 4x4x1 as ONE asm block per 4 k, B read from AccVGPRs", 1024, out, cyc, w);
    run<1>("64 x 4x4x1 + in-quad transpose", 1024, out, cyc, w);
    run<2>("64 x 4x4x1 + ELU + transpose (the whole layer)", 1024, out, cyc, w);
    run<3>("the whole layer, 4 accumulator chains", 1024, out, cyc, w);
    run<4>("the whole layer with the round-5 ELU (v_exp clamp)", 1024, out, cyc, w);
    run<6>("the whole layer with the scaled-domain ELU", 1024, out, cyc, w);
    run<5>("64 x 4x4x1 without the A broadcast (CBSZ = 0)", 1024, out, cyc, w);
    run<7>("64 x (4x4x1 + 1 SALU instruction), nothing else", 1024, out, cyc, w);
    run<8>("64 x (4x4x1 + 2 SALU instructions), nothing else", 1024, out, cyc, w);
    run<0>("64 x 4x4x1 (2 chains), nothing else", 2048, out, cyc, w);
    run<2>("64 x 4x4x1 + ELU + transpose (the whole layer)", 2048, out, cyc, w);
    run16<0, true>("16x16x4 layer as K1 runs it, round-3 ELU", out, cyc, w);
    run16<1, true>("16x16x4 layer as K1 runs it, clamp ELU", out, cyc, w);
    run16<2, true>("16x16x4 layer as K1 runs it, scaled-domain ELU", out, cyc, w);
    run16<1, false>("16x16x4 layer WITHOUT the exchange, clamp ELU", out, cyc, w);
    run16<2, false>("16x16x4 layer WITHOUT the exchange, scaled-domain ELU", out, cyc, w);
    unsigned* nd; hipMalloc(&nd, 4); hipMemset(nd, 0, 4);
    elu_forms<<<(1u << 24) / 256, 256>>>(nd);
    unsigned hnd; hipMemcpy(&hnd, nd, 4, hipMemcpyDeviceToHost);
    printf("ELU forms (min + exp2 vs exp2 with clamp) over 3 x 2^24 inputs of every exponent and sign: %u bitwise differences\n", hnd);
    return 0;
}
