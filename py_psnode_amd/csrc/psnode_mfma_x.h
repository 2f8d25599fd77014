// Device helpers shared by the one-wave-per-4-trajectories integrators K1x (psnode_mfma_x.hip, ODE) and K2x (psnode_mfma_xd.hip, DAE):
// the 4x4x1 MFMA wrappers, the in-quad transpose, the lane folds of the split-K output layer, one H -> H layer.  Layouts: psnode_mfma_x.hip.
#pragma once
#include <type_traits>

#include "psnode_launch.h"
#include "psnode_pack.h"

namespace psnode {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// dim that MFMA m of L1 multiplies: register X01 (m < 4) or X23 of row m & 3 (K1x / K2x's DE: BLGP 4 + (m & 3); K2x's AE head: ABID = 4 (m & 3))
__host__ __device__ constexpr int l1_dim(int m) { return 4 * ((m & 3) >> 1) + 2 * ((m & 3) & 1) + (m >= 4 ? 1 : 0); }

// A image of K1x's output layer (l4_out below).  Weight register m = 4 half + cc multiplies, in block b = lane >> 2, the activation row
// k = 32 half + 4 (b & 7) + cc (the half's blocks are broadcast to the other lane group); row r = lane & 3 of blocks 0..7 belongs to dim r,
// of blocks 8..15 to dim 4 + r.  The bias enters in the first block of each dim-tile (blocks 0 and 8), in the lo chain only.
__host__ __device__ constexpr int l4_k(int m, int lane) { return 32 * (m >> 2) + 4 * ((lane >> 2) & 7) + (m & 3); }
__host__ __device__ constexpr int l4_dim(int lane) { return 4 * (lane >> 5) + (lane & 3); }
__host__ __device__ constexpr int l4_bias_dim(int r, int lane) { return ((lane >> 2) & 7) == 0 ? 4 * (lane >> 5) + r : -1; }     // C register r; -1: zero

template <int ABID>
__device__ __forceinline__ f4 mfx(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0); }
__device__ __forceinline__ f4 mfn(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }
// BLGP 1: every block reads its B row from lanes 0..31 (block b from block b & 7's lanes); 2: from lanes 32..63 (block 8 + (b & 7))
// BLGP 4 + rho: every row of 16 lanes reads its B operand from row rho (block b from block 4 rho + (b & 3)'s lanes)
template <int BLGP>
__device__ __forceinline__ f4 mfl(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, BLGP); }

// 4 x 4 transpose of registers (r0..r3) x lanes (4q..4q+3): two butterfly stages of four v_cndmask_b32_dpp (D = vcc ? src1 : dpp(src0)).
// One asm block (the hazard recognizer does not look inside): s_nop 1 covers VALU write -> DPP read (2 wait states); inside, every DPP
// source was written at least two instructions earlier.
__device__ __forceinline__ f4 quad_transpose(const f4 v) {
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

// The same transpose for a SEQUENCE of seams: the two butterfly stages (lane bit 0 <-> register bit 0, lane bit 1 <-> register bit 1) commute, so
// consecutive seams alternate their order and each starts on the mask the one before left in vcc -- 3 mask moves per seam instead of 4
// (with one wave per SIMD every SALU instruction between two MFMA streams is wall time).  Bit-exact: only moves.
//   ORD 0: enters with vcc = the EVEN lanes, leaves with vcc = the lanes with bit 1 set;   ORD 1: enters with the latter, leaves with EVEN.
// The mask travels as a VALUE (XMask) whose asm operands are pinned to vcc's halves: where nothing else needs vcc between two seams the
// compiler has no move to emit, where something does it saves and restores -- the hand-over is never an assumption about the code between.
// (Two 32-bit register variables: a 64-bit one on vcc crashes the backend of this compiler.)  The caller starts a sequence with xmask_even()
// and keeps ORD alternating; wait states as above.
struct XMask { unsigned lo, hi; };
__device__ __forceinline__ XMask xmask_even() { return XMask{0x55555555u, 0x55555555u}; }
template <int ORD>
__device__ __forceinline__ f4 quad_transpose_seq(const f4 v, XMask& m) {
    float a0, a1, a2, a3, o0, o1, o2, o3;
    const unsigned long long ODD = 0xAAAAAAAAAAAAAAAAull, LO = 0x3333333333333333ull;
    // (readfirstlane: a no-op on a value that is in SGPRs, as in the time loops; it keeps the copy into vcc legal where the compiler carries
    //  the mask through a VGPR -- seen in the saving forwards, across their divergent store branches)
    register unsigned mlo asm("vcc_lo") = __builtin_amdgcn_readfirstlane(m.lo);
    register unsigned mhi asm("vcc_hi") = __builtin_amdgcn_readfirstlane(m.hi);
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
    m.lo = mlo; m.hi = mhi;
    return f4{o0, o1, o2, o3};
}

// (a, b) -> sums over the four blocks of each row of 16 lanes, in every lane: x += row_ror:8 (x); x += row_ror:4 (x) as v_add_f32_dpp.
// One asm block (left to the compiler the rotation is a v_mov_b32_dpp into a zeroed register in front of a packed add: 4 instructions
// per rotation); it carries its own wait states (VALU write -> DPP read: 2).
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
// (a, b) -> one register: lanes 0..31 hold a[l] + a[l + 32], lanes 32..63 hold b[l - 32] + b[l]
__device__ __forceinline__ float fold32(const float a, const float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// (a, b) -> one register: even rows hold a[row] + a[row + 1], odd rows hold b[row - 1] + b[row]
__device__ __forceinline__ float fold16(const float a, const float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// The same on the halves of a register pair, into a fresh pair (operands tied to halves of a pair cost the allocator a copy in and out).
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

// K1x's output layer (64 -> x_dim <= 8), split K over the blocks with the roles swapped (A = weights, B = activations).  The B operand's
// lane-group broadcast lets ONE MFMA serve both dim-tiles: blocks 0..7 accumulate dims 0..3, blocks 8..15 dims 4..7, each over the 8
// activation blocks of one half of k (image: l4_k / l4_dim).  Two chains (k < 32, k >= 32) merged by two packed adds leave what a
// lane-bit-5 fold would: only 8 blocks per dim remain to be summed -- one v_permlane16_swap per register pair (both results are the
// halves of one register pair: one packed add) and the two row rotations.  Returns the state layout {X01, X23}.
__device__ __forceinline__ f2 l4_out(const float (&w4a)[8], const f4 b4c, const f4 hA) {
    f4 lo = b4c, hi = f4{0.f, 0.f, 0.f, 0.f};
    lo = mfl<1>(w4a[0], hA[0], lo); hi = mfl<2>(w4a[4], hA[0], hi);
    lo = mfl<1>(w4a[1], hA[1], lo); hi = mfl<2>(w4a[5], hA[1], hi);
    lo = mfl<1>(w4a[2], hA[2], lo); hi = mfl<2>(w4a[6], hA[2], hi);
    lo = mfl<1>(w4a[3], hA[3], lo); hi = mfl<2>(w4a[7], hA[3], hi);
    const f4 q = lo + hi;
    // (pairs (0,2) / (1,3): a row ends up with two ADJACENT dims)
    const auto e = __builtin_amdgcn_permlane16_swap(__float_as_uint(q[0]), __float_as_uint(q[2]), false, false);
    const auto o = __builtin_amdgcn_permlane16_swap(__float_as_uint(q[1]), __float_as_uint(q[3]), false, false);
    return row_sum2(f2{__uint_as_float(e[0]), __uint_as_float(o[0])} + f2{__uint_as_float(e[1]), __uint_as_float(o[1])});
}

// all 64 k of one H -> H layer: k = 4 bb + cc <-> A register cc, ABID bb.  TWO accumulator chains: on one chain a lone wave issues a 4x4x1
// MFMA every 13.3 cycles instead of every 9.95 (profiles/k1x_one_chain_ubench.txt: 848 against 636 ticks per 64) -- the two wait states of a
// dependent SrcC are NOT hidden in the issue interval, the merge (two packed adds per layer) is the cheaper price.
template <int BB>
__device__ __forceinline__ void hh_block(const float (&wk)[64], const f4 hA, f4& accA, f4& accB) {
    accA = mfx<BB>(hA[0], wk[4 * BB + 0], accA);
    accB = mfx<BB>(hA[1], wk[4 * BB + 1], accB);
    accA = mfx<BB>(hA[2], wk[4 * BB + 2], accA);
    accB = mfx<BB>(hA[3], wk[4 * BB + 3], accB);
}
// ELU of a D tile: the log2e-scaled domain of the inference kernels (SC) or the plain one (the training forwards: their saved rows are
// what the backward kernels read)
template <bool SC>
__device__ __forceinline__ f4 elu_x(const f4 v) {
    if constexpr (SC) return elu_quad_scaled(v);
    else return elu_quad(v);
}
// ORD / m: this seam's place in the caller's sequence of transposes (quad_transpose_seq)
template <bool SC, int ORD>
__device__ __forceinline__ f4 hh_layer(const float (&wk)[64], const float bias, const f4 hA, XMask& m) {
    f4 accA = f4{bias, bias, bias, bias}, accB = f4{0.f, 0.f, 0.f, 0.f};
    hh_block<0>(wk, hA, accA, accB); hh_block<1>(wk, hA, accA, accB); hh_block<2>(wk, hA, accA, accB); hh_block<3>(wk, hA, accA, accB);
    hh_block<4>(wk, hA, accA, accB); hh_block<5>(wk, hA, accA, accB); hh_block<6>(wk, hA, accA, accB); hh_block<7>(wk, hA, accA, accB);
    hh_block<8>(wk, hA, accA, accB); hh_block<9>(wk, hA, accA, accB); hh_block<10>(wk, hA, accA, accB); hh_block<11>(wk, hA, accA, accB);
    hh_block<12>(wk, hA, accA, accB); hh_block<13>(wk, hA, accA, accB); hh_block<14>(wk, hA, accA, accB); hh_block<15>(wk, hA, accA, accB);
    return quad_transpose_seq<ORD>(elu_x<SC>(accA + accB), m);
}

// The same layer with the weights in AccVGPRs (K2x's AE head: 128 B operands that do not fit the 256 architectural VGPRs next to the DE's).
// Left to the register allocator the AGPR-resident weights come back through v_accvgpr_read in front of every MFMA and the scheduler
// serialises the two accumulator chains; here the B operand is READ from the AGPR (`a` constraint) and the order is fixed.  One asm block
// per 4 k; wait states inside (the hazard recognizer does not look): a dependent SrcC needs 2 (the other chain's MFMA + s_nop 0).
template <int BB>
__device__ __forceinline__ void hh_block_acc(const float (&wk)[64], const f4 hA, f4& accA, f4& accB) {
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
template <bool SC, int ORD>
__device__ __forceinline__ f4 hh_layer_acc(const float (&wk)[64], const float bias, const f4 hA, XMask& m) {
    f4 accA = f4{bias, bias, bias, bias}, accB = f4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_nop 1" : "+v"(accA), "+v"(accB));           // VALU write -> MFMA SrcC read
    hh_block_acc<0>(wk, hA, accA, accB); hh_block_acc<1>(wk, hA, accA, accB); hh_block_acc<2>(wk, hA, accA, accB); hh_block_acc<3>(wk, hA, accA, accB);
    hh_block_acc<4>(wk, hA, accA, accB); hh_block_acc<5>(wk, hA, accA, accB); hh_block_acc<6>(wk, hA, accA, accB); hh_block_acc<7>(wk, hA, accA, accB);
    hh_block_acc<8>(wk, hA, accA, accB); hh_block_acc<9>(wk, hA, accA, accB); hh_block_acc<10>(wk, hA, accA, accB); hh_block_acc<11>(wk, hA, accA, accB);
    hh_block_acc<12>(wk, hA, accA, accB); hh_block_acc<13>(wk, hA, accA, accB); hh_block_acc<14>(wk, hA, accA, accB); hh_block_acc<15>(wk, hA, accA, accB);
    asm volatile("s_nop 3" : "+v"(accA), "+v"(accB));           // MFMA write (2 passes) -> VALU read
    return quad_transpose_seq<ORD>(elu_x<SC>(accA + accB), m);
}

template <int Q0, int NQ>
__device__ __forceinline__ f4 ext_mfmas(const float (&we)[16], const float eA, f4 acc) {
    if constexpr (NQ > 0) {
        acc = mfx<Q0>(eA, we[Q0], acc);
        return ext_mfmas<Q0 + 1, NQ - 1>(we, eA, acc);
    } else {
        return acc;
    }
}

// K1x's first layer with the roles swapped (A = weights, lane = unit; B = what sits replicated over the four blocks of a 16-lane row, handed to
// all 16 blocks by BLGP 4 + rho): the accumulator comes out with register <-> unit-in-quad, lane <-> (block, trajectory) -- the A layout of the
// next layer, no transpose behind the ELU.  The state's 8 MFMAs on two chains, in the order of the form they replace (chain A: m = 0, 2, 4, 6
// on top of the per-step constant, chain B: m = 1, 3, 5, 7); the same products, added in the same order.
__device__ __forceinline__ f4 l1_swapped(const float (&w1x)[8], const f2 s, const f4 cz) {
    f4 accA = cz, accB = f4{0.f, 0.f, 0.f, 0.f};
    accA = mfl<4>(w1x[0], s[0], accA);  accB = mfl<5>(w1x[1], s[0], accB);
    accA = mfl<6>(w1x[2], s[0], accA);  accB = mfl<7>(w1x[3], s[0], accB);
    accA = mfl<4>(w1x[4], s[1], accA);  accB = mfl<5>(w1x[5], s[1], accB);
    accA = mfl<6>(w1x[6], s[1], accA);  accB = mfl<7>(w1x[7], s[1], accB);
    return accA + accB;
}
// ... and the external slots' terms of its per-step constant: slot q = 4 j + rho sits in row rho of register eA[j]; one chain, q ascending
template <int Q0, int NQ, int NE>
__device__ __forceinline__ f4 ext_mfmas_swapped(const float (&we)[16], const float (&eA)[NE], f4 acc) {
    if constexpr (NQ > 0) {
        acc = mfl<4 + (Q0 & 3)>(we[Q0], eA[Q0 >> 2], acc);
        return ext_mfmas_swapped<Q0 + 1, NQ - 1, NE>(we, eA, acc);
    } else {
        return acc;
    }
}

constexpr int kXWaves = 4;      // independent waves per workgroup (one per SIMD)

// K1x / K2x address a row as <uniform 64-bit row base> + <32-bit per-lane BYTE offset>: (trajectory * batch stride + column) * 4 must fit
// 32 bits and the batch stride must not be negative (a B-major dataset view of >= 4 GiB, or a negative stride from a C
// caller, would wrap silently).  Views that do not qualify stay on K1 / K2 (64-bit indexing); a forced _WAVE call returns UNSUPPORTED.
inline bool span32_ok(const long long B, const long long sb, const long long cols) {
    if (sb < 0 || B < 1) return false;
    const unsigned long long last = (unsigned long long)(B - 1) * (unsigned long long)sb + (unsigned long long)cols;
    return last < (1ull << 30);                                  // elements: x 4 bytes < 2^32
}

}  // namespace
}  // namespace psnode
