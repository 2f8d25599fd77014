// The tile toolkit of the generic kernels K0 (psnode_generic_impl.h) and K5 (psnode_generic_bwd_impl.h): the workgroup's shape, the quad-row
// index, the fp32 MFMA on four operand pairs and the register-operand tile both kernels' register forms are built from.
#pragma once

namespace psnode {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct NoAct {};                           // what the ELU(1) kernel, which has no `act` argument, names act.de / act.ae
struct NoActPair { NoAct de, ae; };

constexpr int TB = 16;    // trajectories per workgroup
constexpr int NT = 256;   // threads per workgroup (4 waves)

__host__ __device__ constexpr int up16(int v) { return (v + 15) & ~15; }
// float offset of (column r, trajectory c) in a quad-row activation buffer: float index ((col / 4) * 16 + traj) * 4 + col % 4
__device__ __forceinline__ int qi(int r, int c) { return ((((r >> 2) * TB) + c) << 2) | (r & 3); }

#ifndef PSNODE_K0_ABL      // ablation builds (timing only, wrong results; the other values: psnode_generic_impl.h): 1 = a quarter of the MFMAs
#define PSNODE_K0_ABL 0
#endif
__device__ __forceinline__ void mfma_quad(const f4 av, const f4 bv, f4& acc) {
#pragma unroll
    for (int e = 0; e < (PSNODE_K0_ABL == 1 ? 1 : 4); ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
}

// One output tile, Q quads, the A operands in registers (wa) and the B operands read from the quad-row buffer at bq: every read in flight
// before the first MFMA, two accumulator chains.
// Why registers: a ds_read_b128 costs a wave about 64 cycles of LDS-to-register transfer, so reading both operands from LDS (8 reads per
// 16 MFMAs) takes as long as the MFMAs themselves (ablation builds, profiles/r06_k0_generic_mfma.txt).
template <int Q, int QM>
__device__ __forceinline__ f4 tile_reg(const f4* bq, const f4 (&wa)[QM]) {
    f4 bv[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) bv[c] = bq[c * 64];
    __builtin_amdgcn_sched_barrier(0);
    f4 acc = f4{0.f, 0.f, 0.f, 0.f}, acc2 = acc;
#pragma unroll
    for (int c = 0; c < Q; ++c) mfma_quad(wa[c], bv[c], (c & 1) ? acc2 : acc);
    return Q > 1 ? acc + acc2 : acc;
}
// ... with the quads a run-time value: a body each, picked with a switch (with one wave per SIMD nothing hides a loop's taken branches)
template <int QM>
__device__ __forceinline__ f4 tile_reg_any(int S4, const f4* bq, const f4 (&wa)[QM]) {
    if constexpr (QM > 4) {
        switch (S4) {
            case 5: return tile_reg<5, QM>(bq, wa);
            case 6: return tile_reg<6, QM>(bq, wa);
            case 7: return tile_reg<7, QM>(bq, wa);
            case 8: return tile_reg<8, QM>(bq, wa);
            default: break;
        }
    }
    switch (S4) {
        case 1: return tile_reg<1, QM>(bq, wa);
        case 2: return tile_reg<2, QM>(bq, wa);
        case 3: return tile_reg<3, QM>(bq, wa);
        default: return tile_reg<4, QM>(bq, wa);
    }
}

}  // namespace
}  // namespace psnode
