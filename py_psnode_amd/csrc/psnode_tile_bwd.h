// Tile-backward toolkit of the one-launch backward kernels at hidden <= 128: K4f (psnode_backward_fused.hip), its DAE sibling K7f
// (psnode_dae_backward_fused.hip) and K7h (psnode_head_grads.hip).  One workgroup = NWV = hidden/16 waves = 16 trajectories; wave w
// owns units 16w..16w+15.  The waves exchange 16x16 blocks through PADDED LDS tiles, so that a block another wave wrote in D layout can
// be read back as it is (all-gather in front of a layer) or TRANSPOSED (the weight gradient of that layer, contracted over the tile's
// trajectories on MFMA).
//   this header                 the types, the MFMA and the tile's size: all three kernels
//   psnode_tile_bwd_dma.h       the LDS-DMA of a weight image, as text, included in the kernel bodies of K4f and K7f
//   psnode_tile_bwd_chain.h     a chain wave's machinery, as text, included in the same bodies behind their prologues
// What differs between K4f and K7f in that machinery comes in through `Tune` (K4fTune / K7fTune, next to each kernel's knobs).
// (The gradient waves of the two-role forms keep their own sweeps: shared, they moved the register counts of K4f's.)
#pragma once
#include "psnode_common.h"

namespace psnode {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f4 fm4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int FTILE = 64 * 4 + 4 * 8;     // padded 16x16 tile (floats): lane l's four rows 4g..4g+3 of column j at 4l + 8g

}  // namespace
}  // namespace psnode
