// K6: masked, column-weighted squared-error loss + its gradient in one pass over (pred, target, mask).
// HBM-bound: per (t,b) row it reads pred (4D B) + target (4D B) + mask (4 B) and writes grad (4D B); nothing else.
// The two operands arrive in different layouts -- pred is the integrator's time-major [T,B,D], target/mask are the
// scripts' B-major [B,T,D] viewed as [T,B,D] -- so one of them is always strided for a thread-per-row mapping.  Each
// workgroup therefore walks tiles of TT grid points x TB trajectories (TB*D = 256 floats): target/mask are read in
// THEIR contiguous order and transposed into a time-major LDS tile (row pitch chosen so that both the transposing
// writes and the float4 reads are bank-conflict-free), then pred is streamed with float4 loads against the LDS copy and
// grad is streamed out with float4 stores.  Sums: registers across tiles -> fixed-order wave butterflies -> one partial
// row per workgroup -> a second tiny kernel adds the partial rows in double, fixed order (run-to-run bit-identical).
// Shapes off the fast path (D not a power of two, unaligned or oddly strided views) take the scalar kernel.
// The two tile kernels are written in psnode_loss_tile.h (shared with the other loss kinds, psnode_loss_kinds.hip); this object holds their
// squared-error instances -- the code K6 always was -- and the finish kernel.
// Replaces: neural_00_ODE_01_no_encode.py:353-355, neural_01_DAE_01_no_encode.py:414-419 (include/psnode_hip.h).
#include "psnode_loss_tile.h"

namespace psnode {
namespace {

// the squared error on the shared tile walk (psnode_loss_tile.h): K6's kernels, the code they always were
using MseKernels = LossKernels<RhoMse, LossDev, false>;

// out[c] = sum over rows of partial[row][c] (double, fixed order); out[D+1] = total.
// Thread (part, col): part-strided row sums, then column `col` adds its parts in order.
__global__ __launch_bounds__(NT) void masked_mse_finish_kernel(const float* __restrict__ partial, long long rows, int D, float* out) {
    __shared__ double red[NT];
    __shared__ double cols[kMaxLossD + 1];
    const int tid = threadIdx.x, C = D + 1, P = NT / C;
    const int part = tid / C, col = tid % C;
    double s = 0.0;
    if (part < P) {      // four independent chains (the loads of one chain are dependent round trips: 20 us for 2 k partial rows); fixed order
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        long long q = part;
        for (; q + 3 * P < rows; q += 4 * P) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s4[j] += (double)partial[(q + (long long)j * P) * C + col];
        }
        for (int j = 0; q < rows; q += P, ++j) s4[j] += (double)partial[q * C + col];
        s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    red[tid] = s;
    __syncthreads();
    if (tid < C) {
        double tsum = 0.0;
        for (int q = 0; q < P; ++q) tsum += red[q * C + tid];
        cols[tid] = tsum;
        out[tid] = (float)tsum;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int q = 0; q < C; ++q) tot += cols[q];
        out[D + 1] = (float)tot;
    }
}

}  // namespace

hipError_t launch_loss_finish(const float* partial, long long rows, int D, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(masked_mse_finish_kernel, dim3(1), dim3(NT), 0, stream, partial, rows, D, out);
    return hipGetLastError();
}

}  // namespace psnode

using namespace psnode;

extern "C" size_t psnode_masked_mse_workspace_bytes(const psnode_loss_args_f32* a) {
    LossDev d;
    if (!a || !plan(a, d)) return 0;
    return loss_partial_bytes(a, d);
}

extern "C" int32_t psnode_masked_mse_f32(const psnode_loss_args_f32* a, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a) return PSNODE_ERR_NULL;
    LossDev d;
    const int st = loss_call_dev(a, d);
    if (st != PSNODE_OK) return st;
    if (!loss_workspace_ok(workspace, workspace_bytes, loss_partial_bytes(a, d))) return PSNODE_ERR_WORKSPACE;
    d.partial = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long rows = 0;
    if (launch_loss_tiles<MseKernels>(a, d, s, &rows) != hipSuccess) return PSNODE_ERR_HIP;
    return ok_or_hip(launch_loss_finish(d.partial, rows, a->D, a->out, s));
}
