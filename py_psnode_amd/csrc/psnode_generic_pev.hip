// K0 with per-trajectory events on the sub-step build: the BuildPev object (psnode_generic_build.h), and the kernel that makes its event table.
#define PSNODE_BUILD BuildPev
#include "psnode_generic_impl.h"

namespace psnode {
namespace {

// The table this build reads, [n_steps][B]: one thread per (k, b) holds trajectory b's clock at step k against trajectory b's own event
// list -- the exact equality and the lowest-index rule of the shared table (psnode_capi.hip: event_table_kernel), so a NaN entry (the
// padding of a shorter list) never matches.  Every thread that finds two matches stores the same 1: a plain store, no atomic.
__global__ void event_table_pt_kernel(long long n_steps, long long B, const float* clock, long long stride_k, long long stride_b,
                                      const float* ev_times, long long stride_eb, long long stride_e, int n_events, int* event_idx,
                                      int* dup_flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_steps * B) return;
    const long long k = i / B, b = i % B;
    const float tk = clock[k * stride_k + b * stride_b];
    int hit = -1, cnt = 0;
    for (int e = 0; e < n_events; ++e) {
        if (ev_times[b * stride_eb + e * stride_e] == tk) {
            if (hit < 0) hit = e;
            ++cnt;
        }
    }
    event_idx[i] = hit;
    if (cnt > 1 && dup_flag) *dup_flag = 1;
}

}  // namespace

}  // namespace psnode

extern "C" int32_t psnode_event_table_pt_f32(int64_t n_steps, int64_t B, const float* clock, int64_t stride_k, int64_t stride_b,
                                             const float* event_times, int64_t stride_eb, int64_t stride_e, int32_t n_events,
                                             int32_t* event_idx, int32_t* dup_flag, void* stream) {
    if (n_steps <= 0 || B <= 0) return PSNODE_OK;
    if (!clock || !event_idx || (n_events > 0 && !event_times)) return PSNODE_ERR_NULL;
    if (n_events < 0 || n_steps > (int64_t)0x7fffffff * 256 / B) return PSNODE_ERR_DIMS;      // (the grid of 256-thread blocks is 32 bits)
    const unsigned grid = (unsigned)((n_steps * B + 255) / 256);
    hipLaunchKernelGGL(psnode::event_table_pt_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)n_steps,
                       (long long)B, clock, (long long)stride_k, (long long)stride_b, event_times, (long long)stride_eb, (long long)stride_e,
                       (int)n_events, event_idx, dup_flag);
    return psnode::ok_or_hip(hipGetLastError());
}
