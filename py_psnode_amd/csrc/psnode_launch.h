// Host half of the specialised kernels (K1 .. K9w), written once: run-time value -> template instance, the launch with dynamic LDS,
// ABI struct -> device struct, and the small predicates of the entry points.  Host only: no device code, no macro that expands to a launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "psnode_common.h"

namespace psnode {

// ---- dispatch: f gets the value as a type (std::integral_constant) and names its kernel instance with decltype(tag)::value
template <int N>
using Int = std::integral_constant<int, N>;

// f(Int<method>{}); every value but EULER / MIDPOINT runs RK4_38 (the entry points check the range)
template <class F>
auto with_method(int method, F&& f) {
    switch (method) {
        case PSNODE_EULER: return f(Int<PSNODE_EULER>{});
        case PSNODE_MIDPOINT: return f(Int<PSNODE_MIDPOINT>{});
        default: return f(Int<PSNODE_RK4_38>{});
    }
}
// f(std::true_type{}) or f(std::false_type{}): the second template parameter of a doubled ladder (SAVE, DAE, ENC)
template <class F>
auto with_flag(bool on, F&& f) {
    return on ? f(std::true_type{}) : f(std::false_type{});
}
// f(Int<N>{}) for the N of the list that equals `value`; hipErrorNotSupported when none does.  Only the listed instances exist.
// A pair (NZM, NZA) goes through as NZM * 10 + NZA.
template <int... Ns, class F>
hipError_t pick(int value, F&& f) {
    hipError_t e = hipErrorNotSupported;
    (void)((value == Ns ? (e = f(Int<Ns>{}), true) : false) || ...);
    return e;
}

// ---- launch: dynamic LDS above the 48 KiB default needs the attribute.  launch() sets it whenever the launch asks for dynamic LDS at all;
// a site that sets it on a condition of its own (K7h: the 8-wave instance alone, K11: above 48 KiB) says so through launch_attr().
template <class... Params, class... Args>
hipError_t launch_attr(bool set_max_lds, void (*kern)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args&&... args) {
    if (set_max_lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, stream, std::forward<Args>(args)...);
    return hipGetLastError();
}
template <class... Params, class... Args>
hipError_t launch(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args&&... args) {
    return launch_attr(lds_bytes > 0, kern, grid, block, lds_bytes, stream, std::forward<Args>(args)...);
}

// ---- binding: the ABI structs (include/psnode_hip.h) into the device structs
inline ViewDev view(const psnode_view_f32& v) { return ViewDev{v.ptr, v.stride_t, v.stride_b}; }

// z_jump (and, where the args carry one, v_jump) with its strides
template <class Args, class = void>
struct has_v_jump : std::false_type {};
template <class Args>
struct has_v_jump<Args, std::void_t<decltype(std::declval<Args>().v_jump)>> : std::true_type {};
template <class Dev, class Args>
void bind_jumps(Dev& d, const Args& a) {
    d.zj = a.z_jump; d.zjb = a.zj_stride_b; d.zje = a.zj_stride_e;
    if constexpr (has_v_jump<Args>::value) { d.vj = a.v_jump; d.vjb = a.vj_stride_b; d.vje = a.vj_stride_e; }
}

// the widths alone (what the dims-only queries ask with), and with every layer's weight and bias
inline void bind_dims(const psnode_mlp_f32& m, MlpDev& d) {
    d.n_layers = m.n_layers;
    d.in_dim = m.in_dim;
    for (int l = 0; l < m.n_layers && l < kMaxLayers; ++l) d.out_dim[l] = m.out_dim[l];
}
inline void bind_mlp(const psnode_mlp_f32& m, MlpDev& d) {
    bind_dims(m, d);
    for (int l = 0; l < m.n_layers && l < kMaxLayers; ++l) { d.w[l] = m.weight[l]; d.bias[l] = m.bias[l]; }
}

// the four layers of a `in -> h -> h -> h -> out` MLP into a pack struct's w1 .. b4 (PackMfma, PackX, ...)
template <class Pack>
void set_layers(Pack& p, const float* const* w, const float* const* b) {
    p.w1 = w[0]; p.b1 = b[0]; p.w2 = w[1]; p.b2 = b[1];
    p.w3 = w[2]; p.b3 = b[2]; p.w4 = w[3]; p.b4 = b[3];
}
template <class Pack>
void set_layers(Pack& p, const MlpDev& m) { set_layers(p, m.w, m.bias); }
// ... and the two layers of the latent MLPs `in -> h -> h` into w1 .. b2 (PackLatent, Pack64)
template <class Pack>
void set_layers2(Pack& p, const MlpDev& m) { p.w1 = m.w[0]; p.b1 = m.bias[0]; p.w2 = m.w[1]; p.b2 = m.bias[1]; }
template <class Pack>
void set_layers2(Pack& p, const psnode_mlp_f32& m) { p.w1 = m.weight[0]; p.b1 = m.bias[0]; p.w2 = m.weight[1]; p.b2 = m.bias[1]; }
template <class Pack>
void set_layers(Pack& p, const psnode_mlp_f32& m) { set_layers(p, m.weight, m.bias); }

// the AE's forward image of a DAE call, from the DE's: the same shape fields, no folded x columns, NZA external registers
template <class Pack, class Mlp>
Pack ae_pack(const Pack& de, int NZA, const Mlp& ae, int i_dim, float* out) {
    Pack q = de;
    q.ae = 1; q.NB = 0; q.NE = NZA; q.fold = 0;
    set_layers(q, ae);
    q.out_dim = i_dim; q.out = out;
    return q;
}

// ---- predicates
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool workspace_ok(const void* ws, size_t bytes, size_t need) { return ws && !(reinterpret_cast<uintptr_t>(ws) & 255) && bytes >= need; }
inline int ok_or_hip(hipError_t e) { return e == hipSuccess ? PSNODE_OK : PSNODE_ERR_HIP; }

}  // namespace psnode
