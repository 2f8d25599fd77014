// The build policy of the generic kernels K0 (psnode_generic_impl.h) and K5 (psnode_generic_bwd_impl.h): what separates the four objects each
// is compiled into, as constants the language can see.
#pragma once

namespace psnode {

template <bool ACT, bool PRE, bool RK>
struct GenericBuild {
    static constexpr bool act = ACT;      // the hidden-layer activation is a kernel argument (ActPair, psnode_act.h), not ELU(1)
    static constexpr bool pre = PRE;      // the hidden layers' pre-activations u are kept next to h (SiLU / GELU / Mish differentiate from u)
    static constexpr bool rk = RK;        // the stage loops read a psnode_rk_tableau_f32 kernel argument instead of a.method
    // K5's waves per SIMD: the fully streamed instances (STR 2) that fitted 256 registers keep two workgroups per CU -- every one of the
    // act build, the ELU(1) build's with the accumulators in LDS, none of the builds that keep u
    static constexpr int two_waves(bool gg, int str) { return PRE ? 1 : (str == 2 && (ACT || !gg) ? 2 : 1); }
};
using BuildElu1 = GenericBuild<false, false, false>;
using BuildAct = GenericBuild<true, false, false>;
using BuildPre = GenericBuild<true, true, false>;
using BuildRk = GenericBuild<true, true, true>;

}  // namespace psnode
