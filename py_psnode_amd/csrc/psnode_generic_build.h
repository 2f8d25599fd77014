// The build policy of the generic kernels K0 (psnode_generic_impl.h) and K5 (psnode_generic_bwd_impl.h): what separates the nine objects each
// is compiled into, as constants the language can see.
#pragma once

namespace psnode {

template <bool ACT, bool PRE, bool RK, bool SUB = false, bool LIN = false, bool PEV = false, bool AB = false, bool MS = false>
struct GenericBuild {
    static constexpr bool act = ACT;      // the hidden-layer activation is a kernel argument (ActPair, psnode_act.h), not ELU(1)
    static constexpr bool pre = PRE;      // the hidden layers' pre-activations u are kept next to h (SiLU / GELU / Mish differentiate from u)
    static constexpr bool rk = RK;        // the stage loops read a psnode_rk_tableau_f32 kernel argument instead of a.method
    static constexpr bool sub = SUB;      // every grid interval runs SubDev::n equal sub-steps (a further kernel argument, psnode_common.h)
    static constexpr bool lin = LIN;      // every stage reads z | v interpolated linearly between the interval's two grid points (needs sub)
    static constexpr bool pev = PEV;      // the event table is [T-1, B]: every trajectory jumps at its own steps (needs sub; not with lin)
    static constexpr bool ab = AB;        // two-step Adams-Bashforth: one DE evaluation per step, the previous slope and per-column c0 / c1 (AbDev,
                                          // psnode_common.h; needs pev, whose per-column event index also serves a shared table through a column stride of 0)
    static constexpr bool ms = MS;        // multiple shooting: every MsDev::every-th grid point restarts from the dataset row (MsDev, psnode_common.h;
                                          // needs sub; not with lin, pev or ab)
    // K5's waves per SIMD: the fully streamed instances (STR 2) that fitted 256 registers keep two workgroups per CU -- every one of the
    // act build, the ELU(1) build's with the accumulators in LDS, none of the builds that keep u
    static constexpr int two_waves(bool gg, int str) { return PRE ? 1 : (str == 2 && (ACT || !gg) ? 2 : 1); }
};
// The sub-step loop of both kernel bodies: `do { ... } while (si.more())` around what a step does per sub-step.  Without sub-steps it is one
// pass whose every question is a constant, so that the builds without them compile to the code they had before the loop existed.
template <bool SUB> struct SubIter {
    int n, i;
    __host__ __device__ explicit SubIter(int n_) : n(n_), i(0) {}
    __host__ __device__ bool first() const { return i == 0; }
    __host__ __device__ bool last() const { return i + 1 == n; }
    __host__ __device__ bool more() { return ++i < n; }
};
template <> struct SubIter<false> {
    static constexpr int i = 0;
    __host__ __device__ explicit constexpr SubIter(int) {}
    static constexpr bool first() { return true; }
    static constexpr bool last() { return true; }
    static constexpr bool more() { return false; }
};

using BuildElu1 = GenericBuild<false, false, false>;
using BuildAct = GenericBuild<true, false, false>;
using BuildPre = GenericBuild<true, true, false>;
using BuildRk = GenericBuild<true, true, true>;
using BuildSub = GenericBuild<true, true, true, true>;      // BuildRk's policy with sub-steps: all ten activation kinds, the tableau
using BuildLin = GenericBuild<true, true, true, true, true>;      // BuildSub's policy with linearly interpolated externals; every substeps >= 1
using BuildPev = GenericBuild<true, true, true, true, false, true>;      // BuildSub's policy with per-trajectory events; every substeps >= 1
using BuildAb = GenericBuild<true, true, true, true, false, true, true>;      // BuildPev's policy as Adams-Bashforth 2; one sub-step, a one-stage tableau
using BuildMs = GenericBuild<true, true, true, true, false, false, false, true>;      // BuildSub's policy with multiple-shooting restarts; every substeps >= 1

}  // namespace psnode
