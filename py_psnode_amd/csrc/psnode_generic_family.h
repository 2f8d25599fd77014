// The entry-point families of the generic kernels K0 (psnode_capi.hip: psnode_{ode,dae}_integrate_<family>_*) and K5 (psnode_backward.hip:
// psnode_{ode,dae}_backward_<family>_*, psnode_dae_backward_tf_*): what a family takes and which build runs it, stated once as a row of
// kFamilies, and the front of the checks both directions share.  Host only; included by those two files alone.
//
// Order of checks = order of the statuses of a call that is wrong in several ways (py_psnode_amd/_lib.py maps statuses to exception types).
// Every family runs this one sequence; a step in brackets exists where the family's row says so, [K0] / [K5] in that direction alone:
//   [segments struct: NULL PSNODE_ERR_NULL, every < 1 (_msp: or per_group < 1) PSNODE_ERR_DIMS] | [sub-steps struct; substeps == 1 on _sub -> the _rk family (tableau
//   given) or the _act family] | act pair | [ELU(1) pair -> the plain entry point] | [the required tableau] | NULL args | [the tableau: given,
//   or the args' method as one; K5, no tableau: the method] | [K5] T, B | route | [K0] fill_* (method, dims, pointers), then [event_idx] |
//   [K5] pointers, among them [x_sub where substeps > 1 and T >= 2], [event_idx], [x_true where a step restarts: T - 1 > every] |
//   workspace | [K0, in dispatch] T, B, LDS fit of the build.
//   _sth (DAE only): an `interp` that is neither PSNODE_EXT_LINEAR nor PSNODE_EXT_LAGRANGE is PSNODE_ERR_METHOD in front of all of it (its query: 0);
//   behind that it is _lin's / _lag's sequence, row for row (sth_family picks the row).
//   _msp: the _ms family's sequence with psnode_segment_groups_f32 in the segments struct's place; more than 65535 chunks (the grid's second
//   dimension) are PSNODE_ERR_UNSUPPORTED with the route; [K5] its workspace is its own layout's (gbwd_msp_layout).
//   _tf [K5; K0 has no such wrapper]: flags == 0 is the plain entry point, in front of all of it.  _rk, _ab, _ab3 and _rkc do not read `method` (K0's copy
//   of the args carries EULER); _lag is _lin's sequence (the stencil table is not checked: NULL is valid); _pev's event_idx is the [T-1, B] table (event-less calls take the other families), _ab's and _ab3's may be NULL.
//   [K0] route (k0_route_ok): kernel AUTO / GENERIC and no training side outputs -- the _act family looks at save_act alone (a lone
//   save_xstage is fill_*'s status); _ms needs the DAE's x view (the restarts read its rows).  A call without a tableau leaves a bad method
//   to fill_*, its query refuses it in front; _act_supported with an ELU(1) pair answers from method and dims alone.
//   [K5] T, B: a DAE call with flags needs T >= 2.  Route (k5_route_ok): kernel AUTO / GENERIC, no saved_* rows, flags within the struct's and
//   only next to an ELU(1) pair, the recipe dims and the LDS fit of the family's build.  Pointers: the teacher-forcing rows among them.
//   The DAE's _act family takes psnode_dae_bwd_args_f32, the others the _tf struct: its _sub with substeps == 1 and no tableau goes to _tf
//   (ELU(1) pair) or refuses flags (PSNODE_ERR_UNSUPPORTED, before the method is looked at) and goes to _act with the base args.
// A new family adds a value of Family, its row, its wrappers; a new build also a policy alias and a BuildId (psnode_generic_build.h), its line
// in dispatch and in generic_backward, and one two-line file per direction (psnode_generic_<fam>.hip, psnode_generic_bwd_<fam>.hip).
// Code of one direction on purpose, and no column: DESIGN.md, "One family table for both directions".
#pragma once

#include "psnode_act.h"
#include "psnode_launch.h"

namespace psnode {

enum Family { kFamTf, kFamAct, kFamRk, kFamSub, kFamLin, kFamPev, kFamAb, kFamMs, kFamMsp, kFamAb3, kFamLag, kFamRkc, kFamSthLin, kFamSthLag };
// the tableau: no argument, `method` is read | NULL is PSNODE_ERR_NULL | NULL is the args' method as one | no argument, always one stage
enum Tab { kTabNone, kTabRequired, kTabOrMethod, kTabOneStage };
// the sub-steps struct: no argument | NULL is PSNODE_ERR_NULL | NULL is one sub-step
enum Sub { kSubNone, kSubRequired, kSubOrOne };
struct FamilyRow {
    BuildId build;          // kBuildAct: or kBuildPre, by the kinds of the pair (K0: act_pair_pre, K5: act_pair_keeps_u)
    bool elu1_plain;        // an ELU(1) pair is the plain entry point's call, and is forwarded to it
    Tab tab; Sub sub;
    bool demotes;           // substeps == 1 is the family without sub-steps: _rk with a tableau, else _act
    bool seg;               // takes the segments struct
    bool needs_events;      // event_idx NULL: PSNODE_ERR_NULL
    bool no_tf;             // refuses every teacher-forcing flag
    bool saved_all;         // refuses every saved_* row / side output; false: the _act family's own rule, which differs by direction
    bool pre; int lin;      // the LDS fit of its build: the pre-activations kept (K5; kBuildPre's too), the linear-externals layout (2: the Lagrange build's)
    bool par;               // the segments struct is psnode_segment_groups_f32: the grid is tiles x chunks, K5's workspace its own layout
};
constexpr FamilyRow kFamilies[] = {
    //          build       elu1   tableau       sub-steps     demotes seg    events no_tf  saved  pre    lin    par
    /* _tf  */ {kBuildElu1, false, kTabNone,     kSubNone,     false,  false, false, false, true,  false, false},
    /* _act */ {kBuildAct,  true,  kTabNone,     kSubNone,     false,  false, false, false, false, false, false},
    /* _rk  */ {kBuildRk,   false, kTabRequired, kSubNone,     false,  false, false, false, true,  true,  false},
    /* _sub */ {kBuildSub,  false, kTabOrMethod, kSubRequired, true,   false, false, false, true,  true,  false},
    /* _lin */ {kBuildLin,  false, kTabOrMethod, kSubOrOne,    false,  false, false, false, true,  true,  true},
    /* _pev */ {kBuildPev,  false, kTabOrMethod, kSubOrOne,    false,  false, true,  false, true,  true,  false},
    /* _ab  */ {kBuildAb,   false, kTabOneStage, kSubNone,     false,  false, false, true,  true,  true,  false},      // (a multistep history has no teacher-forced form)
    /* _ms  */ {kBuildMs,   false, kTabOrMethod, kSubOrOne,    false,  true,  false, true,  true,  true,  false},      // (every teacher-forced step restarts already)
    /* _msp */ {kBuildMsp,  false, kTabOrMethod, kSubOrOne,    false,  true,  false, true,  true,  true,  false, true},      // (_ms over a tiles x chunks grid)
    /* _ab3 */ {kBuildAb3,  false, kTabOneStage, kSubNone,     false,  false, false, true,  true,  true,  false},      // (_ab's row: the same arguments, checks and fit)
    /* _lag */ {kBuildLag,  false, kTabOrMethod, kSubOrOne,    false,  false, false, false, true,  true,  2},          // (_lin's row and the stencil table, which may be NULL; its own layout)
    /* _rkc */ {kBuildRkc,  false, kTabOneStage, kSubRequired, false,  false, false, false, true,  true,  false},      // (_sub's row without a tableau and without the demotion: the stage count in the sub-steps' place, rkc_as_sub)
    /* _sth */ {kBuildLinSth, false, kTabOrMethod, kSubOrOne,  false,  false, false, false, true,  true,  true},       // (interp PSNODE_EXT_LINEAR: _lin's row on the stage-heads build; DAE only)
    /* _sth */ {kBuildLagSth, false, kTabOrMethod, kSubOrOne,  false,  false, false, false, true,  true,  2},          // (interp PSNODE_EXT_LAGRANGE: _lag's row on the stage-heads build; DAE only)
};
struct CallOpts {      // what a call carries behind its args; a family's wrappers leave what it does not take at NULL / 0
    const psnode_act_f32 *de_act, *ae_act;
    const psnode_rk_tableau_f32* tab;
    const psnode_substeps_f32* sub;
    const psnode_segments_f32* seg;
    int per_trajectory;      // _ab, _ab3: a non-NULL event_idx is the [T-1, B] table (else the shared [T-1])
    const psnode_segment_groups_f32* grp;      // _msp: in seg's place
    const psnode_ext_stencil_f32* stencil;     // _lag: the stencil table [T-1, B], or NULL (one piece 0 .. T - 1 for every trajectory)
    const psnode_rkc_f32* rkc;                 // _rkc: the recurrence; its wrappers hand `sub` what rkc_as_sub makes of it
    // what a family with segments reads, from whichever of the two structs it takes
    bool has_seg() const { return seg || grp; }
    int every() const { return grp ? grp->every : seg->every; }
    const float* x_true() const { return grp ? grp->x_true : seg->x_true; }
    int per_group() const { return grp ? grp->per_group : 1; }
};
// The _rkc family's struct as the sub-steps struct the shared checks read: NULL stays NULL (PSNODE_ERR_NULL), a stage count outside
// 1 .. PSNODE_RKC_MAX_STAGES becomes the sub-step count 0 (PSNODE_ERR_DIMS, what a bad sub-step count gets), x_stage is x_sub.
inline const psnode_substeps_f32* rkc_as_sub(const psnode_rkc_f32* r, psnode_substeps_f32& s) {
    if (!r) return nullptr;
    s.substeps = r->stages >= 1 && r->stages <= PSNODE_RKC_MAX_STAGES ? r->stages : 0;
    s.x_sub = r->x_stage;
    return &s;
}
// the row of an _sth call by its interpolant; false: no such interpolant
inline bool sth_family(int32_t interp, Family& fam) {
    if (interp != PSNODE_EXT_LINEAR && interp != PSNODE_EXT_LAGRANGE) return false;
    fam = interp == PSNODE_EXT_LAGRANGE ? kFamSthLag : kFamSthLin;
    return true;
}
// the time chunks of a segment-parallel call (1 for every other family)
inline long long family_chunks(const FamilyRow& f, const CallOpts& o, long long T) { return f.par ? msp_chunks(T, o.every(), o.per_group()) : 1; }
constexpr long long kMaxChunks = 65535;      // (the launch grid's second dimension)
// The front of every call and query (which answers 0 for every status): segments | sub-steps, where substeps == 1 demotes `fam` | act pair
inline int family_front(Family& fam, const CallOpts& o, ActPair& p, bool& elu1) {
    const FamilyRow& f = kFamilies[fam];
    if (f.seg && (f.par ? !o.grp : !o.seg)) return PSNODE_ERR_NULL;
    if (f.seg && (o.every() < 1 || o.per_group() < 1)) return PSNODE_ERR_DIMS;
    if (f.sub == kSubRequired || (f.sub == kSubOrOne && o.sub)) {
        const int rc = substeps_check(o.sub);
        if (rc) return rc;
        if (f.demotes && o.sub->substeps == 1) fam = o.tab ? kFamRk : kFamAct;
    }
    return act_pair(o.de_act, o.ae_act, p, elu1);
}
// Behind the forward of an ELU(1) pair: the required tableau | NULL args (`method` NULL) | the tableau `t` the build runs -- the given one, the
// args' method as one, or the one-stage one.  A family without a tableau answers for its method alone and leaves `t`.
inline int family_tableau(const FamilyRow& f, const psnode_rk_tableau_f32* tab, const int32_t* method, psnode_rk_tableau_f32& t) {
    const int rc = f.tab == kTabRequired ? rk_tableau_check(tab) : PSNODE_OK;
    if (rc) return rc;
    if (!method) return PSNODE_ERR_NULL;
    if (f.tab == kTabNone) return *method < PSNODE_EULER || *method > PSNODE_RK4_38 ? PSNODE_ERR_METHOD : PSNODE_OK;
    return sub_tableau(tab, f.tab == kTabOneStage ? (int)PSNODE_EULER : *method, t);
}
// the build of the family's call (`pre_pair`: K0 act_pair_pre, K5 act_pair_keeps_u) and its sub-steps per grid interval
inline BuildId family_build(const FamilyRow& f, bool pre_pair) { return f.build == kBuildAct && pre_pair ? kBuildPre : f.build; }
inline int family_substeps(const FamilyRow& f, const CallOpts& o) { return f.sub != kSubNone && o.sub ? o.sub->substeps : 1; }
}  // namespace psnode
