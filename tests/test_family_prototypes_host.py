"""The ctypes prototypes of the 62 K0 / K5 family entry points, which py_psnode_amd/_lib.py builds in one loop from the family table of
py_psnode_amd/fused/_common.py (FAMILIES), against the list its hand-written loops gave before that table existed (no GPU; the built
library is loaded, nothing is called).  P(X): a pointer to the struct X."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from py_psnode_amd import _lib  # noqa: E402

PROTOTYPES = (
    ("psnode_ode_integrate_act_supported", "c_int32", "P(OdeArgsF32) P(ActF32)"),
    ("psnode_ode_integrate_act_f32", "c_int32", "P(OdeArgsF32) P(ActF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_act_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32)"),
    ("psnode_dae_integrate_act_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_act_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32)"),
    ("psnode_ode_backward_act_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_act_supported", "c_int32", "P(DaeBwdArgsF32) P(ActF32) P(ActF32)"),
    ("psnode_dae_backward_act_f32", "c_int32", "P(DaeBwdArgsF32) P(ActF32) P(ActF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_tf_supported", "c_int32", "P(DaeBwdTfArgsF32)"),
    ("psnode_dae_backward_tf_workspace_bytes", "c_size_t", "P(DaeBwdTfArgsF32)"),
    ("psnode_dae_backward_tf_f32", "c_int32", "P(DaeBwdTfArgsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_rk_supported", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32)"),
    ("psnode_ode_integrate_rk_f32", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_rk_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32)"),
    ("psnode_dae_integrate_rk_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_rk_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32)"),
    ("psnode_ode_backward_rk_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_rk_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32)"),
    ("psnode_dae_backward_rk_workspace_bytes", "c_size_t", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32)"),
    ("psnode_dae_backward_rk_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_sub_supported", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_integrate_sub_f32", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_sub_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_integrate_sub_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_sub_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_backward_sub_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_sub_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_backward_sub_workspace_bytes", "c_size_t", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_backward_sub_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_lin_supported", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_integrate_lin_f32", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_lin_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_integrate_lin_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_lin_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_backward_lin_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_lin_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_backward_lin_workspace_bytes", "c_size_t", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_backward_lin_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_pev_supported", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_integrate_pev_f32", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_pev_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_integrate_pev_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_pev_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_ode_backward_pev_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_pev_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32)"),
    ("psnode_dae_backward_pev_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_ab_supported", "c_int32", "P(OdeArgsF32) P(ActF32)"),
    ("psnode_ode_integrate_ab_f32", "c_int32", "P(OdeArgsF32) P(ActF32) c_int32 c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_ab_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32)"),
    ("psnode_dae_integrate_ab_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) c_int32 c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_ab_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32)"),
    ("psnode_ode_backward_ab_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) c_int32 c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_ab_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32)"),
    ("psnode_dae_backward_ab_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) c_int32 c_void_p c_size_t c_void_p"),
    ("psnode_ode_integrate_ms_supported", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32)"),
    ("psnode_ode_integrate_ms_f32", "c_int32", "P(OdeArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_integrate_ms_supported", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32)"),
    ("psnode_dae_integrate_ms_f32", "c_int32", "P(DaeArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32) c_void_p c_size_t c_void_p"),
    ("psnode_ode_backward_ms_supported", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32)"),
    ("psnode_ode_backward_ms_f32", "c_int32", "P(OdeBwdArgsF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32) c_void_p c_size_t c_void_p"),
    ("psnode_dae_backward_ms_supported", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32)"),
    ("psnode_dae_backward_ms_f32", "c_int32", "P(DaeBwdTfArgsF32) P(ActF32) P(ActF32) P(RkTableauF32) P(SubstepsF32) P(SegmentsF32) c_void_p c_size_t c_void_p"),
)
NAMES = {ctypes.c_int32: "c_int32", ctypes.c_size_t: "c_size_t", ctypes.c_void_p: "c_void_p"}


def _name(t) -> str:
    return NAMES[t] if t in NAMES else f"P({t._type_.__name__})"


def test_every_family_prototype_is_the_listed_one():
    lib = _lib.load()
    listed = {n for n, _, _ in PROTOTYPES}
    fams = {n for n in _lib.EXPORTS if any(f"_{f}_" in n for f in ("act", "tf", "rk", "sub", "lin", "pev", "ab", "ms"))
            and ("_integrate_" in n or "_backward_" in n)}
    assert len(PROTOTYPES) == 62 and listed == fams
    for name, restype, argtypes in PROTOTYPES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert (_name(fn.restype), " ".join(_name(t) for t in fn.argtypes)) == (restype, argtypes), name
