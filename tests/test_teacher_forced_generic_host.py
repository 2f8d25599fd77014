"""Teacher-forced training on the generic backward K5, host side (no GPU): the additive C ABI (psnode_dae_bwd_tf_args_f32 and its three
entry points), the status order of the new entry point, and the predicates the solver asks.  The library answers every query here from
the call's dims alone."""
import ctypes

import pytest

from capi_args import R, dae_bwd_args, ode_bwd_args
from capi_args import hip_layers as _layers
from py_psnode_amd import _lib, autograd, fused, models

TF_EXPORTS = ("psnode_dae_backward_tf_supported", "psnode_dae_backward_tf_workspace_bytes", "psnode_dae_backward_tf_f32")
FLAGS = (_lib.FLAG_INPUT_TRUE_X, _lib.FLAG_INPUT_TRUE_I, _lib.FLAG_INPUT_TRUE_X | _lib.FLAG_INPUT_TRUE_I)


def _dae_tf_args(flags, kernel=_lib.KERNEL_AUTO):
    """DAE z4 v6 i6 at hidden 64: a shape without a specialisation (z + v + i > 8)"""
    return dae_bwd_args(kernel, xd=8, zd=4, vd=6, idim=6, hidden=64, flags=flags, method=_lib.RK4_38, T=12, B=5)


def test_the_three_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in TF_EXPORTS:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32), name
    assert lib.psnode_dae_backward_tf_workspace_bytes.restype is ctypes.c_size_t
    assert lib.psnode_abi_version() == 10                     # additive: no struct changed
    a = _lib.DaeBwdTfArgsF32
    assert a.flags.offset == ctypes.sizeof(_lib.DaeBwdArgsF32) and a.x_true.offset == a.flags.offset + 8 and a.i_true.offset == a.x_true.offset + 8
    assert callable(fused.dae_backward_tf)


@pytest.mark.parametrize("flags", FLAGS)
def test_supported_for_a_shape_only_k5_covers(flags):
    lib = _lib.load()
    assert lib.psnode_dae_backward_tf_supported(R(_dae_tf_args(flags))) == 1
    assert lib.psnode_dae_backward_tf_supported(R(_dae_tf_args(flags, kernel=_lib.KERNEL_GENERIC))) == 1
    assert lib.psnode_dae_backward_tf_workspace_bytes(R(_dae_tf_args(flags))) > 0
    m = _dae_tf_args(flags, kernel=_lib.KERNEL_MFMA)
    assert lib.psnode_dae_backward_tf_supported(R(m)) == 0
    assert lib.psnode_dae_backward_tf_workspace_bytes(R(m)) == 0
    assert lib.psnode_dae_backward_tf_f32(R(m), None, 0, None) == -5
    assert lib.psnode_dae_backward_tf_supported(R(_dae_tf_args(flags | 4))) == 0          # an unknown flag bit


def test_flags_zero_is_the_plain_entry_point():
    lib = _lib.load()
    a = _dae_tf_args(0)
    assert lib.psnode_dae_backward_tf_supported(R(a)) == lib.psnode_dae_backward_supported(R(a.base)) > 0      # (K5's mode for the shape)
    assert lib.psnode_dae_backward_tf_workspace_bytes(R(a)) == lib.psnode_dae_backward_workspace_bytes(R(a.base))
    assert lib.psnode_dae_backward_tf_f32(R(a), None, 0, None) == lib.psnode_dae_backward_f32(R(a.base), None, 0, None) == -1


@pytest.mark.parametrize("flags", FLAGS)
def test_status_order_null_pointers_come_after_supported(flags):
    lib = _lib.load()
    assert lib.psnode_dae_backward_tf_f32(None, None, 0, None) == -1
    a = _dae_tf_args(flags)
    assert lib.psnode_dae_backward_tf_f32(R(a), None, 0, None) == -1          # PSNODE_ERR_NULL, not UNSUPPORTED: K5 takes the shape
    bad = _dae_tf_args(flags)
    bad.base.method = 7
    assert lib.psnode_dae_backward_tf_f32(R(bad), None, 0, None) == -3
    one = _dae_tf_args(flags)
    one.base.T = 1                                                            # teacher forcing needs a step
    assert lib.psnode_dae_backward_tf_f32(R(one), None, 0, None) == -2
    sv = _dae_tf_args(flags)
    sv.base.saved_act = 256                                                   # a teacher-forced forward saves nothing
    assert lib.psnode_dae_backward_tf_supported(R(sv)) == 0
    assert lib.psnode_dae_backward_tf_f32(R(sv), None, 0, None) == -5


@pytest.mark.parametrize("flags", FLAGS)
def test_a_flag_without_its_dataset_rows_is_err_null(flags):
    """every pointer of the base call is bound (to one host buffer no kernel will see: the call stops at the pointer check or, with
    the dataset rows there too, at the NULL workspace)"""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    a = _dae_tf_args(flags)
    b = a.base
    for m in (b.de, b.ae):
        for k in range(m.n_layers):
            m.weight[k], m.bias[k] = p, p
    for v in (b.t, b.z, b.v):
        v.ptr, v.stride_t, v.stride_b = p, 0, 0
    for f in ("all_initial", "xs", "is_", "grad_xs", "grad_x_init", "grad_all_initial", "grad_params_de", "grad_params_ae"):
        setattr(b, f, p)
    assert lib.psnode_dae_backward_tf_f32(R(a), None, 0, None) == -1          # x_true / i_true missing
    if flags & _lib.FLAG_INPUT_TRUE_X:
        a.x_true = p
    if flags & _lib.FLAG_INPUT_TRUE_I:
        a.i_true = p
    assert lib.psnode_dae_backward_tf_f32(R(a), None, 0, None) == -4          # all pointers there: PSNODE_ERR_WORKSPACE is next
    b.xs = None
    assert lib.psnode_dae_backward_tf_f32(R(a), None, 0, None) == -1


def test_ode_entry_point_takes_the_flag_on_k5():
    """psnode_ode_backward_f32 with INPUT_TRUE_X: UNSUPPORTED before for kernel = GENERIC or a shape outside K4f's; now the call gets as
    far as the pointer check.  saved_* with the flag and MFMA_WAVE stay refused."""
    lib = _lib.load()

    def args(xd, kernel):
        return ode_bwd_args(kernel, xd=xd, flags=_lib.FLAG_INPUT_TRUE_X, method=_lib.EULER, T=10, B=4)

    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)

    def bind(b):
        for k in range(b.de.n_layers):
            b.de.weight[k], b.de.bias[k] = p, p
        b.t.ptr = b.z.ptr = p
        for f in ("all_initial", "xs", "grad_xs", "grad_x0", "grad_all_initial", "grad_params"):
            setattr(b, f, p)
        return b

    ws = ctypes.create_string_buffer(1 << 20)
    wp = (ctypes.addressof(ws) + 255) & ~255
    for xd, kernel in ((20, _lib.KERNEL_AUTO), (20, _lib.KERNEL_GENERIC), (8, _lib.KERNEL_GENERIC)):
        assert lib.psnode_ode_backward_f32(R(args(xd, kernel)), None, 0, None) == -1
        assert lib.psnode_ode_backward_f32(R(bind(args(xd, kernel))), None, 0, None) == -4
    assert lib.psnode_ode_backward_f32(R(bind(args(20, _lib.KERNEL_MFMA))), None, 0, None) == -5
    b = bind(args(8, _lib.KERNEL_MFMA_WAVE))
    assert lib.psnode_ode_backward_f32(R(b), wp, lib.psnode_ode_backward_workspace_bytes(R(b)), None) == -5
    b = bind(args(20, _lib.KERNEL_AUTO))
    b.saved_act = b.saved_xstage = p
    assert lib.psnode_ode_backward_f32(R(b), wp, lib.psnode_ode_backward_workspace_bytes(R(b)), None) == -5


def test_python_predicates():
    x20 = _layers(models.DE_Func(23, (64, 64, 64), 20).x_dot)
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    for method in ("euler", "midpoint", "rk4"):
        assert autograd.ode_training_supported(method, x20, 20, 3, 50, 33, input_true_x=True)
        assert autograd.ode_training_supported(method, x20, 20, 3, 50, 33, kernel="generic", input_true_x=True)
        assert not autograd.ode_training_supported(method, x20, 20, 3, 50, 33, kernel="mfma", input_true_x=True)      # no K4f at x_dim 20
        assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", input_true_x=True)
        assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="mfma", input_true_x=True)         # K4f
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    assert not autograd.ode_training_supported("rk4", x20, 20, 3, 50, 33, act=tanh, input_true_x=True)
    assert not autograd.ode_training_supported("rk4", ode01, 8, 2, 50, 33, kernel="generic", act=tanh, input_true_x=True)
    assert autograd.ode_training_supported("rk4", x20, 20, 3, 50, 33, act=tanh)                                       # (untied: as before)

    n = 8 + 4 + 6 + 6
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 4 + 6, (64, 64, 64), 6).i_calculator)
    for tx, ti in ((True, False), (False, True), (True, True)):
        assert autograd.dae_training_supported("rk4", de, ae, 8, 4, 6, 6, 50, 33, input_true_x=tx, input_true_i=ti)
        assert autograd.dae_training_supported("euler", de, ae, 8, 4, 6, 6, 50, 33, kernel="generic", input_true_x=tx, input_true_i=ti)
        assert not autograd.dae_training_supported("rk4", de, ae, 8, 4, 6, 6, 50, 33, kernel="mfma", input_true_x=tx, input_true_i=ti)
        assert not autograd.dae_training_supported("rk4", de, ae, 8, 4, 6, 6, 1, 33, input_true_x=tx, input_true_i=ti)        # T < 2
        assert not autograd.dae_training_supported("rk4", de, ae, 8, 4, 6, 6, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti)
    assert fused.dae_backward_supported("rk4", de, ae, 8, 4, 6, 6, kernel="generic")
