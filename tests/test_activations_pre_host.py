"""The pre-activation family (SiLU, GELU erf / tanh form, Mish): recognition and the C ABI's argument checks and fit queries (no GPU)."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

from capi_args import act as _act
from capi_args import dae_args, dae_bwd_args, ode_args, ode_bwd_args
from py_psnode_amd import _lib, fused, models

PRE = [
    (nn.SiLU(), _lib.ACT_SILU),
    (nn.GELU(), _lib.ACT_GELU),
    (nn.GELU(approximate="tanh"), _lib.ACT_GELU_TANH),
    (nn.Mish(), _lib.ACT_MISH),
]


def _seq(*acts, dims=(30, 64, 64, 8)):
    mods = []
    for k in range(len(dims) - 1):
        mods.append(nn.Linear(dims[k], dims[k + 1]))
        if k + 2 < len(dims):
            mods.append(acts[k % len(acts)])
    return nn.Sequential(*mods)


def test_kind_numbers():
    assert (_lib.ACT_SILU, _lib.ACT_GELU, _lib.ACT_GELU_TANH, _lib.ACT_MISH) == (32, 33, 34, 35)


@pytest.mark.parametrize("mod,kind", PRE)
def test_sequential_mlp_any_recognises_each_activation(mod, kind):
    r = fused.sequential_mlp_any(_seq(mod))
    assert r is not None
    layers, act = r
    assert len(layers) == 3 and act.kind == kind
    u = torch.cat((torch.randn(64) * 3, torch.tensor([-30.0, -8.0, 0.0, 8.0, 30.0])))
    torch.testing.assert_close(act(u), mod(u))
    assert fused.sequential_mlp(_seq(mod)) is None          # the output-derivative recogniser keeps its contract


def test_sequential_mlp_any_keeps_the_other_family():
    layers, act = fused.sequential_mlp_any(_seq(nn.Tanh()))
    assert act.kind == _lib.ACT_TANH and len(layers) == 3
    assert fused.sequential_mlp_any(_seq(nn.ELU()))[1] is None


@pytest.mark.parametrize("acts", [
    (nn.SiLU(), nn.GELU()),                 # mixed within the family
    (nn.GELU(), nn.GELU(approximate="tanh")),
    (nn.SiLU(), nn.Tanh()),                 # mixed across the families
    (nn.Mish(), nn.ELU()),
    (nn.Hardswish(),),
])
def test_sequential_mlp_any_refuses_mixed(acts):
    assert fused.sequential_mlp_any(_seq(*acts)) is None


def test_model_recognisers():
    de = models.DE_Func(10, (64, 64, 64), 8, activation=nn.SiLU)
    layers, act = fused.de_mlp_of(de, 10, 8)
    assert len(layers) == 4 and act.kind == _lib.ACT_SILU
    assert fused.de_layers_of(de, 10, 8) is None
    ae = models.AE_Func(12 + 9, (32, 32), 3, activation=lambda: nn.GELU(approximate="tanh"))
    layers, act = fused.ae_mlp_of(ae, 12, 9, 3)
    assert len(layers) == 3 and act.kind == _lib.ACT_GELU_TANH
    d = models.DAE_DE_Func(12, (48, 48), 5, activation=nn.Mish)
    assert fused.de_mlp_of(d, 12, 5)[1].kind == _lib.ACT_MISH
    assert fused.de_mlp_of(de, 11, 8) is None        # recipe widths still checked


def test_recipe_probe_uses_the_modules_activation():
    class MyDE(nn.Module):
        def __init__(self):
            super().__init__()
            self.x_dot = _seq(nn.GELU(), dims=(30, 32, 32, 8))

        def forward(self, t0, xt, zt, all_initial):
            s = torch.cat((xt, zt), -1)
            return self.x_dot(torch.cat((all_initial, s - all_initial, s), -1))

    m = MyDE()
    layers, act = fused.de_mlp_of(m, 10, 8)
    assert act.kind == _lib.ACT_GELU
    assert fused._recipe_ok(m, layers, "de_ode", (8, 2), act)
    assert not fused._recipe_ok(m, layers, "de_ode", (8, 2), fused.Act(_lib.ACT_SILU))


# ----------------------------------------------------------------------------- C ABI
_ode_args = functools.partial(ode_args, hidden=(64, 64, 64), method=_lib.RK4_38, T=10, B=4)
_ode_bwd = functools.partial(ode_bwd_args, hidden=(64, 64, 64), method=_lib.MIDPOINT, T=10, B=4)
DAE = dict(xd=4, zd=2, vd=1, idim=2, hidden=(48, 48), ae_hidden=(32,), method=_lib.RK4_38, T=5, B=3)


def _dae(cls, kernel=_lib.KERNEL_AUTO):
    return dae_args(kernel, **DAE) if cls is _lib.DaeArgsF32 else dae_bwd_args(kernel, **DAE).base


KINDS = [_lib.ACT_SILU, _lib.ACT_GELU, _lib.ACT_GELU_TANH, _lib.ACT_MISH]
MFMA = [_lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA_WAVE]


@pytest.mark.parametrize("kind", KINDS)
def test_capi_supported_at_auto_and_generic(kind):
    lib = _lib.load()
    R = ctypes.byref
    a = _act(kind, alpha=-5.0, beta=-1.0, threshold=float("nan"))        # parameters are ignored for these kinds
    tanh = _act(_lib.ACT_TANH)
    for k in (_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC):
        assert lib.psnode_ode_integrate_act_supported(R(_ode_args(k)), R(a)) == 1
        assert lib.psnode_ode_backward_act_supported(R(_ode_bwd(k)), R(a)) == 1
        assert lib.psnode_dae_integrate_act_supported(R(_dae(_lib.DaeArgsF32, k)), R(a), R(tanh)) == 1
        assert lib.psnode_dae_integrate_act_supported(R(_dae(_lib.DaeArgsF32, k)), None, R(a)) == 1
        assert lib.psnode_dae_backward_act_supported(R(_dae(_lib.DaeBwdArgsF32, k)), R(a), R(tanh)) == 1
        assert lib.psnode_dae_backward_act_supported(R(_dae(_lib.DaeBwdArgsF32, k)), None, R(a)) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_capi_refuses_mfma_kernels_and_teacher_forcing(kind):
    lib = _lib.load()
    R = ctypes.byref
    a = _act(kind)
    for k in MFMA:
        assert lib.psnode_ode_integrate_act_supported(R(_ode_args(k)), R(a)) == 0
        assert lib.psnode_ode_integrate_act_f32(R(_ode_args(k)), R(a), None, 0, None) == -5
        assert lib.psnode_ode_backward_act_supported(R(_ode_bwd(k)), R(a)) == 0
        assert lib.psnode_ode_backward_act_f32(R(_ode_bwd(k)), R(a), None, 0, None) == -5
        assert lib.psnode_dae_integrate_act_f32(R(_dae(_lib.DaeArgsF32, k)), R(a), None, None, 0, None) == -5
        assert lib.psnode_dae_backward_act_supported(R(_dae(_lib.DaeBwdArgsF32, k)), None, R(a)) == 0
        assert lib.psnode_dae_backward_act_f32(R(_dae(_lib.DaeBwdArgsF32, k)), None, R(a), None, 0, None) == -5
    b = _ode_bwd()
    b.flags = _lib.FLAG_INPUT_TRUE_X                 # K5 has no teacher forcing
    assert lib.psnode_ode_backward_act_supported(R(b), R(a)) == 0
    assert lib.psnode_ode_backward_act_f32(R(b), R(a), None, 0, None) == -5


def test_capi_unknown_kinds_and_null_pointers():
    lib = _lib.load()
    R = ctypes.byref
    a, b = _ode_args(), _ode_bwd()
    for kind in (6, 31, 36, 64):
        assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(kind)), None, 0, None) == -3
        assert lib.psnode_ode_integrate_act_supported(R(a), R(_act(kind))) == 0
        assert lib.psnode_ode_backward_act_f32(R(b), R(_act(kind)), None, 0, None) == -3
        assert lib.psnode_ode_backward_act_supported(R(b), R(_act(kind))) == 0
        assert lib.psnode_dae_integrate_act_f32(R(_dae(_lib.DaeArgsF32)), None, R(_act(kind)), None, 0, None) == -3
        assert lib.psnode_dae_backward_act_supported(R(_dae(_lib.DaeBwdArgsF32)), R(_act(kind)), None) == 0
    silu = _act(_lib.ACT_SILU)
    assert lib.psnode_ode_integrate_act_f32(None, R(silu), None, 0, None) == -1
    assert lib.psnode_ode_backward_act_f32(None, R(silu), None, 0, None) == -1
    assert lib.psnode_dae_backward_act_f32(None, R(silu), None, None, 0, None) == -1
    assert lib.psnode_ode_integrate_act_f32(R(a), R(silu), None, 0, None) == -1          # NULL tensors of a well-formed call
    assert lib.psnode_ode_backward_act_f32(R(b), R(silu), None, 0, None) == -1
    assert lib.psnode_ode_integrate_act_supported(None, R(silu)) == 0


def test_capi_backward_fit_boundary():
    """K5's pre build keeps each hidden layer's pre-activation in LDS next to its output, so its fit ends before the other kinds' does:
    hidden 160 x 3 fits up to x_dim 24 (z_dim 2; the staged path with global accumulators) and not at x_dim 32, where Tanh still fits."""
    lib = _lib.load()
    R = ctypes.byref
    silu, tanh = _act(_lib.ACT_SILU), _act(_lib.ACT_TANH)
    inside, outside = _ode_bwd(xd=24, hidden=(160, 160, 160)), _ode_bwd(xd=32, hidden=(160, 160, 160))
    assert lib.psnode_ode_backward_act_supported(R(inside), R(silu)) == 1
    assert lib.psnode_ode_backward_act_supported(R(outside), R(silu)) == 0
    assert lib.psnode_ode_backward_act_supported(R(outside), R(tanh)) == 1
    assert lib.psnode_ode_backward_act_f32(R(outside), R(silu), None, 0, None) == -5
    # the forward needs no pre-activation: it fits wherever the other kinds' does
    assert lib.psnode_ode_integrate_act_supported(R(_ode_args(xd=32, hidden=(160, 160, 160))), R(silu)) == 1
