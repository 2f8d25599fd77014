"""Hidden-layer activations other than ELU(1): recognition, the model classes' `activation` keyword and the C ABI's argument checks
(no GPU)."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

from capi_args import act as _act
from capi_args import dae_bwd_args, ode_args, ode_bwd_args
from py_psnode_amd import _lib, fused, models


def _seq(*acts, dims=(30, 64, 64, 8)):
    mods = []
    for k in range(len(dims) - 1):
        mods.append(nn.Linear(dims[k], dims[k + 1]))
        if k + 2 < len(dims):
            mods.append(acts[k % len(acts)])
    return nn.Sequential(*mods)


@pytest.mark.parametrize("mod,kind,params", [
    (nn.Tanh(), _lib.ACT_TANH, {}),
    (nn.Sigmoid(), _lib.ACT_SIGMOID, {}),
    (nn.ReLU(), _lib.ACT_RELU, {}),
    (nn.LeakyReLU(0.1), _lib.ACT_LEAKY_RELU, {"alpha": 0.1}),
    (nn.LeakyReLU(0.0), _lib.ACT_LEAKY_RELU, {"alpha": 0.0}),
    (nn.Softplus(beta=2.0, threshold=15.0), _lib.ACT_SOFTPLUS, {"beta": 2.0, "threshold": 15.0}),
    (nn.ELU(alpha=0.5), _lib.ACT_ELU, {"alpha": 0.5}),
])
def test_sequential_mlp_recognises_each_activation(mod, kind, params):
    r = fused.sequential_mlp(_seq(mod))
    assert r is not None
    layers, act = r
    assert len(layers) == 3 and act is not None and act.kind == kind
    for k, v in params.items():
        assert getattr(act, k) == pytest.approx(v)
    u = torch.randn(7, 5)
    torch.testing.assert_close(act(u), mod(u))


def test_elu1_is_act_none_and_keeps_the_old_recogniser():
    seq = _seq(nn.ELU())
    layers, act = fused.sequential_mlp(seq)
    assert act is None and len(layers) == 3
    assert fused.sequential_layers(seq) is not None


@pytest.mark.parametrize("acts", [
    (nn.Tanh(), nn.ReLU()),                 # mixed within one MLP
    (nn.ELU(), nn.Tanh()),
    (nn.LeakyReLU(-0.1),),
    (nn.Softplus(beta=0.0),),
    (nn.SiLU(),),
    (nn.GELU(),),
    (nn.ELU(alpha=-1.0),),
])
def test_unrecognised_mlps(acts):
    assert fused.sequential_mlp(_seq(*acts)) is None


def test_old_recognisers_still_refuse_non_elu():
    de = models.DE_Func(10, (64, 64, 64), 8, activation=nn.Tanh)
    assert fused.de_layers_of(de, 10, 8) is None
    assert fused.sequential_layers(de.x_dot) is None
    layers, act = fused.de_mlp_of(de, 10, 8)
    assert len(layers) == 4 and act.kind == _lib.ACT_TANH
    ae = models.AE_Func(12 + 9, (32, 32), 3, activation=lambda: nn.Softplus(beta=3.0))
    assert fused.ae_layers_of(ae, 12, 9, 3) is None
    layers, act = fused.ae_mlp_of(ae, 12, 9, 3)
    assert len(layers) == 3 and act.kind == _lib.ACT_SOFTPLUS and act.beta == 3.0
    assert fused.de_mlp_of(de, 11, 8) is None        # recipe widths still checked


def test_recipe_probe_uses_the_modules_activation():
    class MyDE(nn.Module):       # a user class (no recipe marker): the numeric probe runs, with the MLP's own activation
        def __init__(self):
            super().__init__()
            self.x_dot = _seq(nn.Sigmoid(), dims=(30, 32, 32, 8))

        def forward(self, t0, xt, zt, all_initial):
            s = torch.cat((xt, zt), -1)
            return self.x_dot(torch.cat((all_initial, s - all_initial, s), -1))

    m = MyDE()
    layers, act = fused.de_mlp_of(m, 10, 8)
    assert fused._recipe_ok(m, layers, "de_ode", (8, 2), act)
    m2 = MyDE()
    assert not fused._recipe_ok(m2, fused.de_mlp_of(m2, 10, 8)[0], "de_ode", (8, 2), None)      # ELU would not match Sigmoid


def test_model_activation_keyword_defaults_to_the_reference_modules():
    torch.manual_seed(0)
    a = models.DE_Func(10, (64, 64, 64), 8)
    torch.manual_seed(0)
    b = models.DE_Func(10, (64, 64, 64), 8, activation=nn.ELU)
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict())
    assert [type(m) for m in a.x_dot] == [nn.Linear, nn.ELU] * 3 + [nn.Linear]
    assert all(m.alpha == 1.0 for m in a.x_dot if isinstance(m, nn.ELU))
    torch.manual_seed(0)
    c = models.DE_Func(10, (64, 64, 64), 8, activation=nn.Tanh)
    assert list(c.state_dict()) == list(a.state_dict())
    assert [type(m) for m in c.x_dot] == [nn.Linear, nn.Tanh] * 3 + [nn.Linear]
    d = models.DAE_DE_Func(12, (64, 64), 5, activation=nn.ReLU)
    assert [type(m) for m in d.x_dot] == [nn.Linear, nn.ReLU] * 2 + [nn.Linear]
    e = models.AE_Func(20, (16,), 3, activation=lambda: nn.LeakyReLU(0.2))
    assert [type(m) for m in e.i_calculator] == [nn.Linear, nn.LeakyReLU, nn.Linear]
    torch.jit.script(c)          # the export path still scripts


_ode_args = functools.partial(ode_args, method=_lib.RK4_38, T=10, B=4)


def test_capi_act_argument_checks():
    lib = _lib.load()
    a = _ode_args()
    R = ctypes.byref
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(9)), None, 0, None) == -3          # unknown kind
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(-1)), None, 0, None) == -3
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(_lib.ACT_ELU, alpha=0.0)), None, 0, None) == -2
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(_lib.ACT_LEAKY_RELU, alpha=-0.1)), None, 0, None) == -2
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(_lib.ACT_SOFTPLUS, beta=0.0)), None, 0, None) == -2
    assert lib.psnode_ode_integrate_act_f32(R(a), R(_act(_lib.ACT_SOFTPLUS, threshold=float("inf"))), None, 0, None) == -2
    for k in (_lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA_WAVE):
        m = _ode_args(k)
        assert lib.psnode_ode_integrate_act_f32(R(m), R(_act(_lib.ACT_TANH)), None, 0, None) == -5
        assert lib.psnode_ode_integrate_act_supported(R(m), R(_act(_lib.ACT_TANH))) == 0
    assert lib.psnode_ode_integrate_act_supported(R(a), R(_act(_lib.ACT_TANH))) == 1
    assert lib.psnode_ode_integrate_act_supported(R(_ode_args(_lib.KERNEL_GENERIC)), R(_act(_lib.ACT_SIGMOID))) == 1
    assert lib.psnode_ode_integrate_act_supported(R(a), R(_act(42))) == 0
    # NULL act = ELU(1) = the entry point without _act, status for status
    bad = _ode_args()
    bad.method = 7
    assert lib.psnode_ode_integrate_act_f32(R(bad), None, None, 0, None) == lib.psnode_ode_integrate_f32(R(bad), None, 0, None) == -3
    assert lib.psnode_ode_integrate_act_f32(R(bad), R(_act(_lib.ACT_ELU, alpha=1.0)), None, 0, None) == -3
    assert lib.psnode_ode_integrate_act_f32(R(a), None, None, 0, None) == lib.psnode_ode_integrate_f32(R(a), None, 0, None) == -1
    assert lib.psnode_ode_integrate_act_f32(None, R(_act(_lib.ACT_TANH)), None, 0, None) == -1

    d = _lib.DaeArgsF32()
    d.method, d.kernel, d.x_dim, d.z_dim, d.v_dim, d.i_dim, d.T, d.B = _lib.EULER, _lib.KERNEL_MFMA, 4, 2, 1, 2, 5, 3
    assert lib.psnode_dae_integrate_act_f32(R(d), R(_act(_lib.ACT_TANH)), None, None, 0, None) == -5
    assert lib.psnode_dae_integrate_act_f32(R(d), None, R(_act(_lib.ACT_RELU)), None, 0, None) == -5
    assert lib.psnode_dae_integrate_act_f32(R(d), None, R(_act(17)), None, 0, None) == -3


def test_capi_act_backward_checks():
    lib = _lib.load()
    R = ctypes.byref
    b = ode_bwd_args(method=_lib.MIDPOINT, T=10, B=4)
    tanh = _act(_lib.ACT_TANH)
    assert lib.psnode_ode_backward_act_supported(R(b), R(tanh)) == 1
    assert lib.psnode_ode_backward_act_f32(R(b), R(_act(6)), None, 0, None) == -3
    assert lib.psnode_ode_backward_act_f32(R(b), R(_act(_lib.ACT_SOFTPLUS, beta=-1.0)), None, 0, None) == -2
    assert lib.psnode_ode_backward_act_f32(R(b), R(tanh), None, 0, None) == -1          # (pointers are checked after the kernel)
    for k in (_lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA_WAVE):
        b.kernel = k
        assert lib.psnode_ode_backward_act_supported(R(b), R(tanh)) == 0
        assert lib.psnode_ode_backward_act_f32(R(b), R(tanh), None, 0, None) == -5
    b.kernel, b.flags = _lib.KERNEL_AUTO, _lib.FLAG_INPUT_TRUE_X          # K5 has no teacher forcing
    assert lib.psnode_ode_backward_act_supported(R(b), R(tanh)) == 0
    assert lib.psnode_ode_backward_act_f32(R(b), R(tanh), None, 0, None) == -5
    b.flags = 0
    assert lib.psnode_ode_backward_act_supported(R(b), None) == lib.psnode_ode_backward_supported(R(b))

    g = dae_bwd_args(xd=4, zd=2, vd=1, idim=2, hidden=(48, 48), ae_hidden=(32,), method=_lib.RK4_38, T=5, B=3).base
    assert lib.psnode_dae_backward_act_supported(R(g), R(tanh), R(_act(_lib.ACT_SIGMOID))) == 1
    assert lib.psnode_dae_backward_act_supported(R(g), None, R(_act(_lib.ACT_RELU))) == 1
    assert lib.psnode_dae_backward_act_f32(R(g), R(tanh), R(_act(99)), None, 0, None) == -3
    g.kernel = _lib.KERNEL_MFMA
    assert lib.psnode_dae_backward_act_supported(R(g), R(tanh), None) == 0
    assert lib.psnode_dae_backward_act_f32(R(g), R(tanh), None, None, 0, None) == -5
