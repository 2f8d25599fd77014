"""Explicit Runge-Kutta tableaus (Heun2, Ralston2, Kutta3, SSPRK3, RK4Classic; any ExplicitRK) on the generic kernels: K0 forward, K0 + K5
training.  References: the reference-captured goldens for the Euler / Midpoint / 3/8 tableaus; for the named methods the package's own
callback walk of the SAME modules in float64 on the CPU, gradients from torch autograd through that walk.  Tolerances: helpers.TOL_GPU on
traj_rel_err for trajectories, TOL_GPU of the tensor's max for gradients (generic_cases.close)."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn as nn

import generic_cases as C
from capi_args import state_dict_of as _sd
from generic_cases import DAE_SHAPES, K5_DAE_SHAPES, K5_ODE_SHAPES, ODE_FWD_SHAPES
from helpers import TOL_GPU, T, load, traj_rel_err
from py_psnode_amd import _lib, autograd, models
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

NAMED = {"Heun2": nd.Heun2, "Ralston2": nd.Ralston2, "Kutta3": nd.Kutta3, "SSPRK3": nd.SSPRK3, "RK4Classic": nd.RK4Classic}
BUILTIN = {
    "euler": (((),), (1.0,), 1),
    "midpoint": (((), (0.5,)), (0.0, 1.0), 2),
    "rk4": (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125), 4),
}
B0, T0 = 19, 9          # one full tile of 16 trajectories plus a partial one


def _solver(name, mode, kernel="auto"):
    s = nd.ExplicitRK(*BUILTIN[name], name=f"{name}-tableau") if name in BUILTIN else NAMED[name]()
    s.fused, s.kernel = mode, kernel
    return s


# ----------------------------------------------------------------------------- the reference's goldens through the _rk_ route
@pytest.mark.parametrize("method", list(BUILTIN))
def test_g2_ode_goldens_through_the_tableau_route(method):
    d = load("g2_ode.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "de__"))
    de = de.cuda()
    P = lambda k: T(d[k]).cuda().permute(1, 0, 2)
    t, tr, x, z, a0 = P("t"), P("t_ragged"), P("x"), P("z"), T(d["all_initial"]).cuda()
    ev = nd.ODE_Event()
    ev.set_event(T(d["event_t"]).cuda(), T(d["z_jump"]).cuda())
    no = nd.ODE_Event()
    no.set_event(torch.full_like(T(d["event_t"]), -1.0).cuda(), T(d["z_jump"]).cuda())
    s = _solver(method, "require", "generic")
    with torch.no_grad():
        cases = {
            "plain": s.integrate_ODE(de, t, x, z, a0, no.event_fn, no.jump_change_fn),
            "noevfn": s.integrate_ODE(de, t, x, z, a0),
            "events": s.integrate_ODE(de, t, x, z, a0, ev.event_fn, ev.jump_change_fn),
            "events_truex": s.integrate_ODE(de, t, x, z, a0, ev.event_fn, ev.jump_change_fn, input_true_x=True),
            "ragged": s.integrate_ODE(de, tr, x, z, a0, ev.event_fn, ev.jump_change_fn),
        }
    for name, got in cases.items():
        e = traj_rel_err(got.cpu(), d[f"{method}_{name}"])
        print(method, name, f"{e:.3e}")
        assert e <= TOL_GPU, name


@pytest.mark.parametrize("method", list(BUILTIN))
def test_g3_dae_goldens_through_the_tableau_route(method):
    d = load("g3_dae.npz")
    de = models.DAE_DE_Func(14, (64, 64, 64), 8)
    ae = models.AE_Func(26, (64, 64, 64), 2)
    de.load_state_dict(_sd(d, "de__"))
    ae.load_state_dict(_sd(d, "ae__"))
    de, ae = de.cuda(), ae.cuda()
    P = lambda k: T(d[k]).cuda().permute(1, 0, 2)
    t, x, z, v, i = (P(k) for k in ("t", "x", "z", "v", "i"))
    xi, a0 = T(d["x_init"]).cuda(), T(d["all_initial"]).cuda()
    ev = nd.DAE_Event()
    ev.set_event(T(d["event_t"]).cuda(), T(d["z_jump"]).cuda(), T(d["v_jump"]).cuda())
    s = _solver(method, "require", "generic")
    with torch.no_grad():
        for tx in (False, True):
            for ti in (False, True):
                for use_ev in (False, True):
                    kw = dict(event_fn=ev.event_fn, jump_change_fn=ev.jump_change_fn) if use_ev else {}
                    xs, is_ = s.integrate_DAE(xi, de, ae, t, x, z, v, i, a0, input_true_x=tx, input_true_i=ti, **kw)
                    key = f"{method}_tx{int(tx)}_ti{int(ti)}_ev{int(use_ev)}"
                    ex, ei = traj_rel_err(xs.cpu(), d[key + "_x"]), traj_rel_err(is_.cpu(), d[key + "_i"])
                    print(key, f"{ex:.3e} {ei:.3e}")
                    assert ex <= TOL_GPU and ei <= TOL_GPU, key


def test_g5_long_run_with_the_three_eighths_tableau():
    d = load("g5_long.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "de__"))
    t, z = (T(d[k]).cuda().permute(1, 0, 2) for k in ("t", "z"))
    x = torch.zeros(t.shape[0], t.shape[1], 8, device="cuda")
    x[0] = T(d["x0"])[:, 0].cuda()
    with torch.no_grad():
        got = _solver("rk4", "require", "generic").integrate_ODE(de.cuda(), t, x, z, T(d["all_initial"]).cuda())
    e = traj_rel_err(got.cpu(), d["rk4"])
    print(f"g5, 1001 grid points: {e:.3e}")
    assert e <= TOL_GPU


# ----------------------------------------------------------------------------- cases
def _ode_case(xd, zd, hidden, B, Tn, seed, events=True, pad=True, act=nn.ELU):
    """events at grid rows 1 and T // 2 of the ragged clock"""
    return C.ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=(1, Tn // 2) if events else (), pad=pad, act=act)


def _dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, **acts):
    return C.dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, ev_rows=(1, Tn // 2), **acts)


def _ode_fwd_pair(name, de, t, x, z, ev, zj, tx=False, mode="require", kernel="auto"):
    return C.ode_forward_pair(_solver(name, "off"), _solver(name, mode, kernel), de, t, x, z, ev, zj, tx)


@pytest.mark.parametrize("name", list(NAMED))
@pytest.mark.parametrize("shape", list(ODE_FWD_SHAPES))
@pytest.mark.parametrize("tx", [False, True])
def test_ode_forward(name, shape, tx):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances -- with events, a ragged -1-padded clock and
    teacher forcing"""
    xd, zd, hidden = ODE_FWD_SHAPES[shape]
    de, t, x, z, ev, zj = _ode_case(xd, zd, hidden, B0, T0, seed=3 + xd + len(hidden))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # (a walk under "auto" warns)
        out, ref = _ode_fwd_pair(name, de, t, x, z, ev, zj, tx, mode="auto")
    e = traj_rel_err(out.cpu(), ref)
    print(name, shape, tx, f"{e:.3e}")
    assert torch.isfinite(out).all() and e <= TOL_GPU


@pytest.mark.parametrize("name", list(NAMED))
@pytest.mark.parametrize("B,Tn", [(B0, 1), (B0, 2), (33, T0)])
def test_ode_forward_short_grids_and_three_tiles(name, B, Tn):
    de, t, x, z, ev, zj = _ode_case(8, 2, (64, 64, 64), B, Tn, seed=B + Tn)
    out, ref = _ode_fwd_pair(name, de, t, x, z, ev, zj, kernel="generic")
    assert out.shape == ref.shape and traj_rel_err(out.cpu(), ref) <= TOL_GPU


@pytest.mark.parametrize("name", ["Kutta3", "RK4Classic"])
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(name, shape, mode):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    case = _dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=17 + xd)
    tx, ti = "tx1" in mode, "ti1" in mode
    if mode == "events_no_x":
        case = C.without_x(case)
    out, ref = C.dae_forward_pair(_solver(name, "off"), _solver(name, "require"), case, tx, ti)
    ex, ei = traj_rel_err(out[0].cpu(), ref[0]), traj_rel_err(out[1].cpu(), ref[1])
    print(name, shape, mode, f"{ex:.3e} {ei:.3e}")
    assert ex <= TOL_GPU and ei <= TOL_GPU


# ----------------------------------------------------------------------------- training
# the file's gate: cotangent G from seed 3, the fused function ran, helpers.TOL_GPU of each tensor's max
def _check_ode(name, de, t, x, z, ev, zj, tx=False):
    G, = C.cotangents(3, x.shape)
    C.check_ode_training(functools.partial(_solver, name), (de, t, x, z, ev, zj), G, "_FusedOde", TOL_GPU, tx, what=name)


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("xd,zd,H,nh", K5_ODE_SHAPES)
def test_ode_training(name, xd, zd, H, nh):
    hidden = H if isinstance(H, tuple) else (H,) * nh
    de, t, x, z, ev, zj = _ode_case(xd, zd, hidden, B0, T0, seed=5 + xd, events=zd > 0, pad=False)
    _check_ode(name, de, t, x, z, ev, zj)


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))])
def test_ode_teacher_forced_training(name, xd, zd, hidden):
    de, t, x, z, ev, zj = _ode_case(xd, zd, hidden, B0, T0, seed=9 + xd, pad=False)
    _check_ode(name, de, t, x, z, ev, zj, tx=True)


def _check_dae(name, case, tx=False, ti=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    C.check_dae_training(functools.partial(_solver, name), case, G, Gi, "_FusedDae", TOL_GPU, tx, ti, what=name)


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("shape", list(K5_DAE_SHAPES))
def test_dae_training(name, shape):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    _check_dae(name, _dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=21 + xd))


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("tx,ti", [(True, False), (False, True), (True, True)])
def test_dae_teacher_forced_training(name, tx, ti):
    _check_dae(name, _dae_case(5, 4, 6, 6, (64, 64, 64), (64, 64, 64), B0, T0, seed=23), tx, ti)


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_rk4classic_with_other_activations_ode(act):
    de, t, x, z, ev, zj = _ode_case(8, 2, (64, 64, 64), B0, T0, seed=31, pad=False, act=act)
    out, ref = _ode_fwd_pair("RK4Classic", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), ref) <= TOL_GPU
    _check_ode("RK4Classic", de, t, x, z, ev, zj)


def test_rk4classic_silu_de_tanh_ae_dae():
    _check_dae("RK4Classic", _dae_case(4, 2, 1, 2, (48, 48), (32, 32), B0, T0, seed=33, de_act=nn.SiLU, ae_act=nn.Tanh))


# ----------------------------------------------------------------------------- routing
def test_kernel_wave_raises_under_require_and_walks_under_auto():
    de, t, x, z, ev, zj = _ode_case(8, 2, (64, 64, 64), B0, T0, seed=41, pad=False)
    with pytest.raises(_lib.UnsupportedShapeError):
        _ode_fwd_pair("RK4Classic", de, t, x, z, ev, zj, mode="require", kernel="wave")
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out, ref = _ode_fwd_pair("RK4Classic", de, t, x, z, ev, zj, mode="auto", kernel="wave")
    assert traj_rel_err(out.cpu(), ref) <= TOL_GPU


def test_teacher_forced_tanh_training_is_not_fusable():
    de, t, x, z, ev, zj = _ode_case(8, 2, (64, 64, 64), B0, T0, seed=43, pad=False, act=nn.Tanh)
    G, = C.cotangents(3, x.shape)
    with pytest.raises(nd.NotFusableError):
        C.ode_train(functools.partial(_solver, "RK4Classic"), (de, t, x, z, ev, zj), G, "cuda", tx=True)
    assert not autograd.ode_training_supported(nd.RK4Classic().method, [(m.weight, m.bias) for m in de.x_dot if isinstance(m, nn.Linear)],
                                               8, 2, T0, B0, act=None, kernel="wave")


def test_direct_encode_model_takes_rows_and_k0():
    """ODE_Model(direct_encode=True) at hidden 16: no one-launch encoded form and no latent kernel carries a tableau -- row kernels + K0"""
    torch.manual_seed(51)
    g = torch.Generator().manual_seed(51)
    B, Tn, xd, zd = B0, T0, 8, 2
    m = models.ODE_Model(xd, zd, 16, direct_encode=True, solver=nd.RK4Classic())
    m64 = copy.deepcopy(m).double()
    m64.solver.fused = "off"
    t = (torch.arange(Tn, dtype=torch.float32) * 0.01).view(1, Tn, 1).repeat(B, 1, 1)
    x, z = 0.5 * torch.randn(B, Tn, xd, generator=g), 0.5 * torch.randn(B, Tn, zd, generator=g)
    event_t = t[:, [2, 5], :].contiguous()
    z_jump = 0.5 * torch.randn(B, 2, zd, generator=g)
    with torch.no_grad():
        ref = m64(t=t.double(), x=x.double(), z=z.double(), event_t=event_t.double(), z_jump=z_jump.double())
        mg = m.cuda()
        mg.solver.fused = "require"
        out = mg(t=t.cuda(), x=x.cuda(), z=z.cuda(), event_t=event_t.cuda(), z_jump=z_jump.cuda())
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    out = out if isinstance(out, (tuple, list)) else (out,)
    for o, r in zip(out, ref):
        assert traj_rel_err(o.cpu(), r, bdim=0) <= TOL_GPU
