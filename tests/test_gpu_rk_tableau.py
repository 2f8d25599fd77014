"""Explicit Runge-Kutta tableaus (Heun2, Ralston2, Kutta3, SSPRK3, RK4Classic; any ExplicitRK) on the generic kernels: K0 forward, K0 + K5
training.  References: the reference-captured goldens for the Euler / Midpoint / 3/8 tableaus; for the named methods the package's own
callback walk of the SAME modules in float64 on the CPU, gradients from torch autograd through that walk.  Tolerances: helpers.TOL_GPU on
traj_rel_err for trajectories, TOL_GPU of the tensor's max for gradients."""
import copy
import warnings

import pytest
import torch
import torch.nn as nn

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


def _close(a, b, what):
    if a is None and b is None:          # (a call without events has no jump gradient on either side)
        return
    if b is None:
        b = torch.zeros(a.shape, dtype=torch.float64)
    assert a is not None, what
    if b.numel() == 0:          # (z_dim 0: nothing to compare but the shape)
        assert tuple(a.shape) == tuple(b.shape), what
        return
    scale = float(b.abs().max())
    err = float((a.double().cpu() - b).abs().max())
    print(f"{what}: max abs err {err:.3e}, tensor max {scale:.3e}, ratio {err / max(scale, 1e-6):.3e}")
    assert err <= TOL_GPU * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _sd(d, prefix):
    return {k[len(prefix):].replace("__", "."): T(v) for k, v in d.items() if k.startswith(prefix)}


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
def _grid(Tn, B, g, pad=False, dt=0.01):
    """per-trajectory step sizes (ragged); pad: the last grid points of some trajectories are -1, as the datasets pad short curves.
    Trajectory 0 (whose clock decides the events) stays whole."""
    t = (torch.arange(Tn, dtype=torch.float32) * dt).view(Tn, 1, 1).repeat(1, B, 1)
    if B > 1:
        t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, B - 1, 1, generator=g))
    if pad and Tn > 3 and B > 2:
        t[-2:, 2::3] = -1.0
    return t


def _ode_case(xd, zd, hidden, B, Tn, seed, events=True, pad=True, act=nn.ELU):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    de = models.DE_Func(xd + zd, hidden, xd, activation=act)
    t = _grid(Tn, B, g, pad)
    x = 0.5 * torch.randn(Tn, B, xd, generator=g)
    z = 0.5 * torch.randn(Tn, B, zd, generator=g)
    ev = zj = None
    if events and Tn > 2:
        ev = t[[1, Tn // 2]].permute(1, 0, 2).contiguous()      # [B, 2, 1]
        zj = 0.5 * torch.randn(B, 2, zd, generator=g)
    return de, t, x, z, ev, zj


def _run_ode(solver, de, t, x, z, a0, ev, zj, tx=False):
    event = nd.ODE_Event()
    if ev is not None:
        event.set_event(ev, zj)
    return solver.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0, event_fn=event.event_fn if ev is not None else None,
                                jump_change_fn=event.jump_change_fn if ev is not None else None, input_true_x=tx)


def _ode_fwd_pair(name, de, t, x, z, ev, zj, tx=False, mode="require", kernel="auto"):
    d = lambda a: None if a is None else a.double()
    c = lambda a: None if a is None else a.cuda()
    with torch.no_grad():
        ref = _run_ode(_solver(name, "off"), copy.deepcopy(de).double(), d(t), d(x), d(z), torch.cat((d(x)[0], d(z)[0]), -1), d(ev), d(zj), tx)
        xc, zc = c(x), c(z)
        out = _run_ode(_solver(name, mode, kernel), copy.deepcopy(de).cuda(), c(t), xc, zc, torch.cat((xc[0], zc[0]), -1), c(ev), c(zj), tx)
    return out, ref


ODE_FWD_SHAPES = {"reg": (8, 2, (64, 64, 64)), "streamed": (20, 3, (96, 96)), "wide": (20, 3, (128, 128)), "deep": (8, 2, (32,) * 7)}


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


def _dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, events, de_act=nn.ELU, ae_act=nn.ELU):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd + vd + idim
    de = models.DAE_DE_Func(n, de_hidden, xd, activation=de_act)
    ae = models.AE_Func(n + xd + zd + vd, ae_hidden, idim, activation=ae_act)
    t = _grid(Tn, B, g)
    x, z, v, i = (0.5 * torch.randn(Tn, B, w, generator=g) for w in (xd, zd, vd, idim))
    x_init = x[0].clone()
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1)
    ev = zj = vj = None
    if events:
        ev = t[[1, Tn // 2]].permute(1, 0, 2).contiguous()
        zj = 0.5 * torch.randn(B, 2, zd, generator=g)
        vj = 0.5 * torch.randn(B, 2, vd, generator=g)
    return de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj


def _run_dae(solver, de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, tx=False, ti=False):
    event = nd.DAE_Event()
    if ev is not None:
        event.set_event(ev, zj, vj)
    return solver.integrate_DAE(x_init=x_init, x_func=de, i_func=ae, t=t, x=x, z=z, v=v, i=i, all_initial=a0,
                                event_fn=event.event_fn if ev is not None else None,
                                jump_change_fn=event.jump_change_fn if ev is not None else None, input_true_x=tx, input_true_i=ti)


DAE_SHAPES = {"x8z2v2i2": (8, 2, 2, 2, (64, 64, 64), (64, 64, 64)), "x5z4v6i6": (5, 4, 6, 6, (64, 64, 64), (64, 64, 64))}


@pytest.mark.parametrize("name", ["Kutta3", "RK4Classic"])
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(name, shape, mode):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    case = list(_dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=17 + xd, events=True))
    tx, ti = "tx1" in mode, "ti1" in mode
    if mode == "events_no_x":
        case[3] = case[3][:, :, :0]          # the dataset x is not read without teacher forcing: what the models pass then
    d = lambda a: None if a is None else a.double()
    c = lambda a: None if a is None else a.cuda()
    de, ae = case[0], case[1]
    with torch.no_grad():
        ref = _run_dae(_solver(name, "off"), copy.deepcopy(de).double(), copy.deepcopy(ae).double(), *(d(q) for q in case[2:]), tx, ti)
        out = _run_dae(_solver(name, "require"), copy.deepcopy(de).cuda(), copy.deepcopy(ae).cuda(), *(c(q) for q in case[2:]), tx, ti)
    ex, ei = traj_rel_err(out[0].cpu(), ref[0]), traj_rel_err(out[1].cpu(), ref[1])
    print(name, shape, mode, f"{ex:.3e} {ei:.3e}")
    assert ex <= TOL_GPU and ei <= TOL_GPU


# ----------------------------------------------------------------------------- training
def _ode_train(name, de, t, x, z, ev, zj, G, dev, tx=False, mode="require"):
    dtype = torch.float32 if dev == "cuda" else torch.float64
    cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
    m = copy.deepcopy(de).to(device=dev, dtype=dtype)
    xg = cv(x) if tx else cv(x).requires_grad_(True)           # (teacher forcing: the dataset rows get no gradient)
    zg = cv(z).requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = cv(zj).requires_grad_(True) if zj is not None else None
    xs = _run_ode(_solver(name, mode if dev == "cuda" else "off"), m, cv(t), xg, zg, a0, cv(ev), zjg, tx)
    (xs * cv(G)).sum().backward()
    grads = {"z": zg.grad, "a0": a0.grad, "zj": zjg.grad if zjg is not None else None}
    if not tx:
        grads["x"] = xg.grad
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def _check_ode_training(name, de, t, x, z, ev, zj, tx=False):
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    ref_xs, ref = _ode_train(name, de, t, x, z, ev, zj, G, "cpu", tx)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _ode_train(name, de, t, x, z, ev, zj, G, "cuda", tx)
        _, again = _ode_train(name, de, t, x, z, ev, zj, G, "cuda", tx)
    assert type(xs.grad_fn).__name__.startswith("_FusedOde"), xs.grad_fn
    assert traj_rel_err(xs.detach().cpu(), ref_xs.detach()) <= TOL_GPU
    for k in ref:
        _close(got[k], ref[k], f"{name} grad {k}")
        assert (got[k] is None and again[k] is None) or torch.equal(got[k], again[k]), f"backward not repeatable: {k}"


# the shape list of tests/test_gpu_backward.py::test_generic_backward_kernel_ode: K5's register path and its edges, the streamed path with
# LDS and (hidden 128) global accumulators, the staged path (132 input columns)
K5_ODE_SHAPES = [(8, 2, 64, 3), (16, 16, 16, 1), (5, 3, 24, 2), (8, 2, 128, 3), (8, 2, 32, 3), (20, 2, 64, 3), (32, 4, 48, 2), (17, 0, 33, 3),
                 (40, 2, 64, 1), (8, 2, (33, 17, 64), 3), (5, 3, (16, 64, 16), 3), (44, 0, 40, 2), (8, 2, 64, 4)]


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("xd,zd,H,nh", K5_ODE_SHAPES)
def test_ode_training(name, xd, zd, H, nh):
    hidden = H if isinstance(H, tuple) else (H,) * nh
    de, t, x, z, ev, zj = _ode_case(xd, zd, hidden, B0, T0, seed=5 + xd, events=zd > 0, pad=False)
    _check_ode_training(name, de, t, x, z, ev, zj)


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))])
def test_ode_teacher_forced_training(name, xd, zd, hidden):
    de, t, x, z, ev, zj = _ode_case(xd, zd, hidden, B0, T0, seed=9 + xd, pad=False)
    _check_ode_training(name, de, t, x, z, ev, zj, tx=True)


def _dae_train(name, case, G, Gi, dev, tx=False, ti=False):
    dtype = torch.float32 if dev == "cuda" else torch.float64
    cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    de, ae = copy.deepcopy(de).to(device=dev, dtype=dtype), copy.deepcopy(ae).to(device=dev, dtype=dtype)
    leaf = lambda a: cv(a).requires_grad_(True)
    xi, zg, vg, a0g, zjg, vjg = leaf(x_init), leaf(z), leaf(v), leaf(a0), leaf(zj), leaf(vj)
    xs, is_ = _run_dae(_solver(name, "require" if dev == "cuda" else "off"), de, ae, cv(t), cv(x), zg, vg, cv(i), xi, a0g, cv(ev), zjg, vjg, tx, ti)
    ((xs * cv(G)).sum() + (is_ * cv(Gi)).sum()).backward()
    grads = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad, "zj": zjg.grad, "vj": vjg.grad}
    grads.update({f"de{k}": p.grad for k, p in enumerate(de.parameters())})
    grads.update({f"ae{k}": p.grad for k, p in enumerate(ae.parameters())})
    return xs, is_, grads


def _check_dae_training(name, case, tx=False, ti=False):
    g = torch.Generator().manual_seed(4)
    G, Gi = torch.randn(case[3].shape, generator=g), torch.randn(case[6].shape, generator=g)
    rx, ri, ref = _dae_train(name, case, G, Gi, "cpu", tx, ti)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, is_, got = _dae_train(name, case, G, Gi, "cuda", tx, ti)
        _, _, again = _dae_train(name, case, G, Gi, "cuda", tx, ti)
    assert type(xs.grad_fn).__name__.startswith("_FusedDae"), xs.grad_fn
    assert traj_rel_err(xs.detach().cpu(), rx.detach()) <= TOL_GPU and traj_rel_err(is_.detach().cpu(), ri.detach()) <= TOL_GPU
    for k in ref:
        _close(got[k], ref[k], f"{name} grad {k}")
        assert (got[k] is None and again[k] is None) or torch.equal(got[k], again[k]), f"backward not repeatable: {k}"


# K5's DAE paths: register DE + streamed head, everything streamed (hidden 96; hidden 128: global accumulators), a five-layer staged MLP
K5_DAE_SHAPES = {"reg": (8, 2, 2, 2, (64, 64, 64), (64, 64, 64)), "zvi16": (5, 4, 6, 6, (64, 64, 64), (64, 64, 64)),
                 "streamed": (8, 2, 2, 2, (96, 96), (96, 96)), "h128": (8, 2, 2, 2, (128, 128, 128), (128, 128, 128)),
                 "deep": (4, 2, 1, 2, (32,) * 5, (24,) * 5)}


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("shape", list(K5_DAE_SHAPES))
def test_dae_training(name, shape):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    _check_dae_training(name, _dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=21 + xd, events=True))


@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic"])
@pytest.mark.parametrize("tx,ti", [(True, False), (False, True), (True, True)])
def test_dae_teacher_forced_training(name, tx, ti):
    _check_dae_training(name, _dae_case(5, 4, 6, 6, (64, 64, 64), (64, 64, 64), B0, T0, seed=23, events=True), tx, ti)


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_rk4classic_with_other_activations_ode(act):
    de, t, x, z, ev, zj = _ode_case(8, 2, (64, 64, 64), B0, T0, seed=31, pad=False, act=act)
    out, ref = _ode_fwd_pair("RK4Classic", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), ref) <= TOL_GPU
    _check_ode_training("RK4Classic", de, t, x, z, ev, zj)


def test_rk4classic_silu_de_tanh_ae_dae():
    _check_dae_training("RK4Classic", _dae_case(4, 2, 1, 2, (48, 48), (32, 32), B0, T0, seed=33, events=True, de_act=nn.SiLU, ae_act=nn.Tanh))


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
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    with pytest.raises(nd.NotFusableError):
        _ode_train("RK4Classic", de, t, x, z, ev, zj, G, "cuda", tx=True)
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
