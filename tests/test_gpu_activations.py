"""Fused forward and training for right-hand sides whose MLPs use activations other than ELU(1) (generic kernels K0 / K5).  References:
the package's own walk of the SAME modules in float64 on the CPU, gradients from torch autograd through that walk."""
import copy
import warnings

import pytest
import torch
import torch.nn as nn

from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import fused, models
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

TOL = 2e-4          # gradient gate of tests/test_gpu_backward.py (max abs error <= TOL x the tensor's max)

ACTS = {
    "elu05": lambda: nn.ELU(alpha=0.5),
    "tanh": nn.Tanh,
    "sigmoid": nn.Sigmoid,
    "relu": nn.ReLU,
    "leaky": lambda: nn.LeakyReLU(0.1),
    "softplus": lambda: nn.Softplus(beta=2.0, threshold=5.0),
    "elu1": nn.ELU,          # the DAE's other MLP only: ELU(1) next to another activation
}
NON_ELU1 = [k for k in ACTS if k != "elu1"]
SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4}


def _close(a, b, what):
    if b is None:
        b = torch.zeros(a.shape, dtype=torch.float64)
    scale = float(b.abs().max())
    err = float((a.double().cpu() - b).abs().max())
    assert err <= TOL * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _solver(method, fused_mode):
    s = SOLVERS[method]()
    s.fused = fused_mode
    return s


def _grid(Tn, B, g, dt=0.01):
    t = (torch.arange(Tn, dtype=torch.float32) * dt).view(Tn, 1, 1).repeat(1, B, 1)
    if B > 1:
        t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, B - 1, 1, generator=g))
    return t


def _ode_case(act, xd, zd, hidden, B, Tn, seed, events):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    de = models.DE_Func(xd + zd, hidden, xd, activation=ACTS[act])
    t = _grid(Tn, B, g)
    x = 0.5 * torch.randn(Tn, B, xd, generator=g)
    z = 0.5 * torch.randn(Tn, B, zd, generator=g)
    ev = zj = None
    if events:
        ev = t[[3, Tn // 2]].permute(1, 0, 2).contiguous()     # [B, 2, 1]: trajectory 0's clock decides
        zj = 0.5 * torch.randn(B, 2, zd, generator=g)
    return de, t, x, z, ev, zj


def _run_ode(solver, de, t, x, z, a0, ev, zj):
    event = nd.ODE_Event()
    if ev is not None:
        event.set_event(ev, zj)
    return solver.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0, event_fn=event.event_fn if ev is not None else None,
                                jump_change_fn=event.jump_change_fn if ev is not None else None)


def _ode_ref(method, de, t, x, z, ev, zj):
    d = lambda a: None if a is None else a.double()
    de64 = copy.deepcopy(de).double()
    with torch.no_grad():
        return _run_ode(_solver(method, "off"), de64, d(t), d(x), d(z), torch.cat((d(x)[0], d(z)[0]), -1), d(ev), d(zj))


def _ode_gpu(method, de, t, x, z, ev, zj, fused_mode="require"):
    c = lambda a: None if a is None else a.cuda()
    xc, zc = c(x), c(z)
    with torch.no_grad():
        return _run_ode(_solver(method, fused_mode), copy.deepcopy(de).cuda(), c(t), xc, zc, torch.cat((xc[0], zc[0]), -1), c(ev), c(zj))


def test_tanh_de_func_runs_fused_under_require():
    """Before this feature: NotFusableError (the MLP is not an ELU(1) one)."""
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), 37, 25, seed=1, events=True)
    out = _ode_gpu("rk4", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), _ode_ref("rk4", de, t, x, z, ev, zj)) <= TOL_GPU


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("act", NON_ELU1)
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))])
def test_ode_forward(method, act, xd, zd, hidden):
    de, t, x, z, ev, zj = _ode_case(act, xd, zd, hidden, 45, 30, seed=10 * NON_ELU1.index(act) + xd, events=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = _ode_gpu(method, de, t, x, z, ev, zj, fused_mode="auto")       # auto must not walk (a walk warns)
    assert torch.isfinite(out).all()
    assert traj_rel_err(out.cpu(), _ode_ref(method, de, t, x, z, ev, zj)) <= TOL_GPU


@pytest.mark.parametrize("act", ["tanh", "softplus"])
@pytest.mark.parametrize("hidden", [(160, 160, 160), (160, 160), (32,) * 6])
def test_ode_forward_staged_streamed_deep(act, hidden):
    """K0's other modes: weight images streamed from L2 / resident in LDS, and the eight-layer unrolled instances"""
    de, t, x, z, ev, zj = _ode_case(act, 8, 2, hidden, 40, 16, seed=len(hidden), events=True)
    out = _ode_gpu("rk4", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), _ode_ref("rk4", de, t, x, z, ev, zj)) <= TOL_GPU


def test_full_size_subset_vs_fp64_walk():
    """B = 4096, T = 1000, RK4, Tanh: trajectories are independent, so a few dozen of the full GPU run must match the fp64 walk on just
    those."""
    B, Tn = 4096, 1000
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), B, Tn, seed=7, events=False)
    out = _ode_gpu("rk4", de, t, x, z, None, None)
    torch.cuda.synchronize()
    idx = torch.tensor(sorted(set(range(0, B, 131)) | {B - 1, 15, 16, 17}))
    ref = _ode_ref("rk4", de, t[:, idx], x[:, idx], z[:, idx], None, None)
    assert torch.isfinite(out).all()
    assert traj_rel_err(out[:, idx.cuda()].cpu(), ref) <= TOL_GPU


# ----------------------------------------------------------------------------- DAE
def _dae_case(de_act, ae_act, xd, zd, vd, idim, B, Tn, seed, events, hidden=(48, 48)):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd + vd + idim
    de = models.DAE_DE_Func(n, hidden, xd, activation=ACTS[de_act])
    ae = models.AE_Func(n + xd + zd + vd, (32, 32), idim, activation=ACTS[ae_act])
    t = _grid(Tn, B, g)
    x = 0.5 * torch.randn(Tn, B, xd, generator=g)
    z = 0.5 * torch.randn(Tn, B, zd, generator=g)
    v = 0.5 * torch.randn(Tn, B, vd, generator=g)
    i = 0.5 * torch.randn(Tn, B, idim, generator=g)
    x_init = x[0].clone()
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1)
    ev = zj = vj = None
    if events:
        ev = t[[2, Tn // 2]].permute(1, 0, 2).contiguous()
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


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", [("tanh", "softplus"), ("relu", "sigmoid"), ("leaky", "elu05"), ("elu1", "sigmoid")])
@pytest.mark.parametrize("mode", ["events_no_x", "true_x", "true_i"])
def test_dae_forward(method, de_act, ae_act, mode):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = _dae_case(de_act, ae_act, 4, 2, 1, 2, 33, 20, seed=11, events=mode == "events_no_x")
    tx, ti = mode == "true_x", mode == "true_i"
    if mode == "events_no_x":
        x = x[:, :, :0]           # the dataset x is not read without teacher forcing: x_dim == 0 is what the models pass then
    d = lambda a: None if a is None else a.double()
    with torch.no_grad():
        ref = _run_dae(_solver(method, "off"), copy.deepcopy(de).double(), copy.deepcopy(ae).double(), d(t), d(x), d(z), d(v), d(i),
                       d(x_init), d(a0), d(ev), d(zj), d(vj), tx, ti)
        c = lambda a: None if a is None else a.cuda()
        out = _run_dae(_solver(method, "require"), copy.deepcopy(de).cuda(), copy.deepcopy(ae).cuda(), c(t), c(x), c(z), c(v), c(i),
                       c(x_init), c(a0), c(ev), c(zj), c(vj), tx, ti)
    assert traj_rel_err(out[0].cpu(), ref[0]) <= TOL_GPU
    assert traj_rel_err(out[1].cpu(), ref[1]) <= TOL_GPU


# ----------------------------------------------------------------------------- training
def _ode_train(method, de, t, x, z, ev, zj, G, dev, dtype):
    cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
    m = copy.deepcopy(de).to(device=dev, dtype=dtype)
    xg, zg = cv(x).requires_grad_(True), cv(z).requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)       # a leaf of its own: its gradient is checked separately
    zjg = cv(zj).requires_grad_(True) if zj is not None else None
    solver = _solver(method, "require" if dev == "cuda" else "off")
    xs = _run_ode(solver, m, cv(t), xg, zg, a0, cv(ev), zjg)
    (xs * cv(G)).sum().backward()
    grads = {"x": xg.grad, "z": zg.grad, "a0": a0.grad, "zj": zjg.grad if zjg is not None else None}
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("act", NON_ELU1)
def test_ode_training(method, act):
    de, t, x, z, ev, zj = _ode_case(act, 8, 2, (64, 64, 64), 37, 14, seed=5, events=True)
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    _, ref = _ode_train(method, de, t, x, z, ev, zj, G, "cpu", torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _ode_train(method, de, t, x, z, ev, zj, G, "cuda", torch.float32)
    assert type(xs.grad_fn).__name__.startswith("_FusedOde")
    for k, r in ref.items():
        _close(got[k], r, f"grad {k}")


@pytest.mark.parametrize("xd,zd,hidden", [(20, 3, (96, 96)), (8, 2, (160, 160, 160)), (8, 2, (32,) * 6)])
def test_ode_training_other_paths(xd, zd, hidden):
    """shapes outside every specialisation: K5's streamed / staged paths and deep MLPs"""
    de, t, x, z, ev, zj = _ode_case("softplus", xd, zd, hidden, 19, 9, seed=9, events=True)
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    _, ref = _ode_train("rk4", de, t, x, z, ev, zj, G, "cpu", torch.float64)
    _, got = _ode_train("rk4", de, t, x, z, ev, zj, G, "cuda", torch.float32)
    for k, r in ref.items():
        _close(got[k], r, f"grad {k}")


def test_ode_backward_is_deterministic():
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), 200, 12, seed=2, events=True)
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    _, g1 = _ode_train("rk4", de, t, x, z, ev, zj, G, "cuda", torch.float32)
    _, g2 = _ode_train("rk4", de, t, x, z, ev, zj, G, "cuda", torch.float32)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", [("tanh", "softplus"), ("relu", "leaky"), ("sigmoid", "elu05")])
def test_dae_training(method, de_act, ae_act):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = _dae_case(de_act, ae_act, 4, 2, 1, 2, 29, 12, seed=21, events=True)
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    H = torch.randn(i.shape, generator=torch.Generator().manual_seed(7))

    def run(dev, dtype):
        cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
        dm, am = copy.deepcopy(de).to(device=dev, dtype=dtype), copy.deepcopy(ae).to(device=dev, dtype=dtype)
        xi, zg, vg, a0g = (cv(q).requires_grad_(True) for q in (x_init, z, v, a0))
        zjg, vjg = cv(zj).requires_grad_(True), cv(vj).requires_grad_(True)
        xs, is_ = _run_dae(_solver(method, "require" if dev == "cuda" else "off"), dm, am, cv(t), cv(x)[:, :, :0], zg, vg, cv(i), xi, a0g,
                           cv(ev), zjg, vjg)
        ((xs * cv(G)).sum() + (is_ * cv(H)).sum()).backward()
        g = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad, "zj": zjg.grad, "vj": vjg.grad}
        g.update({f"de{k}": p.grad for k, p in enumerate(dm.parameters())})
        g.update({f"ae{k}": p.grad for k, p in enumerate(am.parameters())})
        return xs, g

    _, ref = run("cpu", torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = run("cuda", torch.float32)
    assert type(xs.grad_fn).__name__.startswith("_FusedDae")
    for k, r in ref.items():
        _close(got[k], r, f"grad {k}")


# ----------------------------------------------------------------------------- routing
def test_non_elu_with_an_mfma_kernel_walks_or_raises():
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), 16, 6, seed=3, events=False)
    s = _solver("rk4", "require")
    s.kernel = "wave"
    c = lambda a: a.cuda()
    m = copy.deepcopy(de).cuda()
    with pytest.raises(fused._lib.UnsupportedShapeError):
        with torch.no_grad():
            _run_ode(s, m, c(t), c(x), c(z), torch.cat((c(x)[0], c(z)[0]), -1), None, None)
    s = _solver("rk4", "auto")
    s.kernel = "wave"
    with pytest.warns(RuntimeWarning, match="not fusable"):
        with torch.no_grad():
            out = _run_ode(s, m, c(t), c(x), c(z), torch.cat((c(x)[0], c(z)[0]), -1), None, None)
    assert traj_rel_err(out.cpu(), _ode_ref("rk4", de, t, x, z, None, None)) <= TOL_GPU


def test_teacher_forced_training_with_non_elu_walks():
    de, t, x, z, ev, zj = _ode_case("relu", 8, 2, (64, 64, 64), 16, 6, seed=4, events=False)
    m = copy.deepcopy(de).cuda()
    s = _solver("euler", "require")
    with pytest.raises(nd.NotFusableError):
        s.integrate_ODE(x_func=m, t=t.cuda(), x=x.cuda(), z=z.cuda(), all_initial=torch.cat((x[0], z[0]), -1).cuda(), input_true_x=True)


def test_null_act_is_the_elu1_entry_point(monkeypatch):
    """psnode_ode_integrate_act_f32 with a NULL act: bitwise the output of psnode_ode_integrate_f32 at kernel = GENERIC."""
    from py_psnode_amd.fused import _common
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), 40, 20, seed=8, events=True)
    de = models.DE_Func(10, (64, 64, 64), 8).cuda()
    layers = [(m.weight.detach(), m.bias.detach()) for m in de.x_dot if isinstance(m, nn.Linear)]
    c = lambda a: a.cuda()
    a0 = torch.cat((x[0], z[0]), -1).cuda()
    ref = fused.ode_integrate("rk4", layers, c(t), c(x), c(z), a0, event_t=c(ev), z_jump=c(zj), kernel="generic")
    monkeypatch.setattr(_common, "_act_ptrs", lambda acts: [None])
    got = fused.ode_integrate("rk4", layers, c(t), c(x), c(z), a0, event_t=c(ev), z_jump=c(zj), kernel="generic", act=object())
    elu1 = fused.Act(fused._lib.ACT_ELU, alpha=1.0)
    monkeypatch.undo()
    got2 = fused.ode_integrate("rk4", layers, c(t), c(x), c(z), a0, event_t=c(ev), z_jump=c(zj), kernel="generic", act=elu1)
    assert torch.equal(ref, got) and torch.equal(ref, got2)
