"""Fused forward and training for right-hand sides whose MLPs use activations other than ELU(1) (generic kernels K0 / K5).  References:
the package's own walk of the SAME modules in float64 on the CPU, gradients from torch autograd through that walk."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn as nn

import generic_cases as C
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


def _solver(method, fused_mode):
    s = SOLVERS[method]()
    s.fused = fused_mode
    return s


def _ode_case(act, xd, zd, hidden, B, Tn, seed, events):
    """events at grid rows 3 and T // 2 of the ragged clock"""
    return C.ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=(3, Tn // 2) if events else (), act=ACTS[act])


def _dae_case(de_act, ae_act, xd, zd, vd, idim, B, Tn, seed, events, hidden=(48, 48)):
    return C.dae_case(xd, zd, vd, idim, hidden, (32, 32), B, Tn, seed, ev_rows=(2, Tn // 2) if events else (), de_act=ACTS[de_act],
                      ae_act=ACTS[ae_act])


def _ode_ref(method, de, t, x, z, ev, zj):
    return C.ode_walk64(_solver(method, "off"), de, t, x, z, ev, zj)


def _ode_gpu(method, de, t, x, z, ev, zj, fused_mode="require"):
    return C.ode_gpu(_solver(method, fused_mode), de, t, x, z, ev, zj)


def _train(method, case, G, dev):
    """-> xs, gradients by name; x is a leaf here (no teacher forcing in this file)"""
    return C.ode_train(functools.partial(_solver, method), case, G, dev)


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
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", [("tanh", "softplus"), ("relu", "sigmoid"), ("leaky", "elu05"), ("elu1", "sigmoid")])
@pytest.mark.parametrize("mode", ["events_no_x", "true_x", "true_i"])
def test_dae_forward(method, de_act, ae_act, mode):
    case = _dae_case(de_act, ae_act, 4, 2, 1, 2, 33, 20, seed=11, events=mode == "events_no_x")
    tx, ti = mode == "true_x", mode == "true_i"
    if mode == "events_no_x":
        case = C.without_x(case)
    out, ref = C.dae_forward_pair(_solver(method, "off"), _solver(method, "require"), case, tx, ti)
    assert traj_rel_err(out[0].cpu(), ref[0]) <= TOL_GPU
    assert traj_rel_err(out[1].cpu(), ref[1]) <= TOL_GPU


# ----------------------------------------------------------------------------- training
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("act", NON_ELU1)
def test_ode_training(method, act):
    case = _ode_case(act, 8, 2, (64, 64, 64), 37, 14, seed=5, events=True)
    G, = C.cotangents(3, case[2].shape)
    _, ref = _train(method, case, G, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _train(method, case, G, "cuda")
    C.judge_ode_training(ref, got, None, xs, None, "_FusedOde", TOL)          # (gradients and grad_fn: this file's gate)


@pytest.mark.parametrize("xd,zd,hidden", [(20, 3, (96, 96)), (8, 2, (160, 160, 160)), (8, 2, (32,) * 6)])
def test_ode_training_other_paths(xd, zd, hidden):
    """shapes outside every specialisation: K5's streamed / staged paths and deep MLPs"""
    case = _ode_case("softplus", xd, zd, hidden, 19, 9, seed=9, events=True)
    G, = C.cotangents(4, case[2].shape)
    _, ref = _train("rk4", case, G, "cpu")
    xs, got = _train("rk4", case, G, "cuda")
    C.judge_ode_training(ref, got, None, xs, None, None, TOL)


def test_ode_backward_is_deterministic():
    case = _ode_case("tanh", 8, 2, (64, 64, 64), 200, 12, seed=2, events=True)
    G, = C.cotangents(5, case[2].shape)
    _, g1 = _train("rk4", case, G, "cuda")
    _, g2 = _train("rk4", case, G, "cuda")
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", [("tanh", "softplus"), ("relu", "leaky"), ("sigmoid", "elu05")])
def test_dae_training(method, de_act, ae_act):
    case = _dae_case(de_act, ae_act, 4, 2, 1, 2, 29, 12, seed=21, events=True)
    G, H = C.cotangents(6, case[3].shape)[0], C.cotangents(7, case[6].shape)[0]
    run = lambda dev: C.dae_train(functools.partial(_solver, method), case, G, H, dev, no_x=True)
    _, _, ref = run("cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, is_, got = run("cuda")
    C.judge_dae_training(ref, got, None, (xs, is_), None, "_FusedDae", TOL)


# ----------------------------------------------------------------------------- routing
def test_non_elu_with_an_mfma_kernel_walks_or_raises():
    de, t, x, z, ev, zj = _ode_case("tanh", 8, 2, (64, 64, 64), 16, 6, seed=3, events=False)
    s = _solver("rk4", "require")
    s.kernel = "wave"
    c = lambda a: a.cuda()
    m = copy.deepcopy(de).cuda()
    with pytest.raises(fused._lib.UnsupportedShapeError):
        with torch.no_grad():
            C.run_ode(s, m, c(t), c(x), c(z), torch.cat((c(x)[0], c(z)[0]), -1), None, None)
    s = _solver("rk4", "auto")
    s.kernel = "wave"
    with pytest.warns(RuntimeWarning, match="not fusable"):
        with torch.no_grad():
            out = C.run_ode(s, m, c(t), c(x), c(z), torch.cat((c(x)[0], c(z)[0]), -1), None, None)
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
