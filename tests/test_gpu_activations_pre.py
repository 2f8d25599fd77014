"""Fused forward and training for right-hand sides whose MLPs use SiLU, GELU (erf / tanh form) or Mish: the pre-activation builds of K0 / K5.
References: the package's own walk of the SAME modules in float64 on the CPU, gradients from torch autograd through that walk."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn as nn

import generic_cases as C
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import fused
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

TOL = 2e-4          # gradient gate of tests/test_gpu_backward.py (max abs error <= TOL x the tensor's max)

ACTS = {
    "silu": nn.SiLU,
    "gelu": nn.GELU,
    "gelu_tanh": lambda: nn.GELU(approximate="tanh"),
    "mish": nn.Mish,
    "tanh": nn.Tanh,         # the DAE's other MLP: the output-derivative family next to the pre-activation one
    "elu1": nn.ELU,
}
PRE = ["silu", "gelu", "gelu_tanh", "mish"]
SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4}


def _solver(method, fused_mode):
    s = SOLVERS[method]()
    s.fused = fused_mode
    return s


_close = functools.partial(C.close, tol=TOL)


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


def test_silu_de_func_runs_fused_under_require():
    """Before this feature: NotFusableError (SiLU is no activation the fused kernels applied)."""
    de, t, x, z, ev, zj = _ode_case("silu", 8, 2, (64, 64, 64), 37, 25, seed=1, events=True)
    out = _ode_gpu("rk4", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), _ode_ref("rk4", de, t, x, z, ev, zj)) <= TOL_GPU


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("act", PRE)
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))])
def test_ode_forward(method, act, xd, zd, hidden):
    de, t, x, z, ev, zj = _ode_case(act, xd, zd, hidden, 45, 30, seed=10 * PRE.index(act) + xd, events=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = _ode_gpu(method, de, t, x, z, ev, zj, fused_mode="auto")       # auto must not walk (a walk warns)
    assert torch.isfinite(out).all()
    assert traj_rel_err(out.cpu(), _ode_ref(method, de, t, x, z, ev, zj)) <= TOL_GPU


@pytest.mark.parametrize("act", PRE)
@pytest.mark.parametrize("hidden", [(160, 160, 160), (160, 160), (32,) * 6])
def test_ode_forward_staged_streamed_deep(act, hidden):
    """K0's other modes: weight images streamed from L2 / resident in LDS, and the eight-layer unrolled instances"""
    de, t, x, z, ev, zj = _ode_case(act, 8, 2, hidden, 40, 16, seed=len(hidden), events=True)
    out = _ode_gpu("rk4", de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), _ode_ref("rk4", de, t, x, z, ev, zj)) <= TOL_GPU


def test_full_size_subset_vs_fp64_walk():
    """B = 4096, T = 1000, RK4, SiLU on the ODE_01 shape: trajectories are independent, so a few dozen of the full GPU run must match the
    fp64 walk on just those."""
    B, Tn = 4096, 1000
    de, t, x, z, ev, zj = _ode_case("silu", 8, 2, (64, 64, 64), B, Tn, seed=7, events=False)
    out = _ode_gpu("rk4", de, t, x, z, None, None)
    torch.cuda.synchronize()
    idx = torch.tensor(sorted(set(range(0, B, 131)) | {B - 1, 15, 16, 17}))
    ref = _ode_ref("rk4", de, t[:, idx], x[:, idx], z[:, idx], None, None)
    assert torch.isfinite(out).all()
    assert traj_rel_err(out[:, idx.cuda()].cpu(), ref) <= TOL_GPU


# ----------------------------------------------------------------------------- DAE
MIXED = [("silu", "tanh"), ("gelu", "mish"), ("elu1", "gelu_tanh")]


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", MIXED)
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
@pytest.mark.parametrize("act", PRE)
def test_ode_training(method, act):
    case = _ode_case(act, 8, 2, (64, 64, 64), 37, 14, seed=5, events=True)
    G, = C.cotangents(3, case[2].shape)
    _, ref = _train(method, case, G, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _train(method, case, G, "cuda")
    C.judge_ode_training(ref, got, None, xs, None, "_FusedOde", TOL)          # (gradients and grad_fn: this file's gate)


# which K5 path each shape takes (psnode_generic_bwd_impl.h, gbwd_mode, with the pre build's u rows counted):
K5_PATHS = {
    "register, LDS accumulators": (8, 2, (64, 64, 64)),
    "streamed, global accumulators": (20, 3, (96, 96)),
    "streamed deep, LDS accumulators": (8, 2, (32,) * 6),
    "streamed, hidden 160 x 3, global accumulators": (8, 2, (160, 160, 160)),
    "staged (weights through LDS, u as [unit][TP] rows), global accumulators": (8, 2, (256, 256)),
}


@pytest.mark.parametrize("path", list(K5_PATHS))
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_ode_training_each_k5_path(path, act):
    xd, zd, hidden = K5_PATHS[path]
    case = _ode_case(act, xd, zd, hidden, 19, 9, seed=9, events=True)
    G, = C.cotangents(4, case[2].shape)
    _, ref = _train("rk4", case, G, "cpu")
    xs, got = _train("rk4", case, G, "cuda")
    C.judge_ode_training(ref, got, None, xs, None, None, TOL)


@pytest.mark.parametrize("act", PRE)
def test_wide_range_inputs(act):
    """|u| up to ~30 through a scaled first layer, and a few rows at +-1e4 (where every exponential of the forms overflows): finite outputs
    and gradients that match the fp64 walk."""
    de, t, x, z, ev, zj = _ode_case(act, 8, 2, (64, 64, 64), 24, 8, seed=13, events=False)
    with torch.no_grad():
        de.x_dot[0].weight.mul_(12.0)
    x[:, 5:8] = 1e4
    x[:, 9:11] = -1e4
    z[:, 12] = 1e4
    out = _ode_gpu("euler", de, t, x, z, None, None)
    assert torch.isfinite(out).all()
    assert traj_rel_err(out.cpu(), _ode_ref("euler", de, t, x, z, None, None)) <= TOL_GPU
    G, = C.cotangents(8, x.shape)
    _, ref = _train("euler", (de, t, x, z, None, None), G, "cpu")
    _, got = _train("euler", (de, t, x, z, None, None), G, "cuda")
    for k, r in ref.items():
        if r is None:
            continue
        assert torch.isfinite(got[k]).all(), k
        _close(got[k], r, f"grad {k}")


def test_ode_backward_is_deterministic():
    case = _ode_case("silu", 8, 2, (64, 64, 64), 200, 12, seed=2, events=True)
    G, = C.cotangents(5, case[2].shape)
    _, g1 = _train("rk4", case, G, "cuda")
    _, g2 = _train("rk4", case, G, "cuda")
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("de_act,ae_act", MIXED)
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
def test_silu_with_an_mfma_kernel_walks_or_raises():
    de, t, x, z, ev, zj = _ode_case("silu", 8, 2, (64, 64, 64), 16, 6, seed=3, events=False)
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


def test_teacher_forced_silu_training_raises_under_require():
    de, t, x, z, ev, zj = _ode_case("silu", 8, 2, (64, 64, 64), 16, 6, seed=4, events=False)
    m = copy.deepcopy(de).cuda()
    s = _solver("euler", "require")
    with pytest.raises(nd.NotFusableError):
        s.integrate_ODE(x_func=m, t=t.cuda(), x=x.cuda(), z=z.cuda(), all_initial=torch.cat((x[0], z[0]), -1).cuda(), input_true_x=True)
