"""Sub-steps per grid interval (solver.substeps) on the generic kernels: K0 forward, K0 + K5 training, ODE and DAE.

Yardsticks.  Where the n-times refined problem (tests/generic_cases.py) expresses the case -- no teacher forcing, a whole clock, one of the
reference's three formulas -- the fp32 CPU oracle on that problem, read at rows ::n, under helpers.TOL_GPU on traj_rel_err.  Otherwise
(teacher forcing, a -1-padded ragged clock, Kutta3, other activations) the package's callback walk of the same modules with the same
substeps in float64 on the CPU -- the definition of the semantics, pinned to the oracle by tests/test_substeps_host.py -- under the same
gate.  Gradients: torch autograd through that float64 walk, each tensor within TOL_GPU of its own max (the gate `close` of
tests/generic_cases.py).  B = 33: three tiles of 16 trajectories, the last with one; T = 6; events at steps 0 and 3."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import generic_cases as C
from generic_cases import DAE_SHAPES, K5_DAE_SHAPES, ODE_FWD_SHAPES
from helpers import TOL_GPU, traj_rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib, fused, models
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

SOLVERS = {"euler": nd.Euler, "rk4": nd.RK4, "Kutta3": nd.Kutta3}
B0, T0 = 33, 6
EV = (0, 3)          # the grid rows that carry the events
_c = C.to_cuda
_close = functools.partial(C.close, tol=TOL_GPU)


def _solver(name, n, mode="require", kernel="auto"):
    s = SOLVERS[name](substeps=n)
    s.fused, s.kernel = mode, kernel
    return s


def _ode_reference(name, n, de, t, x, z, ev, zj, tx=False, oracle=True):
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        if oracle and name != "Kutta3" and not tx:
            tf = C.refine_clock(t, n)
            xf = torch.zeros(tf.shape[0], x.shape[1], x.shape[2])
            xf[0] = x[0]
            return O.integrate_ode(name, C.layers_of(de.x_dot), tf, xf, C.refine_rows(z, n, t, ev, zj), a0, ev, zj)[::n]
    return C.ode_walk64(_solver(name, n, "off"), de, t, x, z, ev, zj, tx)


def _ode_gpu(name, n, de, t, x, z, ev, zj, tx=False, mode="require", kernel="auto"):
    return C.ode_gpu(_solver(name, n, mode, kernel), de, t, x, z, ev, zj, tx)


# ----------------------------------------------------------------------------- ODE forward
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("shape", list(ODE_FWD_SHAPES))
def test_ode_forward(shape, name, n):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances -- with events at steps 0 and 3"""
    xd, zd, hidden = ODE_FWD_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n)
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=3 + xd + len(hidden) + n, t=t, ev_rows=EV)
    out = _ode_gpu(name, n, de, t, x, z, ev, zj)          # fused = "require"
    e = traj_rel_err(out.cpu(), _ode_reference(name, n, de, t, x, z, ev, zj))
    print(shape, name, n, f"{e:.3e}")
    assert out.shape == x.shape and torch.isfinite(out).all() and e <= TOL_GPU


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("case", ["truex", "ragged", "ragged_truex"])
def test_ode_forward_teacher_forced_and_ragged(case, name, n):
    xd, zd, hidden = ODE_FWD_SHAPES["streamed" if n == 3 else "reg"]
    t = C.dyadic_clock(T0, B0, n) * 0.7          # (no longer dyadic: h is a rounded quotient)
    if "ragged" in case:
        t = C.padded(t)
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=40 + n, t=t, ev_rows=EV)
    tx = "truex" in case
    out = _ode_gpu(name, n, de, t, x, z, ev, zj, tx)
    ref = _ode_reference(name, n, de, t, x, z, ev, zj, tx, oracle=False)
    _close(out, ref, f"{case} {name} n={n}")


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("B,Tn", [(B0, 1), (B0, 2), (16, T0), (1, T0)])
def test_ode_forward_short_grids_and_batch_edges(B, Tn, n):
    t = C.dyadic_clock(Tn, B, n)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B, Tn, seed=B + Tn, t=t, ev_rows=EV)
    out = _ode_gpu("rk4", n, de, t, x, z, ev, zj, kernel="generic")
    ref = _ode_reference("rk4", n, de, t, x, z, ev, zj)
    assert out.shape == ref.shape and traj_rel_err(out.cpu(), ref) <= TOL_GPU


# ----------------------------------------------------------------------------- DAE forward
def _dae_reference(name, n, case, tx, ti, oracle):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    with torch.no_grad():
        if oracle and name != "Kutta3" and not (tx or ti):
            tf = C.refine_clock(t, n)
            xf, i_f = torch.zeros(tf.shape[0], x.shape[1], x.shape[2]), torch.zeros(tf.shape[0], i.shape[1], i.shape[2])
            rx, ri = O.integrate_dae(name, C.layers_of(de.x_dot), C.layers_of(ae.i_calculator), x_init, tf, xf, C.refine_rows(z, n, t, ev, zj),
                                     C.refine_rows(v, n, t, ev, vj), i_f, a0, ev, zj, vj)
            return rx[::n], ri[::n]
    return C.dae_walk64(_solver(name, n, "off"), case, tx, ti)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", ["rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(mode, shape, name, n):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n)
    case = C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=17 + xd + n, t=t, ev_rows=EV)
    tx, ti = "tx1" in mode, "ti1" in mode
    if mode == "events_no_x":
        case = C.without_x(case)
    out = C.dae_gpu(_solver(name, n), case, tx, ti)
    ref = _dae_reference(name, n, case, tx, ti, oracle=True)
    ex, ei = traj_rel_err(out[0].cpu(), ref[0]), traj_rel_err(out[1].cpu(), ref[1])
    print(mode, shape, name, n, f"{ex:.3e} {ei:.3e}")
    assert out[0].shape == (T0, B0, xd) and out[1].shape == (T0, B0, idim) and ex <= TOL_GPU and ei <= TOL_GPU


# ----------------------------------------------------------------------------- x_sub
@pytest.mark.parametrize("n", [2, 3, 4])
def test_x_sub_rows_are_the_refined_runs_intermediate_rows_ode(n):
    xd, zd, hidden = 8, 2, (64, 64, 64)
    t = C.dyadic_clock(T0, B0, n)
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=60 + n, t=t, ev_rows=EV)
    a0 = torch.cat((x[0], z[0]), -1)
    tf = C.refine_clock(t, n)
    xf = torch.zeros(tf.shape[0], B0, xd)
    xf[0] = x[0]
    fine = O.integrate_ode("rk4", C.layers_of(de.x_dot), tf, xf, C.refine_rows(z, n, t, ev, zj), a0, ev, zj)
    layers = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    args = ("rk4", layers, _c(t), _c(x[:1]), _c(z), _c(a0))
    kw = dict(event_t=_c(ev), z_jump=_c(zj), substeps=n)
    xs, x_sub = fused.ode_integrate(*args, save_sub=True, **kw)
    plain = fused.ode_integrate(*args, **kw)
    assert torch.equal(xs, plain)                                      # with x_sub = NULL the outputs are bitwise the same
    assert x_sub.shape == (T0 - 1, n - 1, B0, xd) and torch.isfinite(x_sub).all()
    want = fine[:-1].view(T0 - 1, n, B0, xd)[:, 1:]                    # rows kn + j, 1 <= j < n
    e = traj_rel_err(x_sub.cpu().reshape(-1, B0, xd), want.reshape(-1, B0, xd))
    print(n, f"{e:.3e}")
    assert e <= TOL_GPU and traj_rel_err(xs.cpu(), fine[::n]) <= TOL_GPU


@pytest.mark.parametrize("n", [2, 3])
def test_x_sub_rows_are_the_refined_runs_intermediate_rows_dae(n):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["x5z4v6i6"]
    t = C.dyadic_clock(T0, B0, n)
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=70 + n, t=t, ev_rows=EV)
    tf = C.refine_clock(t, n)
    xf, i_f = torch.zeros(tf.shape[0], B0, xd), torch.zeros(tf.shape[0], B0, idim)
    fine, _ = O.integrate_dae("rk4", C.layers_of(de.x_dot), C.layers_of(ae.i_calculator), x_init, tf, xf, C.refine_rows(z, n, t, ev, zj),
                              C.refine_rows(v, n, t, ev, vj), i_f, a0, ev, zj, vj)
    dl = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    al = [(w.cuda(), b.cuda()) for w, b in C.layers_of(ae.i_calculator)]
    args = ("rk4", dl, al, _c(x_init), _c(t), _c(x), _c(z), _c(v), _c(i), _c(a0))
    kw = dict(event_t=_c(ev), z_jump=_c(zj), v_jump=_c(vj), substeps=n)
    xs, is_, x_sub = fused.dae_integrate(*args, save_sub=True, **kw)
    xs2, is2 = fused.dae_integrate(*args, **kw)
    assert torch.equal(xs, xs2) and torch.equal(is_, is2)
    want = fine[:-1].view(T0 - 1, n, B0, xd)[:, 1:]
    assert x_sub.shape == want.shape and traj_rel_err(x_sub.cpu().reshape(-1, B0, xd), want.reshape(-1, B0, xd)) <= TOL_GPU


# ----------------------------------------------------------------------------- training
# the file's gate: cotangent G from seed 3 unless given, the fused function ran, helpers.TOL_GPU of each tensor's max
def _check_ode(name, n, de, t, x, z, ev, zj, tx=False, G=None):
    G = C.cotangents(3, x.shape)[0] if G is None else G
    return C.check_ode_training(functools.partial(_solver, name, n), (de, t, x, z, ev, zj), G, "_FusedOdeSub", TOL_GPU, tx, what=f"{name} n={n}")


# K5's paths (tests/generic_cases.py, K5_ODE_SHAPES): the register path and one of its edges, the streamed path with LDS (hidden 96)
# and with global (hidden 128) accumulators, the staged path (132 input columns)
SUB_K5_ODE_SHAPES = [(8, 2, 64, 3), (5, 3, 24, 2), (8, 2, 96, 2), (8, 2, 128, 3), (44, 0, 40, 2)]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("xd,zd,H,nh", SUB_K5_ODE_SHAPES)
def test_ode_training(xd, zd, H, nh, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, (H,) * nh, B0, T0, seed=5 + xd + n, t=t, ev_rows=EV)          # (z_dim 0: no events)
    _check_ode(name, n, de, t, x, z, ev, zj)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
def test_ode_training_without_events(name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=7 + n, t=t, ev_rows=())
    _check_ode(name, n, de, t, x, z, ev, zj)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))])
def test_ode_teacher_forced_training(xd, zd, hidden, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=9 + xd + n, t=t, ev_rows=EV)
    _check_ode(name, n, de, t, x, z, ev, zj, tx=True)


def _check_dae(name, n, case, tx=False, ti=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    C.check_dae_training(functools.partial(_solver, name, n), case, G, Gi, "_FusedDaeSub", TOL_GPU, tx, ti, what=f"{name} n={n}")


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("shape", list(K5_DAE_SHAPES))
def test_dae_training(shape, name, n):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n) * 0.7
    _check_dae(name, n, C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=21 + xd + n, t=t, ev_rows=EV))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
def test_dae_training_without_events(name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    _check_dae(name, n, C.dae_case(8, 2, 2, 2, (64, 64, 64), (64, 64, 64), B0, T0, seed=25 + n, t=t, ev_rows=()))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("tx,ti", [(True, False), (False, True), (True, True)])
def test_dae_teacher_forced_training(tx, ti, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    _check_dae(name, n, C.dae_case(5, 4, 6, 6, (64, 64, 64), (64, 64, 64), B0, T0, seed=23 + n, t=t, ev_rows=EV), tx, ti)


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_other_activations_ode(act):
    t = C.dyadic_clock(T0, B0, 3) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=31, t=t, act=act, ev_rows=EV)
    out = _ode_gpu("rk4", 3, de, t, x, z, ev, zj)
    assert traj_rel_err(out.cpu(), _ode_reference("rk4", 3, de, t, x, z, ev, zj, oracle=False)) <= TOL_GPU
    _check_ode("rk4", 3, de, t, x, z, ev, zj)


def test_silu_de_tanh_ae_dae():
    t = C.dyadic_clock(T0, B0, 2) * 0.7
    _check_dae("Kutta3", 2, C.dae_case(4, 2, 1, 2, (48, 48), (32, 32), B0, T0, seed=33, t=t, de_act=nn.SiLU, ae_act=nn.Tanh, ev_rows=EV))


def test_teacher_forced_tanh_training_is_not_fusable():
    t = C.dyadic_clock(T0, B0, 2)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=43, t=t, act=nn.Tanh, ev_rows=EV)
    G, = C.cotangents(3, x.shape)
    with pytest.raises(nd.NotFusableError):
        C.ode_train(functools.partial(_solver, "rk4", 2), (de, t, x, z, ev, zj), G, "cuda", tx=True)


# ----------------------------------------------------------------------------- routing
def test_kernel_wave_raises_under_require_and_walks_under_auto():
    t = C.dyadic_clock(T0, B0, 2)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=41, t=t, ev_rows=EV)
    with pytest.raises(_lib.UnsupportedShapeError):
        _ode_gpu("rk4", 2, de, t, x, z, ev, zj, mode="require", kernel="wave")
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out = _ode_gpu("rk4", 2, de, t, x, z, ev, zj, mode="auto", kernel="wave")
    assert traj_rel_err(out.cpu(), _ode_reference("rk4", 2, de, t, x, z, ev, zj)) <= TOL_GPU


def test_direct_encode_model_takes_rows_and_k0():
    """ODE_Model(direct_encode=True) at hidden 16: neither the one-launch encoded form nor a latent kernel carries sub-steps -- row kernels + K0"""
    torch.manual_seed(51)
    g = torch.Generator().manual_seed(51)
    B, Tn, xd, zd = B0, T0, 8, 2
    m = models.ODE_Model(xd, zd, 16, direct_encode=True, solver=nd.RK4(substeps=2))
    m64 = copy.deepcopy(m).double()
    m64.solver.fused = "off"
    t = (torch.arange(Tn, dtype=torch.float32) * 0.01).view(1, Tn, 1).repeat(B, 1, 1)
    x, z = 0.5 * torch.randn(B, Tn, xd, generator=g), 0.5 * torch.randn(B, Tn, zd, generator=g)
    event_t = t[:, [0, 3], :].contiguous()
    z_jump = 0.5 * torch.randn(B, 2, zd, generator=g)
    with torch.no_grad():
        ref = m64(t=t.double(), x=x.double(), z=z.double(), event_t=event_t.double(), z_jump=z_jump.double())
        mg = m.cuda()
        mg.solver.fused = "require"
        out = mg(t=t.cuda(), x=x.cuda(), z=z.cuda(), event_t=event_t.cuda(), z_jump=z_jump.cuda())
        m1 = copy.deepcopy(mg)
        m1.solver = nd.RK4()
        m1.solver.fused = "require"
        one = m1(t=t.cuda(), x=x.cuda(), z=z.cuda(), event_t=event_t.cuda(), z_jump=z_jump.cuda())
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    out = out if isinstance(out, (tuple, list)) else (out,)
    one = one if isinstance(one, (tuple, list)) else (one,)
    for o, r in zip(out, ref):
        assert traj_rel_err(o.cpu(), r, bdim=0) <= TOL_GPU
    assert not torch.equal(out[0], one[0])          # (two sub-steps are not one step)


# ----------------------------------------------------------------------------- substeps = 1
def test_substeps_one_is_bitwise_the_route_without_substeps():
    """through the solver, and through the fused entries with substeps=1 spelled out: the same kernels, the same bits"""
    t = C.dyadic_clock(T0, B0, 1) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=81, t=t, ev_rows=EV)
    for name in ("rk4", "Kutta3"):
        a = _ode_gpu(name, 1, de, t, x, z, ev, zj)
        s = SOLVERS[name]()
        s.fused = "require"
        b = C.ode_gpu(s, de, t, x, z, ev, zj)
        assert torch.equal(a, b)
    layers = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    args = ("rk4", layers, _c(t), _c(x[:1]), _c(z), _c(torch.cat((x[0], z[0]), -1)))
    kw = dict(event_t=_c(ev), z_jump=_c(zj), kernel="generic")
    xs, x_sub = fused.ode_integrate(*args, substeps=1, save_sub=True, **kw)
    assert x_sub is None and torch.equal(xs, fused.ode_integrate(*args, **kw))
    case = C.dae_case(8, 2, 2, 2, (64, 64, 64), (64, 64, 64), B0, T0, seed=83, t=t, ev_rows=EV)
    for name in ("rk4", "Kutta3"):
        outs = []
        for s in (_solver(name, 1), SOLVERS[name]()):
            s.fused = "require"
            outs.append(C.dae_gpu(s, case))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
