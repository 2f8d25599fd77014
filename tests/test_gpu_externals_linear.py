"""Linearly interpolated external inputs (solver.externals = "linear") on the generic kernels: K0 forward, K0 + K5 training, ODE and DAE.

Yardsticks.  Euler without teacher forcing on a whole clock: the fp32 CPU oracle on the linearly refined problem
(tests/externals_linear_cases.py), read at rows ::n, under helpers.TOL_GPU on traj_rel_err.  Every other case: the package's callback walk of
the same modules in float64 on the CPU -- the definition of the semantics, pinned to the oracle and to a stand-alone restatement by
tests/test_externals_linear_host.py -- under the same gate.  Gradients: torch autograd through that float64 walk, each tensor within
TOL_GPU of its own max (`close` of tests/generic_cases.py).  B = 33: three tiles of 16 trajectories, the last with one; T = 6;
events at steps 0 and 3.

An ODE output must also differ from the "hold" run on the same inputs by more than 100 x TOL_GPU, so that a kernel that silently holds cannot
pass.  The one exception is Euler with one sub-step: its only stage has theta = 0, the left rows themselves, so "linear" IS "hold" there by
definition and the test asserts that instead (within TOL_GPU)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import externals_linear_cases as L
import generic_cases as C
from generic_cases import DAE_SHAPES, K5_DAE_SHAPES, ODE_FWD_SHAPES
from helpers import TOL_GPU, traj_rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib, fused, models
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

SOLVERS = {"euler": nd.Euler, "rk4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
B0, T0 = 33, 6
EV = (0, 3)          # the grid rows that carry the events
_c = C.to_cuda
_close = functools.partial(C.close, tol=TOL_GPU)


def _solver(name, n, mode="require", kernel="auto", externals="linear"):
    s = SOLVERS[name](substeps=n, externals=externals)
    s.fused, s.kernel = mode, kernel
    return s


def _ode_reference(name, n, de, t, x, z, ev, zj, tx=False, oracle=True):
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        if oracle and name == "euler" and not tx:
            tf = C.refine_clock(t, n)
            xf = torch.zeros(tf.shape[0], x.shape[1], x.shape[2])
            xf[0] = x[0]
            return O.integrate_ode(name, C.layers_of(de.x_dot), tf, xf, L.refine_rows_linear(z, n, t, ev, zj), a0, ev, zj)[::n]
    return C.ode_walk64(_solver(name, n, "off"), de, t, x, z, ev, zj, tx)


def _ode_gpu(name, n, de, t, x, z, ev, zj, tx=False, mode="require", kernel="auto", externals="linear"):
    return C.ode_gpu(_solver(name, n, mode, kernel, externals), de, t, x, z, ev, zj, tx)


# ----------------------------------------------------------------------------- ODE forward
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(ODE_FWD_SHAPES))
def test_ode_forward(shape, name, n):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances -- with events at steps 0 and 3.  Four times the
    builders' clock (still dyadic) and externals: the eight-layer MLP of 32 units is so insensitive to z that at the builders' scale Euler
    with two sub-steps differs from the hold by 4e-4 only, below what the second gate asks of a kernel that does interpolate."""
    xd, zd, hidden = ODE_FWD_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n) * 4.0
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=3 + xd + len(hidden) + n, t=t, ev_rows=EV)
    z, zj = 4.0 * z, 4.0 * zj
    out = _ode_gpu(name, n, de, t, x, z, ev, zj)          # fused = "require"
    hold = _ode_gpu(name, n, de, t, x, z, ev, zj, externals="hold")
    e = traj_rel_err(out.cpu(), _ode_reference(name, n, de, t, x, z, ev, zj))
    dh = traj_rel_err(out.cpu(), hold.cpu())
    print(shape, name, n, f"{e:.3e}", f"against hold {dh:.3e}")
    assert out.shape == x.shape and torch.isfinite(out).all() and e <= TOL_GPU
    if name == "euler" and n == 1:
        assert dh <= TOL_GPU          # (one stage at theta = 0: the hold, by definition)
    else:
        assert dh > 100 * TOL_GPU


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("case", ["truex", "ragged", "ragged_truex"])
def test_ode_forward_teacher_forced_and_ragged(case, name, n):
    xd, zd, hidden = ODE_FWD_SHAPES["streamed" if n == 3 else "reg"]
    t = C.dyadic_clock(T0, B0, n) * 0.7          # (no longer dyadic: h is a rounded quotient)
    if "ragged" in case:
        t = C.padded(t)                           # (theta does not depend on the clock: h = 0 or h < 0 needs no special case)
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=40 + n, t=t, ev_rows=EV)
    tx = "truex" in case
    out = _ode_gpu(name, n, de, t, x, z, ev, zj, tx)
    ref = _ode_reference(name, n, de, t, x, z, ev, zj, tx, oracle=False)
    assert torch.isfinite(out).all()
    _close(out, ref, f"{case} {name} n={n}")


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("B,Tn", [(B0, 1), (B0, 2), (16, T0), (1, T0)])
def test_ode_forward_short_grids_and_batch_edges(B, Tn, n):
    t = C.dyadic_clock(Tn, B, n)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B, Tn, seed=B + Tn, t=t, ev_rows=EV)
    out = _ode_gpu("rk4", n, de, t, x, z, ev, zj, kernel="generic")
    ref = _ode_reference("rk4", n, de, t, x, z, ev, zj)
    assert out.shape == ref.shape and traj_rel_err(out.cpu(), ref.float()) <= TOL_GPU


@pytest.mark.parametrize("dae", [False, True])
def test_rows_beyond_the_last_grid_point_are_never_read(dae):
    """z (and v) are the first T rows of a [T + 1] buffer whose last row is NaN: finite outputs, equal to the run on a tight copy"""
    t = C.dyadic_clock(T0, B0, 2)
    canary = lambda a: torch.cat((a, torch.full((1, *a.shape[1:]), float("nan"))), 0).cuda()[:-1]
    if not dae:
        de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=91, t=t, ev_rows=EV)
        xc, m = _c(x), copy.deepcopy(de).cuda()
        outs = []
        for zc in (_c(z), canary(z)):
            assert zc.shape == z.shape and zc.is_contiguous()
            with torch.no_grad():
                outs.append(C.run_ode(_solver("rk4", 2), m, _c(t), xc, zc, torch.cat((xc[0], _c(z)[0]), -1), _c(ev), _c(zj)))
        assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1])
        return
    case = C.dae_case(5, 4, 6, 6, (64, 64, 64), (64, 64, 64), B0, T0, seed=93, t=t, ev_rows=EV)
    de, ae = copy.deepcopy(case[0]).cuda(), copy.deepcopy(case[1]).cuda()
    outs = []
    for wrap in (_c, canary):
        rest = [_c(q) for q in case[2:]]
        rest[2], rest[3] = wrap(case[4]), wrap(case[5])          # z, v
        with torch.no_grad():
            outs.append(C.run_dae(_solver("rk4", 2), de, ae, *rest))
    assert all(torch.isfinite(q).all() for q in outs[1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- DAE forward
@functools.lru_cache(maxsize=None)
def _dae_forward_case(shape, n, no_x):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n)
    case = C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=17 + xd + n, t=t, ev_rows=EV)
    return C.without_x(case) if no_x else case


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(mode, shape, name, n):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    case = _dae_forward_case(shape, n, mode == "events_no_x")
    tx, ti = "tx1" in mode, "ti1" in mode
    out = C.dae_gpu(_solver(name, n), case, tx, ti)
    hold = C.dae_gpu(_solver(name, n, externals="hold"), case, tx, ti)
    ref = C.dae_walk64(_solver(name, n, "off"), case, tx, ti)
    ex, ei = traj_rel_err(out[0].cpu(), ref[0].float()), traj_rel_err(out[1].cpu(), ref[1].float())
    print(mode, shape, name, n, f"{ex:.3e} {ei:.3e}", f"against hold {traj_rel_err(out[0].cpu(), hold[0].cpu()):.3e}")
    assert out[0].shape == (T0, B0, xd) and out[1].shape == (T0, B0, idim) and ex <= TOL_GPU and ei <= TOL_GPU
    assert traj_rel_err(out[0].cpu(), hold[0].cpu()) > 100 * TOL_GPU


# ----------------------------------------------------------------------------- training
# the file's gate: cotangent G from seed 3 unless given, the fused function ran, helpers.TOL_GPU of each tensor's max; the reference trajectory
# rounded to float32 first
def _check_ode(name, n, de, t, x, z, ev, zj, tx=False, G=None):
    G = C.cotangents(3, x.shape)[0] if G is None else G
    return C.check_ode_training(functools.partial(_solver, name, n), (de, t, x, z, ev, zj), G, "_FusedOdeLin", TOL_GPU, tx, what=f"{name} n={n}",
                                ref_float=True)


# K5's paths (tests/generic_cases.py, K5_ODE_SHAPES): the register path, the streamed path (hidden 128, global accumulators) and a wide
# input on the register path (108 columns, z_dim 4); LIN_STAGED is the staged path (132 input columns) with externals -- the list's own
# staged entry has z_dim 0, where there is nothing to interpolate
LIN_K5_ODE_SHAPES = [(8, 2, 64, 3), (8, 2, 128, 3), (32, 4, 48, 2)]
LIN_STAGED = (40, 4, 40, 2)
TRAIN = ["euler", "Heun2", "RK4Classic"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", TRAIN)
@pytest.mark.parametrize("events", [True, False])
@pytest.mark.parametrize("xd,zd,H,nh", LIN_K5_ODE_SHAPES)
def test_ode_training(xd, zd, H, nh, events, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, (H,) * nh, B0, T0, seed=5 + xd + n, t=t, ev_rows=EV if events else ())
    _check_ode(name, n, de, t, x, z, ev, zj)


@pytest.mark.parametrize("n", [1, 3])
def test_ode_training_on_the_staged_path(n):
    xd, zd, H, nh = LIN_STAGED
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, (H,) * nh, B0, T0, seed=6 + n, t=t, ev_rows=EV)
    _check_ode("RK4Classic", n, de, t, x, z, ev, zj)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", TRAIN)
@pytest.mark.parametrize("xd,zd,hidden", [(8, 2, (64, 64, 64)), (8, 2, (128, 128, 128))])
def test_ode_teacher_forced_training(xd, zd, hidden, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=9 + xd + n, t=t, ev_rows=EV)
    _check_ode(name, n, de, t, x, z, ev, zj, tx=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "RK4Classic"])
def test_the_right_hand_contribution_reaches_the_next_rows_gradient(name, n):
    """a loss on xs[k + 1] alone: grad z[k + 1] is the right-hand share theta g of interval k's stages -- zero when the inputs are held (an
    ODE has no head at grid point k + 1), non-zero and the fp64 value when they are interpolated.  Euler with one sub-step reads theta = 0
    only: zero there too."""
    k = 2
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=13 + n, t=t, ev_rows=())
    G = torch.zeros(x.shape)
    G[k + 1] = torch.randn(x.shape[1:], generator=torch.Generator().manual_seed(8))
    got, ref = _check_ode(name, n, de, t, x, z, ev, zj, G=G)
    gz, rz = got["z"].cpu(), ref["z"]
    assert float(gz[k + 2:].abs().max()) == 0.0 and float(rz[k + 2:].abs().max()) == 0.0
    if name == "euler" and n == 1:
        assert float(gz[k + 1].abs().max()) == 0.0 and float(rz[k + 1].abs().max()) == 0.0
    else:
        assert float(rz[k + 1].abs().max()) > 1e-3 * float(rz.abs().max())
        _close(gz[k + 1], rz[k + 1], f"{name} n={n} grad z[k + 1]")


def _check_dae(name, n, case, tx=False, ti=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    C.check_dae_training(functools.partial(_solver, name, n), case, G, Gi, "_FusedDaeLin", TOL_GPU, tx, ti, what=f"{name} n={n}", ref_float=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", TRAIN)
@pytest.mark.parametrize("events", [True, False])
@pytest.mark.parametrize("shape", ["reg", "zvi16"])
def test_dae_training(shape, events, name, n):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n) * 0.7
    _check_dae(name, n, C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=21 + xd + n, t=t, ev_rows=EV if events else ()))


@pytest.mark.parametrize("shape", ["streamed", "h128", "deep"])
def test_dae_training_on_the_other_k5_paths(shape):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, 3) * 0.7
    _check_dae("RK4Classic", 3, C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=27 + xd, t=t, ev_rows=EV))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", TRAIN)
@pytest.mark.parametrize("tx,ti", [(True, False), (False, True), (True, True)])
def test_dae_teacher_forced_training(tx, ti, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    _check_dae(name, n, C.dae_case(5, 4, 6, 6, (64, 64, 64), (64, 64, 64), B0, T0, seed=23 + n, t=t, ev_rows=EV), tx, ti)


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_other_activations_ode(act):
    t = C.dyadic_clock(T0, B0, 3) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=31, t=t, act=act, ev_rows=EV)
    _check_ode("rk4", 3, de, t, x, z, ev, zj)


def test_silu_de_tanh_ae_dae():
    t = C.dyadic_clock(T0, B0, 2) * 0.7
    _check_dae("Kutta3", 2, C.dae_case(4, 2, 1, 2, (48, 48), (32, 32), B0, T0, seed=33, t=t, de_act=nn.SiLU, ae_act=nn.Tanh, ev_rows=EV))


# ----------------------------------------------------------------------------- routing
def test_kernel_wave_raises_under_require_and_walks_under_auto():
    """one sub-step, so that it is the externals' predicate that speaks (with more, the sub-steps' one refuses the kernel first)"""
    t = C.dyadic_clock(T0, B0, 1)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=41, t=t, ev_rows=EV)
    with pytest.raises(_lib.UnsupportedShapeError, match="externals"):
        _ode_gpu("rk4", 1, de, t, x, z, ev, zj, mode="require", kernel="wave")
    with pytest.raises(_lib.UnsupportedShapeError):
        _ode_gpu("rk4", 2, de, t, x, z, ev, zj, mode="require", kernel="wave")
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out = _ode_gpu("rk4", 1, de, t, x, z, ev, zj, mode="auto", kernel="wave")
    assert traj_rel_err(out.cpu(), _ode_reference("rk4", 1, de, t, x, z, ev, zj).float()) <= TOL_GPU


def test_direct_encode_model_takes_rows_and_k0():
    """ODE_Model(direct_encode=True) at hidden 16: neither the one-launch encoded form nor a latent kernel interpolates -- row kernels + K0"""
    torch.manual_seed(51)
    g = torch.Generator().manual_seed(51)
    B, Tn, xd, zd = B0, T0, 8, 2
    m = models.ODE_Model(xd, zd, 16, direct_encode=True, solver=nd.RK4(externals="linear"))
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
        assert traj_rel_err(o.cpu(), r.float(), bdim=0) <= TOL_GPU
    assert not torch.equal(out[0], one[0])          # (interpolated inputs are not held ones)


@pytest.mark.parametrize("n", [1, 3])
def test_externals_hold_is_bitwise_the_present_route(n):
    """through the solver, and through the fused entries with externals="hold" spelled out: the same kernels, the same bits"""
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=81, t=t, ev_rows=EV)
    for name in ("rk4", "Kutta3"):
        a = _ode_gpu(name, n, de, t, x, z, ev, zj, externals="hold")
        s = SOLVERS[name](substeps=n)
        s.fused = "require"
        b = C.ode_gpu(s, de, t, x, z, ev, zj)
        assert torch.equal(a, b)
    layers = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    args = ("rk4", layers, _c(t), _c(x[:1]), _c(z), _c(torch.cat((x[0], z[0]), -1)))
    kw = dict(event_t=_c(ev), z_jump=_c(zj), kernel="generic", substeps=n)
    assert torch.equal(fused.ode_integrate(*args, externals="hold", **kw), fused.ode_integrate(*args, **kw))
    case = C.dae_case(8, 2, 2, 2, (64, 64, 64), (64, 64, 64), B0, T0, seed=83, t=t, ev_rows=EV)
    for name in ("rk4", "Kutta3"):
        outs = []
        for s in (_solver(name, n, externals="hold"), SOLVERS[name](substeps=n)):
            s.fused = "require"
            outs.append(C.dae_gpu(s, case))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
