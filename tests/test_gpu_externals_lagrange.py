"""Four-point Lagrange interpolated external inputs (solver.externals = "lagrange") on the generic kernels: K0 forward, K0 + K5 training,
ODE and DAE.

Yardstick: the package's callback walk of the same modules in float64 on the CPU -- the definition of the semantics, pinned to a stand-alone
restatement, to polynomial reproduction and to its order by tests/test_externals_lagrange_host.py -- under helpers.TOL_GPU on traj_rel_err.
Gradients: torch autograd through that float64 walk, each tensor within TOL_GPU of its own max (`close` of tests/generic_cases.py); two
fused runs bit for bit the same.  B = 33: three tiles of 16 trajectories, the last with one; T = 12; events at steps 0, 2, 3 and 6, which
cut the record into pieces of 3, 2, 4 and 6 nodes -- every q and every offset of a stencil.

An ODE output must also differ from the "linear" run on the same inputs by more than 100 x TOL_GPU (and the two float64 walks must, too), so
that a kernel that silently interpolates linearly cannot pass.  The one exception is Euler with one sub-step: its only stage has
theta = 0, the left rows themselves, so the run IS "hold" there by definition and the test asserts that instead (within TOL_GPU)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import generic_cases as C
from externals_lagrange_cases import EV_ROWS as EV
from generic_cases import DAE_SHAPES, K5_DAE_SHAPES, ODE_FWD_SHAPES
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

SOLVERS = {"euler": nd.Euler, "rk4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
B0, T0 = 33, 12
_c = C.to_cuda
_close = functools.partial(C.close, tol=TOL_GPU)


def _solver(name, n, mode="require", kernel="auto", externals="lagrange"):
    s = SOLVERS[name](substeps=n, externals=externals)
    s.fused, s.kernel = mode, kernel
    return s


def _ode_reference(name, n, de, t, x, z, ev, zj, tx=False, externals="lagrange"):
    return C.ode_walk64(_solver(name, n, "off", externals=externals), de, t, x, z, ev, zj, tx)


def _ode_gpu(name, n, de, t, x, z, ev, zj, tx=False, mode="require", kernel="auto", externals="lagrange"):
    return C.ode_gpu(_solver(name, n, mode, kernel, externals), de, t, x, z, ev, zj, tx)


# ----------------------------------------------------------------------------- ODE forward
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(ODE_FWD_SHAPES))
def test_ode_forward(shape, name, n):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances.  Four times the builders' clock (still dyadic) and
    externals, as the linear test scales them: the eight-layer MLP of 32 units is insensitive to z at the builders' scale."""
    xd, zd, hidden = ODE_FWD_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n) * 4.0
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=3 + xd + len(hidden) + n, t=t, ev_rows=EV)
    z, zj = 4.0 * z, 4.0 * zj
    out = _ode_gpu(name, n, de, t, x, z, ev, zj)          # fused = "require"
    other = _ode_gpu(name, n, de, t, x, z, ev, zj, externals="hold" if (name == "euler" and n == 1) else "linear")
    ref = _ode_reference(name, n, de, t, x, z, ev, zj)
    ref_lin = _ode_reference(name, n, de, t, x, z, ev, zj, externals="linear")
    e = traj_rel_err(out.cpu(), ref)
    d_gpu, d_cpu = traj_rel_err(out.cpu(), other.cpu()), traj_rel_err(ref, ref_lin)
    print(shape, name, n, f"{e:.3e}", f"against linear / hold {d_gpu:.3e}", f"the walks {d_cpu:.3e}")
    assert out.shape == x.shape and torch.isfinite(out).all() and e <= TOL_GPU
    if name == "euler" and n == 1:
        assert d_gpu <= TOL_GPU          # (one stage at theta = 0: the hold, by definition)
    else:
        assert d_cpu > 100 * TOL_GPU and d_gpu > 100 * TOL_GPU


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("case", ["truex", "ragged", "ragged_truex"])
def test_ode_forward_teacher_forced_and_ragged(case, name, n):
    xd, zd, hidden = ODE_FWD_SHAPES["streamed" if n == 3 else "reg"]
    t = C.dyadic_clock(T0, B0, n) * 0.7          # (no longer dyadic: h is a rounded quotient)
    if "ragged" in case:
        t = C.padded(t)                           # (trajectories 2, 5, ...: two invalid intervals at the end, pieces of their own)
    de, _, x, z, ev, zj = C.ode_case(xd, zd, hidden, B0, T0, seed=40 + n, t=t, ev_rows=EV)
    tx = "truex" in case
    out = _ode_gpu(name, n, de, t, x, z, ev, zj, tx)
    ref = _ode_reference(name, n, de, t, x, z, ev, zj, tx)
    assert torch.isfinite(out).all()
    _close(out, ref, f"{case} {name} n={n}")


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("B,Tn", [(B0, 1), (B0, 2), (B0, 3), (B0, 4), (16, T0), (1, T0)])
def test_ode_forward_short_grids_and_batch_edges(B, Tn, n):
    """T = 2, 3, 4 without events: the whole record is one piece of q = 2, 3, 4 nodes"""
    t = C.dyadic_clock(Tn, B, n)
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B, Tn, seed=B + Tn, t=t, ev_rows=EV if Tn == T0 else ())
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


@functools.lru_cache(maxsize=None)
def _dae_forward_ref(shape, name, n, mode):
    case = _dae_forward_case(shape, n, mode == "events_no_x")
    return C.dae_walk64(_solver(name, n, "off"), case, "tx1" in mode, "ti1" in mode)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(mode, shape, name, n):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    case = _dae_forward_case(shape, n, mode == "events_no_x")
    tx, ti = "tx1" in mode, "ti1" in mode
    out = C.dae_gpu(_solver(name, n), case, tx, ti)
    ref = _dae_forward_ref(shape, name, n, mode)
    ex, ei = traj_rel_err(out[0].cpu(), ref[0].float()), traj_rel_err(out[1].cpu(), ref[1].float())
    print(mode, shape, name, n, f"{ex:.3e} {ei:.3e}")
    assert out[0].shape == (T0, B0, xd) and out[1].shape == (T0, B0, idim) and ex <= TOL_GPU and ei <= TOL_GPU


# ----------------------------------------------------------------------------- training
# the file's gate: cotangent G from seed 3 unless given, the fused function ran, helpers.TOL_GPU of each tensor's max; the reference trajectory
# rounded to float32 first
def _check_ode(name, n, de, t, x, z, ev, zj, tx=False, G=None):
    G = C.cotangents(3, x.shape)[0] if G is None else G
    return C.check_ode_training(functools.partial(_solver, name, n), (de, t, x, z, ev, zj), G, "_FusedOdeLag", TOL_GPU, tx, what=f"{name} n={n}",
                                ref_float=True)


# K5's paths (tests/generic_cases.py, K5_ODE_SHAPES): the register path, the streamed path (hidden 128, global accumulators) and a wide
# input on the register path (108 columns, z_dim 4); LAG_STAGED is the staged path (132 input columns) with externals
LAG_K5_ODE_SHAPES = [(8, 2, 64, 3), (8, 2, 128, 3), (32, 4, 48, 2)]
LAG_STAGED = (40, 4, 40, 2)
TRAIN = ["euler", "Heun2", "RK4Classic"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", TRAIN)
@pytest.mark.parametrize("events", [True, False])
@pytest.mark.parametrize("xd,zd,H,nh", LAG_K5_ODE_SHAPES)
def test_ode_training(xd, zd, H, nh, events, name, n):
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(xd, zd, (H,) * nh, B0, T0, seed=5 + xd + n, t=t, ev_rows=EV if events else ())
    _check_ode(name, n, de, t, x, z, ev, zj)


@pytest.mark.parametrize("n", [1, 3])
def test_ode_training_on_the_staged_path_and_a_padded_clock(n):
    xd, zd, H, nh = LAG_STAGED
    t = C.padded(C.dyadic_clock(T0, B0, n) * 0.7)
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
@pytest.mark.parametrize("name", ["Kutta3", "RK4Classic"])      # (stages strictly inside the interval: all four weights non-zero)
def test_an_interior_row_s_loss_reaches_the_four_rows_of_its_stencil_and_no_other(name, n):
    """Teacher-forced, no events, a loss on xs[k + 1] alone: only interval k's stages see it, whose stencil is rows k - 1 .. k + 2 -- those
    get their fp64 values (all four non-zero), every other row of grad z exactly zero.  Free-running, the earlier intervals reach it too,
    but nothing behind row k + 2 does."""
    k = 5
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=13 + n, t=t, ev_rows=())
    G = torch.zeros(x.shape)
    G[k + 1] = torch.randn(x.shape[1:], generator=torch.Generator().manual_seed(8))
    got, ref = _check_ode(name, n, de, t, x, z, ev, zj, tx=True, G=G)
    gz, rz = got["z"].cpu(), ref["z"]
    for row in range(T0):
        if k - 1 <= row <= k + 2:
            assert float(rz[row].abs().max()) > 1e-3 * float(rz.abs().max()), row
            _close(gz[row], rz[row], f"{name} n={n} grad z[{row}]")
        else:
            assert float(gz[row].abs().max()) == 0.0 and float(rz[row].abs().max()) == 0.0, row
    got, ref = _check_ode(name, n, de, t, x, z, ev, zj, G=G)
    assert float(got["z"][k + 3:].abs().max()) == 0.0 and float(ref["z"][k + 3:].abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 3])
def test_a_jumped_node_s_share_lands_in_the_jump_gradient_not_in_grad_z(n):
    """Teacher-forced, an event at step k, a loss on xs[k + 2] alone: interval k + 1 lies in the piece that starts at k, its stencil is the
    jumped node k and rows k + 1 .. k + 3 -- grad z[k] is exactly zero, grad z_jump of that event its fp64 value."""
    k = 3
    t = C.dyadic_clock(T0, B0, n) * 0.7
    de, _, x, z, ev, zj = C.ode_case(8, 2, (64, 64, 64), B0, T0, seed=15 + n, t=t, ev_rows=(k,))
    G = torch.zeros(x.shape)
    G[k + 2] = torch.randn(x.shape[1:], generator=torch.Generator().manual_seed(9))
    got, ref = _check_ode("RK4Classic", n, de, t, x, z, ev, zj, tx=True, G=G)
    gz, rz = got["z"].cpu(), ref["z"]
    assert float(gz[k].abs().max()) == 0.0 and float(rz[k].abs().max()) == 0.0
    assert float(ref["zj"].abs().max()) > 1e-3 * float(rz.abs().max())
    _close(got["zj"], ref["zj"], f"n={n} grad z_jump")
    for row in range(T0):
        if not k + 1 <= row <= k + 3:
            assert float(gz[row].abs().max()) == 0.0 and float(rz[row].abs().max()) == 0.0, row


def _check_dae(name, n, case, tx=False, ti=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    C.check_dae_training(functools.partial(_solver, name, n), case, G, Gi, "_FusedDaeLag", TOL_GPU, tx, ti, what=f"{name} n={n}", ref_float=True)


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
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='lagrange'"):
        _ode_gpu("rk4", 1, de, t, x, z, ev, zj, mode="require", kernel="wave")
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out = _ode_gpu("rk4", 1, de, t, x, z, ev, zj, mode="auto", kernel="wave")
    assert traj_rel_err(out.cpu(), _ode_reference("rk4", 1, de, t, x, z, ev, zj).float()) <= TOL_GPU
