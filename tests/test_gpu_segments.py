"""Multiple-shooting segments (solver.segment) on the generic kernels: K0 forward, K0 + K5 training, ODE and DAE.

Yardsticks.  Euler: the fp32 CPU oracle's free run on the slices [m w : (m + 1) w + 1] started from the dataset row x[m w] (sub-steps
through the n-times refined problem of tests/generic_cases.py), under helpers.TOL_GPU on traj_rel_err.  Every other formula: the package's
callback walk with the same segment in float64 on the CPU -- pinned to the oracle on the slices, and bitwise to its own free runs on them,
by tests/test_segments_host.py -- under the same gate.  Gradients: torch autograd through that float64 walk, each tensor within 1e-5 of its
own max (`close` of tests/generic_cases.py), bitwise repeatable.  Cases: tests/segment_cases.py -- B = 33, T = 8, w in {1, 3, 7, 100},
events at steps 0, 3 (a restart point for w = 3) and 4 (inside a segment), dataset x = the free run + 0.05."""
import warnings

import pytest
import torch
import torch.nn as nn

import generic_cases as C
import segment_cases as S
from helpers import TOL_GPU, traj_rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-5
B0, T0 = S.B0, S.T0


def _gpu(name, w, n=1, mode="require", kernel="auto"):
    return S.solver(name, w, n, mode, kernel)


def _factory(name, w, n):
    return lambda mode: S.solver(name, w, n, mode)


def _ode_reference(name, n, w, de, t, x, z, ev, zj):
    if name != "euler":
        return S.walk_ode(name, n, w, de, t, x, z, ev, zj)
    a0, L = torch.cat((x[0], z[0]), -1), C.layers_of(de.x_dot)

    def free(ts, xs, zs, start):
        tf = C.refine_clock(ts, n)
        xf = torch.zeros(tf.shape[0], xs.shape[1], xs.shape[2])
        xf[0] = start
        return O.integrate_ode("euler", L, tf, xf, C.refine_rows(zs, n, ts, ev, zj), a0, ev, zj)[::n]
    with torch.no_grad():
        return S.sliced_ode(S.Free(w, free), t, x, z)


def _dae_reference(name, n, w, case):
    if name != "euler":
        return S.walk_dae(name, n, w, case)
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    Ld, La = C.layers_of(de.x_dot), C.layers_of(ae.i_calculator)

    def free(ts, xs, zs, vs, is_, start):
        tf = C.refine_clock(ts, n)
        xf = torch.zeros(tf.shape[0], xs.shape[1], xs.shape[2])
        rx, ri = O.integrate_dae("euler", Ld, La, start, tf, xf, C.refine_rows(zs, n, ts, ev, zj), C.refine_rows(vs, n, ts, ev, vj),
                                 C.refine_rows(is_, n), a0, ev, zj, vj)
        return rx[::n], ri[::n]
    with torch.no_grad():
        return S.sliced_dae(S.Free(w, free), t, x, z, v, i, x_init)


# ----------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(C.ODE_FWD_SHAPES))
def test_k0_ode_forward(shape, name, n):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances"""
    xd, zd, hidden = C.ODE_FWD_SHAPES[shape]
    de, t, x, z, ev, zj = S.ode_case(xd, zd, hidden, seed=3 + xd + n, t=C.dyadic_clock(T0, B0, n))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        free = C.ode_gpu(_gpu(name, None, n), de, t, x, z, ev, zj)
        for w in S.WS:
            out = C.ode_gpu(_gpu(name, w, n), de, t, x, z, ev, zj)
            e = traj_rel_err(out.cpu(), _ode_reference(name, n, w, de, t, x, z, ev, zj))
            gap = float(S.row_gap(out.cpu(), free.cpu(), 4).min())
            print(shape, name, n, w, f"err {e:.3e} gap to the free run at row 4 {gap:.3e}")
            assert out.shape == x.shape and torch.isfinite(out).all() and e <= TOL_GPU
            if w == 3:
                assert gap > 100 * TOL_GPU


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(C.DAE_SHAPES))
def test_k0_dae_forward(shape, name, n):
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES[shape]
    case = S.dae_case(xd, zd, vd, idim, dh, ah, seed=7 + n, t=C.dyadic_clock(T0, B0, n))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fx, fi = C.dae_gpu(_gpu(name, None, n), case)
        for w in S.WS:
            gx, gi = C.dae_gpu(_gpu(name, w, n), case)
            rx, ri = _dae_reference(name, n, w, case)
            ex, ei = traj_rel_err(gx.cpu(), rx), traj_rel_err(gi.cpu(), ri)
            gap = float(S.row_gap(gx.cpu(), fx.cpu(), 4).min())
            print(shape, name, n, w, f"xs {ex:.3e} is {ei:.3e} gap {gap:.3e}")
            assert torch.isfinite(gx).all() and torch.isfinite(gi).all() and ex <= TOL_GPU and ei <= TOL_GPU
            if w == 3:
                assert gap > 100 * TOL_GPU


def _canary(a):
    """`a` on the device as a view of an allocation whose next row is NaN: a read past the last grid point shows in the outputs"""
    if a is None:
        return None
    return torch.cat((a, torch.full_like(a[:1], float("nan"))), 0).cuda()[:-1]


@pytest.mark.parametrize("edge", ["ragged", "T1", "T2", "B16", "B1"])
def test_forward_edges(edge):
    Tn = {"T1": 1, "T2": 2}.get(edge, T0)
    B = {"B16": 16, "B1": 1}.get(edge, B0)
    pad = edge == "ragged"
    de, t, x, z, ev, zj = S.ode_case(8, 2, (64, 64, 64), B=B, Tn=Tn, seed=50, pad=pad)
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES["x5z4v6i6"]
    case = S.dae_case(xd, zd, vd, idim, dh, ah, B=B, Tn=Tn, seed=51, pad=pad)
    for name, n in (("rk4", 1), ("euler", 3)):
        for w in (1, 3, 100):
            xc, zc = _canary(x), _canary(z)
            assert torch.isnan(xc._base[Tn]).all() and xc._base.is_cuda and xc.data_ptr() == xc._base.data_ptr()          # (the NaN row IS behind row T - 1, on the device)
            with torch.no_grad():
                out = C.run_ode(_gpu(name, w, n), C.deepcopy(de).cuda(), t.cuda(), xc, zc, torch.cat((xc[0], zc[0]), -1), C.to_cuda(ev), C.to_cuda(zj))
            ref = S.walk_ode(name, n, w, de, t, x, z, ev, zj)
            assert out.shape == x.shape and not torch.isnan(out).any()
            C.close(out, ref, f"{edge} ode {name} n={n} w={w}", TOL_GPU)
            dz = tuple(_canary(q) for q in case[3:6]) + tuple(C.to_cuda(q) for q in case[6:])          # x, z, v behind a canary | i, x_init, a0, events
            with torch.no_grad():
                gx, gi = C.run_dae(_gpu(name, w, n), C.deepcopy(case[0]).cuda(), C.deepcopy(case[1]).cuda(), case[2].cuda(), *dz)
            rx, ri = S.walk_dae(name, n, w, case)
            assert not torch.isnan(gx).any() and not torch.isnan(gi).any()
            C.close(gx, rx, f"{edge} dae xs {name} n={n} w={w}", TOL_GPU)
            C.close(gi, ri, f"{edge} dae is {name} n={n} w={w}", TOL_GPU)


# ----------------------------------------------------------------------------- 2. training
# one shape per K5 path: register, streamed with LDS accumulators, streamed with global accumulators (hidden 128), wide input (3 (32 + 4) =
# 108 input columns, two hidden layers), staged (132 input columns)
K5_ODE_PATHS = {"register": C.K5_ODE_SHAPES[0], "streamed": C.K5_ODE_SHAPES[5], "global": C.K5_ODE_SHAPES[3], "wide-input": C.K5_ODE_SHAPES[6],
                "staged": (42, 2, 40, 2)}
assert K5_ODE_PATHS["wide-input"] == (32, 4, 48, 2)
TRAIN_GRID = [(name, n) for name in ("euler", "Heun2", "RK4Classic") for n in (1, 3)]
RUNS = [(True, 1), (True, 3), (True, 100), (False, 3)]          # (events, w)


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("path", list(K5_ODE_PATHS))
def test_k5_ode_training_per_path(path, name, n):
    xd, zd, h, nl = K5_ODE_PATHS[path]
    for events, w in RUNS:
        case = S.ode_case(xd, zd, (h,) * nl, seed=23, events=events)
        G, = C.cotangents(21, case[2].shape)
        S.check_ode_training(_factory(name, w, n), case, G, GRAD_TOL, what=f"{path} events={events} w={w}")


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("shape", list(C.K5_DAE_SHAPES))
def test_k5_dae_training_every_shape(shape, name, n):
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES[shape]
    for events, w in RUNS:
        case = S.dae_case(xd, zd, vd, idim, dh, ah, seed=24, events=events)
        G, Gi = C.cotangents(22, (T0, B0, xd), case[6].shape)
        S.check_dae_training(_factory(name, w, n), case, G, Gi, GRAD_TOL, what=f"{shape} events={events} w={w}")


def test_exact_zeros_and_the_restart_point_s_own_gradient():
    """A loss on segment 0 alone (rows 1 .. 3, w = 3) leaves every input gradient beyond row 3 exactly zero; a loss on row 4 alone reaches
    row 3 of z | v -- through the restart step and its head -- and nothing else of the inputs, x_init included."""
    ode = S.ode_case(8, 2, (64, 64, 64), seed=27, events=False)
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = S.dae_case(xd, zd, vd, idim, dh, ah, seed=28, events=False)
    G, = C.cotangents(31, ode[2].shape)
    Gd, Gi = C.cotangents(32, (T0, B0, xd), dae[6].shape)
    head, row4 = torch.zeros(T0, 1, 1), torch.zeros(T0, 1, 1)
    head[:4], row4[4] = 1.0, 1.0
    got, _ = S.check_ode_training(_factory("RK4Classic", 3, 1), ode, G * head, GRAD_TOL, what="ode segment 0")
    S.rows_beyond_are_zero(got, ("z",), 3, "ode segment 0")
    assert not got["z"][3:].any() and got["x_init"].abs().sum() > 0
    got, _ = S.check_ode_training(_factory("RK4Classic", 3, 2), ode, G * row4, GRAD_TOL, what="ode row 4")
    assert not got["z"][:3].any() and not got["z"][4:].any() and got["z"][3].abs().sum() > 0 and not got["x_init"].any()
    got, _ = S.check_dae_training(_factory("RK4Classic", 3, 1), dae, Gd * head, Gi * head, GRAD_TOL, what="dae segment 0")
    S.rows_beyond_are_zero(got, ("z", "v"), 3, "dae segment 0")
    assert got["x_init"].abs().sum() > 0
    for n in (1, 2):
        got, _ = S.check_dae_training(_factory("euler", 3, n), dae, Gd * row4, Gi * 0, GRAD_TOL, what=f"dae row 4 n={n}")
        for k in ("z", "v"):
            assert not got[k][:3].any() and not got[k][4:].any() and got[k][3].abs().sum() > 0, k
        assert not got["x_init"].any()


@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_other_activations(act):
    ode = S.ode_case(8, 2, (64, 64, 64), seed=30, act=act)
    assert traj_rel_err(C.ode_gpu(_gpu("rk4", 3), *ode).cpu(), S.walk_ode("rk4", 1, 3, *ode)) <= TOL_GPU
    G, = C.cotangents(33, ode[2].shape)
    S.check_ode_training(_factory("Heun2", 3, 2), ode, G, GRAD_TOL, what=act.__name__)
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = S.dae_case(xd, zd, vd, idim, dh, ah, seed=31, de_act=act, ae_act=act)
    Gd, Gi = C.cotangents(34, (T0, B0, xd), dae[6].shape)
    S.check_dae_training(_factory("euler", 3, 1), dae, Gd, Gi, GRAD_TOL, what=act.__name__)


# ----------------------------------------------------------------------------- 3. routing
def test_routing_on_the_device():
    ode = S.ode_case(8, 2, (64, 64, 64), seed=32)
    ref = S.walk_ode("rk4", 1, 3, *ode)
    for kernel in ("wave", "tile", "mfma", "wide"):
        with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
            C.ode_gpu(_gpu("rk4", 3, kernel=kernel), *ode)
        with pytest.warns(RuntimeWarning, match="not fusable"):
            out = C.ode_gpu(_gpu("rk4", 3, mode="auto", kernel=kernel), *ode)
        assert traj_rel_err(out.cpu(), ref) <= TOL_GPU          # the walk
    assert traj_rel_err(C.ode_gpu(_gpu("rk4", 3, kernel="generic"), *ode).cpu(), ref) <= TOL_GPU
    lin = nd.RK4(segment=3, externals="linear")
    lin.fused = "require"
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        C.ode_gpu(lin, *ode)
    # a dataset x that requires grad: fused while no step restarts (x[0] gets its gradient), refused under "require" once one does
    de, t, x, z, ev, zj = ode
    xg, zc = x.cuda().requires_grad_(True), z.cuda()
    a0 = torch.cat((x[0], z[0]), -1).cuda()
    xs = C.run_ode(_gpu("rk4", 100), C.deepcopy(de).cuda(), t.cuda(), xg, zc, a0, ev.cuda(), zj.cuda())
    assert type(xs.grad_fn).__name__.startswith("_FusedOdeMs")
    xs.sum().backward()
    assert xg.grad[0].abs().sum() > 0 and not xg.grad[1:].any()
    with pytest.raises(nd.NotFusableError, match="segment"):
        C.run_ode(_gpu("rk4", 3), C.deepcopy(de).cuda(), t.cuda(), xg, zc, a0, ev.cuda(), zj.cuda())
