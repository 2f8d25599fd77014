"""Stage-wise algebraic heads (solver.algebraic = "stage") on the generic kernels: K0 forward, K0 + K5 training, linear and Lagrange
externals.

Yardstick: the package's callback walk of the same modules in float64 on the CPU -- the definition of the semantics, pinned to a
stand-alone restatement, to its order and to a hand-written adjoint by tests/test_stage_heads_host.py -- under helpers.TOL_GPU on
traj_rel_err; gradients: torch autograd through that walk, each tensor within 1e-5 of its own max (`close` of tests/generic_cases.py), the
gate of the option families.  B = 33: three tiles of 16 trajectories, the last with one; T = 6; events at steps 0 and 3.

A forward output must also differ from the "step" run on the same inputs by more than 100 x TOL_GPU, so that a kernel that never runs a
stage head cannot pass; tests/test_stage_heads_host.py asserts on the CPU that the cases (tests/stage_head_cases.py) give the fp64
solutions that distance."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn as nn

import generic_cases as C
import stage_head_cases as S
from generic_cases import K5_DAE_SHAPES
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

B0, T0, EV = S.B0, S.T0, S.EV
TOL_GRAD = 1e-5
_close = functools.partial(C.close, tol=TOL_GPU)


def _solver(name, n, ext, mode="require", kernel="auto", algebraic="stage"):
    return S.solver(name, n, ext, algebraic, mode, kernel)


def _walk64(name, n, ext, case, tx=False, ti=False):
    return C.dae_walk64(S.solver(name, n, ext), case, tx, ti)


def _gates(out, ref, what):
    ex, ei = traj_rel_err(out[0].cpu(), ref[0].float()), traj_rel_err(out[1].cpu(), ref[1].float())
    print(what, f"xs {ex:.3e} is {ei:.3e}")
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and ex <= TOL_GPU and ei <= TOL_GPU, (what, ex, ei)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", S.METHODS)
@pytest.mark.parametrize("shape", list(S.FWD_SHAPES))
def test_forward(shape, name, n, ext):
    """every form of K0 that has a DAE instance -- register (QM 4, QM 8), resident, streamed, the eight-layer loop"""
    case = S.forward_case(shape, n)
    out = C.dae_gpu(_solver(name, n, ext), case)          # fused = "require"
    step = C.dae_gpu(_solver(name, n, ext, algebraic="step"), case)
    _gates(out, _walk64(name, n, ext, case), f"{shape} {name} n={n} {ext}")
    gap = traj_rel_err(out[0].cpu(), step[0].cpu())
    print(f"against step {gap:.3e}")
    assert gap > 100 * TOL_GPU


# ----------------------------------------------------------------------------- edges
@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("mode", ["no_x", "truex", "ragged", "ragged_truex"])
def test_forward_without_dataset_x_teacher_forced_and_ragged(mode, n, ext):
    case = S.forward_case("reg", n, no_x=mode == "no_x", pad="ragged" in mode)
    tx = "truex" in mode
    for name in ("rk4", "Kutta3"):
        _gates(C.dae_gpu(_solver(name, n, ext), case, tx), _walk64(name, n, ext, case, tx), f"{mode} {name} n={n} {ext}")


@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 2])
def test_input_true_i_is_the_step_launch_bit_for_bit(n, ext):
    case = S.forward_case("reg", n)
    for tx in (False, True):
        a, b = C.dae_gpu(_solver("RK4Classic", n, ext), case, tx, True), C.dae_gpu(_solver("RK4Classic", n, ext, algebraic="step"), case, tx, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = C.dae_gpu(_solver("euler", n, ext), case), C.dae_gpu(_solver("euler", n, ext, algebraic="step"), case)          # one stage: the parent family
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("B,Tn", [(B0, 1), (B0, 2), (16, T0), (1, T0)])
def test_forward_short_grids_and_batch_edges(B, Tn, n):
    case = S.forward_case("reg", n, Tn=Tn, B=B)
    for ext in S.INTERP:
        out = C.dae_gpu(_solver("RK4Classic", n, ext, kernel="generic"), case)
        assert out[0].shape == (Tn, B, 8) and out[1].shape == (Tn, B, 2)
        _gates(out, _walk64("RK4Classic", n, ext, case), f"B={B} T={Tn} n={n} {ext}")


@pytest.mark.parametrize("ext", S.INTERP)
def test_rows_beyond_the_last_grid_point_are_never_read(ext):
    """z and v are the first T rows of [T + 1] buffers whose last row is NaN: finite outputs, equal to the run on tight copies"""
    case = S.forward_case("reg", 2)
    canary = lambda a: torch.cat((a, torch.full((1, *a.shape[1:]), float("nan"))), 0).cuda()[:-1]
    de, ae = copy.deepcopy(case[0]).cuda(), copy.deepcopy(case[1]).cuda()
    outs = []
    for wrap in (C.to_cuda, canary):
        rest = [C.to_cuda(q) for q in case[2:]]
        rest[2], rest[3] = wrap(case[4]), wrap(case[5])          # z, v
        with torch.no_grad():
            outs.append(C.run_dae(_solver("RK4Classic", 2, ext), de, ae, *rest))
    assert all(torch.isfinite(q).all() for q in outs[1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- training
def _train_case(shape, n, events=True, seed=0):
    xd, zd, vd, idim, dh, ah = K5_DAE_SHAPES[shape]
    t = C.dyadic_clock(T0, B0, n) * 2.0
    return C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=29 + xd + n + seed, t=t, ev_rows=EV if events else (), perturb_x_init=True)


def _check(name, n, ext, case, tx=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    return C.check_dae_training(lambda mode: _solver(name, n, ext, mode), case, G, Gi, "_FusedDaeSth", TOL_GRAD, tx, False,
                                what=f"{name} n={n} {ext}", ref_float=True)


# K5's paths (tests/generic_cases.py, K5_DAE_SHAPES): the register path, a wide input on it (z | v | i of 16 columns), the streamed path
# with global accumulators (hidden 128) and the staged path (five layers)
@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["Heun2", "RK4Classic"])
@pytest.mark.parametrize("shape", ["reg", "zvi16", "h128", "deep"])
def test_training(shape, name, n, ext):
    _check(name, n, ext, _train_case(shape, n))


@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["Heun2", "RK4Classic"])
def test_training_without_events(name, n, ext):
    _check(name, n, ext, _train_case("reg", n, events=False))


@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["Heun2", "RK4Classic"])
def test_teacher_forced_training_elu1(name, n, ext):
    """input_true_x: sub-step 0 starts from x[k], the stage heads still see X_s"""
    _check(name, n, ext, _train_case("zvi16", n, seed=1), tx=True)


@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("which", ["is", "xs"])
def test_a_loss_on_one_row_reaches_the_next_grid_point_s_externals_through_the_stage_heads(which, ext):
    """A loss on is[k + 1] alone, and one on xs[k + 1] alone: grad z[k + 1] / grad v[k + 1] carry the right-hand (stencil) shares of the
    stages of interval k, a stage head's among them, and have their fp64 values."""
    k, n = 1, 1          # (no event at step 1)
    case = _train_case("reg", n)
    G, Gi = C.cotangents(6, case[3].shape, case[6].shape)
    mask = torch.zeros(T0, 1, 1)
    mask[k + 1] = 1.0
    G, Gi = (G * mask, Gi * 0.0) if which == "xs" else (G * 0.0, Gi * mask)
    make = lambda mode: _solver("RK4Classic", n, ext, mode)
    _, _, ref = C.dae_train(make, case, G, Gi, "cpu")
    _, _, got = C.dae_train(make, case, G, Gi, "cuda")
    for key in ("z", "v"):
        assert float(ref[key][k + 1].abs().max()) > 1e-3 * float(ref[key].abs().max())
        C.close(got[key][k + 1], ref[key][k + 1], f"{which} {ext} grad {key}[k + 1]", TOL_GRAD)
        C.close(got[key], ref[key], f"{which} {ext} grad {key}", TOL_GRAD)


def test_tanh_de_silu_ae():
    t = C.dyadic_clock(T0, B0, 2) * 2.0
    case = C.dae_case(4, 2, 1, 2, (48, 48), (32, 32), B0, T0, seed=33, t=t, de_act=nn.Tanh, ae_act=nn.SiLU, ev_rows=EV)
    for ext in S.INTERP:
        _check("Kutta3", 2, ext, case)


# ----------------------------------------------------------------------------- routing
def test_kernel_wave_segments_and_per_trajectory_events_raise_under_require_and_walk_under_auto():
    case = S.forward_case("reg", 1)
    ref = _walk64("rk4", 1, "linear", case)
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        C.dae_gpu(_solver("rk4", 1, "linear", "require", "wave"), case)
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out = C.dae_gpu(_solver("rk4", 1, "linear", "auto", "wave"), case)
    _gates(out, ref, "wave, auto")
    for mode in ("require", "auto"):
        seg = nd.RK4(externals="linear", algebraic="stage", segment=2)
        seg.fused = mode
        if mode == "require":
            with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
                C.dae_gpu(seg, case)
        else:
            with pytest.warns(RuntimeWarning, match="not fusable"):
                out = C.dae_gpu(seg, case)
            off = nd.RK4(externals="linear", algebraic="stage", segment=2)
            off.fused = "off"
            _gates(out, C.dae_walk64(off, case), "segment, auto")
    # per-trajectory events: the solver's predicate speaks before any launch
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
        _solver("rk4", 1, "linear", "require")._generic_only_ok("integrate_DAE", (None, None), True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert not _solver("rk4", 1, "linear", "auto")._generic_only_ok("integrate_DAE", (None, None), True)
