"""Runge-Kutta-Chebyshev steps (neural_dae.RKC1 / RKC2) on the generic kernels: K0 forward, K0 + K5 training, ODE and DAE.

Yardstick: the package's callback walk of the same modules in float64 on the CPU -- the definition of the semantics, pinned to the
stand-alone restatement by tests/test_rkc_host.py -- and torch autograd through it for the gradients.  Gate: generic_cases.close, each
tensor within helpers.TOL_GPU of its own max.  The recurrence amplifies rounding with s^2, so the host suite measures d, the distance of
the package's own fp32 walk from the fp64 walk, on every case here of s <= 5 and asserts 4 d <= TOL_GPU: the plain gate binds for them.
Only the two forward cases of tests/rkc_cases.py WIDE (s = 8, s = 16) use max(TOL_GPU, 4 d).  B = 33: three tiles of 16 trajectories, the last with
one; T = 6; grid step 0.1; events at steps 0 and 3."""
import functools

import pytest
import torch
import torch.nn as nn

import generic_cases as C
import rkc_cases as K
from helpers import TOL_GPU
from py_psnode_amd import _lib, fused
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

_c = C.to_cuda
_close = functools.partial(C.close, tol=TOL_GPU)


def _ode_pair(order, s, case, tx=False, mode="require", kernel="auto"):
    return C.ode_forward_pair(K.solver(order, s, "off"), K.solver(order, s, mode, kernel), *case, tx)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("order,s", K.METHODS)
@pytest.mark.parametrize("shape", list(C.ODE_FWD_SHAPES))
def test_ode_forward(shape, order, s):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances -- with events at steps 0 and 3"""
    case = K.ode_fwd_case(shape, order, s)
    out, ref = _ode_pair(order, s, case)
    assert out.shape == case[2].shape and torch.isfinite(out).all()
    _close(out, ref, f"{shape} RKC{order} s={s}")


@pytest.mark.parametrize("order,s", K.WIDE)
def test_ode_forward_many_stages(order, s):
    """the two cases under the widened gate max(TOL_GPU, 4 d), d measured here on the CPU"""
    case = K.ode_fwd_case("reg", order, s)
    d = K.ode_floor(order, s, case)
    out, ref = _ode_pair(order, s, case)
    print(f"s={s}: d = {d:.3e}")
    C.close(out, ref, f"RKC{order} s={s}", max(TOL_GPU, 4 * d))


@pytest.mark.parametrize("order,s", [(1, 3), (2, 5)])
@pytest.mark.parametrize("edge", ["padded", "padded_truex", "T1", "T2", "B16", "B1", "nan_canary"])
def test_ode_forward_edges(edge, order, s):
    Tn = {"T1": 1, "T2": 2}.get(edge, K.T0)
    B = {"B16": 16, "B1": 1}.get(edge, K.B0)
    case = K.ode_fwd_case("reg", order, s, B=B, Tn=Tn, pad="padded" in edge)
    tx = edge == "padded_truex"
    if edge == "nan_canary":          # a row behind the grid must not be read: the tensors are views that end in front of a NaN row
        de, t, x, z, ev, zj = case
        ref = C.ode_walk64(K.solver(order, s, "off"), de, t, x, z, ev, zj)
        canary = lambda q: torch.cat((q, torch.full_like(q[:1], float("nan"))), 0).cuda()[:-1]
        xc, zc = x.cuda(), canary(z)
        with torch.no_grad():
            out = C.run_ode(K.solver(order, s), C.deepcopy(de).cuda(), canary(t), xc, zc, torch.cat((xc[0], zc[0]), -1), _c(ev), _c(zj))
    else:
        out, ref = _ode_pair(order, s, case, tx, kernel="generic")
    assert out.shape == ref.shape and torch.isfinite(out[:Tn]).all()
    _close(out, ref, f"{edge} RKC{order} s={s}")


@pytest.mark.parametrize("order,s", [(1, 3), (2, 2), (2, 5)])
@pytest.mark.parametrize("shape", list(C.DAE_SHAPES))
@pytest.mark.parametrize("mode", ["events_no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_dae_forward(mode, shape, order, s):
    case = K.dae_fwd_case(shape, order, s, no_x=mode == "events_no_x")
    tx, ti = "tx1" in mode, "ti1" in mode
    out, ref = C.dae_forward_pair(K.solver(order, s, "off"), K.solver(order, s), case, tx, ti)
    _close(out[0], ref[0], f"{mode} {shape} RKC{order} s={s} xs")
    _close(out[1], ref[1], f"{mode} {shape} RKC{order} s={s} is")


# ----------------------------------------------------------------------------- the stage buffer
@pytest.mark.parametrize("order,s", [(1, 1), (1, 3), (2, 2), (2, 5)])
def test_stage_rows_are_the_walks_intermediate_states_ode(order, s):
    de, t, x, z, ev, zj = K.ode_fwd_case("reg", order, s)
    xd = x.shape[-1]
    rows = []
    with torch.no_grad():
        ref = K.ref_ode(order, s, C.deepcopy(de).double(), t.double(), x.double(), z.double(), ev.double(), zj.double(), stages_out=rows)
    method = K.solver(order, s).method
    layers = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    args = (method, layers, _c(t), _c(x[:1]), _c(z), _c(torch.cat((x[0], z[0]), -1)))
    kw = dict(event_t=_c(ev), z_jump=_c(zj))
    xs, x_sub = fused.ode_integrate(*args, save_sub=True, **kw)
    assert torch.equal(xs, fused.ode_integrate(*args, **kw))          # with no stage buffer the outputs are bitwise the same
    assert x_sub.shape == (K.T0 - 1, s - 1, K.B0, xd) and torch.isfinite(x_sub).all()
    _close(xs, ref, f"RKC{order} s={s} xs")
    if s > 1:
        want = torch.stack([torch.stack(r) for r in rows])          # [T-1, s-1, B, xd]: Y_1 .. Y_{s-1}
        _close(x_sub, want, f"RKC{order} s={s} stage rows")


@pytest.mark.parametrize("order,s", [(1, 3), (2, 5)])
def test_stage_rows_are_the_walks_intermediate_states_dae(order, s):
    case = K.dae_fwd_case("x5z4v6i6", order, s)
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    rows = []
    case64 = (C.deepcopy(de).double(), C.deepcopy(ae).double()) + tuple(C.to64(q) for q in case[2:])
    with torch.no_grad():
        K.ref_dae(order, s, case64, stages_out=rows)
    dl = [(w.cuda(), b.cuda()) for w, b in C.layers_of(de.x_dot)]
    al = [(w.cuda(), b.cuda()) for w, b in C.layers_of(ae.i_calculator)]
    args = (K.solver(order, s).method, dl, al, _c(x_init), _c(t), _c(x), _c(z), _c(v), _c(i), _c(a0))
    kw = dict(event_t=_c(ev), z_jump=_c(zj), v_jump=_c(vj))
    xs, is_, x_sub = fused.dae_integrate(*args, save_sub=True, **kw)
    xs2, is2 = fused.dae_integrate(*args, **kw)
    assert torch.equal(xs, xs2) and torch.equal(is_, is2)
    _close(x_sub, torch.stack([torch.stack(r) for r in rows]), f"RKC{order} s={s} stage rows")


# ----------------------------------------------------------------------------- gradients
def _check_ode(order, s, case, tx=False):
    G, = C.cotangents(3, case[2].shape)
    return C.check_ode_training(functools.partial(K.solver, order, s), case, G, "_FusedOdeRkc", TOL_GPU, tx, what=f"RKC{order} s={s}")


def _check_dae(order, s, case, tx=False, ti=False):
    G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
    C.check_dae_training(functools.partial(K.solver, order, s), case, G, Gi, "_FusedDaeRkc", TOL_GPU, tx, ti, what=f"RKC{order} s={s}")


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS)
@pytest.mark.parametrize("xd,zd,H,nh", K.K5_ODE_SHAPES)
def test_ode_training(xd, zd, H, nh, order, s):
    """K5's register, streamed (LDS and global accumulators), staged and wide-input paths (z_dim 0: no events)"""
    _check_ode(order, s, K.ode_train_case(xd, zd, H, nh, order, s))


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS + [(1, 1)])
def test_ode_training_without_events_and_teacher_forced(order, s):
    _check_ode(order, s, K.ode_train_case(8, 2, 64, 3, order, s, events=False))
    _check_ode(order, s, K.ode_train_case(8, 2, 64, 3, order, s), tx=True)


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS)
@pytest.mark.parametrize("shape", list(C.K5_DAE_SHAPES))
def test_dae_training(shape, order, s):
    _check_dae(order, s, K.dae_train_case(shape, order, s))


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS)
def test_dae_training_without_events(order, s):
    _check_dae(order, s, K.dae_train_case("reg", order, s, events=False))


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS)
@pytest.mark.parametrize("tx,ti", [(True, False), (False, True), (True, True)])
def test_dae_teacher_forced_training(tx, ti, order, s):
    _check_dae(order, s, K.dae_train_case("zvi16", order, s), tx, ti)


# ----------------------------------------------------------------------------- activations, stability, routing
@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_other_activations_ode(act):
    case = K.ode_train_case(8, 2, 64, 3, 2, 3, act=act)
    out, ref = _ode_pair(2, 3, case)
    _close(out, ref, f"{act.__name__} forward")
    _check_ode(2, 3, case)


def test_silu_de_tanh_ae_dae():
    _check_dae(1, 3, C.dae_case(4, 2, 1, 2, (48, 48), (32, 32), K.B0, K.T0, seed=33, t=K.clock(), de_act=nn.SiLU, ae_act=nn.Tanh, ev_rows=K.EV))


def test_stability_on_the_device():
    """a ReLU DE_Func with W_1 = [I; -I] on the s block, W_2 = -lambda [I, -I] is x' = -lambda x exactly: at h lambda = 100 RKC1(stages=8) stays
    bounded over T = 6 where Euler(substeps=8), the same eight evaluations, overflows"""
    xd, lam, h = 4, 1000.0, 0.1
    from py_psnode_amd import models
    de = models.DE_Func(xd, (2 * xd,), xd, activation=nn.ReLU)          # the input is a0 | s - a0 | s, 3 xd columns
    lin1, lin2 = [m for m in de.x_dot if isinstance(m, nn.Linear)]
    with torch.no_grad():
        lin1.weight.zero_()
        lin1.bias.zero_()
        lin2.bias.zero_()
        lin1.weight[:xd, 2 * xd:] = torch.eye(xd)
        lin1.weight[xd:, 2 * xd:] = -torch.eye(xd)
        lin2.weight.copy_(-lam * torch.cat((torch.eye(xd), -torch.eye(xd)), 1))
    t = (torch.arange(K.T0, dtype=torch.float32) * h).view(K.T0, 1, 1).repeat(1, K.B0, 1)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(K.T0, K.B0, xd, generator=g)
    z = torch.zeros(K.T0, K.B0, 0)
    stable = C.ode_gpu(K.solver(1, 8), de, t, x, z, None, None)
    assert torch.isfinite(stable).all() and float(stable.abs().max()) <= float(x[0].abs().max())
    e = nd.Euler(substeps=8)
    e.fused = "require"
    blown = C.ode_gpu(e, de, t, x, z, None, None)
    assert not torch.isfinite(blown[-1]).all() or float(blown[-1].abs().max()) > 1e6


def test_routing():
    case = K.ode_fwd_case("reg", 1, 3)
    with pytest.raises(_lib.UnsupportedShapeError):
        _ode_pair(1, 3, case, mode="require", kernel="wave")
    with pytest.warns(RuntimeWarning, match="not fusable"):
        out, ref = _ode_pair(1, 3, case, mode="auto", kernel="wave")
    _close(out, ref, "walk under auto")
    a, _ = _ode_pair(1, 1, case)          # one stage: Euler's formula on the recurrence build, against the built-in Euler kernel's fp64 walk
    e = nd.Euler()
    e.fused = "off"
    _close(a, C.ode_walk64(e, *case), "RKC1 s=1 against the Euler walk")
