"""Per-trajectory events on the generic kernels (ODE_Event / DAE_Event with per_trajectory=True -> the _pev builds of K0 / K5), on the GPU:
the [T-1, B] event table against a numpy restatement, K0 forward against the per-trajectory oracle runs (tests/pev_cases.py) in every
form of the kernel and next to the shared-rule GPU run, its edge cases, the DAE with teacher forcing, training against fp64 autograd
through the per-trajectory walk (1e-5 of each tensor's max, the project's gate; bitwise repeatable; the fused grad_fn), the gradient
entries that have to be exact, two more activations, and the routing under fused = "require"."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import generic_cases as C
import pev_cases as P
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib, fused
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu

SOLVERS = {"Euler": nd.Euler, "Midpoint": nd.Midpoint, "RK4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
GRAD_TOL = 1e-5


def _solver(name, n=1, mode="require", kernel="auto", **kw):
    s = SOLVERS[name](substeps=n, **kw)
    s.fused, s.kernel = mode, kernel
    return s


def _factory(name, n=1):
    return lambda mode: _solver(name, n, mode)


def _yardstick_ode(name, case, n=1, tx=False):
    """the per-trajectory oracle runs for the built-in formulas, the fp64 per-trajectory walk for a tableau"""
    if name in P.ORACLE_NAME:
        return P.oracle_ode(P.ORACLE_NAME[name], case, n, tx)
    return P.ode_walk64(_solver(name, n, "off"), case, tx)


# ----------------------------------------------------------------------------- 1. the table
def _table_numpy(t, ev):
    """[T-1, B] and the duplicate flag, restated: trajectory b's clock at step k against its own list, lowest matching column"""
    t, ev = t.numpy()[:, :, 0], ev.numpy().reshape(ev.shape[0], -1)
    tab = np.full((t.shape[0] - 1, t.shape[1]), -1, dtype=np.int32)
    dup = False
    for k in range(t.shape[0] - 1):
        for b in range(t.shape[1]):
            m = np.nonzero(ev[b] == t[k, b])[0]
            if m.size:
                tab[k, b] = m[0]
            dup = dup or m.size > 1
    return tab, dup


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_event_table_equals_the_numpy_restatement(pattern, pad):
    g = torch.Generator().manual_seed(3)
    t = C.ragged_clock(P.T0, P.B0, g, pad=pad and pattern == "mixed")          # (no event time may be a -1 pad: mixed stays below row 4)
    ev = P.event_times(pattern, t)
    want, dup = _table_numpy(t, ev)
    assert not dup and np.array_equal(want, P.step_table(pattern, P.T0, P.B0).numpy())
    got = fused.event_table(t.cuda(), ev.cuda(), check_duplicates=True, per_trajectory=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (P.T0 - 1, P.B0) and np.array_equal(got.cpu().numpy(), want)
    # a strided clock view (the scripts' permute) and an event list without the trailing axis give the same table
    tb = t.permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)
    assert torch.equal(fused.event_table(tb, ev.cuda()[:, :, 0], per_trajectory=True), got)
    # the shared rule still reads trajectory 0 alone
    shared = fused.event_table(t.cuda(), ev.cuda())
    assert tuple(shared.shape) == (P.T0 - 1,) and np.array_equal(shared.cpu().numpy(), want[:, 0])


def test_event_table_duplicate_in_trajectory_17_only_and_the_smallest_grid():
    g = torch.Generator().manual_seed(4)
    t = C.ragged_clock(P.T0, P.B0, g)
    ev = P.event_times("mixed", t)
    ev[17, 0, 0] = ev[17, 1, 0] = t[1, 17, 0]
    want, dup = _table_numpy(t, ev)
    assert dup and want[1, 17] == 0
    assert np.array_equal(fused.event_table(t.cuda(), ev.cuda(), per_trajectory=True).cpu().numpy(), want)
    fused._DUP_OK.clear()
    with pytest.raises(RuntimeError, match="one trajectory"):
        fused.event_table(t.cuda(), ev.cuda(), check_duplicates=True, per_trajectory=True)
    fused.event_table(t.cuda(), ev.cuda(), check_duplicates=True)          # trajectory 0 has none: the shared rule's check passes
    t2 = torch.tensor([[[0.0]], [[0.5]]])
    one = fused.event_table(t2.cuda(), torch.tensor([[[float("nan")], [0.0]]]).cuda(), check_duplicates=True, per_trajectory=True)
    assert one.cpu().tolist() == [[1]]
    assert fused.event_table(t2[:1].cuda(), torch.zeros(1, 2, 1).cuda(), per_trajectory=True) is None          # T = 1: no step


# ----------------------------------------------------------------------------- 2. K0 forward
@functools.lru_cache(maxsize=None)
def _forward_case(shape, pattern):
    """(case, the trajectories that differ from trajectory 0): made once per shape and pattern, never modified"""
    xd, zd, hidden = C.ODE_FWD_SHAPES[shape]
    return P.sensitive_ode_case(C.ode_case(xd, zd, hidden, P.B0, P.T0, seed=11, t=P.clock()), pattern)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["Euler", "RK4", "Kutta3"])
@pytest.mark.parametrize("shape", list(C.ODE_FWD_SHAPES))
def test_k0_forward_every_form_method_and_pattern(shape, name, n):
    for pattern in P.PATTERNS:
        case, differ = _forward_case(shape, pattern)
        ref = _yardstick_ode(name, case, n)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            got = P.ode_gpu(_solver(name, n), case)
            shared = P.ode_gpu(_solver(name, n), case, per_trajectory=False)
        e = traj_rel_err(got.cpu(), ref)
        gap = P.per_traj_err(got, shared)
        print(shape, name, n, pattern, f"err {e:.3e}, gap to the shared rule: min over the {int(differ.sum())} that differ {float(gap[differ].min()):.3e}, "
              f"max over the others {float(gap[~differ].max()) if bool((~differ).any()) else 0.0:.3e}")
        assert e <= TOL_GPU, (pattern, e)
        assert bool((gap[differ] >= 100 * TOL_GPU).all()), (pattern, gap)
        assert bool((gap[~differ] <= TOL_GPU).all()), (pattern, gap)          # ... and the trajectories that share trajectory 0's steps agree


@pytest.mark.parametrize("edge", ["teacher_forced", "padded_clock", "T1", "T2", "B16", "B1", "nan_canary"])
def test_k0_forward_edge_cases(edge):
    Tn = {"T1": 1, "T2": 2}.get(edge, P.T0)
    B = {"B16": 16, "B1": 1}.get(edge, P.B0)
    tx = edge == "teacher_forced"
    base = C.ode_case(8, 2, (64, 64, 64), B, Tn, seed=12, t=P.clock(Tn, B, pad=edge == "padded_clock"))
    case = P.with_pattern(base, "mixed", 2.0)
    if edge == "nan_canary":          # a jump row no trajectory ever reads must not be read: NaN in every column that never fires
        zj = case[5].clone()
        tab = P.step_table("mixed", Tn, B)
        for b in range(B):
            for col in range(P.NE):
                if not bool((tab[:, b] == col).any()):
                    zj[b, col] = float("nan")
        case = case[:5] + (zj,)
    for name, n in (("RK4", 1), ("Euler", 2)):
        if tx and n > 1:
            continue
        if Tn == 1:
            ref = case[2][:1]
        elif edge == "nan_canary":
            ref = P.ode_walk64(_solver(name, n, "off"), case)          # (the oracle's one-trajectory runs read the same finite rows)
        else:
            ref = P.oracle_ode(P.ORACLE_NAME[name], case, n, tx)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            got = P.ode_gpu(_solver(name, n), case, tx)
        assert bool(torch.isfinite(got).all())
        e = traj_rel_err(got.cpu(), ref)
        print(edge, name, n, f"{e:.3e}")
        assert e <= TOL_GPU
    if tx:      # teacher forcing with sub-steps: the fp64 walk is the yardstick
        ref = P.ode_walk64(_solver("RK4", 2, "off"), case, True)
        assert traj_rel_err(P.ode_gpu(_solver("RK4", 2), case, True).cpu(), ref) <= TOL_GPU


@pytest.mark.parametrize("tx,ti", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", list(C.DAE_SHAPES))
def test_k0_dae_forward_with_teacher_forcing(shape, tx, ti):
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES[shape]
    base = C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=13, t=P.clock(), perturb_x_init=True)
    for pattern in P.PATTERNS if not (tx or ti) else ("mixed",):
        case, differ = P.sensitive_dae_case(base, pattern)
        for name, n in (("RK4", 1), ("Euler", 3)):
            if n > 1 and (tx or ti):
                ref = P.dae_walk64(_solver(name, n, "off"), case, tx, ti)
            else:
                ref = P.oracle_dae(P.ORACLE_NAME[name], case, n, tx, ti)
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                gx, gi = P.dae_gpu(_solver(name, n), case, tx, ti)
                sx, _ = P.dae_gpu(_solver(name, n), case, tx, ti, per_trajectory=False)
            ex, ei = traj_rel_err(gx.cpu(), ref[0]), traj_rel_err(gi.cpu(), ref[1])
            gap = P.per_traj_err(gx, sx)
            print(shape, pattern, name, n, tx, ti, f"xs {ex:.3e} is {ei:.3e} gap {float(gap[differ].min()):.3e}")
            assert ex <= TOL_GPU and ei <= TOL_GPU
            if not tx:          # (with dataset x every step restarts from the data: a jump moves one interval only, the gate is the oracle's)
                assert bool((gap[differ] >= 100 * TOL_GPU).all())


def test_k0_dae_events_without_dataset_x():
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES["x5z4v6i6"]
    case = C.without_x(P.with_pattern(C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=14, t=P.clock()), "blocks", 2.0, dae=True))
    ref = P.oracle_dae("rk4", case)
    gx, gi = P.dae_gpu(_solver("RK4"), case)
    assert gx.shape == (P.T0, P.B0, xd) and traj_rel_err(gx.cpu(), ref[0]) <= TOL_GPU and traj_rel_err(gi.cpu(), ref[1]) <= TOL_GPU


# ----------------------------------------------------------------------------- 3. training
def _check_ode_training(name, n, case, tx=False, what=""):
    G, = C.cotangents(21, case[2].shape)
    ref_xs, ref = P.ode_train(_factory(name, n), case, G, "cpu", tx)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = P.ode_train(_factory(name, n), case, G, "cuda", tx)
        _, again = P.ode_train(_factory(name, n), case, G, "cuda", tx)
    C.judge_ode_training(ref, got, again, xs, ref_xs, "_FusedOdePev", GRAD_TOL, what)
    return got, ref


def _check_dae_training(name, n, case, tx=False, ti=False, what=""):
    G, Gi = C.cotangents(22, (case[2].shape[0], case[2].shape[1], case[7].shape[-1]), case[6].shape)
    rx, ri, ref = P.dae_train(_factory(name, n), case, G, Gi, "cpu", tx, ti)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, is_, got = P.dae_train(_factory(name, n), case, G, Gi, "cuda", tx, ti)
        _, _, again = P.dae_train(_factory(name, n), case, G, Gi, "cuda", tx, ti)
    C.judge_dae_training(ref, got, again, (xs, is_), (rx, ri), "_FusedDaePev", GRAD_TOL, what)
    return got, ref


# one shape per K5 path, as generic_cases.K5_ODE_SHAPES' comment names them: register, streamed with LDS accumulators, streamed with
# global accumulators (hidden 128), staged (132 input columns; with z_dim 2, not 0 as there: a call without z has no events)
K5_ODE_PATHS = {"register": C.K5_ODE_SHAPES[0], "streamed": C.K5_ODE_SHAPES[5], "global": C.K5_ODE_SHAPES[3], "staged": (42, 2, 40, 2)}
assert (K5_ODE_PATHS["register"], K5_ODE_PATHS["streamed"], K5_ODE_PATHS["global"]) == ((8, 2, 64, 3), (20, 2, 64, 3), (8, 2, 128, 3))
assert C.K5_ODE_SHAPES[11] == (44, 0, 40, 2)          # the list's staged entry: 3 (44 + 0) = 132 = 3 (42 + 2) input columns
TRAIN_GRID = [(name, n) for name in ("Euler", "Heun2", "RK4Classic") for n in (1, 3)]


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("path", list(K5_ODE_PATHS))
def test_k5_ode_training_per_path(path, name, n):
    xd, zd, h, nl = K5_ODE_PATHS[path]
    base = C.ode_case(xd, zd, (h,) * nl, P.B0, P.T0, seed=23, t=P.clock())
    for pattern in ("mixed", "blocks"):
        _check_ode_training(name, n, P.with_pattern(base, pattern, 2.0), what=f"{path} {pattern}")


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("shape", list(C.K5_DAE_SHAPES))
def test_k5_dae_training_every_shape(shape, name, n):
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES[shape]
    base = C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=24, t=P.clock(), perturb_x_init=True)
    for pattern in ("mixed", "blocks"):
        _check_dae_training(name, n, P.with_pattern(base, pattern, 2.0, dae=True), what=f"{shape} {pattern}")


@pytest.mark.parametrize("n", [1, 3])
def test_k5_teacher_forced_training_elu1(n):
    ode = P.with_pattern(C.ode_case(8, 2, (64, 64, 64), P.B0, P.T0, seed=25, t=P.clock()), "mixed", 2.0)
    _check_ode_training("RK4Classic", n, ode, tx=True, what="ode tx")
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = P.with_pattern(C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=26, t=P.clock(), perturb_x_init=True), "mixed", 2.0, dae=True)
    for tx, ti in ((True, False), (False, True), (True, True)):
        _check_dae_training("Euler", n, dae, tx, ti, what=f"dae tx={tx} ti={ti}")


def test_exact_gradient_entries():
    """grad z_jump[b, e] (and v_jump) is exactly 0 where event e of b never fires -- ODE and DAE; the ODE's grad z[k, b] is exactly 0 where b
    hits at k."""
    tab = P.step_table("mixed", P.T0, P.B0)
    fires = torch.stack([(tab == col).any(0) for col in range(P.NE)], 1)          # [B, nE]
    ode = P.with_pattern(C.ode_case(8, 2, (64, 64, 64), P.B0, P.T0, seed=27, t=P.clock()), "mixed", 2.0)
    got, _ = _check_ode_training("RK4Classic", 1, ode)
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = P.with_pattern(C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=28, t=P.clock(), perturb_x_init=True), "mixed", 2.0, dae=True)
    gd, _ = _check_dae_training("RK4Classic", 1, dae)
    for zj in (got["zj"], gd["zj"], gd["vj"]):
        zj = zj.cpu()
        assert bool((zj[~fires] == 0).all()) and bool((zj[fires].abs().amax(-1) > 0).all())
    # (the ODE's rows alone: a DAE's z[k] | v[k] also feed the head at grid point k, whose output carries a cotangent of its own)
    z = got["z"].cpu()
    assert bool((z[:-1][tab >= 0] == 0).all()) and bool((z[:-1][tab < 0].abs().amax(-1) > 0).all())


def test_head_weight_gradient_with_hits_in_one_workgroup_only():
    """blocks without trajectory 32's event: only trajectories 16-31 -- one workgroup -- have a hit (step 1).  The event-time head runs there
    alone; were the non-hit columns of a workgroup not masked out of its VJP (or the head run elsewhere), the AE's weight gradient would
    be off.  Also B = 48 with hits in 16-31: a workgroup behind the one with the hits."""
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    for B in (32, 48):
        base = C.dae_case(xd, zd, vd, idim, dh, ah, B, P.T0, seed=29, t=P.clock(P.T0, B), perturb_x_init=True)
        case = P.with_pattern(base, "blocks", 2.0, dae=True)          # (B <= 32: trajectory 32 does not exist)
        if B == 48:
            ev = case[9].clone()
            ev[32:] = float("nan")
            ev[20, 0, 0] = float("nan")          # ... and one column of the hit workgroup without a hit
            case = case[:9] + (ev,) + case[10:]
        got, ref = _check_dae_training("Euler", 1, case, what=f"B={B}")
        for k in ref:
            if k.startswith("ae"):
                C.close(got[k], ref[k], f"B={B} {k}", GRAD_TOL)


@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_other_activations(act):
    ode = P.with_pattern(C.ode_case(8, 2, (64, 64, 64), P.B0, P.T0, seed=30, t=P.clock(), act=act), "mixed", 2.0)
    ref = P.ode_walk64(_solver("RK4", 1, "off"), ode)
    assert traj_rel_err(P.ode_gpu(_solver("RK4"), ode).cpu(), ref) <= TOL_GPU
    _check_ode_training("Heun2", 2, ode, what=act.__name__)
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = P.with_pattern(C.dae_case(xd, zd, vd, idim, dh, ah, P.B0, P.T0, seed=31, t=P.clock(), de_act=act, ae_act=act, perturb_x_init=True), "blocks", 2.0,
                         dae=True)
    _check_dae_training("Euler", 1, dae, what=act.__name__)


# ----------------------------------------------------------------------------- 4. routing
def test_routing_under_require():
    ode = P.with_pattern(C.ode_case(8, 2, (64, 64, 64), P.B0, P.T0, seed=32, t=P.clock()), "mixed", 2.0)
    for kernel in ("wave", "tile", "mfma", "wide"):
        with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
            P.ode_gpu(_solver("RK4", kernel=kernel), ode)
        s = _solver("RK4", mode="auto", kernel=kernel)
        with pytest.warns(RuntimeWarning, match="not fusable"):
            out = P.ode_gpu(s, ode)
        assert traj_rel_err(out.cpu(), P.oracle_ode("rk4", ode)) <= TOL_GPU          # the walk, per trajectory
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        P.ode_gpu(_solver("RK4", externals="linear"), ode)
    # kernel "generic" runs K0; an event object without events is the event-less call, on whatever kernel that takes
    assert traj_rel_err(P.ode_gpu(_solver("RK4", kernel="generic"), ode).cpu(), P.oracle_ode("rk4", ode)) <= TOL_GPU
    none = ode[:4] + (None, None)
    a = P.ode_gpu(_solver("RK4", kernel="wave"), none)
    b = C.ode_gpu(_solver("RK4", kernel="wave"), *none)
    assert torch.equal(a, b)
    # ... the one-launch encoded forward of a direct_encode model included; with events the model takes the rows + solver route
    from py_psnode_amd import models
    torch.manual_seed(33)
    m = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4()).cuda()
    m.event.per_trajectory = True
    t, x, z = (q.permute(1, 0, 2).contiguous().cuda() for q in ode[1:4])          # the models take [B, T, D]
    with torch.no_grad():
        assert m._forward_encoded(t, x, z, None, None) is not None
        assert m._forward_encoded(t, x, z, ode[4].cuda(), ode[5].cuda()) is None
