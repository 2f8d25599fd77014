"""Four-point Lagrange interpolation of the external inputs (solver.externals = "lagrange"), host side (no GPU): the stencil helper against
a loop restatement, polynomial reproduction and exact nodes of the walk's interpolant, the callback walk against a stand-alone fp64
restatement (tests/externals_lagrange_cases.py), its observed order in the grid and its floor in the number of sub-steps next to
"linear"'s, teacher forcing, and the additive C ABI (the nine _lag entry points: argument checks from the dims alone)."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn

import capi_args as A
import externals_lagrange_cases as G
import generic_cases as C
from capi_args import R
from capi_args import sub as _sub
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd
from py_psnode_amd.neural_dae.my_solvers import _LagWalk

SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
LAG_EXPORTS = ("psnode_ode_integrate_lag_supported", "psnode_ode_integrate_lag_f32", "psnode_dae_integrate_lag_supported",
               "psnode_dae_integrate_lag_f32", "psnode_ode_backward_lag_supported", "psnode_ode_backward_lag_f32",
               "psnode_dae_backward_lag_supported", "psnode_dae_backward_lag_workspace_size", "psnode_dae_backward_lag_f32")
B0, T0 = 5, 12
EV = G.EV_ROWS


def _solver(name, n=1, externals="lagrange"):
    s = SOLVERS[name](substeps=n, externals=externals)
    s.fused = "off"
    return s


def _whole(Tn, B=3, dtype=torch.float32):
    return (torch.arange(Tn, dtype=dtype) * 0.125).view(Tn, 1, 1).repeat(1, B, 1)


# ----------------------------------------------------------------------------- 1. the stencil helper vs the loop restatement
def _table(t, ev_steps=()):
    Tn = t.shape[0]
    ev = None
    if ev_steps:
        ev = torch.full((Tn - 1,), -1, dtype=torch.int32)
        for e, k in enumerate(ev_steps):
            ev[k] = e
    return fused.lagrange_stencils(t, ev)


def _same(t, ev_steps=()):
    tab = _table(t, ev_steps)
    codes, pieces = G.stencils_brute(t, ev_steps)
    assert tab.dtype == torch.int8 and tuple(tab.shape) == (t.shape[0] - 1, t.reshape(t.shape[0], -1).shape[1])
    assert tab.tolist() == codes, (tab.tolist(), codes)
    return tab, pieces


@pytest.mark.parametrize("Tn", range(1, 10))
def test_stencils_of_whole_clocks(Tn):
    t = _whole(Tn)
    if Tn == 1:
        assert tuple(fused.lagrange_stencils(t).shape) == (0, 3)
        return
    tab, pieces = _same(t)
    assert pieces[0] == [(0, Tn - 1)]
    q = min(4, Tn)
    assert [((c >> 2) & 7) for c in tab[:, 0].tolist()] == [q] * (Tn - 1)
    assert [c & 3 for c in tab[:, 0].tolist()] == [min(max(k - 1, 0), Tn - q) * -1 + k for k in range(Tn - 1)]


def test_stencils_with_events_a_late_event_padding_and_shared_clocks():
    t = _whole(12)
    tab, pieces = _same(t, EV)
    assert pieces[0] == [(0, 2), (2, 3), (3, 6), (6, 11)]                       # pieces of 3, 2, 4 and 6 nodes
    assert [((c >> 2) & 7) for c in tab[:, 0].tolist()] == [3, 3, 2, 4, 4, 4, 4, 4, 4, 4, 4]
    assert [c & 3 for c in tab[:, 0].tolist()] == [0, 1, 0, 0, 1, 2, 0, 1, 1, 1, 2]
    _, pieces = _same(t, (10,))                                                  # an event at step T - 2: a two-node piece at the end
    assert pieces[0] == [(0, 10), (10, 11)]
    g = torch.Generator().manual_seed(3)
    tr = C.ragged_clock(12, 7, g, pad=True)                                      # trajectories 2 and 5 end in two -1 rows
    tab, pieces = _same(tr, EV)
    assert pieces[2][-3:] == [(6, 9), (9, 10), (10, 11)] and pieces[1] == pieces[0]
    assert (tab[9:, 2] == fused.stencil_code(0, 2)).all()                        # the invalid intervals: two-node pieces of their own
    assert int((tab[8, 2] >> 2) & 7) == 4 and int(tab[8, 2] & 3) == 2            # no padded row in a valid interval's stencil: 6 .. 9
    shared = _table(t[:, :1], EV)                                                # one shared clock against per-trajectory copies of it
    assert tuple(shared.shape) == (11, 1) and torch.equal(shared.expand(11, 3), _table(t, EV))
    assert torch.equal(_table(t[:, :, 0], EV), _table(t, EV))


# ----------------------------------------------------------------------------- 2. polynomial reproduction, exact nodes
def _walk_of(z, ev_steps=(), zj=None, t=None):
    Tn, B = z.shape[0], z.shape[1]
    t = _whole(Tn, B, z.dtype) if t is None else t
    if ev_steps:
        ev = nd.ODE_Event()
        ev.set_event(t[list(ev_steps)].permute(1, 0, 2).contiguous(), zj)
        return _LagWalk(t, ev.event_fn, ev.jump_change_fn, (z,))
    return _LagWalk(t, None, None, (z,))


@pytest.mark.parametrize("Tn,deg", [(9, 3), (4, 3), (3, 2), (2, 1)])
def test_polynomials_up_to_the_piece_s_degree_are_reproduced_fp64(Tn, deg):
    g = torch.Generator().manual_seed(Tn)
    coef = torch.randn(deg + 1, 2, 3, generator=g, dtype=torch.float64)                    # [power, B, D]
    p = lambda s: sum(coef[d] * s ** d for d in range(deg + 1))
    z = torch.stack([p(float(k)) for k in range(Tn)])
    w = _walk_of(z)
    worst = 0.0
    for name in ("RK4Classic", "Kutta3", "rk4"):
        a, _ = G.TABLEAUS[name]
        cs = [sum(row) for row in a] + [1.0]
        for n in (1, 3):
            for k in range(Tn - 1):
                for j in range(n):
                    at = w.ext_at(k, j, n)
                    for c in cs:
                        worst = max(worst, float((at(c)[0] - p(k + (j + c) / n)).abs().max()))
    print(Tn, deg, f"{worst:.3e}")
    assert worst <= 1e-13 * max(1.0, float(z.abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_theta_0_and_1_return_the_node_bit_for_bit(dtype):
    g = torch.Generator().manual_seed(9)
    z = torch.randn(12, 4, 3, generator=g, dtype=dtype)
    zj = torch.randn(4, len(EV), 3, generator=g, dtype=dtype)
    for ev_steps in ((), EV):
        w = _walk_of(z, ev_steps, zj)
        for k in range(11):
            left = zj[:, ev_steps.index(k)] if k in ev_steps else z[k]
            for n in (1, 3, 7):
                assert torch.equal(w.ext_at(k, 0, n)(0.0)[0], left), (k, n)
                assert torch.equal(w.ext_at(k, n - 1, n)(1.0)[0], z[k + 1]), (k, n)          # never jumped, even where k + 1 is an event step


# ----------------------------------------------------------------------------- 3. the walk vs the stand-alone restatement
def _rel64(y, ref):
    return float((y - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["midpoint", "rk4", "Kutta3", "RK4Classic"])
def test_ode_walk_equals_the_stand_alone_restatement_fp64(name, n):
    t = C.padded(C.dyadic_clock(T0, B0, n, dtype=torch.float64) * 1.3)
    de, _, x, z, ev, zj = C.ode_case(6, 2, (32, 32), B0, T0, seed=60 + n, t=t, ev_rows=EV)
    de, x, z, zj = de.double(), x.double(), z.double(), zj.double()
    a0 = torch.cat((x[0], z[0]), -1)
    a, b = G.TABLEAUS[name]
    f = lambda xx, w: de(t0=None, xt=xx, zt=w[0], all_initial=a0)
    with torch.no_grad():
        got = C.run_ode(_solver(name, n), de, t, x, z, a0, ev, zj)
        ref = G.ode_lagrange_reference(f, a, b, t, x[0], z, n, EV, zj)
        lin = C.run_ode(_solver(name, n, "linear"), de, t, x, z, a0, ev, zj)
        got_tx = C.run_ode(_solver(name, n), de, t, x, z, a0, ev, zj, tx=True)
        ref_tx = G.ode_lagrange_reference(f, a, b, t, x[0], z, n, EV, zj, x_true=x)
    e = _rel64(got, ref)
    print(name, n, f"{e:.3e}", f"linear differs by {_rel64(lin, ref):.3e}", f"teacher-forced {_rel64(got_tx, ref_tx):.3e}")
    assert e <= 1e-12 and _rel64(got_tx, ref_tx) <= 1e-12 and _rel64(lin, ref) > 1e-4


@pytest.mark.parametrize("no_x", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["midpoint", "rk4", "Kutta3", "RK4Classic"])
def test_dae_walk_equals_the_restated_de_step_with_the_package_s_head_fp64(name, n, no_x):
    """The DE step restated; i comes from the package's head module: at grid point 0, at an event (jumped rows), in front of every sub-step
    j >= 1 at the interpolant of theta = j / n, and at grid point k + 1 with rows k + 1."""
    t = C.dyadic_clock(T0, B0, n, dtype=torch.float64) * 1.3
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), B0, T0, seed=70 + n, t=t, ev_rows=EV)
    de, ae = de.double(), ae.double()
    x, z, v, i, x_init, a0, zj, vj = (q.double() for q in (x, z, v, i, x_init, a0, zj, vj))
    a, b = G.TABLEAUS[name]
    codes, _ = G.stencils_brute(t, EV)
    with torch.no_grad():
        gx, gi = C.run_dae(_solver(name, n), de, ae, t, x[:, :, :0] if no_x else x, z, v, i, x_init, a0, ev, zj, vj)
        cur = x_init
        ci = ae(xt=cur, zt=z[0], vt=v[0], all_initial=a0)
        rx, ri = [cur], [ci]
        for k in range(T0 - 1):
            offs, qs, nodes = G.interval_nodes((z, v), (zj, vj), EV, codes, k)
            ext = lambda th: G.ext_at_theta(offs, qs, nodes, th)
            if k in EV:
                ci = ae(xt=cur, zt=zj[:, EV.index(k)], vt=vj[:, EV.index(k)], all_initial=a0)
            h = (t[k + 1] - t[k]) / n
            for j in range(n):
                if j > 0:
                    w = ext(j / n)
                    ci = ae(xt=cur, zt=w[0], vt=w[1], all_initial=a0)
                f = lambda xx, w, ci=ci: de(t0=None, xt=xx, zt=w[0], vt=w[1], it=ci, all_initial=a0)
                cur = G.rk_step_lagrange(f, a, b, h, cur, ext, j, n)
            ci = ae(xt=cur, zt=z[k + 1], vt=v[k + 1], all_initial=a0)
            rx.append(cur)
            ri.append(ci)
        rx, ri = torch.stack(rx), torch.stack(ri)
    ex, ei = _rel64(gx, rx), _rel64(gi, ri)
    print(name, n, no_x, f"{ex:.3e} {ei:.3e}")
    assert ex <= 1e-12 and ei <= 1e-12


@pytest.mark.parametrize("n", [1, 3])
def test_teacher_forced_intervals_start_from_their_dataset_row_only(n):
    t = C.dyadic_clock(T0, B0, n)
    de, _, x, z, ev, zj = C.ode_case(6, 2, (32, 32), B0, T0, seed=31, t=t, ev_rows=EV)
    a0 = torch.cat((x[0], z[0]), -1)
    s = _solver("rk4", n)
    with torch.no_grad():
        base = C.run_ode(s, de, t, x, z, a0, ev, zj, tx=True)
        for k in range(T0 - 1):
            x2 = x + 1.0
            x2[k] = x[k]                     # every row but x[k] perturbed (the running state of every other interval with them)
            assert torch.equal(C.run_ode(s, de, t, x2, z, a0, ev, zj, tx=True)[k + 1], base[k + 1]), k
        free = C.run_ode(s, de, t, x, z, a0, ev, zj)
    assert not torch.equal(free[2], base[2])
    # DAE: with input_true_x the running state never enters an interval; with input_true_i no head is evaluated inside one
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), B0, T0, seed=33, t=t, ev_rows=EV)
    calls = []
    hook = ae.register_forward_hook(lambda *_: calls.append(1))
    with torch.no_grad():
        xs, is_ = C.run_dae(s, de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, tx=True, ti=True)
        n_ti = len(calls)
        xs2, _ = C.run_dae(s, de, ae, t, x, z, v, i, x_init + 1.0, a0, ev, zj, vj, tx=True, ti=True)
        calls.clear()
        C.run_dae(s, de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj)
        n_free = len(calls)
    hook.remove()
    assert torch.equal(xs[1:], xs2[1:])
    assert n_ti == T0 + len(EV)                                    # one head per grid point, one per event
    assert n_free == T0 + len(EV) + (T0 - 1) * (n - 1)             # ... and one in front of every sub-step behind an interval's first


def test_per_trajectory_events_next_to_lagrange_are_refused_by_the_walk():
    t = C.dyadic_clock(6, 3, 1)
    de, _, x, z, ev, zj = C.ode_case(4, 2, (8,), 3, 6, seed=3, t=t, ev_rows=(1,))
    event = nd.ODE_Event(per_trajectory=True)
    event.set_event(ev, zj)
    with pytest.raises(ValueError, match="lagrange"):
        _solver("rk4").integrate_ODE(de, t, x, z, torch.cat((x[0], z[0]), -1), event.event_fn, event.jump_change_fn)


# ----------------------------------------------------------------------------- 4. observed order and floor, fp64: smooth sampled forcing
def _forced_problem(points, B=3):
    """The linear test's problem: Tanh DE_Func, x 3 / z 2 / hidden 16 x 16, z(t) = 0.5 sin(3 t + phi) sampled on `points` points of [0, 1]."""
    torch.manual_seed(5)
    de = models.DE_Func(5, (16, 16), 3, activation=nn.Tanh).double()
    g = torch.Generator().manual_seed(6)
    x0 = 0.5 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    phi = torch.rand(B, 2, generator=g, dtype=torch.float64) * 3.0
    t = torch.linspace(0.0, 1.0, points, dtype=torch.float64).view(-1, 1, 1).repeat(1, B, 1)
    z = 0.5 * torch.sin(3.0 * t + phi.unsqueeze(0))
    x = torch.zeros(points, B, 3, dtype=torch.float64)
    x[0] = x0
    return de, t, x, z, torch.cat((x0, z[0]), -1), phi


def _run_forced(solver, points):
    de, t, x, z, a0, _ = _forced_problem(points)
    solver.fused = "off"
    with torch.no_grad():
        return solver.integrate_ODE(de, t, x, z, a0)


_FINE = 4096


def _yardstick():
    """Classic RK4 on 4097 points with z(t) evaluated analytically at every stage: stand-alone, no interpolation anywhere."""
    if not hasattr(_yardstick, "xs"):
        de, t, x, z, a0, phi = _forced_problem(_FINE + 1)
        zt = lambda s: 0.5 * torch.sin(3.0 * s + phi)
        f = lambda s, xx: de(t0=None, xt=xx, zt=zt(s), all_initial=a0)
        h, cur, xs = 1.0 / _FINE, x[0], [x[0]]
        with torch.no_grad():
            for k in range(_FINE):
                s = k * h
                k1 = f(s, cur)
                k2 = f(s + h / 2, cur + h / 2 * k1)
                k3 = f(s + h / 2, cur + h / 2 * k2)
                k4 = f(s + h, cur + h * k3)
                cur = cur + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
                xs.append(cur)
        _yardstick.xs = torch.stack(xs)
    return _yardstick.xs


def _err(solver, points):
    return float((_run_forced(solver, points) - _yardstick()[::_FINE // (points - 1)]).abs().max())


def test_observed_order_in_the_grid_is_fourth_and_twenty_times_under_linear():
    """RK4Classic on grids of 9 / 17 / 33 / 65 points against the analytic-forcing yardstick.  Measured in fp64 (the table of DESIGN.md):
    linear 4.48e-4 / 1.12e-4 / 2.80e-5 / 6.99e-6 (orders 2.00), lagrange 7.65e-6 / 6.33e-7 / 4.29e-8 / 2.76e-9 (orders 3.59 / 3.88 / 3.96),
    58 / 177 / 651 / 2532 times lower."""
    errs = {ext: [_err(nd.RK4Classic(externals=ext), p) for p in (9, 17, 33, 65)] for ext in ("linear", "lagrange")}
    orders = {ext: [math.log2(e[k] / e[k + 1]) for k in range(3)] for ext, e in errs.items()}
    print("errors", errs, "orders", orders)
    assert min(orders["lagrange"][1:]) >= 3.5, orders                      # each doubling from 17 points on
    assert all(g <= l / 20 for g, l in zip(errs["lagrange"], errs["linear"])), errs


def test_the_floor_on_nine_points_stays_twenty_times_under_linear_s_for_every_substeps():
    for n in (1, 4, 16):
        lin, lag = _err(nd.RK4Classic(substeps=n, externals="linear"), 9), _err(nd.RK4Classic(substeps=n, externals="lagrange"), 9)
        print("substeps", n, "linear", lin, "lagrange", lag, "ratio", lin / lag)
        assert lag <= lin / 20, (n, lin, lag)


# ----------------------------------------------------------------------------- 5. C ABI, dims only; routing; the constructor
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))
_supported, _call = G.supported, G.call
ST = 256      # a stencil "pointer": the checks never follow it


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    for name in LAG_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for stem, _, n_act in ENTRIES:
        lin_q, lin_c = getattr(lib, f"psnode_{stem}_lin_supported").argtypes, getattr(lib, f"psnode_{stem}_lin_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_lag_supported").argtypes == lin_q + [ctypes.c_void_p]
        assert getattr(lib, f"psnode_{stem}_lag_f32").argtypes == lin_c[:-3] + [ctypes.c_void_p] + lin_c[-3:]
    assert lib.psnode_dae_backward_lag_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert lib.psnode_dae_backward_lag_workspace_size.restype is ctypes.c_size_t
    assert fused.FAMILIES["lag"] == fused.FAMILIES["lin"]._replace(stencil=True) and fused.stencil_code(2, 4) == 18


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_lag_argument_checks_in_the_lin_family_s_order(stem, make, n_act):
    lib = _lib.load()
    lin_s = lambda a, tb, sb, act=None: A.supported(lib, stem, a, n_act, tb, sb, act, family="lin")
    lin_c = lambda a, tb, sb, act=None: A.call(lib, stem, a, n_act, tb, sb, act, family="lin")
    tab = R(nd.Kutta3().method.abi())
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    unknown = _lib.ActF32()
    unknown.kind = 17
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    for st in (None, ST):                                    # a NULL table is one piece 0 .. T - 1: accepted everywhere
        for tb in (None, tab):
            assert _supported(lib, stem, make(), n_act, tb, None, None, st) == 1 and _call(lib, stem, make(), n_act, tb, None, None, st) == -1
            for n in (0, -3, 1025):
                assert _call(lib, stem, make(), n_act, tb, _sub(n), None, st) == -2 and _supported(lib, stem, make(), n_act, tb, _sub(n), None, st) == 0
            for n in (1, 2, 3, 1024):
                assert _supported(lib, stem, make(), n_act, tb, _sub(n), None, st) == 1
                assert _supported(lib, stem, make(kernel=_lib.KERNEL_GENERIC), n_act, tb, _sub(n), None, st) == 1
                assert _call(lib, stem, make(), n_act, tb, _sub(n), None, st) == -1          # as far as the pointer checks, nothing launched
                for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                    assert _supported(lib, stem, make(kernel=kernel), n_act, tb, _sub(n), None, st) == 0
                    assert _call(lib, stem, make(kernel=kernel), n_act, tb, _sub(n), None, st) == -5
            assert _call(lib, stem, None, n_act, tb, _sub(2), None, st) == -1          # NULL args
            assert _call(lib, stem, None, n_act, tb, None, None, st) == -1
        for sb in (None, _sub(1), _sub(2)):
            assert _call(lib, stem, make(method=77), n_act, None, sb, None, st) == -3 and _supported(lib, stem, make(method=77), n_act, None, sb, None, st) == 0
            assert _supported(lib, stem, make(method=77), n_act, tab, sb, None, st) == 1
        assert _call(lib, stem, make(), n_act, R(bad), _sub(2), None, st) == -3 and _supported(lib, stem, make(), n_act, R(bad), _sub(2), None, st) == 0
        assert _call(lib, stem, make(), n_act, tab, _sub(2), R(unknown), st) == -3
        assert _supported(lib, stem, make(), n_act, None, _sub(2), tanh, st) == 1
        # a call wrong in several ways: the status is the _lin family's
        for a, tb, sb, act in ((make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(0), R(unknown)), (make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(2), R(unknown)),
                               (make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(2), None), (make(kernel=_lib.KERNEL_MFMA), R(bad), _sub(2), None),
                               (None, R(bad), _sub(2), None), (make(kernel=_lib.KERNEL_MFMA), tab, _sub(2), None)):
            assert _call(lib, stem, a, n_act, tb, sb, act, st) == lin_c(a, tb, sb, act)
            if a is not None:
                assert _supported(lib, stem, a, n_act, tb, sb, act, st) == lin_s(a, tb, sb, act)


def test_side_outputs_teacher_forced_activations_and_a_missing_x_sub_are_refused():
    lib = _lib.load()
    sub = _sub(3)
    a = _ode_args()
    a.save_act = a.save_xstage = 256
    assert _supported(lib, "ode_integrate", a, 1, None, sub) == 0 and _call(lib, "ode_integrate", a, 1, None, sub) == -5
    d = _dae_args()
    d.save_act = d.save_xstage = d.save_ae_act = 256
    assert _supported(lib, "dae_integrate", d, 2, None, sub) == 0 and _call(lib, "dae_integrate", d, 2, None, sub) == -5
    b = _ode_bwd_args()
    b.saved_act = b.saved_xstage = 256
    assert _supported(lib, "ode_backward", b, 1, None, sub) == 0 and _call(lib, "ode_backward", b, 1, None, sub) == -5
    e = _dae_bwd_args()
    e.base.saved_act = 256
    assert _supported(lib, "dae_backward", e, 2, None, sub) == 0 and _call(lib, "dae_backward", e, 2, None, sub) == -5
    assert lib.psnode_dae_backward_lag_workspace_size(R(e), None, None, None, R(sub), None) == 0
    assert lib.psnode_dae_backward_lag_workspace_size(R(_dae_bwd_args()), None, None, None, R(sub), ST) > 0
    assert lib.psnode_dae_backward_lag_workspace_size(R(_dae_bwd_args()), None, None, None, None, None) == \
        lib.psnode_dae_backward_lin_workspace_bytes(R(_dae_bwd_args()), None, None, None, None)
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    tfo = _ode_bwd_args(flags=_lib.FLAG_INPUT_TRUE_X)
    assert _supported(lib, "ode_backward", tfo, 1, None, sub) == 1
    assert _supported(lib, "ode_backward", tfo, 1, None, sub, tanh) == 0 and _call(lib, "ode_backward", tfo, 1, None, sub, tanh) == -5
    for flags in (1, 2, 3):
        tfd = _dae_bwd_args(flags=flags)
        assert _supported(lib, "dae_backward", tfd, 2, None, sub) == 1
        assert _supported(lib, "dae_backward", tfd, 2, None, sub, tanh) == 0 and _call(lib, "dae_backward", tfd, 2, None, sub, tanh) == -5
        one = _dae_bwd_args(flags=flags)
        one.base.T = 1
        assert _call(lib, "dae_backward", one, 2, None, sub) == -2
    # a backward call with every other pointer in place and no x_sub: PSNODE_ERR_NULL before the workspace is looked at; one sub-step needs none
    b = _ode_bwd_args()
    for l in range(4):
        b.de.weight[l] = b.de.bias[l] = 256
    b.t.ptr = b.z.ptr = b.all_initial = b.xs = b.grad_xs = b.grad_x0 = b.grad_all_initial = b.grad_params = 256
    assert _call(lib, "ode_backward", b, 1, None, _sub(2)) == -1
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256)) == -4          # with one: as far as the workspace check
    assert _call(lib, "ode_backward", b, 1, None, _sub(1)) == -4 and _call(lib, "ode_backward", b, 1, None, None, None, ST) == -4
    e = _dae_bwd_args()
    q = e.base
    for m in (q.de, q.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
    q.grad_params_de = q.grad_params_ae = 256
    assert _call(lib, "dae_backward", e, 2, None, _sub(2)) == -1
    assert _call(lib, "dae_backward", e, 2, None, _sub(2, 256)) == -4
    assert _call(lib, "dae_backward", e, 2, None, None) == -4


def test_supported_answers_for_the_lagrange_build_s_own_lds_fit():
    """K0 keeps 4 (z_dim + v_dim) more rows of LDS in this build where "lin" keeps one, K5 eight where "lin" keeps three: along a growing
    z_dim the _lag query says no before the _lin query does, and never the other way round -- in both directions."""
    lib = _lib.load()
    for stem, make in (("ode_integrate", _ode_args), ("ode_backward", _ode_bwd_args)):
        first_lag = first_lin = None
        for zd in range(32, 660, 4):
            a = make(kernel=_lib.KERNEL_GENERIC, xd=8, zd=zd, hidden=32)
            lag, lin = _supported(lib, stem, a, 1, None, _sub(2)), A.supported(lib, stem, a, 1, None, _sub(2), family="lin")
            assert not (lag and not lin), (stem, zd)
            if not lag and first_lag is None:
                first_lag = zd
            if not lin and first_lin is None:
                first_lin = zd
        print(stem, "first z_dim refused: lag", first_lag, "lin", first_lin)
        assert first_lag is not None and first_lin is not None and first_lag < first_lin, (stem, first_lag, first_lin)


_layers = A.hip_layers


def test_python_predicates_refusals_and_the_constructor():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    lag = dict(externals="lagrange")
    assert fused.EXTERNALS == ("hold", "linear", "lagrange")
    assert fused.is_linear("lagrange") and fused.is_lagrange("lagrange") and not fused.is_lagrange("linear") and not fused.is_lagrange("hold")
    for method in ("euler", "rk4", nd.Kutta3().method):
        for sub in (1, 2, 7):
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, substeps=sub, **lag)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", act=tanh, substeps=sub, **lag)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, substeps=sub, **lag)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True, substeps=sub, **lag)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, substeps=sub, **lag)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), substeps=sub, **lag)
            for tx, ti in ((True, False), (False, True), (True, True)):
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **lag)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti,
                                                           substeps=sub, **lag)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 1, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **lag)
            for kernel in ("wave", "tile", "mfma", "wide"):
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, substeps=sub, **lag)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel, substeps=sub, **lag)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, substeps=sub, **lag)
            assert fused.ode_backward_supported(method, ode01, 8, 2, "generic", substeps=sub, **lag)
            assert fused.dae_backward_supported(method, de, ae, 8, 2, 2, 2, kernel="generic", substeps=sub, **lag)
            assert fused.ode_save_hidden(method, ode01, 8, 2, substeps=sub, **lag) == 0
            assert fused.dae_save_hidden(method, de, ae, 8, 2, 2, 2, substeps=sub, **lag) == 0
    for bad in ("cubic", "", None, 1, "Linear", "Lagrange", "LAGRANGE"):
        with pytest.raises(ValueError, match="externals must be one of"):
            autograd.ode_training_supported("rk4", ode01, 8, 2, 50, 33, externals=bad)
    with pytest.raises(_lib.UnsupportedShapeError, match="lagrange"):
        fused.dae_backward_wide_supported("rk4", de, ae, 8, 2, 2, 2, **lag)
    with pytest.raises(_lib.UnsupportedShapeError, match="lagrange"):
        fused.latent_backward_wide("rk4", ode01, None, None, None, None, None, torch.zeros(2, 1, 16), None, None, None, saved=(), **lag)
    opts = lambda substeps, externals, **kw: fused.GenericOpts.of("rk4", (None,), substeps, externals, **kw)
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='lagrange'"):
        opts(1, "lagrange").require_plain("a specialised entry")
    with pytest.raises(ValueError):
        opts(1, "cubic")
    for kernel, save in (("wave", False), ("mfma", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="externals='lagrange'"):
            opts(1, "lagrange").require_generic("x", kernel, save)
    opts(1, "lagrange").require_generic("x", "generic", False)
    o = opts(5, "lagrange")
    assert o.family == "lag" and opts(1, "lagrange").family == "lag" and opts(5, "linear").family == "lin" and o.takes.stencil
    args = o.c_args()
    assert len(args) == 4 and args[-2]._obj.substeps == 5 and args[-1].value is None          # act, tableau, sub-steps, the (NULL) table
    tab = torch.zeros(3, 2, dtype=torch.int8)
    assert o.c_args(stencil=tab)[-1].value == tab.data_ptr() and len(opts(5, "linear").c_args()) == 3
    # the refusals next to segments, per-trajectory events and Adams-Bashforth: "linear"'s, naming the value
    assert opts(1, "lagrange", segment=4).family == "none" and opts(1, "lagrange", per_trajectory=True).family == "none"
    with pytest.raises(_lib.UnsupportedShapeError, match="segment=4.*externals='lagrange'"):
        opts(1, "lagrange", segment=4).require_generic("x", "auto", False)
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory.*externals='lagrange'"):
        opts(1, "lagrange", per_trajectory=True).require_generic("x", "auto", False)
    for m in ("ab2", "ab3"):
        with pytest.raises(ValueError, match="lagrange"):
            fused.GenericOpts.of(m, (None,), 1, "lagrange")
    for cls in (nd.AB2, nd.AB3):
        with pytest.raises(ValueError, match="lagrange"):
            cls(externals="lagrange")
    # the constructor: reached through **kw by every solver class
    for cls in (nd.Euler, nd.Midpoint, nd.RK4, nd.Heun2, nd.Ralston2, nd.Kutta3, nd.SSPRK3, nd.RK4Classic):
        assert cls(externals="lagrange").externals == "lagrange" and cls(substeps=4, externals="lagrange").substeps == 4
        for bad in ("cubic", "", None, 1, True, "Linear", "LINEAR", "Lagrange"):
            with pytest.raises(ValueError, match="externals must be one of"):
                cls(externals=bad)
    assert nd.ExplicitRK(((), (1.0,)), (0.5, 0.5), 2, externals="lagrange").externals == "lagrange"
    assert "lagrange" in nd.FixedGridODESolver.__init__.__doc__
    assert autograd._FusedOdeLag.__name__ == "_FusedOdeLag" and autograd._FusedDaeLag.__name__ == "_FusedDaeLag"


def test_routing_of_lagrange_externals_next_to_a_forced_kernel():
    for cls in (nd.RK4, nd.Kutta3):
        for kernel in ("auto", "generic"):
            for n in (1, 3):
                s = cls(substeps=n, externals="lagrange")
                s.kernel, s.fused = kernel, "require"
                assert s._generic_only_ok("integrate_ODE", (None,))
                assert s._generic_kwargs() == dict(externals="lagrange", **(dict(substeps=n) if n > 1 else {}))
        for kernel in ("wave", "tile", "mfma", "wide"):
            s = cls(externals="lagrange")
            s.kernel, s.fused = kernel, "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,))
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match="externals='lagrange'" if cls is nd.RK4 else "tableau"):
                s._generic_only_ok("integrate_ODE", (None,))
        s = cls(externals="lagrange")
        s.kernel, s.fused = "auto", "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="externals='lagrange'"):
            s._generic_only_ok("integrate_ODE", (None,), per_trajectory=True)
        s = cls(externals="lagrange", segment=3)
        s.kernel, s.fused = "auto", "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="segment=3.*externals='lagrange'"):
            s._generic_only_ok("integrate_ODE", (None,))
    m = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4(externals="lagrange"))
    t = torch.zeros(3, 4, 1)
    assert m._forward_encoded(t, torch.zeros(3, 4, 8), torch.zeros(3, 4, 2), None, None) is None
