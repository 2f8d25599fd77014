"""Linear interpolation of the external inputs (solver.externals = "linear"), host side (no GPU): the callback walk against the CPU oracle
on the linearly refined problem (Euler), against a stand-alone fp64 restatement of the stage formula (tests/externals_linear_cases.py), its
observed order in the grid and in the number of sub-steps next to the zero-order hold's, teacher forcing, externals = "hold" against the walk
as it was, and the additive C ABI (the nine _lin entry points: argument checks from the dims alone)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn as nn

import capi_args as A
import externals_linear_cases as L
import generic_cases as C
from capi_args import R
from capi_args import state_dict_of as _sd
from capi_args import sub as _sub
from helpers import TOL_ORACLE, T, load, rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
LIN_EXPORTS = ("psnode_ode_integrate_lin_supported", "psnode_ode_integrate_lin_f32", "psnode_dae_integrate_lin_supported",
               "psnode_dae_integrate_lin_f32", "psnode_ode_backward_lin_supported", "psnode_ode_backward_lin_f32",
               "psnode_dae_backward_lin_supported", "psnode_dae_backward_lin_workspace_bytes", "psnode_dae_backward_lin_f32")
B0, T0 = 5, 6
EV = (0, 3)          # the grid rows that carry the events


def _solver(name, n=1, externals="linear"):
    s = SOLVERS[name](substeps=n, externals=externals)
    s.fused = "off"
    return s


# ----------------------------------------------------------------------------- 1. Euler: the walk vs the oracle on the linearly refined problem
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ode_euler_walk_equals_the_oracle_on_the_linearly_refined_problem(n):
    t = C.dyadic_clock(T0, B0, n)
    de, _, x, z, ev, zj = C.ode_case(6, 2, (32, 32), B0, T0, seed=40 + n, t=t, ev_rows=EV)          # events at steps 0 and 3
    a0 = torch.cat((x[0], z[0]), -1)
    tf, zf = C.refine_clock(t, n), L.refine_rows_linear(z, n, t, ev, zj)
    xf = torch.zeros(tf.shape[0], B0, 6)
    xf[0] = x[0]
    assert torch.equal(tf[::n], t) and torch.equal(zf[::n], z)
    with torch.no_grad():
        got = C.run_ode(_solver("euler", n), de, t, x, z, a0, ev, zj)
        hold = C.run_ode(_solver("euler", n, "hold"), de, t, x, z, a0, ev, zj)
        ref = O.integrate_ode("euler", C.layers_of(de.x_dot), tf, xf, zf, a0, ev, zj)
    e = rel_err(got, ref[::n])
    print(n, f"{e:.3e}", f"hold differs by {rel_err(hold, ref[::n]):.3e}")
    assert got.shape == x.shape and e <= TOL_ORACLE
    assert (rel_err(hold, ref[::n]) > 100 * TOL_ORACLE) == (n > 1)          # (Euler with one sub-step reads theta = 0 only: the hold)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("no_x", [False, True])
def test_dae_euler_walk_equals_the_oracle_on_the_linearly_refined_problem(n, no_x):
    t = C.dyadic_clock(T0, B0, n)
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), B0, T0, seed=50 + n, t=t, ev_rows=EV)
    if no_x:
        x = x[:, :, :0]                      # the dataset x is not read without teacher forcing: what the models pass then
    tf, zf, vf = C.refine_clock(t, n), L.refine_rows_linear(z, n, t, ev, zj), L.refine_rows_linear(v, n, t, ev, vj)
    xf, i_f = torch.zeros(tf.shape[0], B0, x.shape[-1]), torch.zeros(tf.shape[0], B0, 2)
    with torch.no_grad():
        gx, gi = C.run_dae(_solver("euler", n), de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj)
        rx, ri = O.integrate_dae("euler", C.layers_of(de.x_dot), C.layers_of(ae.i_calculator), x_init, tf, xf, zf, vf, i_f, a0, ev, zj, vj)
    ex, ei = rel_err(gx, rx[::n]), rel_err(gi, ri[::n])
    print(n, no_x, f"{ex:.3e} {ei:.3e}")
    assert gx.shape == (T0, B0, 5) and gi.shape == (T0, B0, 2) and ex <= TOL_ORACLE and ei <= TOL_ORACLE


# ----------------------------------------------------------------------------- 2. every formula vs the stand-alone fp64 restatement
def _rel64(y, ref):
    return float((y - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["midpoint", "rk4", "Kutta3", "RK4Classic"])
def test_ode_walk_equals_the_stand_alone_restatement_fp64(name, n):
    t = C.dyadic_clock(T0, B0, n, dtype=torch.float64) * 1.3
    de, _, x, z, ev, zj = C.ode_case(6, 2, (32, 32), B0, T0, seed=60 + n, t=t, ev_rows=EV)
    de, x, z, zj = de.double(), x.double(), z.double(), zj.double()
    a0 = torch.cat((x[0], z[0]), -1)
    a, b = L.TABLEAUS[name]
    with torch.no_grad():
        got = C.run_ode(_solver(name, n), de, t, x, z, a0, ev, zj)
        ref = L.ode_linear_reference(lambda xx, w: de(t0=None, xt=xx, zt=w[0], all_initial=a0), a, b, t, x[0], z, n, (0, 3), zj)
        hold = C.run_ode(_solver(name, n, "hold"), de, t, x, z, a0, ev, zj)
    e = _rel64(got, ref)
    print(name, n, f"{e:.3e}", f"hold differs by {_rel64(hold, ref):.3e}")
    assert e <= 1e-12 and _rel64(hold, ref) > 1e-4


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["midpoint", "rk4", "Kutta3", "RK4Classic"])
def test_dae_walk_equals_the_restated_de_step_with_the_package_s_head_fp64(name, n):
    """The DE step restated; i comes from the package's head module: at grid point 0, at an event (jumped rows), in front of every sub-step
    j >= 1 at the z | v of theta = j / n, and at grid point k + 1 with rows k + 1."""
    t = C.dyadic_clock(T0, B0, n, dtype=torch.float64) * 1.3
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), B0, T0, seed=70 + n, t=t, ev_rows=EV)
    de, ae = de.double(), ae.double()
    x, z, v, i, x_init, a0, zj, vj = (q.double() for q in (x, z, v, i, x_init, a0, zj, vj))
    a, b = L.TABLEAUS[name]
    with torch.no_grad():
        gx, gi = C.run_dae(_solver(name, n), de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj)
        cur = x_init
        ci = ae(xt=cur, zt=z[0], vt=v[0], all_initial=a0)
        rx, ri = [cur], [ci]
        for k in range(T0 - 1):
            left = (z[k], v[k])
            if k in (0, 3):
                left = (zj[:, (0, 3).index(k)], vj[:, (0, 3).index(k)])
                ci = ae(xt=cur, zt=left[0], vt=left[1], all_initial=a0)
            right = (z[k + 1], v[k + 1])
            h = (t[k + 1] - t[k]) / n
            for j in range(n):
                if j > 0:
                    th = j / n
                    ci = ae(xt=cur, zt=left[0] + th * (right[0] - left[0]), vt=left[1] + th * (right[1] - left[1]), all_initial=a0)
                f = lambda xx, w, ci=ci: de(t0=None, xt=xx, zt=w[0], vt=w[1], it=ci, all_initial=a0)
                cur = L.rk_step_linear(f, a, b, h, cur, left, right, j, n)
            ci = ae(xt=cur, zt=z[k + 1], vt=v[k + 1], all_initial=a0)
            rx.append(cur)
            ri.append(ci)
        rx, ri = torch.stack(rx), torch.stack(ri)
    ex, ei = _rel64(gx, rx), _rel64(gi, ri)
    print(name, n, f"{ex:.3e} {ei:.3e}")
    assert ex <= 1e-12 and ei <= 1e-12


# ----------------------------------------------------------------------------- 3. observed order, fp64: smooth sampled forcing
def _forced_problem(points, B=3):
    """Tanh DE_Func, x 3 / z 2 / hidden 16 x 16, forcing z(t) = 0.5 sin(3 t + phi) sampled on `points` grid points of [0, 1]."""
    torch.manual_seed(5)
    de = models.DE_Func(5, (16, 16), 3, activation=nn.Tanh).double()
    g = torch.Generator().manual_seed(6)
    x0 = 0.5 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    phi = torch.rand(B, 2, generator=g, dtype=torch.float64) * 3.0
    t = torch.linspace(0.0, 1.0, points, dtype=torch.float64).view(-1, 1, 1).repeat(1, B, 1)
    z = 0.5 * torch.sin(3.0 * t + phi.unsqueeze(0))
    x = torch.zeros(points, B, 3, dtype=torch.float64)
    x[0] = x0
    return de, t, x, z, torch.cat((x0, z[0]), -1)


def _run_forced(solver, points):
    de, t, x, z, a0 = _forced_problem(points)
    solver.fused = "off"
    with torch.no_grad():
        return solver.integrate_ODE(de, t, x, z, a0)


def test_observed_order_in_the_grid_hold_is_first_order_linear_second():
    """RK4Classic on grids of 9 / 17 / 33 / 65 points against the 2049-point linear run: holding the sampled forcing is first order whatever
    the method, interpolating it second (the interpolation error of a smooth input).  Measured in fp64: 0.98 - 1.00 and 2.00 - 2.01."""
    ref = _run_forced(nd.RK4Classic(externals="linear"), 2049)
    errs = {"hold": [], "linear": []}
    for points in (9, 17, 33, 65):
        for ext in errs:
            got = _run_forced(nd.RK4Classic(externals=ext), points)
            errs[ext].append(float((got - ref[::2048 // (points - 1)]).abs().max()))
    orders = {ext: [math.log2(e[k] / e[k + 1]) for k in range(3)] for ext, e in errs.items()}
    print("errors", errs, "orders", orders)
    assert max(orders["hold"]) <= 1.2, orders
    assert min(orders["linear"]) >= 1.8, orders
    assert all(l < h for l, h in zip(errs["linear"], errs["hold"])), errs


def test_observed_order_in_the_number_of_substeps_needs_the_interpolation():
    """5 grid points, substeps 1, 2, 4, 8 against substeps 128 (RK4Classic, linear): with interpolated inputs every method gains its own
    order per doubling; with held inputs the sub-steps buy nothing.  Measured in fp64: hold 6.1e-3 at every n, linear 7e-11 at n = 8."""
    ref = _run_forced(nd.RK4Classic(substeps=128, externals="linear"), 5)
    err = lambda cls, n, ext: float((_run_forced(cls(substeps=n, externals=ext), 5) - ref).abs().max())
    for cls, order in ((nd.Euler, 1), (nd.Heun2, 2), (nd.RK4Classic, 4)):
        errs = [err(cls, n, "linear") for n in (1, 2, 4, 8)]
        ratios = [errs[k] / errs[k + 1] for k in range(3)]
        print(cls.__name__, "linear", errs, ratios)
        assert min(ratios) >= 2 ** (order - 0.5), (cls.__name__, errs, ratios)
    hold = [err(nd.RK4Classic, n, "hold") for n in (1, 2, 4, 8)]
    lin8 = err(nd.RK4Classic, 8, "linear")
    print("RK4Classic hold", hold, "linear at n = 8", lin8)
    assert max(hold) / min(hold) < 1.01, hold
    assert hold[3] >= 100 * lin8, (hold, lin8)


# ----------------------------------------------------------------------------- 4. teacher forcing; "hold" is the walk as it was
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
    assert n_ti == T0 + 2                                    # one head per grid point, one per event
    assert n_free == T0 + 2 + (T0 - 1) * (n - 1)             # ... and one in front of every sub-step behind an interval's first


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
def test_externals_hold_is_bitwise_the_walk_as_it_was_g2(name, n):
    d = load("g2_ode.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "de__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, tr, x, z, a0 = P("t"), P("t_ragged"), P("x"), P("z"), T(d["all_initial"])
    ev = nd.ODE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]))
    s, dflt = _solver(name, n, "hold"), SOLVERS[name](substeps=n)
    dflt.fused = "off"
    assert s.externals == dflt.externals == "hold"
    with torch.no_grad():
        for clock in (t, tr):
            for tx in (False, True):
                ref = C.walk_ode_hold(s, de, clock, x, z, a0, ev.event_fn, ev.jump_change_fn, tx)
                for q in (s, dflt):
                    assert torch.equal(q.integrate_ODE(de, clock, x, z, a0, ev.event_fn, ev.jump_change_fn, input_true_x=tx), ref)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
def test_externals_hold_is_bitwise_the_walk_as_it_was_g3(name, n):
    d = load("g3_dae.npz")
    de, ae = models.DAE_DE_Func(14, (64, 64, 64), 8), models.AE_Func(26, (64, 64, 64), 2)
    de.load_state_dict(_sd(d, "de__"))
    ae.load_state_dict(_sd(d, "ae__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, x, z, v, i = (P(k) for k in ("t", "x", "z", "v", "i"))
    xi, a0 = T(d["x_init"]), T(d["all_initial"])
    ev = nd.DAE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]), T(d["v_jump"]))
    s = _solver(name, n, "hold")
    with torch.no_grad():
        for tx in (False, True):
            for ti in (False, True):
                got = s.integrate_DAE(xi, de, ae, t, x, z, v, i, a0, ev.event_fn, ev.jump_change_fn, input_true_x=tx, input_true_i=ti)
                ref = C.walk_dae_hold(s, xi, de, ae, t, x, z, v, i, a0, ev.event_fn, ev.jump_change_fn, tx, ti)
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (tx, ti)


# ----------------------------------------------------------------------------- 5. C ABI, dims only; routing; the constructor
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))
_supported, _call = functools.partial(A.supported, family="lin"), functools.partial(A.call, family="lin")


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    for name in LIN_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    sub_p = ctypes.POINTER(_lib.SubstepsF32)
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_lin_supported").argtypes == getattr(lib, f"psnode_{stem}_sub_supported").argtypes
        assert getattr(lib, f"psnode_{stem}_lin_f32").argtypes == getattr(lib, f"psnode_{stem}_sub_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_lin_f32").argtypes[2 + n_act] == sub_p
    assert lib.psnode_dae_backward_lin_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert lib.psnode_dae_backward_lin_workspace_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_lin_argument_checks(stem, make, n_act):
    lib = _lib.load()
    tab = R(nd.Kutta3().method.abi())
    for tb in (None, tab):                               # NULL tableau: the args' method
        # a NULL struct is one sub-step: supported, and the call gets as far as the pointer checks
        assert _supported(lib, stem, make(), n_act, tb, None) == 1 and _call(lib, stem, make(), n_act, tb, None) == -1
        for n in (0, -3, 1025):
            assert _call(lib, stem, make(), n_act, tb, _sub(n)) == -2 and _supported(lib, stem, make(), n_act, tb, _sub(n)) == 0
        for n in (1, 2, 3, 1024):                        # every substeps >= 1 runs in this build
            assert _supported(lib, stem, make(), n_act, tb, _sub(n)) == 1
            assert _supported(lib, stem, make(kernel=_lib.KERNEL_GENERIC), n_act, tb, _sub(n)) == 1
            assert _call(lib, stem, make(), n_act, tb, _sub(n)) == -1          # as far as the pointer checks, nothing launched
            for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                assert _supported(lib, stem, make(kernel=kernel), n_act, tb, _sub(n)) == 0
                assert _call(lib, stem, make(kernel=kernel), n_act, tb, _sub(n)) == -5
        assert _call(lib, stem, None, n_act, tb, _sub(2)) == -1          # NULL args
        assert _call(lib, stem, None, n_act, tb, None) == -1
    # a NULL tableau needs a valid method, also with one sub-step; a tableau makes the method unread
    for sub in (None, _sub(1), _sub(2)):
        assert _call(lib, stem, make(method=77), n_act, None, sub) == -3 and _supported(lib, stem, make(method=77), n_act, None, sub) == 0
        assert _supported(lib, stem, make(method=77), n_act, tab, sub) == 1
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    assert _call(lib, stem, make(), n_act, R(bad), _sub(2)) == -3 and _supported(lib, stem, make(), n_act, R(bad), _sub(2)) == 0
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _call(lib, stem, make(), n_act, tab, _sub(2), R(unknown)) == -3 and _supported(lib, stem, make(), n_act, tab, _sub(2), R(unknown)) == 0
    tanh, silu = R(fused.Act(_lib.ACT_TANH).abi()), R(fused.Act(_lib.ACT_SILU).abi())
    assert _supported(lib, stem, make(), n_act, None, _sub(2), tanh) == 1 and _supported(lib, stem, make(), n_act, tab, None, silu) == 1


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
    assert lib.psnode_dae_backward_lin_workspace_bytes(R(e), None, None, None, R(sub)) == 0
    assert lib.psnode_dae_backward_lin_workspace_bytes(R(_dae_bwd_args()), None, None, None, R(sub)) > 0
    assert lib.psnode_dae_backward_lin_workspace_bytes(R(_dae_bwd_args()), None, None, None, None) > 0
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
    assert _call(lib, "ode_backward", b, 1, None, _sub(1)) == -4 and _call(lib, "ode_backward", b, 1, None, None) == -4
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


def test_supported_answers_for_the_linear_build_s_own_lds_fit():
    """K0 keeps z_dim + v_dim more rows of LDS in this build, K5 three times that: somewhere along a growing z_dim the _lin query says no
    where the _sub query still says yes, and never the other way round."""
    lib = _lib.load()
    for stem, make in (("ode_integrate", _ode_args), ("ode_backward", _ode_bwd_args)):
        first_lin = first_sub = None
        for zd in range(64, 660, 4):
            a = make(kernel=_lib.KERNEL_GENERIC, xd=8, zd=zd, hidden=32)
            lin, sub = _supported(lib, stem, a, 1, None, _sub(2)), _supported(lib, stem, a, 1, None, _sub(2), family="sub")
            assert not (lin and not sub), (stem, zd)
            if not lin and first_lin is None:
                first_lin = zd
            if not sub and first_sub is None:
                first_sub = zd
        print(stem, "first z_dim refused: lin", first_lin, "sub", first_sub)
        assert first_lin is not None and (first_sub is None or first_lin < first_sub), (stem, first_lin, first_sub)


_layers = A.hip_layers


def test_python_predicates_refusals_and_the_constructor():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    lin = dict(externals="linear")
    for method in ("euler", "rk4", nd.Kutta3().method):
        for sub in (1, 2, 7):
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, substeps=sub, **lin)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", act=tanh, substeps=sub, **lin)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, substeps=sub, **lin)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True, substeps=sub, **lin)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, substeps=sub, **lin)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), substeps=sub, **lin)
            for tx, ti in ((True, False), (False, True), (True, True)):
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **lin)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti,
                                                           substeps=sub, **lin)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 1, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **lin)
            for kernel in ("wave", "tile", "mfma", "wide"):
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, substeps=sub, **lin)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel, substeps=sub, **lin)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, substeps=sub, **lin)
            assert fused.ode_backward_supported(method, ode01, 8, 2, "generic", substeps=sub, **lin)
            assert fused.dae_backward_supported(method, de, ae, 8, 2, 2, 2, kernel="generic", substeps=sub, **lin)
            assert fused.ode_save_hidden(method, ode01, 8, 2, substeps=sub, **lin) == 0
            assert fused.dae_save_hidden(method, de, ae, 8, 2, 2, 2, substeps=sub, **lin) == 0
    for bad in ("cubic", "", None, 1, "Linear"):
        with pytest.raises(ValueError):
            autograd.ode_training_supported("rk4", ode01, 8, 2, 50, 33, externals=bad)
    # every specialised, latent, encoded and saved-row entry refuses interpolated externals
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.dae_backward_wide_supported("rk4", de, ae, 8, 2, 2, 2, **lin)
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.dae_backward_wide("rk4", de, ae, None, None, None, None, torch.zeros(2, 1, 8), torch.zeros(2, 1, 2), None, None, **lin)
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.latent_backward_wide("rk4", ode01, None, None, None, None, None, torch.zeros(2, 1, 16), None, None, None, saved=(), **lin)
    opts = lambda substeps, externals: fused.GenericOpts.of("rk4", (None,), substeps, externals)
    with pytest.raises(_lib.UnsupportedShapeError):
        opts(1, "linear").require_plain("a specialised entry")
    opts(1, "hold").require_plain("a specialised entry")
    with pytest.raises(ValueError):
        opts(1, "cubic")
    for kernel, save in (("wave", False), ("mfma", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="externals"):
            opts(1, "linear").require_generic("x", kernel, save)
    opts(1, "linear").require_generic("x", "generic", False)
    opts(1, "hold").require_generic("x", "wave", True)
    assert opts(1, "hold").family == "plain" and opts(1, "hold").c_args() == []
    one = opts(1, "linear").c_args()[-1]._obj
    assert one.substeps == 1 and not one.x_sub and opts(1, "linear").family == "lin" and opts(5, "hold").family == "sub"
    assert opts(5, "linear").family == "lin"
    # the constructor: "hold" | "linear", reached through **kw by every solver class
    for cls in (nd.Euler, nd.Midpoint, nd.RK4, nd.Heun2, nd.Kutta3, nd.RK4Classic):
        assert cls().externals == "hold" and cls(externals="linear").externals == "linear" and cls(externals="hold").externals == "hold"
        assert cls(substeps=4, externals="linear").substeps == 4
        for bad in ("cubic", "", None, 1, True, "Linear", "LINEAR"):
            with pytest.raises(ValueError):
                cls(externals=bad)
        assert cls(interp="linear").externals == "hold" and cls(interp="cubic", externals="linear").interp == "cubic"      # interp stays unread
    assert nd.ExplicitRK(((), (1.0,)), (0.5, 0.5), 2, externals="linear").externals == "linear"
    assert "externals" in nd.FixedGridODESolver.__init__.__doc__


def test_routing_of_linear_externals_next_to_a_forced_kernel():
    """The solver's route predicate, from the attributes alone: 'auto' / 'generic' keep a call fusable, a specialised kernel walks under
    fused = 'auto' and raises under 'require' -- for a built-in method and for a Tableau alike."""
    for cls in (nd.RK4, nd.Kutta3):
        for kernel in ("auto", "generic"):
            for n in (1, 3):
                s = cls(substeps=n, externals="linear")
                s.kernel, s.fused = kernel, "require"
                assert s._generic_only_ok("integrate_ODE", (None,))
        for kernel in ("wave", "tile", "mfma", "wide"):
            s = cls(externals="linear")
            s.kernel, s.fused = kernel, "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,))
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match="externals" if cls is nd.RK4 else "tableau"):      # (the Tableau comes first)
                s._generic_only_ok("integrate_ODE", (None,))
            h = cls()
            h.kernel, h.fused = kernel, "require"
            if cls is nd.RK4:
                assert h._generic_only_ok("integrate_ODE", (None,))              # "hold": nothing to say
            else:
                with pytest.raises(_lib.UnsupportedShapeError, match="tableau"):
                    h._generic_only_ok("integrate_ODE", (None,))
        s = cls(substeps=1025, externals="linear")              # too many sub-steps next to "linear": the sub-steps are named first
        s.kernel, s.fused = "auto", "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="substeps"):
            s._generic_only_ok("integrate_ODE", (None,))
    # a direct_encode model with a "linear" solver does not take the one-launch encoded forward
    m = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4(externals="linear"))
    t = torch.zeros(3, 4, 1)
    assert m._forward_encoded(t, torch.zeros(3, 4, 8), torch.zeros(3, 4, 2), None, None) is None


def test_a_solver_without_the_private_step_cannot_interpolate():
    """A user subclass that only defines `_step_func` keeps working under "hold" and says what is missing under "linear"."""
    class Mine(nd.FixedGridODESolver):
        order, method = 1, "euler"

        def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
            f0 = func(t0=t0, xt=x0, zt=z0, all_initial=all_initial)
            return dt * f0, f0

    t = C.dyadic_clock(3, 2, 1)
    de, _, x, z, _, _ = C.ode_case(4, 1, (8,), 2, 3, seed=3, t=t, ev_rows=())
    a0 = torch.cat((x[0], z[0]), -1)
    s = Mine()
    s.fused = "off"
    with torch.no_grad():
        assert s.integrate_ODE(de, t, x, z, a0).shape == x.shape
        s = Mine(externals="linear")
        s.fused = "off"
        with pytest.raises(NotImplementedError, match="_step_func_lin"):
            s.integrate_ODE(de, t, x, z, a0)
