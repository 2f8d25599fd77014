"""Sub-steps per grid interval (solver.substeps), host side (no GPU): the callback walk against the CPU oracle on the n-times refined
problem (tests/generic_cases.py), its observed order in the number of sub-steps, teacher forcing, substeps = 1 against the walk as it was
before sub-steps existed, and the additive C ABI (psnode_substeps_f32 and its nine entry points: argument checks from the dims alone).

The oracle carries the reference's three formulas.  Kutta3 has no oracle form: its yardstick is this package's own one-step-per-interval
walk on the same refined problem, the walk the oracle pins for the three built-in formulas in this file and the goldens pin elsewhere."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn as nn

import capi_args as A
import generic_cases as C
from capi_args import R
from capi_args import state_dict_of as _sd
from capi_args import sub as _sub
from helpers import TOL_ORACLE, T, load, rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4, "Kutta3": nd.Kutta3}
SUB_EXPORTS = ("psnode_ode_integrate_sub_supported", "psnode_ode_integrate_sub_f32", "psnode_dae_integrate_sub_supported",
               "psnode_dae_integrate_sub_f32", "psnode_ode_backward_sub_supported", "psnode_ode_backward_sub_f32",
               "psnode_dae_backward_sub_supported", "psnode_dae_backward_sub_workspace_bytes", "psnode_dae_backward_sub_f32")
B0, T0 = 5, 6
EV = (0, 3)          # the grid rows that carry the events


def _solver(name, n=1):
    s = SOLVERS[name](substeps=n)
    s.fused = "off"
    return s


# ----------------------------------------------------------------------------- 1. the walk vs the oracle on the refined problem
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", list(SOLVERS))
def test_ode_walk_equals_the_refined_problem(name, n):
    t = C.dyadic_clock(T0, B0, n)
    de, _, x, z, ev, zj = C.ode_case(6, 2, (32, 32), B0, T0, seed=10 + n, t=t, ev_rows=EV)          # events at steps 0 and 3
    a0 = torch.cat((x[0], z[0]), -1)
    tf, zf = C.refine_clock(t, n), C.refine_rows(z, n, t, ev, zj)
    xf = torch.zeros(tf.shape[0], B0, 6)
    xf[0] = x[0]
    assert torch.equal(tf[::n], t) and torch.equal((tf[1:] - tf[:-1])[:, 1], torch.full((tf.shape[0] - 1, 1), 1 / 64))
    with torch.no_grad():
        got = C.run_ode(_solver(name, n), de, t, x, z, a0, ev, zj)
        if name == "Kutta3":
            ref = C.run_ode(_solver(name), de, tf, xf, zf, a0, ev, zj)
        else:
            ref = O.integrate_ode(name, C.layers_of(de.x_dot), tf, xf, zf, a0, ev, zj)
    e = rel_err(got, ref[::n])
    print(name, n, f"{e:.3e}")
    assert got.shape == x.shape and e <= TOL_ORACLE


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("no_x", [False, True])
def test_dae_walk_equals_the_refined_problem(name, n, no_x):
    t = C.dyadic_clock(T0, B0, n)
    de, ae, _, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), B0, T0, seed=20 + n, t=t, ev_rows=EV)
    if no_x:
        x = x[:, :, :0]                      # the dataset x is not read without teacher forcing: what the models pass then
    tf, zf, vf = C.refine_clock(t, n), C.refine_rows(z, n, t, ev, zj), C.refine_rows(v, n, t, ev, vj)
    xf, i_f = torch.zeros(tf.shape[0], B0, x.shape[-1]), torch.zeros(tf.shape[0], B0, 2)
    with torch.no_grad():
        gx, gi = C.run_dae(_solver(name, n), de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj)
        if name == "Kutta3":
            rx, ri = C.run_dae(_solver(name), de, ae, tf, xf, zf, vf, i_f, x_init, a0, ev, zj, vj)
        else:
            rx, ri = O.integrate_dae(name, C.layers_of(de.x_dot), C.layers_of(ae.i_calculator), x_init, tf, xf, zf, vf, i_f, a0, ev, zj, vj)
    ex, ei = rel_err(gx, rx[::n]), rel_err(gi, ri[::n])
    print(name, n, no_x, f"{ex:.3e} {ei:.3e}")
    assert gx.shape == (T0, B0, 5) and gi.shape == (T0, B0, 2) and ex <= TOL_ORACLE and ei <= TOL_ORACLE


# ----------------------------------------------------------------------------- 2. observed order in the number of sub-steps, fp64
class _TanhRhs(nn.Module):
    """A smooth autonomous right-hand side with the solvers' callback signature."""

    def __init__(self, xd=4, zd=1, hidden=16):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.x_dot = nn.Sequential(nn.Linear(xd + zd, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, xd)).double()
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.5 if p.dim() == 2 else 0.3))

    def forward(self, t0, xt, zt, all_initial):
        return self.x_dot(torch.cat((xt, zt), -1))


@pytest.mark.parametrize("name,cls,order", [("Euler", nd.Euler, 1), ("Heun2", nd.Heun2, 2), ("Kutta3", nd.Kutta3, 3), ("RK4Classic", nd.RK4Classic, 4)])
def test_observed_order_in_the_number_of_substeps(name, cls, order):
    """One coarse grid of 16 intervals over [0, 1] (the h at which tests/test_rk_tableau_host.py finds every method in its asymptotic range),
    substeps 1, 2, 4, 8 against substeps 64 of RK4Classic: the error at t = 1 falls by at least 2^(order - 0.5) per doubling."""
    g = torch.Generator().manual_seed(11)
    B, steps = 3, 16
    x0, z0 = torch.randn(B, 4, generator=g, dtype=torch.float64), torch.randn(B, 1, generator=g, dtype=torch.float64)
    f = _TanhRhs()
    t = (torch.arange(steps + 1, dtype=torch.float64) / steps).view(-1, 1, 1).repeat(1, B, 1)
    x = torch.zeros(steps + 1, B, 4, dtype=torch.float64)
    x[0] = x0
    z = z0.view(1, B, -1).repeat(steps + 1, 1, 1)

    def run(solver):
        solver.fused = "off"
        with torch.no_grad():
            return solver.integrate_ODE(f, t, x, z, torch.cat((x0, z0), -1))[-1]

    ref = run(nd.RK4Classic(substeps=64))
    errs = [float((run(cls(substeps=n)) - ref).abs().max()) for n in (1, 2, 4, 8)]
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print(name, "errors", errs, "ratios", ratios)
    assert min(ratios) >= 2 ** (order - 0.5), (errs, ratios)


# ----------------------------------------------------------------------------- 3. teacher forcing
@pytest.mark.parametrize("n", [2, 3])
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
    hook = ae.register_forward_hook(lambda *_: calls.append(1))          # (a hook keeps the walk: this solver is fused = "off" anyway)
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


# ----------------------------------------------------------------------------- 4. substeps = 1 is the walk as it was
# generic_cases.walk_*_hold with substeps == 1: the walk as it stood before sub-steps existed
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
def test_substeps_one_is_bitwise_the_walk_as_it_was_g2(name):
    d = load("g2_ode.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "de__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, tr, x, z, a0 = P("t"), P("t_ragged"), P("x"), P("z"), T(d["all_initial"])
    ev = nd.ODE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]))
    s = _solver(name)
    assert s.substeps == 1
    with torch.no_grad():
        for clock in (t, tr):
            for tx in (False, True):
                got = s.integrate_ODE(de, clock, x, z, a0, ev.event_fn, ev.jump_change_fn, input_true_x=tx)
                assert torch.equal(got, C.walk_ode_hold(s, de, clock, x, z, a0, ev.event_fn, ev.jump_change_fn, tx))


@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
def test_substeps_one_is_bitwise_the_walk_as_it_was_g3(name):
    d = load("g3_dae.npz")
    de, ae = models.DAE_DE_Func(14, (64, 64, 64), 8), models.AE_Func(26, (64, 64, 64), 2)
    de.load_state_dict(_sd(d, "de__"))
    ae.load_state_dict(_sd(d, "ae__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, x, z, v, i = (P(k) for k in ("t", "x", "z", "v", "i"))
    xi, a0 = T(d["x_init"]), T(d["all_initial"])
    ev = nd.DAE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]), T(d["v_jump"]))
    s = _solver(name)
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
_supported, _call = functools.partial(A.supported, family="sub"), functools.partial(A.call, family="sub")


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    for name in SUB_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    sub_p = ctypes.POINTER(_lib.SubstepsF32)
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_sub_supported").argtypes[-1] == sub_p
        assert getattr(lib, f"psnode_{stem}_sub_f32").argtypes[2 + n_act] == sub_p
    assert lib.psnode_dae_backward_sub_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert lib.psnode_dae_backward_sub_workspace_bytes.restype is ctypes.c_size_t
    s = _lib.SubstepsF32
    assert (s.substeps.offset, s.x_sub.offset, ctypes.sizeof(s)) == (0, 8, 16)


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_substeps_argument_checks(stem, make, n_act):
    lib = _lib.load()
    tab = R(nd.Kutta3().method.abi())
    for tb in (None, tab):                               # NULL tableau: the args' method
        assert _call(lib, stem, make(), n_act, tb, None) == -1 and _supported(lib, stem, make(), n_act, tb, None) == 0          # NULL struct
        for n in (0, -3, 1025):
            assert _call(lib, stem, make(), n_act, tb, _sub(n)) == -2 and _supported(lib, stem, make(), n_act, tb, _sub(n)) == 0
        for n in (2, 3, 1024):
            assert _supported(lib, stem, make(), n_act, tb, _sub(n)) == 1
            assert _supported(lib, stem, make(kernel=_lib.KERNEL_GENERIC), n_act, tb, _sub(n)) == 1
            assert _call(lib, stem, make(), n_act, tb, _sub(n)) == -1          # as far as the pointer checks, nothing launched
            for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                assert _supported(lib, stem, make(kernel=kernel), n_act, tb, _sub(n)) == 0
                assert _call(lib, stem, make(kernel=kernel), n_act, tb, _sub(n)) == -5
        assert _call(lib, stem, None, n_act, tb, _sub(2)) == -1          # NULL args
    # a NULL tableau needs a valid method; a tableau makes the method unread
    assert _call(lib, stem, make(method=77), n_act, None, _sub(2)) == -3 and _supported(lib, stem, make(method=77), n_act, None, _sub(2)) == 0
    assert _supported(lib, stem, make(method=77), n_act, tab, _sub(2)) == 1
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    assert _call(lib, stem, make(), n_act, R(bad), _sub(2)) == -3
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _call(lib, stem, make(), n_act, tab, _sub(2), R(unknown)) == -3
    tanh, silu = R(fused.Act(_lib.ACT_TANH).abi()), R(fused.Act(_lib.ACT_SILU).abi())
    assert _supported(lib, stem, make(), n_act, None, _sub(2), tanh) == 1 and _supported(lib, stem, make(), n_act, tab, _sub(4), silu) == 1
    # substeps == 1 is the entry point without sub-steps: its statuses, its method range
    for tb in (None, tab):
        assert _supported(lib, stem, make(), n_act, tb, _sub(1)) == 1 and _call(lib, stem, make(), n_act, tb, _sub(1)) == -1
    assert _call(lib, stem, make(method=77), n_act, None, _sub(1)) == -3


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
    assert lib.psnode_dae_backward_sub_workspace_bytes(R(e), None, None, None, R(sub)) == 0
    assert lib.psnode_dae_backward_sub_workspace_bytes(R(_dae_bwd_args()), None, None, None, R(sub)) > 0
    assert lib.psnode_dae_backward_sub_workspace_bytes(R(_dae_bwd_args()), None, None, None, R(_sub(1))) > 0
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
    # a backward call with every other pointer in place and no x_sub: PSNODE_ERR_NULL before the workspace is looked at
    b = _ode_bwd_args()
    for l in range(4):
        b.de.weight[l] = b.de.bias[l] = 256
    b.t.ptr = b.z.ptr = b.all_initial = b.xs = b.grad_xs = b.grad_x0 = b.grad_all_initial = b.grad_params = 256
    assert _call(lib, "ode_backward", b, 1, None, _sub(2)) == -1
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256)) == -4          # with one: as far as the workspace check
    e = _dae_bwd_args()
    q = e.base
    for m in (q.de, q.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
    q.grad_params_de = q.grad_params_ae = 256
    assert _call(lib, "dae_backward", e, 2, None, _sub(2)) == -1
    assert _call(lib, "dae_backward", e, 2, None, _sub(2, 256)) == -4


_layers = A.hip_layers


def test_python_predicates_refusals_and_the_constructor():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    for method in ("euler", "rk4", nd.Kutta3().method):
        for sub in (2, 7):
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, substeps=sub)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", act=tanh, substeps=sub)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, substeps=sub)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True, substeps=sub)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, substeps=sub)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), substeps=sub)
            for tx, ti in ((True, False), (False, True), (True, True)):
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti, substeps=sub)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti,
                                                           substeps=sub)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 1, 33, input_true_x=tx, input_true_i=ti, substeps=sub)
            for kernel in ("wave", "tile", "mfma", "wide"):
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, substeps=sub)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel, substeps=sub)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, substeps=sub)
            assert fused.ode_save_hidden(method, ode01, 8, 2, substeps=sub) == 0 and fused.dae_save_hidden(method, de, ae, 8, 2, 2, 2, substeps=sub) == 0
    # every specialised, latent, encoded and saved-row entry refuses sub-steps
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.dae_backward_wide_supported("rk4", de, ae, 8, 2, 2, 2, substeps=2)
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.dae_backward_wide("rk4", de, ae, None, None, None, None, torch.zeros(2, 1, 8), torch.zeros(2, 1, 2), None, None, substeps=2)
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.latent_backward_wide("rk4", ode01, None, None, None, None, None, torch.zeros(2, 1, 16), None, None, None, saved=(), substeps=2)
    opts = lambda substeps: fused.GenericOpts.of("rk4", (None,), substeps)
    with pytest.raises(_lib.UnsupportedShapeError):
        opts(2).require_plain("a specialised entry")
    opts(1).require_plain("a specialised entry")
    for kernel, save in (("wave", False), ("mfma", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError):
            opts(2).require_generic("x", kernel, save)
    opts(2).require_generic("x", "generic", False)
    opts(1).require_generic("x", "wave", True)
    assert opts(1).family == "plain" and opts(1).c_args() == [] and opts(5).family == "sub"
    five = opts(5).c_args()[-1]._obj          # (ode: act, tableau, psnode_substeps_f32)
    assert opts(5).c_args()[:2] == [None, None] and five.substeps == 5 and not five.x_sub
    for bad in (0, -1, 1025, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            opts(bad)
    # the constructor: an int >= 1, reached through **kw by every solver class
    for cls in (nd.Euler, nd.Midpoint, nd.RK4, nd.Heun2, nd.Kutta3, nd.RK4Classic):
        assert cls().substeps == 1 and cls(substeps=4).substeps == 4
        for bad in (0, -2, 1.5, 2.0, True, None, "3"):
            with pytest.raises(ValueError):
                cls(substeps=bad)
    assert nd.ExplicitRK(((), (1.0,)), (0.5, 0.5), 2, substeps=3).substeps == 3
    assert "substeps" in nd.FixedGridODESolver.__init__.__doc__


def test_routing_of_substeps_next_to_a_tableau_and_a_forced_kernel():
    """The solver's route predicate, from the attributes alone: 'auto' / 'generic' keep a call fusable, a specialised kernel or more than
    1024 sub-steps walks under fused = 'auto' and raises under 'require' -- for a built-in method and for a Tableau alike (on a specialised
    kernel the Tableau is what the one predicate names first, as integrate_ODE's chain of four always did)."""
    for cls in (nd.RK4, nd.Kutta3):
        for kernel in ("auto", "generic"):
            s = cls(substeps=3)
            s.kernel, s.fused = kernel, "require"
            assert s._generic_only_ok("integrate_ODE", (None,))
        for kernel, sub in (("wave", 3), ("tile", 2), ("mfma", 2), ("wide", 4), ("auto", 1025)):
            s = cls(substeps=sub)
            s.kernel, s.fused = kernel, "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,))
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match="substeps" if cls is nd.RK4 or kernel == "auto" else "tableau"):
                s._generic_only_ok("integrate_ODE", (None,))
        s = cls()
        s.kernel, s.fused = "wave", "require"
        if cls is nd.RK4:
            assert s._generic_only_ok("integrate_ODE", (None,))              # substeps == 1: nothing to say
        else:
            with pytest.raises(_lib.UnsupportedShapeError, match="tableau"):
                s._generic_only_ok("integrate_ODE", (None,))
        s = nd.Kutta3(substeps=3)              # the order of complaint: act, tableau, sub-steps
        s.kernel, s.fused = "wave", "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="activation"):
            s._generic_only_ok("integrate_ODE", (fused.Act(_lib.ACT_TANH, name="Tanh"),))
    # a direct_encode model with sub-steps does not take the one-launch encoded forward
    m = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4(substeps=2))
    t = torch.zeros(3, 4, 1)
    assert m._forward_encoded(t, torch.zeros(3, 4, 8), torch.zeros(3, 4, 2), None, None) is None
