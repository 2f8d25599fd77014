"""Explicit Runge-Kutta tableaus on the generic kernels, host side (no GPU): the solver classes and fused.Tableau, the callback walk of
ExplicitRK against the reference-captured goldens (which pins the tableau formula to the reference itself), the order of accuracy of the
named methods in fp64, and the additive C ABI (psnode_rk_tableau_f32 and its nine entry points: argument checks from the dims alone)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn as nn

from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd
import capi_args as A
from capi_args import R
from capi_args import state_dict_of as _sd
from helpers import TOL_GPU, T, load, traj_rel_err

NAMED = {"Heun2": (nd.Heun2, 2), "Ralston2": (nd.Ralston2, 2), "Kutta3": (nd.Kutta3, 3), "SSPRK3": (nd.SSPRK3, 3), "RK4Classic": (nd.RK4Classic, 4)}
# the three formulas of the reference (my_fixed_grid.py:12-59) as tableaus
BUILTIN = {
    "euler": (((),), (1.0,), 1),
    "midpoint": (((), (0.5,)), (0.0, 1.0), 2),
    "rk4": (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125), 4),
}
RK_EXPORTS = ("psnode_ode_integrate_rk_supported", "psnode_ode_integrate_rk_f32", "psnode_dae_integrate_rk_supported",
              "psnode_dae_integrate_rk_f32", "psnode_ode_backward_rk_supported", "psnode_ode_backward_rk_f32",
              "psnode_dae_backward_rk_supported", "psnode_dae_backward_rk_workspace_bytes", "psnode_dae_backward_rk_f32")


def _builtin_solver(method):
    a, b, order = BUILTIN[method]
    s = nd.ExplicitRK(a, b, order, name=f"{method}-tableau")
    s.fused = "off"
    return s


# ----------------------------------------------------------------------------- names, Tableau
def test_names_orders_and_public_surface():
    assert issubclass(nd.ExplicitRK, nd.FixedGridODESolver)
    for name, (cls, order) in NAMED.items():
        assert name in nd.__all__ and issubclass(cls, nd.ExplicitRK) and cls.order == order
        s = cls()
        assert isinstance(s.method, fused.Tableau) and s.method.name == name and s.method.order == s.order == order
        for attr in ("order", "step_size", "interp", "grid_constructor", "enable_cal_time", "assert_time", "cal_time", "total_time", "fused", "kernel"):
            assert hasattr(s, attr)
    assert "ExplicitRK" in nd.__all__
    tab = {name: cls().method for name, (cls, _) in NAMED.items()}
    assert tab["Heun2"].a == ((0.0, 0.0), (1.0, 0.0)) and tab["Heun2"].b == (0.5, 0.5)
    assert tab["Ralston2"].a[1][0] == 2 / 3 and tab["Ralston2"].b == (0.25, 0.75)
    assert tab["Kutta3"].a == ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (-1.0, 2.0, 0.0)) and tab["Kutta3"].b == (1 / 6, 2 / 3, 1 / 6)
    assert tab["SSPRK3"].a == ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.25, 0.25, 0.0)) and tab["SSPRK3"].b == (1 / 6, 1 / 6, 2 / 3)
    assert tab["RK4Classic"].a == ((0.0,) * 4, (0.5, 0.0, 0.0, 0.0), (0.0, 0.5, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))
    assert tab["RK4Classic"].b == (1 / 6, 1 / 3, 1 / 3, 1 / 6) and tab["RK4Classic"].c == (0.0, 0.5, 0.5, 1.0)
    assert [t.stages for t in tab.values()] == [2, 2, 3, 3, 4]
    with pytest.raises(ValueError):
        nd.Heun2(step_size=0.1, grid_constructor=lambda f, x, t: t)


def test_tableau_validation_and_hash():
    Tb = fused.Tableau
    ok = Tb("heun", ((), (1.0,)), (0.5, 0.5), 2)
    assert ok == Tb("heun", ((0.0, 0.0), (1.0, 0.0)), [0.5, 0.5], 2) and hash(ok) == hash(Tb("heun", ((), (1,)), (0.5, 0.5), 2))
    assert len({ok, Tb("heun", ((), (1.0,)), (0.5, 0.5), 2), Tb("other", ((), (0.5,)), (0.0, 1.0), 2)}) == 2
    with pytest.raises(dataclasses_error()):
        ok.b = (1.0, 0.0)
    for a, b in (
            (((1.0,),), (1.0,)),                                  # diagonal entry: implicit
            (((), (1.0, 0.5)), (0.5, 0.5)),                       # a[1][1] != 0
            (((0.0, 1.0), (1.0,)), (0.5, 0.5)),                   # above the diagonal
            ((), ()),                                             # no stage
            (((),) * 5, (0.2,) * 5),                              # five stages
            (((), (1.0,)), (0.5, 0.4)),                           # sum b != 1
            (((), (1.0,)), (0.5, 0.5 + 3e-6)),
            (((), (float("nan"),)), (0.5, 0.5)),
            (((),), (0.5, 0.5)),                                  # rows of a != stages
    ):
        with pytest.raises(ValueError):
            Tb("bad", a, b, 1)
    Tb("edge", ((), (1.0,)), (0.5, 0.5 + 5e-7), 2)              # within 1e-6
    abi = ok.abi()
    assert abi.stages == 2 and abi.a[1][0] == 1.0 and abi.a[0][0] == 0.0 and abi.b[1] == 0.5 and abi.b[2] == 0.0


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


# ----------------------------------------------------------------------------- the walk against the reference's goldens
@pytest.mark.parametrize("method", list(BUILTIN))
def test_walk_reproduces_g1_single_step(method):
    d = load("g1_single_step.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "ode__"))
    dd = models.DAE_DE_Func(14, (64, 64, 64), 8)
    dd.load_state_dict(_sd(d, "dae__"))
    x0, z0, v0, i0, t0, dt, t1 = (T(d[k]) for k in ("x0", "z0", "v0", "i0", "t0", "dt", "t1"))
    s = _builtin_solver(method)
    with torch.no_grad():
        x1, f0 = s.step_integrate(func=de, t0=t0, dt=dt, t1=t1, x0=x0, z0=z0, all_initial=T(d["a0_ode"]))
        assert traj_rel_err(x1, d[f"ode_{method}_x1"], bdim=0) <= TOL_GPU and traj_rel_err(f0, d[f"ode_{method}_f0"], bdim=0) <= TOL_GPU
        x1, f0 = s.step_integrate(func=dd, t0=t0, dt=dt, t1=t1, x0=x0, z0=z0, v0=v0, i0=i0, all_initial=T(d["a0_dae"]))
        assert traj_rel_err(x1, d[f"dae_{method}_x1"], bdim=0) <= TOL_GPU and traj_rel_err(f0, d[f"dae_{method}_f0"], bdim=0) <= TOL_GPU


@pytest.mark.parametrize("method", list(BUILTIN))
def test_walk_reproduces_g2_ode(method):
    d = load("g2_ode.npz")
    de = models.DE_Func(10, (64, 64, 64), 8)
    de.load_state_dict(_sd(d, "de__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, tr, x, z, a0 = P("t"), P("t_ragged"), P("x"), P("z"), T(d["all_initial"])
    ev = nd.ODE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]))
    no = nd.ODE_Event()
    no.set_event(torch.full_like(T(d["event_t"]), -1.0), T(d["z_jump"]))
    s = _builtin_solver(method)
    with torch.no_grad():
        cases = {
            "plain": s.integrate_ODE(de, t, x, z, a0, no.event_fn, no.jump_change_fn),
            "noevfn": s.integrate_ODE(de, t, x, z, a0),
            "events": s.integrate_ODE(de, t, x, z, a0, ev.event_fn, ev.jump_change_fn),
            "events_truex": s.integrate_ODE(de, t, x, z, a0, ev.event_fn, ev.jump_change_fn, input_true_x=True),
            "ragged": s.integrate_ODE(de, tr, x, z, a0, ev.event_fn, ev.jump_change_fn),
        }
    for name, got in cases.items():
        assert traj_rel_err(got, d[f"{method}_{name}"]) <= TOL_GPU, name


@pytest.mark.parametrize("method", list(BUILTIN))
def test_walk_reproduces_g3_dae(method):
    d = load("g3_dae.npz")
    de = models.DAE_DE_Func(14, (64, 64, 64), 8)
    ae = models.AE_Func(26, (64, 64, 64), 2)
    de.load_state_dict(_sd(d, "de__"))
    ae.load_state_dict(_sd(d, "ae__"))
    P = lambda k: T(d[k]).permute(1, 0, 2)
    t, x, z, v, i = (P(k) for k in ("t", "x", "z", "v", "i"))
    xi, a0 = T(d["x_init"]), T(d["all_initial"])
    ev = nd.DAE_Event()
    ev.set_event(T(d["event_t"]), T(d["z_jump"]), T(d["v_jump"]))
    s = _builtin_solver(method)
    with torch.no_grad():
        for tx in (False, True):
            for ti in (False, True):
                for use_ev in (False, True):
                    kw = dict(event_fn=ev.event_fn, jump_change_fn=ev.jump_change_fn) if use_ev else {}
                    xs, is_ = s.integrate_DAE(xi, de, ae, t, x, z, v, i, a0, input_true_x=tx, input_true_i=ti, **kw)
                    key = f"{method}_tx{int(tx)}_ti{int(ti)}_ev{int(use_ev)}"
                    assert traj_rel_err(xs, d[key + "_x"]) <= TOL_GPU and traj_rel_err(is_, d[key + "_i"]) <= TOL_GPU, key


# ----------------------------------------------------------------------------- order of accuracy, fp64
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


def _integrate(solver, f, x0, z0, n_steps, horizon=1.0):
    B = x0.shape[0]
    t = (torch.arange(n_steps + 1, dtype=torch.float64) * (horizon / n_steps)).view(-1, 1, 1).repeat(1, B, 1)
    x = torch.zeros(n_steps + 1, B, x0.shape[1], dtype=torch.float64)
    x[0] = x0
    z = z0.view(1, B, -1).repeat(n_steps + 1, 1, 1)
    with torch.no_grad():
        return solver.integrate_ODE(f, t, x, z, torch.cat((x0, z0), -1))[-1]


@pytest.mark.parametrize("name", list(NAMED))
def test_observed_order_of_accuracy(name):
    """Error at t = 1 against a 16x finer RK4Classic run, at h = 1/16 and three halvings: every observed order log2(e_h / e_{h/2}) must be
    >= order - 0.5.  (h: small enough that every method is in its asymptotic range for this right-hand side -- at h = 1/8 the second-order
    methods are not yet --, large enough that the fourth-order error at h = 1/128 stays orders above fp64 roundoff and above the
    reference run's own error, 16^-4 of it.)"""
    cls, order = NAMED[name]
    g = torch.Generator().manual_seed(11)
    x0, z0 = torch.randn(3, 4, generator=g, dtype=torch.float64), torch.randn(3, 1, generator=g, dtype=torch.float64)
    f = _TanhRhs()
    steps = (16, 32, 64, 128)
    ref_solver = nd.RK4Classic()
    ref_solver.fused = "off"
    ref = _integrate(ref_solver, f, x0, z0, 16 * steps[-1])
    s = cls()
    s.fused = "off"
    errs = [float((_integrate(s, f, x0, z0, n) - ref).abs().max()) for n in steps]
    orders = [math.log2(errs[k] / errs[k + 1]) for k in range(len(errs) - 1)]
    print(name, "errors", errs, "observed orders", orders)
    assert min(orders) >= order - 0.5, (errs, orders)


# ----------------------------------------------------------------------------- C ABI, dims only
def _tab(name="RK4Classic"):
    return NAMED[name][0]().method.abi()


# `method` 77: not read next to a tableau
DIMS = dict(method=77, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
# (stem, args builder, number of activations)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))
_supported, _call = functools.partial(A.supported, family="rk"), functools.partial(A.call, family="rk")


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    for name in RK_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    rk_p = ctypes.POINTER(_lib.RkTableauF32)
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_rk_supported").argtypes[-1] == rk_p
        assert getattr(lib, f"psnode_{stem}_rk_f32").argtypes[1 + n_act] == rk_p
    assert lib.psnode_dae_backward_rk_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert lib.psnode_dae_backward_rk_workspace_bytes.restype is ctypes.c_size_t
    t = _lib.RkTableauF32
    assert (t.stages.offset, t.a.offset, t.b.offset, ctypes.sizeof(t)) == (0, 4, 68, 84)


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
@pytest.mark.parametrize("name", list(NAMED))
def test_supported_for_the_ode01_class_and_not_on_wave(stem, make, n_act, name):
    lib = _lib.load()
    tab = R(_tab(name))
    assert _supported(lib, stem, make(), n_act, tab) == 1
    assert _supported(lib, stem, make(kernel=_lib.KERNEL_GENERIC), n_act, tab) == 1
    for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA):
        assert _supported(lib, stem, make(kernel=kernel), n_act, tab) == 0
        assert _call(lib, stem, make(kernel=kernel), n_act, tab) == -5
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    silu = R(fused.Act(_lib.ACT_SILU).abi())
    assert _supported(lib, stem, make(), n_act, tab, act=tanh) == 1 and _supported(lib, stem, make(), n_act, tab, act=silu) == 1


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_tableau_argument_checks(stem, make, n_act):
    lib = _lib.load()
    assert _call(lib, stem, make(), n_act, None) == -1 and _supported(lib, stem, make(), n_act, None) == 0          # NULL tableau
    assert _call(lib, stem, None, n_act, R(_tab())) == -1                                                             # NULL args

    def bad(edit):
        t = _tab()
        edit(t)
        assert _call(lib, stem, make(), n_act, R(t)) == -3
        assert _supported(lib, stem, make(), n_act, R(t)) == 0

    bad(lambda t: setattr(t, "stages", 0))
    bad(lambda t: setattr(t, "stages", 5))
    bad(lambda t: setattr(t, "stages", -1))
    bad(lambda t: t.a[1].__setitem__(0, float("nan")))
    bad(lambda t: t.b.__setitem__(2, float("inf")))
    bad(lambda t: t.a[0].__setitem__(0, 0.5))            # diagonal
    bad(lambda t: t.a[1].__setitem__(1, 0.5))
    bad(lambda t: t.a[1].__setitem__(3, 0.5))            # above the diagonal
    t3 = _tab("Kutta3")
    t3.a[3][0] = 0.5                                      # a row beyond `stages`
    assert _call(lib, stem, make(), n_act, R(t3)) == -3
    # a valid tableau gets as far as the pointer checks; an unknown activation kind keeps its status
    assert _call(lib, stem, make(), n_act, R(_tab())) == -1
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _call(lib, stem, make(), n_act, R(_tab()), act=R(unknown)) == -3


def test_side_outputs_and_teacher_forced_activations_are_refused():
    lib = _lib.load()
    tab = R(_tab("Kutta3"))
    a = _ode_args()
    a.save_act = a.save_xstage = 256
    assert lib.psnode_ode_integrate_rk_supported(R(a), None, tab) == 0 and _call(lib, "ode_integrate", a, 1, tab) == -5
    d = _dae_args()
    d.save_act = d.save_xstage = d.save_ae_act = 256
    assert lib.psnode_dae_integrate_rk_supported(R(d), None, None, tab) == 0 and _call(lib, "dae_integrate", d, 2, tab) == -5
    b = _ode_bwd_args()
    b.saved_act = b.saved_xstage = 256
    assert lib.psnode_ode_backward_rk_supported(R(b), None, tab) == 0 and _call(lib, "ode_backward", b, 1, tab) == -5
    e = _dae_bwd_args()
    e.base.saved_act = 256
    assert lib.psnode_dae_backward_rk_supported(R(e), None, None, tab) == 0 and _call(lib, "dae_backward", e, 2, tab) == -5
    assert lib.psnode_dae_backward_rk_workspace_bytes(R(e), None, None, tab) == 0
    # teacher forcing: ELU(1) only, as the built-in methods
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    elu1 = _lib.ActF32()
    elu1.kind, elu1.alpha = _lib.ACT_ELU, 1.0
    tfo = _ode_bwd_args(flags=_lib.FLAG_INPUT_TRUE_X)
    assert lib.psnode_ode_backward_rk_supported(R(tfo), None, tab) == 1 and lib.psnode_ode_backward_rk_supported(R(tfo), R(elu1), tab) == 1
    assert lib.psnode_ode_backward_rk_supported(R(tfo), tanh, tab) == 0 and _call(lib, "ode_backward", tfo, 1, tab, act=tanh) == -5
    for flags in (1, 2, 3):
        tfd = _dae_bwd_args(flags=flags)
        assert lib.psnode_dae_backward_rk_supported(R(tfd), None, None, tab) == 1
        assert lib.psnode_dae_backward_rk_workspace_bytes(R(tfd), None, None, tab) > 0
        assert lib.psnode_dae_backward_rk_supported(R(tfd), tanh, None, tab) == 0
        assert lib.psnode_dae_backward_rk_f32(R(tfd), None, tanh, tab, None, 0, None) == -5
        one = _dae_bwd_args(flags=flags)
        one.base.T = 1
        assert lib.psnode_dae_backward_rk_f32(R(one), None, None, tab, None, 0, None) == -2
    assert lib.psnode_dae_backward_rk_supported(R(_dae_bwd_args(flags=4)), None, None, tab) == 0
    assert lib.psnode_dae_backward_rk_workspace_bytes(R(_dae_bwd_args()), None, None, tab) > 0


def test_existing_entry_points_keep_their_method_range():
    lib = _lib.load()
    for a, f in ((_ode_args(), lib.psnode_ode_integrate_f32), (_dae_args(), lib.psnode_dae_integrate_f32),
                 (_ode_bwd_args(), lib.psnode_ode_backward_f32)):
        for m in (-1, 3, 77):
            a.method = m
            assert f(R(a), None, 0, None) == -3
    b = _dae_bwd_args()
    b.base.method = 3
    assert lib.psnode_dae_backward_f32(R(b.base), None, 0, None) == -3 and lib.psnode_dae_backward_tf_f32(R(b), None, 0, None) == -3


# ----------------------------------------------------------------------------- the Python predicates
_layers = A.hip_layers


def test_python_predicates_and_refusals():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    for name, (cls, _) in NAMED.items():
        tab = cls().method
        assert fused.method_info(tab) == (_lib.EULER, tab.stages, tab)
        assert autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33) and autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33, kernel="generic")
        assert autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33, act=tanh)
        assert autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33, input_true_x=True)
        assert not autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True)
        for kernel in ("wave", "tile", "mfma"):
            assert not autograd.ode_training_supported(tab, ode01, 8, 2, 50, 33, kernel=kernel)
            assert not fused.ode_backward_supported(tab, ode01, 8, 2, kernel)
        assert autograd.dae_training_supported(tab, de, ae, 8, 2, 2, 2, 50, 33)
        assert autograd.dae_training_supported(tab, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None))
        for tx, ti in ((True, False), (False, True), (True, True)):
            assert autograd.dae_training_supported(tab, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti)
            assert not autograd.dae_training_supported(tab, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti)
            assert not autograd.dae_training_supported(tab, de, ae, 8, 2, 2, 2, 50, 33, kernel="mfma", input_true_x=tx, input_true_i=ti)
        assert not autograd._want_saved(tab, "auto", ode01, 8, 2, 50, 33) and not autograd._want_saved_dae(tab, "auto", de, ae, 8, 2, 2, 2, 50, 33)
        assert fused.ode_save_hidden(tab, ode01, 8, 2) == 0 and fused.dae_save_hidden(tab, de, ae, 8, 2, 2, 2) == 0
    tab = nd.Kutta3().method
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.dae_backward_wide_supported(tab, de, ae, 8, 2, 2, 2)
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.builtin_method(tab, "a specialised entry")
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.latent_backward_wide(tab, ode01, None, None, None, None, None, torch.zeros(2, 1, 16), None, None, None, saved=())
    assert fused.builtin_method("rk4", "x") == (_lib.RK4_38, 4) and fused.method_info("midpoint") == (_lib.MIDPOINT, 2, None)


def test_sharded_entries_pass_a_tableau_through_unchanged():
    """sharded.integrate_*_sharded / _pipelined hand `method` to the local integrator as it is: a Tableau arrives as the same object (no
    process group needed: gather=False, no events)."""
    from py_psnode_amd import sharded
    tab = nd.Kutta3().method
    seen = []
    Tn, B, xd, zd, vd, idim = 6, 3, 4, 2, 1, 2

    def ode_fn(method, de_layers, t, x, z, all_initial, out=None, **kw):
        seen.append(method)
        res = torch.zeros(t.shape[0], t.shape[1], xd)
        if out is not None:
            out.copy_(res)
        return res

    def dae_fn(method, de_layers, ae_layers, x_init, t, x, z, v, i, all_initial, out=None, **kw):
        seen.append(method)
        res = torch.zeros(t.shape[0], t.shape[1], xd), torch.zeros(t.shape[0], t.shape[1], idim)
        if out is not None:
            out[0].copy_(res[0]); out[1].copy_(res[1])
        return res

    t = torch.arange(Tn, dtype=torch.float32).view(Tn, 1, 1).repeat(1, B, 1)
    x, z, v, i = (torch.zeros(Tn, B, w) for w in (xd, zd, vd, idim))
    sharded.integrate_ode_sharded(tab, [], t, x, z, torch.zeros(B, xd + zd), gather=False, local_fn=ode_fn)
    sharded.integrate_dae_sharded(tab, [], [], x[0], t, x, z, v, i, torch.zeros(B, xd + zd + vd + idim), gather=False, local_fn=dae_fn)
    sharded.integrate_ode_pipelined(tab, [], t, x, z, torch.zeros(B, xd + zd), chunks=2, gather=False, local_fn=ode_fn)
    sharded.integrate_dae_pipelined(tab, [], [], x[0], t, z, v, i, torch.zeros(B, xd + zd + vd + idim), chunks=2, gather=False, local_fn=dae_fn)
    assert len(seen) == 6 and all(m is tab for m in seen)
