"""Runge-Kutta-Chebyshev steps (neural_dae.RKC1 / RKC2, fused.rkc_table) without a GPU: the table and the formula, stability and order,
the walk against the stand-alone restatement of tests/rkc_cases.py, the refusals, the C ABI's checks against the _sub family's, routing,
and the rounding floor d of every case tests/test_gpu_rkc.py gates with the plain helpers.TOL_GPU (4 d <= TOL_GPU, asserted here)."""
import ctypes
import dataclasses
import functools
import math

import pytest
import torch
import torch.nn as nn

import capi_args as A
import generic_cases as C
import rkc_cases as K
from capi_args import R
from helpers import TOL_GPU
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

STAGES = (2, 3, 4, 8, 16, 32)
RKC_EXPORTS = tuple(f"psnode_{s}_rkc_{k}" for s in ("ode_integrate", "dae_integrate", "ode_backward", "dae_backward")
                    for k in ("supported", "f32")) + ("psnode_dae_backward_rkc_workspace_size",)


# ----------------------------------------------------------------------------- 1. the table and the formula
@pytest.mark.parametrize("order", [1, 2])
def test_table_equals_the_loop_restatement(order):
    for s in range(order, 33):
        for eps in (None, 0.3):
            tab, ref = fused.rkc_table(s, order, eps), K.table_loop(s, order, eps)
            assert tab.stages == s and tab.order == order and len(tab.mu) == s
            for name in ("kappa", "mu", "nu", "mu_t", "gamma_t", "c"):
                for j in range(1, s + 1):
                    got, want = getattr(tab, name)[j - 1], ref[name][j]
                    assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (s, name, j, got, want)
            assert abs(tab.beta - ref["beta"]) <= 1e-13 * ref["beta"]
            assert abs(tab.c[-1] - 1.0) <= 1e-12                                    # consistency: the last stage stands at t + h
            assert all(q == 0.0 for q in tab.kappa) if order == 1 else tab.kappa[0] == 0.0          # set, not computed
            assert all(q == 0.0 for q in tab.gamma_t) if order == 1 else True
            for name in ("kappa", "mu", "nu", "mu_t", "gamma_t"):          # rounded once to fp32: the values are the method
                assert all(float(torch.tensor(q, dtype=torch.float32)) == q for q in getattr(tab, name))
            # the consistency of the ROUNDED method, checked on its own (the restatement repeats the rule): kappa + mu + nu is exactly 1, the
            # coefficient that carries the correction lies within 2^-22 of the formula's rounded value (the half ulps of mu < 4, nu < 2 and of itself), and a constant
            # state stays constant bit for bit -- R(0) = 1
            for j in range(1, s):
                assert tab.kappa[j] + tab.mu[j] + tab.nu[j] == 1.0, (s, j)
            plain = K.table_loop(s, order, eps, consistent=False)
            for name in ("kappa", "nu"):
                assert all(abs(getattr(tab, name)[j - 1] - plain[name][j]) <= 2.0 ** -22 for j in range(1, s + 1)), (s, name)
            assert all(abs(q) < 4.0 for q in tab.mu) and all(abs(q) < 2.0 for q in tab.nu + tab.kappa)
            one = torch.ones(3, 1, dtype=torch.float64)
            sol = (nd.RKC1 if order == 1 else nd.RKC2)(s, eps)
            assert torch.equal(sol._step_state(lambda t0, xt, zt, all_initial: 0.0 * xt, 0.0, 1.0, 1.0, one), one)
    for bad in ([4], {"s": 4}, 4.0, "4", None, True):          # refused with the documented error, whatever the type
        with pytest.raises(ValueError):
            fused.rkc_table(bad, order)
    for bad in ([0.1], "0.1", True, 0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            fused.rkc_table(4, order, bad)
    assert fused.rkc_table(1, 1).mu_t == (1.0,)                                     # s = 1: Euler
    assert fused.rkc_table(8, 1) is fused.rkc_table(8, 1) and hash(fused.rkc_table(8, 2)) != hash(fused.rkc_table(8, 1))
    b1 = [fused.rkc_table(s, 1).beta / s ** 2 for s in STAGES]
    b2 = [fused.rkc_table(s, 2).beta / s ** 2 for s in STAGES if s >= 4]
    assert all(abs(q - 1.936) < 5e-3 for q in b1) and all(0.61 <= q <= 0.655 for q in b2)


def test_rkc1_with_one_stage_is_bitwise_the_euler_walk():
    case = K.ode_fwd_case("reg", 1, 1)
    de, t, x, z, ev, zj = case
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        e = nd.Euler()
        e.fused = "off"
        for tx in (False, True):
            assert torch.equal(C.run_ode(K.solver(1, 1, "off"), de, t, x, z, a0, ev, zj, tx), C.run_ode(e, de, t, x, z, a0, ev, zj, tx))
        dcase = K.dae_fwd_case("x5z4v6i6", 1, 1)
        got, want = C.run_dae(K.solver(1, 1, "off"), *dcase), C.run_dae(e, *dcase)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ----------------------------------------------------------------------------- 2. stability and order
def _linear(lam):
    return lambda t0, xt, zt, all_initial: lam * xt


def _walk_linear(solver, hl, steps=1):
    """x' = lambda x through the walk with a plain callable: h = 1, lambda = hl [N] as a batch of N trajectories"""
    N = hl.numel()
    t = torch.arange(steps + 1, dtype=torch.float64).view(-1, 1, 1).repeat(1, N, 1)
    x = torch.ones(steps + 1, N, 1, dtype=torch.float64)
    return solver.integrate_ODE(_linear(hl.view(N, 1)), t, x, torch.zeros(steps + 1, N, 0, dtype=torch.float64), None)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("s", STAGES)
def test_the_amplification_stays_within_one_up_to_the_boundary(order, s):
    sol = K.solver(order, s, "off")
    hl = torch.linspace(-0.98 * sol.method.beta, 0.0, 2000, dtype=torch.float64)
    amp = _walk_linear(sol, hl)[1].abs().view(-1)
    print(order, s, f"beta {sol.method.beta:.4f}, max |R| {float(amp.max()):.6f}")
    assert float(amp.max()) <= 1.0


def test_eight_evaluations_at_h_lambda_minus_100():
    hl = torch.tensor([-100.0], dtype=torch.float64)
    e = nd.Euler(substeps=8)
    e.fused = "off"
    assert float(_walk_linear(e, hl, 10).abs().max()) > 1e6
    assert float(_walk_linear(K.solver(1, 8, "off"), hl, 10).abs().max()) <= 1.0


@pytest.mark.parametrize("order,s", [(1, 3), (1, 8), (2, 2), (2, 4), (2, 8)])
def test_observed_order_on_a_tanh_mlp(order, s):
    """the rule of test_rk_tableau_host: at least order - 0.5 per doubling from h = 1/16 to 1/128, against a 16 x finer RK4Classic run.
    (The coefficients are fp32 values: the method they define meets its order conditions to 6e-8, an error floor of that size that no step
    removes -- with the default initialisation RKC2 with 8 stages reaches it at h = 1/32: 4.5e-7, 6.2e-8, 5.9e-8, 7.5e-8.  The weights are
    therefore scaled by 3: a right-hand side whose truncation error stays two orders above that floor down to h = 1/128.)"""
    torch.manual_seed(11)
    de = models.DE_Func(3 + 2, (16, 16), 3, activation=nn.Tanh).double()
    with torch.no_grad():
        for p in de.parameters():
            p.mul_(3.0)
    g = torch.Generator().manual_seed(12)
    x0, z0 = torch.randn(4, 3, generator=g, dtype=torch.float64), torch.randn(4, 2, generator=g, dtype=torch.float64)
    a0 = torch.cat((x0, z0), -1)

    def run(solver, n):
        t = torch.linspace(0.0, 1.0, n + 1, dtype=torch.float64).view(-1, 1, 1).repeat(1, 4, 1)
        x = x0.unsqueeze(0).repeat(n + 1, 1, 1)
        solver.fused = "off"
        with torch.no_grad():
            return solver.integrate_ODE(de, t, x, z0.unsqueeze(0).repeat(n + 1, 1, 1), a0)[-1]

    ref = run(nd.RK4Classic(), 128 * 16)
    errs = [float((run(K.solver(order, s, "off"), n) - ref).abs().max()) for n in (16, 32, 64, 128)]
    rates = [math.log2(errs[k] / errs[k + 1]) for k in range(3)]
    print(order, s, errs, rates)
    assert all(r >= order - 0.5 for r in rates)


# ----------------------------------------------------------------------------- 3. the walk against the restatement
@pytest.mark.parametrize("order,s", K.METHODS + K.WIDE)
def test_walk_equals_the_restatement_ode(order, s):
    for pad in (False, True):
        for tx in (False, True):
            de, t, x, z, ev, zj = K.ode_fwd_case("reg", order, s, pad=pad)
            d64 = C.deepcopy(de).double()
            with torch.no_grad():
                want = K.ref_ode(order, s, d64, t.double(), x.double(), z.double(), ev.double(), zj.double(), tx)
            got = C.ode_walk64(K.solver(order, s, "off"), de, t, x, z, ev, zj, tx)
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("order,s", [(1, 3), (2, 2), (2, 5)])
@pytest.mark.parametrize("mode", ["no_x", "tx0_ti0", "tx1_ti0", "tx0_ti1", "tx1_ti1"])
def test_walk_equals_the_restatement_dae(mode, order, s):
    case = K.dae_fwd_case("x5z4v6i6", order, s, no_x=mode == "no_x")
    tx, ti = "tx1" in mode, "ti1" in mode
    case64 = (C.deepcopy(case[0]).double(), C.deepcopy(case[1]).double()) + tuple(C.to64(q) for q in case[2:])
    with torch.no_grad():
        want = K.ref_dae(order, s, case64, tx, ti)
    got = C.dae_walk64(K.solver(order, s, "off"), case, tx, ti)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("ti", [False, True])
def test_head_evaluations_per_interval(ti):
    s = 4
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = C.dae_case(5, 4, 6, 6, (16,), (16,), 3, K.T0, seed=5, t=K.clock(K.T0, 3), ev_rows=())
    calls = []
    head = lambda **kw: (calls.append(1), ae(**kw))[1]
    with torch.no_grad():
        K.solver(1, s, "off").integrate_DAE(x_init=x_init, x_func=de, i_func=head, t=t, x=x, z=z, v=v, i=i, all_initial=a0, input_true_i=ti)
    grid_heads = K.T0          # one per grid point
    assert len(calls) - grid_heads == (0 if ti else (K.T0 - 1) * (s - 1))


# ----------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("cls", [nd.RKC1, nd.RKC2])
def test_constructor_refusals(cls):
    lo = 1 if cls is nd.RKC1 else 2
    ok = cls(lo)
    assert ok.order == (1 if cls is nd.RKC1 else 2) and isinstance(ok.method, fused.Recurrence) and ok.method.stages == lo and ok.substeps == 1
    assert cls(32).method.stages == 32 and cls(stages=4, damping=0.2).method != cls(4).method
    for kw in (dict(substeps=2), dict(externals="linear"), dict(externals="lagrange"), dict(segment=3), dict(segment=3, segment_parallel=2)):
        with pytest.raises(ValueError):
            cls(4, **kw)
    for bad in (lo - 1, 0, -1, 33, True, 2.0, "3", None, [4]):
        with pytest.raises(ValueError):
            cls(bad)
    for bad in (0, 0.0, -0.1, "x", True):
        with pytest.raises(ValueError):
            cls(4, damping=bad)
    assert {"RKC1", "RKC2"} <= set(nd.__all__)


def test_options_and_routing():
    m = nd.RKC2(5).method
    o = fused.GenericOpts.of(m, (None,))
    assert o.family == "rkc" and o.tab is m and o.substeps == 5 and o.stages == 1 and fused.FAMILIES["rkc"].rkc and fused.FAMILIES["rkc"].x_sub
    assert fused.GenericOpts.of(m, (None,), 5) == o          # (the stage count a saved call hands on)
    assert [f.name for f in dataclasses.fields(fused.GenericOpts)][-2:] == ["ab", "family"]
    assert fused.EXTERNALS == ("hold", "linear", "lagrange")
    for kw in (dict(substeps=2), dict(externals="linear"), dict(segment=2)):
        with pytest.raises(ValueError):
            fused.GenericOpts.of(m, (None,), **kw)
    r = o.c_args()[-1]._obj
    assert isinstance(r, _lib.RkcF32) and r.stages == 5 and not r.x_stage and list(r.mu)[:5] == list(m.mu) and list(r.gamma_t)[:5] == list(m.gamma_t)
    o.require_generic("x", "auto", False)
    o.require_generic("x", "generic", False)
    for kernel, saved in (("wave", False), ("tile", False), ("mfma", False), ("wide", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="Chebyshev"):
            o.require_generic("x", kernel, saved)
    with pytest.raises(_lib.UnsupportedShapeError, match="Chebyshev"):
        o.require_plain("a specialised entry")
    with pytest.raises(_lib.UnsupportedShapeError, match="Chebyshev"):
        fused.builtin_method(m, "x")
    pt = fused.GenericOpts.of(m, (None,), per_trajectory=True)
    assert pt.family == "none"
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
        pt.require_generic("x", "auto", False)
    assert autograd._FAMILY_CLASSES["rkc"] == "Rkc" and autograd._FusedOdeRkc.__mro__[1] is autograd._FusedOdeGeneric
    assert autograd._FusedDaeRkc.__mro__[1] is autograd._FusedDaeGeneric
    for kernel in ("auto", "generic"):
        s = K.solver(1, 4, "require", kernel)
        assert s._generic_only_ok("integrate_ODE", (None,))
    for kernel in ("wave", "tile", "mfma", "wide"):
        s = K.solver(1, 4, "auto", kernel)
        assert not s._generic_only_ok("integrate_ODE", (None,))
        s.fused = "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="Chebyshev"):
            s._generic_only_ok("integrate_ODE", (None,))
    s = K.solver(1, 4, "auto")
    assert not s._generic_only_ok("integrate_ODE", (None,), True)          # per-trajectory events: no kernel
    s.fused = "require"
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
        s._generic_only_ok("integrate_ODE", (None,), True)
    t = torch.zeros(3, 4, 1)
    mo = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RKC1(3))
    assert mo._forward_encoded(t, torch.zeros(3, 4, 8), torch.zeros(3, 4, 2), None, None) is None


def test_training_predicates():
    ode01 = A.hip_layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    n = 8 + 2 + 2 + 2
    de = A.hip_layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = A.hip_layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    for m in (nd.RKC1(1).method, nd.RKC1(8).method, nd.RKC2(5).method):
        assert autograd.ode_training_supported(m, ode01, 8, 2, 50, 33)
        assert autograd.ode_training_supported(m, ode01, 8, 2, 50, 33, kernel="generic", act=tanh)
        assert autograd.ode_training_supported(m, ode01, 8, 2, 50, 33, input_true_x=True)
        assert not autograd.ode_training_supported(m, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True)
        assert autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33)
        for tx, ti in ((True, False), (False, True), (True, True)):
            assert autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti)
            assert not autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), input_true_x=tx, input_true_i=ti)
        for kernel in ("wave", "tile", "mfma", "wide"):
            assert not autograd.ode_training_supported(m, ode01, 8, 2, 50, 33, kernel=kernel)
            assert not autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel)
        assert fused.ode_save_hidden(m, ode01, 8, 2) == 0 and fused.dae_save_hidden(m, de, ae, 8, 2, 2, 2) == 0


# ----------------------------------------------------------------------------- 5. the C ABI, dims only
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))


def _rkc(stages, x_stage=None, order=1):
    r = fused.rkc_table(min(max(stages, order), 32), order).abi(x_stage)
    r.stages = stages
    return r


def _q(lib, stem, a, n_act, rkc, act=None):
    return getattr(lib, f"psnode_{stem}_rkc_supported")(R(a), *([act] * n_act), R(rkc) if rkc is not None else None)


def _f(lib, stem, a, n_act, rkc, act=None):
    return getattr(lib, f"psnode_{stem}_rkc_f32")(R(a) if a is not None else None, *([act] * n_act), R(rkc) if rkc is not None else None, None, 0, None)


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION and _lib.RKC_MAX_STAGES == 32
    for name in RKC_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert len([n for n in _lib.EXPORTS if "_rkc_" in n]) == 9 and not any(n.endswith("_rkc_workspace_bytes") for n in _lib.EXPORTS)
    p = ctypes.POINTER(_lib.RkcF32)
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_rkc_supported").argtypes[-1] == p
        assert getattr(lib, f"psnode_{stem}_rkc_f32").argtypes[1 + n_act] == p and len(getattr(lib, f"psnode_{stem}_rkc_f32").argtypes) == 5 + n_act
    assert lib.psnode_dae_backward_rkc_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert lib.psnode_dae_backward_rkc_workspace_size.restype is ctypes.c_size_t
    r = _lib.RkcF32
    assert (r.stages.offset, r.kappa.offset, r.mu.offset, r.nu.offset, r.mu_t.offset, r.gamma_t.offset, r.x_stage.offset, ctypes.sizeof(r)) == \
        (0, 4, 132, 260, 388, 516, 648, 656)


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_argument_checks_are_the_sub_familys(stem, make, n_act):
    """status for status what the _sub entry point answers for the same sub-step count (NULL struct, a bad count, NULL args, a forced
    kernel, an unknown activation), except that no stage count forwards to another family and that `method` is never read"""
    lib = _lib.load()
    sub_call, sub_q = functools.partial(A.call, family="sub"), functools.partial(A.supported, family="sub")
    assert _f(lib, stem, make(), n_act, None) == -1 == sub_call(lib, stem, make(), n_act, None, None) and _q(lib, stem, make(), n_act, None) == 0
    for n in (0, -3, 33, 1025):
        assert _f(lib, stem, make(), n_act, _rkc(n)) == -2 == sub_call(lib, stem, make(), n_act, None, A.sub(n if n != 33 else 1025))
        assert _q(lib, stem, make(), n_act, _rkc(n)) == 0
    for n, order in ((1, 1), (2, 1), (2, 2), (5, 2), (32, 1), (32, 2)):
        r = _rkc(n, order=order)
        assert _q(lib, stem, make(), n_act, r) == 1 and _q(lib, stem, make(kernel=_lib.KERNEL_GENERIC), n_act, r) == 1
        assert _q(lib, stem, make(method=77), n_act, r) == 1                               # (the method is not read)
        assert _f(lib, stem, make(), n_act, r) == -1                                       # as far as the pointer checks, nothing launched
        for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
            assert _q(lib, stem, make(kernel=kernel), n_act, r) == 0 == sub_q(lib, stem, make(kernel=kernel), n_act, None, A.sub(3))
            assert _f(lib, stem, make(kernel=kernel), n_act, r) == -5 == sub_call(lib, stem, make(kernel=kernel), n_act, None, A.sub(3))
    assert _f(lib, stem, None, n_act, _rkc(3)) == -1
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _f(lib, stem, make(), n_act, _rkc(3), R(unknown)) == -3 == sub_call(lib, stem, make(), n_act, None, A.sub(3), R(unknown))
    for kind in (_lib.ACT_TANH, _lib.ACT_SIGMOID, _lib.ACT_RELU, _lib.ACT_LEAKY_RELU, _lib.ACT_SOFTPLUS, _lib.ACT_SILU, _lib.ACT_GELU,
                 _lib.ACT_GELU_TANH, _lib.ACT_MISH):
        assert _q(lib, stem, make(), n_act, _rkc(4), R(fused.Act(kind).abi())) == 1          # all ten kinds (ELU above)


def test_side_outputs_teacher_forced_activations_and_a_missing_stage_buffer_are_refused():
    lib = _lib.load()
    r = _rkc(3)
    a = _ode_args()
    a.save_act = a.save_xstage = 256
    assert _q(lib, "ode_integrate", a, 1, r) == 0 and _f(lib, "ode_integrate", a, 1, r) == -5
    b = _ode_bwd_args()
    b.saved_act = b.saved_xstage = 256
    assert _q(lib, "ode_backward", b, 1, r) == 0 and _f(lib, "ode_backward", b, 1, r) == -5
    e = _dae_bwd_args()
    e.base.saved_act = 256
    assert _q(lib, "dae_backward", e, 2, r) == 0 and _f(lib, "dae_backward", e, 2, r) == -5
    assert lib.psnode_dae_backward_rkc_workspace_size(R(e), None, None, R(r)) == 0
    assert lib.psnode_dae_backward_rkc_workspace_size(R(_dae_bwd_args()), None, None, None) == 0
    size = lib.psnode_dae_backward_rkc_workspace_size(R(_dae_bwd_args()), None, None, R(r))
    assert size > 0 and size == lib.psnode_dae_backward_sub_workspace_bytes(R(_dae_bwd_args()), None, None, None, R(A.sub(3)))
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    tfo = _ode_bwd_args(flags=_lib.FLAG_INPUT_TRUE_X)
    assert _q(lib, "ode_backward", tfo, 1, r) == 1 and _q(lib, "ode_backward", tfo, 1, r, tanh) == 0 and _f(lib, "ode_backward", tfo, 1, r, tanh) == -5
    for flags in (1, 2, 3):
        tfd = _dae_bwd_args(flags=flags)
        assert _q(lib, "dae_backward", tfd, 2, r) == 1 and _q(lib, "dae_backward", tfd, 2, r, tanh) == 0
        one = _dae_bwd_args(flags=flags)
        one.base.T = 1
        assert _f(lib, "dae_backward", one, 2, r) == -2
    # a backward call with every other pointer in place and no stage buffer: PSNODE_ERR_NULL before the workspace is looked at
    b = _ode_bwd_args()
    for l in range(4):
        b.de.weight[l] = b.de.bias[l] = 256
    b.t.ptr = b.z.ptr = b.all_initial = b.xs = b.grad_xs = b.grad_x0 = b.grad_all_initial = b.grad_params = 256
    assert _f(lib, "ode_backward", b, 1, _rkc(2)) == -1
    assert _f(lib, "ode_backward", b, 1, _rkc(2, 256)) == -4          # with one: as far as the workspace check
    assert _f(lib, "ode_backward", b, 1, _rkc(1)) == -4               # one stage keeps no rows
    e = _dae_bwd_args()
    q = e.base
    for m in (q.de, q.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
    q.grad_params_de = q.grad_params_ae = 256
    assert _f(lib, "dae_backward", e, 2, _rkc(2)) == -1 and _f(lib, "dae_backward", e, 2, _rkc(2, 256)) == -4


def test_lds_fit_is_the_sub_builds():
    """no LDS region of its own (the coefficients are read from the kernel's argument segment): the fit answers as the _sub family's"""
    lib = _lib.load()
    for hidden, xd in ((64, 8), (512, 8), (1024, 8), (1024, 64), ((1024,) * 7, 200)):
        for stem, make, n_act in ENTRIES:
            kw = dict(hidden=hidden, xd=xd)
            assert _q(lib, stem, make(**kw), n_act, _rkc(4)) == A.supported(lib, stem, make(**kw), n_act, None, A.sub(4), family="sub"), (stem, hidden, xd)


# ----------------------------------------------------------------------------- 6. the rounding floor of the GPU cases
def _assert_floor(d, what):
    print(f"{what}: d = {d:.3e}")
    assert 4 * d <= TOL_GPU, f"{what}: 4 d = {4 * d:.3e} > TOL_GPU"


@pytest.mark.parametrize("order,s", K.METHODS)
def test_forward_cases_of_the_gpu_suite_round_below_the_plain_gate(order, s):
    for shape in C.ODE_FWD_SHAPES:
        _assert_floor(K.ode_floor(order, s, K.ode_fwd_case(shape, order, s)), f"ode {shape}")
    _assert_floor(K.ode_floor(order, s, K.ode_fwd_case("reg", order, s, pad=True)), "ode padded")
    if (order, s) in ((1, 3), (2, 5)):          # the edge shapes of the GPU suite
        _assert_floor(K.ode_floor(order, s, K.ode_fwd_case("reg", order, s, pad=True), tx=True), "ode padded, teacher-forced")
        for B, Tn in ((K.B0, 2), (16, K.T0), (1, K.T0)):
            _assert_floor(K.ode_floor(order, s, K.ode_fwd_case("reg", order, s, B=B, Tn=Tn)), f"ode B={B} T={Tn}")
    for shape in C.DAE_SHAPES:
        for tx, ti in ((False, False), (True, False), (False, True), (True, True)):
            _assert_floor(K.dae_floor(order, s, K.dae_fwd_case(shape, order, s), tx, ti), f"dae {shape} tx={tx} ti={ti}")


@pytest.mark.parametrize("order,s", K.TRAIN_METHODS)
def test_training_cases_of_the_gpu_suite_round_below_the_plain_gate(order, s):
    sol = functools.partial(K.solver, order, s)
    runs = []
    for xd, zd, H, nh in K.K5_ODE_SHAPES:
        runs.append((f"ode {xd}/{zd}/{H}x{nh}", K.ode_train_case(xd, zd, H, nh, order, s), False))
    runs.append(("ode no events", K.ode_train_case(8, 2, 64, 3, order, s, events=False), False))
    runs.append(("ode tx", K.ode_train_case(8, 2, 64, 3, order, s), True))
    for what, case, tx in runs:
        G, = C.cotangents(3, case[2].shape)
        _, g32 = K.ode_train_dtype(sol, case, G, torch.float32, tx)
        _, g64 = K.ode_train_dtype(sol, case, G, torch.float64, tx)
        for k, d in K.grad_floors(g32, g64).items():
            _assert_floor(d, f"{what} grad {k}")
    druns = [(f"dae {shape}", K.dae_train_case(shape, order, s), False, False) for shape in C.K5_DAE_SHAPES]
    druns.append(("dae no events", K.dae_train_case("reg", order, s, events=False), False, False))
    druns += [(f"dae tx={tx} ti={ti}", K.dae_train_case("zvi16", order, s), tx, ti) for tx, ti in ((True, False), (False, True), (True, True))]
    for what, case, tx, ti in druns:
        G, Gi = C.cotangents(4, case[3].shape, case[6].shape)
        _, _, g32 = K.dae_train_dtype(sol, case, G, Gi, torch.float32, tx, ti)
        _, _, g64 = K.dae_train_dtype(sol, case, G, Gi, torch.float64, tx, ti)
        for k, d in K.grad_floors(g32, g64).items():
            _assert_floor(d, f"{what} grad {k}")
