"""Stage-wise algebraic heads (solver.algebraic = "stage") without a GPU: the walk that defines them, its order, its adjoint, the
refusals, the C ABI's argument checks from the dims alone, the routing predicates -- and the precondition of the GPU test.

algebraic="step" is the walk as it was; "stage" evaluates the head in front of every stage s >= 1 at that stage's argument and
interpolated externals (tests/stage_head_cases.py says it once more, stand-alone)."""
import copy
import ctypes

import pytest
import torch

import capi_args as A
import generic_cases as C
import stage_head_cases as S
from capi_args import R
from capi_args import sub as _sub
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd
from py_psnode_amd.neural_dae import my_fixed_grid as fg


def _c64(case):
    return (copy.deepcopy(case[0]).double(), copy.deepcopy(case[1]).double(), *(C.to64(q) for q in case[2:]))


def _walk(s, case, tx=False, ti=False):
    with torch.no_grad():
        return C.run_dae(s, *case, tx, ti)


# ----------------------------------------------------------------------------- 1. bitwise no-ops
def _walk_dae_before(s, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i):
    """FixedGridODESolver._walk_dae's interpolated-externals arm as it stood before `algebraic` existed (shared events, no segments), on
    the step formulas as they stood: `_step_func_lin` without its keyword."""
    cur_x = x_init
    cur_i = i_func(xt=x[0] if input_true_x else cur_x, zt=z[0], vt=v[0], all_initial=all_initial)
    xs = torch.zeros(x.shape, dtype=x.dtype)
    is_ = torch.zeros(i.shape, dtype=i.dtype)
    xs[0], is_[0] = cur_x, cur_i
    lag = s._lag_walk("integrate_DAE", t, event_fn, jump_change_fn, (z, v))
    for k in range(t.shape[0] - 1):
        t0, t1, zk, vk = t[k], t[k + 1], z[k], v[k]
        if lag.hits[k] if lag is not None else (event_fn is not None and event_fn(t0) == True):  # noqa: E712
            zk, vk = lag.jumped[k] if lag is not None else jump_change_fn(t0, zk, vk)
            cur_i = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
        start = x[k] if input_true_x else cur_x
        i_in = i[k] if input_true_i else cur_i
        h = (t1 - t0) / s.substeps
        cur_x = start
        for j in range(s.substeps):
            ext_at = s._lin_ext(j, s.substeps, (zk, vk), (z[k + 1], v[k + 1])) if lag is None else lag.ext_at(k, j, s.substeps)
            if j > 0 and not input_true_i:
                zj_, vj_ = ext_at(0.0)
                i_in = i_func(xt=cur_x, zt=zj_, vt=vj_, all_initial=all_initial)
            cur_x = cur_x + s._step_func_lin(func=x_func, t0=t0 + j * h if j else t0, dt=h, x0=cur_x, ext_at=ext_at, i0=i_in, all_initial=all_initial)
        cur_i = i_func(xt=x[k + 1] if input_true_x else cur_x, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
        xs[k + 1], is_[k + 1] = cur_x, cur_i
    return xs, is_


def _g3_case(n):
    """a G3-style batch: perturbed x_init, events at rows 0 and 3, a ragged padded clock"""
    return C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), 7, 6, seed=9 + n, ev_rows=(0, 3), perturb_x_init=True, pad=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Heun2", "Kutta3", "RK4Classic"])
def test_step_is_the_walk_as_it_was_bit_for_bit(name, ext, n):
    case = _g3_case(n)
    de, ae, t, x, z, v, i, xi, a0, ev, zj, vj = case
    for tx, ti in ((False, False), (True, False), (False, True), (True, True)):
        s = S.solver(name, n, ext, "step")
        event = nd.DAE_Event()
        event.set_event(ev, zj, vj)
        with torch.no_grad():
            ref = _walk_dae_before(s, xi, de, ae, t, x, z, v, i, a0, event.event_fn, event.jump_change_fn, tx, ti)
        got = _walk(s, case, tx, ti)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (tx, ti)
        assert torch.equal(_walk(_default_solver(name, n, ext), case, tx, ti)[0], ref[0])          # the default IS "step"


def _default_solver(name, n, ext):
    s = S.SOLVERS[name](substeps=n, externals=ext)
    s.fused = "off"
    assert s.algebraic == "step"
    return s


@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 3])
def test_one_stage_methods_and_input_true_i_under_stage_are_the_step_walk_bit_for_bit(n, ext):
    case = _g3_case(n)
    for name, tx, ti in (("euler", False, False), ("euler", True, False), ("rk4", False, True), ("RK4Classic", True, True), ("Kutta3", False, True)):
        a, b = _walk(S.solver(name, n, ext, "stage"), case, tx, ti), _walk(S.solver(name, n, ext, "step"), case, tx, ti)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, tx, ti)
    one = nd.ExplicitRK(((),), (1.0,), 1, substeps=n, externals=ext, algebraic="stage")
    one.fused = "off"
    assert not one._stage_heads() and torch.equal(_walk(one, case)[0], _walk(S.solver("euler", n, ext, "step"), case)[0])
    # ... and the routing says the same: such a call carries no `algebraic` to the fused entries
    assert S.solver("euler", n, ext)._generic_kwargs(False, S.solver("euler", n, ext)._stage_heads()).get("algebraic") is None
    s = S.solver("rk4", n, ext)
    assert s._stage_heads() and not s._stage_heads(True)
    assert s._generic_kwargs(False, True)["algebraic"] == "stage" and "algebraic" not in s._generic_kwargs(False, s._stage_heads(True))
    assert "algebraic" not in S.solver("rk4", n, ext, "step")._generic_kwargs()


def test_integrate_ode_ignores_the_option():
    de, t, x, z, ev, zj = C.ode_case(6, 2, (32, 32), 7, 6, seed=8, ev_rows=(0, 3))
    a0 = torch.cat((x[0], z[0]), -1)
    for ext in S.INTERP:
        with torch.no_grad():
            outs = [C.run_ode(S.solver("RK4Classic", 2, ext, alg), de, t, x, z, a0, ev, zj) for alg in fused.ALGEBRAIC]
        assert torch.equal(outs[0], outs[1])
    assert fused.GenericOpts.of(nd.RK4Classic().method, (None,), 2, "linear", False, None, None, "stage").family == "lin"


# ----------------------------------------------------------------------------- 2. the stand-alone restatement, fp64
@pytest.mark.parametrize("tx", [False, True])
@pytest.mark.parametrize("ext", S.INTERP)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", S.METHODS)
def test_walk_equals_the_stand_alone_restatement_fp64(name, n, ext, tx):
    """events at step 0 and at an interior step, a -1-padded clock, with and without input_true_x"""
    case = _c64(S.forward_case("reg", n, Tn=7, B=5, pad=True))
    got = _walk(S.solver(name, n, ext), case, tx)
    with torch.no_grad():
        ref = S.restate_dae(name, n, ext, case, tx)
    for a, b, what in zip(got, ref, ("xs", "is")):
        err = float((a - b).abs().max())
        assert err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)
    step = _walk(S.solver(name, n, ext, "step"), case, tx)
    assert float((got[0] - step[0]).abs().max()) > 1e-6          # the restatement is not the frozen walk's


# ----------------------------------------------------------------------------- 3. the order gates, fp64
# The project's gate (tests/test_rk_tableau_host.py): observed order >= order - 0.5 per doubling.  The coarsest doubling (9 -> 17 points) is
# left out, as in tests/test_externals_lagrange_host.py: at h = 1 / 8 the frozen-head Heun step is pre-asymptotic -- its second-order terms
# still outweigh the O(h) term the freeze adds, so the doubling shows an order between the two (1.75) that belongs to neither.
def _orders(name, ext, alg):
    errs, orders = S.observed_orders(lambda: S.SOLVERS[name](externals=ext, algebraic=alg))
    print(name, ext, alg, "errors", errs, "orders", orders)
    return orders[1:]


def test_rk4classic_lagrange_stage_is_fourth_order_on_a_dae_and_step_is_first():
    """fp64, against the same solver on 1025 points.  Measured: stage 1.10e-5 / 7.54e-7 / 5.36e-8 / 3.56e-9 (orders 3.87 / 3.81 / 3.91);
    step 2.81e-4 / 1.40e-4 / 6.93e-5 / 3.37e-5 (orders 1.00 / 1.02 / 1.04)."""
    assert min(_orders("RK4Classic", "lagrange", "stage")) >= 3.5
    assert max(_orders("RK4Classic", "lagrange", "step")) < 1.5


def test_heun2_linear_stage_is_second_order_on_a_dae_and_step_is_first():
    """Measured: stage 5.36e-4 / 1.34e-4 / 3.34e-5 / 8.32e-6 (orders 2.00 / 2.00 / 2.00); step 6.35e-4 / 1.89e-4 / 7.19e-5 / 3.43e-5
    (orders 1.75 / 1.39 / 1.07)."""
    assert min(_orders("Heun2", "linear", "stage")) >= 1.5
    assert max(_orders("Heun2", "linear", "step")) < 1.5


# ----------------------------------------------------------------------------- 4. the adjoint
@pytest.mark.parametrize("events", [True, False])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["Heun2", "Kutta3", "RK4Classic", "rk4"])
def test_autograd_through_the_walk_equals_the_reverse_recursion_by_hand(name, n, events):
    case = S.forward_case("reg", n, Tn=5, B=3, events=events)
    Gx, Gi = C.cotangents(3, (5, 3, 8), (5, 3, 2))
    _, _, ref = C.dae_train(lambda mode: S.solver(name, n, "linear", "stage", mode), case, Gx, Gi, "cpu")
    got = S.adjoint_by_hand(name, n, _c64(case), Gx.double(), Gi.double())
    for k, g in got.items():
        if g is None:
            assert ref[k] is None
            continue
        err = float((g - ref[k]).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref[k].abs().max())), (k, err)


# ----------------------------------------------------------------------------- 5. refusals
def test_constructor_refusals_name_their_reason():
    assert fused.ALGEBRAIC == ("step", "stage")
    for bad in ("stages", None, 1, "hold"):
        with pytest.raises(ValueError, match="algebraic must be one of"):
            nd.RK4Classic(externals="linear", algebraic=bad)
    for cls in (nd.Euler, nd.Midpoint, nd.RK4, nd.Heun2, nd.RK4Classic):
        with pytest.raises(ValueError, match="held rows cap every"):
            cls(algebraic="stage")
        with pytest.raises(ValueError, match="held rows cap every"):
            cls(algebraic="stage", externals="hold", substeps=3)
        assert cls(algebraic="stage", externals="linear").algebraic == "stage" and cls().algebraic == "step"
    for cls in (nd.AB2, nd.AB3):
        with pytest.raises(ValueError, match="grid points only"):
            cls(algebraic="stage")
    for cls, st in ((nd.RKC1, 4), (nd.RKC2, 4)):
        with pytest.raises(ValueError, match="already evaluates the algebraic head"):
            cls(st, algebraic="stage")
        assert cls(st).algebraic == "step"
    # the options value refuses the same pairs
    rk4 = nd.RK4Classic().method
    with pytest.raises(ValueError, match="algebraic must be one of"):
        fused.GenericOpts.of(rk4, (None, None), 1, "linear", False, None, None, "both")
    with pytest.raises(ValueError, match="held rows"):
        fused.GenericOpts.of(rk4, (None, None), 1, "hold", False, None, None, "stage")
    with pytest.raises(ValueError, match="grid points only"):
        fused.GenericOpts.of("ab2", (None, None), 1, "hold", False, None, None, "stage")
    with pytest.raises(ValueError, match="already evaluates"):
        fused.GenericOpts.of(nd.RKC1(4).method, (None, None), 1, "hold", False, None, None, "stage")


def test_a_step_formula_without_the_keyword_is_refused_under_stage_only():
    class Old(nd.Midpoint):
        def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
            return super()._step_func_lin(func, t0, dt, x0, ext_at, i0, all_initial)

    case = _g3_case(1)
    for alg in fused.ALGEBRAIC:
        s = Old(externals="linear", algebraic=alg)
        s.fused = "off"
        if alg == "step":
            assert torch.equal(_walk(s, case)[0], _walk(S.solver("midpoint", 1, "linear", "step"), case)[0])
        else:
            with pytest.raises(NotImplementedError, match="head"):
                _walk(s, case)
    # head=None leaves every statement as it is: the formulas called directly
    f = lambda **kw: kw["xt"] * 0.5 + kw["zt"].sum(-1, keepdim=True)
    ext_at = lambda c: (torch.full((2, 1), c), torch.zeros(2, 1))
    x0 = torch.ones(2, 3)
    for name in S.SOLVERS:
        s = S.solver(name)
        assert torch.equal(s._step_func_lin(f, 0.0, 0.1, x0, ext_at, i0=torch.zeros(2, 1)), s._step_func_lin(f, 0.0, 0.1, x0, ext_at, i0=torch.zeros(2, 1), head=None))
    assert fg._rhs_at(f, ext_at, None, None, None).__name__ == "f"


# ----------------------------------------------------------------------------- 6. the C ABI from the dims alone
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_, _dae_args, _, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("dae_integrate", _dae_args), ("dae_backward", _dae_bwd_args))
STH_EXPORTS = ("psnode_dae_integrate_sth_supported", "psnode_dae_integrate_sth_f32", "psnode_dae_backward_sth_supported",
               "psnode_dae_backward_sth_workspace_size", "psnode_dae_backward_sth_f32")
ST = 256      # a stencil "pointer": the checks never follow it
LINEAR, LAGRANGE = fused.EXT_LINEAR, fused.EXT_LAGRANGE


def _tail(tab, sub, act, st, interp):
    return [act, act, tab, R(sub) if sub is not None else None, st, interp]


def _supported(lib, stem, a, tab=None, sub=None, act=None, st=None, interp=LINEAR):
    return getattr(lib, f"psnode_{stem}_sth_supported")(R(a), *_tail(tab, sub, act, st, interp))


def _call(lib, stem, a, tab=None, sub=None, act=None, st=None, interp=LINEAR):
    return getattr(lib, f"psnode_{stem}_sth_f32")(R(a) if a is not None else None, *_tail(tab, sub, act, st, interp), None, 0, None)


def _sibling(interp):
    return "lag" if interp == LAGRANGE else "lin"


def _sib_tail(tab, sub, act, st, interp):
    return [act, act, tab, R(sub) if sub is not None else None] + ([st] if interp == LAGRANGE else [])


def _sib_supported(lib, stem, a, tab, sub, act, st, interp):
    return getattr(lib, f"psnode_{stem}_{_sibling(interp)}_supported")(R(a), *_sib_tail(tab, sub, act, st, interp))


def _sib_call(lib, stem, a, tab, sub, act, st, interp):
    return getattr(lib, f"psnode_{stem}_{_sibling(interp)}_f32")(R(a) if a is not None else None, *_sib_tail(tab, sub, act, st, interp), None, 0, None)


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    header = open(A.__file__.replace("tests/capi_args.py", "include/psnode_hip.h")).read()
    for name in STH_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert not [n for n in _lib.EXPORTS if "_sth_" in n and n not in STH_EXPORTS] and not hasattr(lib, "psnode_ode_integrate_sth_f32")
    for stem in ("dae_integrate", "dae_backward"):
        lag_q, lag_c = getattr(lib, f"psnode_{stem}_lag_supported").argtypes, getattr(lib, f"psnode_{stem}_lag_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_sth_supported").argtypes == lag_q + [ctypes.c_int32]
        assert getattr(lib, f"psnode_{stem}_sth_f32").argtypes == lag_c[:-3] + [ctypes.c_int32] + lag_c[-3:]
    assert lib.psnode_dae_backward_sth_workspace_size.restype is ctypes.c_size_t
    assert fused.FAMILIES["sth"] == fused.FAMILIES["lag"]._replace(interp=True, dae_only=True)
    assert not any(tag in "_sth_" for tag in ("_act_", "_tf_", "_rk_", "_sub_", "_lin_", "_pev_", "_ab_", "_ms_"))


@pytest.mark.parametrize("interp", [LINEAR, LAGRANGE])
@pytest.mark.parametrize("stem,make", ENTRIES)
def test_sth_argument_checks_in_the_sibling_family_s_order(stem, make, interp):
    lib = _lib.load()
    tab = R(nd.Kutta3().method.abi())
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    unknown = _lib.ActF32()
    unknown.kind = 17
    tanh = R(fused.Act(_lib.ACT_TANH).abi())
    # an interpolant that is neither: PSNODE_ERR_METHOD in front of everything, NULL args included
    for wrong in (0, 3, -1):
        assert _supported(lib, stem, make(), tab, _sub(2), None, ST, wrong) == 0 and _call(lib, stem, make(), tab, _sub(2), None, ST, wrong) == -3
        assert _call(lib, stem, None, None, None, None, None, wrong) == -3
    for st in (None, ST):
        for tb in (None, tab):
            assert _supported(lib, stem, make(), tb, None, None, st, interp) == 1 and _call(lib, stem, make(), tb, None, None, st, interp) == -1
            for n in (0, -3, 1025):
                assert _call(lib, stem, make(), tb, _sub(n), None, st, interp) == -2 and _supported(lib, stem, make(), tb, _sub(n), None, st, interp) == 0
            for n in (1, 2, 3, 1024):
                assert _supported(lib, stem, make(), tb, _sub(n), None, st, interp) == 1
                assert _supported(lib, stem, make(kernel=_lib.KERNEL_GENERIC), tb, _sub(n), None, st, interp) == 1
                assert _call(lib, stem, make(), tb, _sub(n), None, st, interp) == -1          # as far as the pointer checks, nothing launched
                for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                    assert _supported(lib, stem, make(kernel=kernel), tb, _sub(n), None, st, interp) == 0
                    assert _call(lib, stem, make(kernel=kernel), tb, _sub(n), None, st, interp) == -5
            assert _call(lib, stem, None, tb, _sub(2), None, st, interp) == -1          # NULL args
        for sb in (None, _sub(1), _sub(2)):
            assert _call(lib, stem, make(method=77), None, sb, None, st, interp) == -3 and _supported(lib, stem, make(method=77), None, sb, None, st, interp) == 0
            assert _supported(lib, stem, make(method=77), tab, sb, None, st, interp) == 1
        assert _call(lib, stem, make(), R(bad), _sub(2), None, st, interp) == -3 and _supported(lib, stem, make(), R(bad), _sub(2), None, st, interp) == 0
        assert _call(lib, stem, make(), tab, _sub(2), R(unknown), st, interp) == -3
        assert _supported(lib, stem, make(), None, _sub(2), tanh, st, interp) == 1
        # a call wrong in several ways: the status is the sibling family's
        for a, tb, sb, act in ((make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(0), R(unknown)), (make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(2), R(unknown)),
                               (make(method=77, kernel=_lib.KERNEL_MFMA), None, _sub(2), None), (make(kernel=_lib.KERNEL_MFMA), R(bad), _sub(2), None),
                               (None, R(bad), _sub(2), None), (make(kernel=_lib.KERNEL_MFMA), tab, _sub(2), None)):
            assert _call(lib, stem, a, tb, sb, act, st, interp) == _sib_call(lib, stem, a, tb, sb, act, st, interp)
            if a is not None:
                assert _supported(lib, stem, a, tb, sb, act, st, interp) == _sib_supported(lib, stem, a, tb, sb, act, st, interp)


def test_side_outputs_teacher_forced_activations_a_missing_x_sub_and_the_workspace():
    lib = _lib.load()
    sub = _sub(3)
    for interp in (LINEAR, LAGRANGE):
        d = _dae_args()
        d.save_act = d.save_xstage = d.save_ae_act = 256
        assert _supported(lib, "dae_integrate", d, None, sub, None, None, interp) == 0 and _call(lib, "dae_integrate", d, None, sub, None, None, interp) == -5
        e = _dae_bwd_args()
        e.base.saved_act = 256
        assert _supported(lib, "dae_backward", e, None, sub, None, None, interp) == 0 and _call(lib, "dae_backward", e, None, sub, None, None, interp) == -5
        ws = lib.psnode_dae_backward_sth_workspace_size
        assert ws(R(e), None, None, None, R(sub), None, interp) == 0 and ws(R(_dae_bwd_args()), None, None, None, R(sub), ST, 7) == 0
        assert ws(R(_dae_bwd_args()), None, None, None, R(sub), ST, interp) == lib.psnode_dae_backward_lin_workspace_bytes(R(_dae_bwd_args()), None, None, None, R(sub)) > 0
        tanh = R(fused.Act(_lib.ACT_TANH).abi())
        for flags in (1, 2, 3):
            tfd = _dae_bwd_args(flags=flags)
            assert _supported(lib, "dae_backward", tfd, None, sub, None, None, interp) == 1
            assert _supported(lib, "dae_backward", tfd, None, sub, tanh, None, interp) == 0 and _call(lib, "dae_backward", tfd, None, sub, tanh, None, interp) == -5
            one = _dae_bwd_args(flags=flags)
            one.base.T = 1
            assert _call(lib, "dae_backward", one, None, sub, None, None, interp) == -2
        e = _dae_bwd_args()
        q = e.base
        for m in (q.de, q.ae):
            for l in range(4):
                m.weight[l] = m.bias[l] = 256
        q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
        q.grad_params_de = q.grad_params_ae = 256
        assert _call(lib, "dae_backward", e, None, _sub(2), None, None, interp) == -1          # no x_sub: PSNODE_ERR_NULL before the workspace
        assert _call(lib, "dae_backward", e, None, _sub(2, 256), None, None, interp) == -4
        assert _call(lib, "dae_backward", e, None, None, None, None, interp) == -4


def test_supported_answers_for_the_build_s_own_lds_fit():
    """The stage-heads builds keep the LDS of their interpolant's build: along a growing z_dim each query says no exactly where its sibling
    does, and the Lagrange one before the linear one."""
    lib = _lib.load()
    for stem, make in ENTRIES:
        first = {}
        for zd in range(32, 660, 4):
            a = make(kernel=_lib.KERNEL_GENERIC, xd=8, zd=zd, vd=2, idim=2, hidden=32)
            for interp in (LINEAR, LAGRANGE):
                got = _supported(lib, stem, a, None, _sub(2), None, None, interp)
                assert got == _sib_supported(lib, stem, a, None, _sub(2), None, None, interp), (stem, zd, interp)
                if not got:
                    first.setdefault(interp, zd)
        print(stem, "first z_dim refused", first)
        assert first[LAGRANGE] < first[LINEAR]


# ----------------------------------------------------------------------------- 7. the Python predicates and the routing
_layers = A.hip_layers


def test_python_predicates_the_options_value_and_require_plain():
    de = _layers(models.DAE_DE_Func(14, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(26, (64, 64, 64), 2).i_calculator)
    rk4c, heun = nd.RK4Classic().method, nd.Heun2().method
    for ext in S.INTERP:
        o = fused.GenericOpts.of(rk4c, (None, None), 2, ext, False, None, None, "stage")
        assert o.family == "sth" and o.algebraic == "stage" and o.takes is fused.FAMILIES["sth"] and o.externals == ext
        assert o != fused.GenericOpts.of(rk4c, (None, None), 2, ext) and fused.GenericOpts.of(rk4c, (None, None), 2, ext).algebraic == "step"
        assert o.c_args()[-1].value == (LAGRANGE if ext == "lagrange" else LINEAR)
        # one stage, or an ODE: the "step" families
        assert fused.GenericOpts.of("euler", (None, None), 2, ext, False, None, None, "stage").family == ("lag" if ext == "lagrange" else "lin")
        for m in ("rk4", "midpoint", rk4c, heun):
            assert fused.dae_backward_supported(m, de, ae, 8, 2, 2, 2, externals=ext, algebraic="stage")
            assert autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, externals=ext, algebraic="stage", substeps=3)
            assert autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, externals=ext, algebraic="stage", input_true_x=True)
            for kernel in ("wave", "tile", "mfma", "wide"):
                assert not autograd.dae_training_supported(m, de, ae, 8, 2, 2, 2, 50, 33, externals=ext, algebraic="stage", kernel=kernel)
                assert not fused.dae_backward_supported(m, de, ae, 8, 2, 2, 2, externals=ext, algebraic="stage", kernel=kernel)
        tanh = (fused.Act(_lib.ACT_TANH, name="Tanh"), fused.Act(_lib.ACT_SILU, name="SiLU"))
        assert autograd.dae_training_supported(rk4c, de, ae, 8, 2, 2, 2, 50, 33, externals=ext, algebraic="stage", act=tanh)
        assert not autograd.dae_training_supported(rk4c, de, ae, 8, 2, 2, 2, 50, 33, externals=ext, algebraic="stage", act=tanh, input_true_x=True)
        # per-trajectory events and segments next to interpolated externals have no kernel, with or without stage heads
        assert fused.GenericOpts.of(rk4c, (None, None), 1, ext, True, None, None, "stage").family == "none"
        assert fused.GenericOpts.of(rk4c, (None, None), 1, ext, False, 3, None, "stage").family == "none"
        with pytest.raises(_lib.UnsupportedShapeError):
            o.require_plain("dae_encoded_integrate")
        with pytest.raises(_lib.UnsupportedShapeError, match="generic kernels"):
            o.require_generic("dae_integrate", "wave", False)
        with pytest.raises(_lib.UnsupportedShapeError, match="generic kernels"):
            o.require_generic("dae_integrate", "auto", True)
    assert autograd._FAMILY_CLASSES["sth"] == "Sth" and autograd._FusedDaeSth.__mro__[1] is autograd._FusedDaeGeneric
    assert [f.name for f in __import__("dataclasses").fields(fused.GenericOpts)][-2:] == ["ab", "family"]


def test_routing_in_the_solver_and_the_models():
    for ext in S.INTERP:
        for kernel in ("auto", "generic"):
            s = S.solver("RK4Classic", 2, ext, "stage", "require", kernel)
            assert s._generic_only_ok("integrate_DAE", (None, None))
            assert s._generic_kwargs(False, s._stage_heads()) == dict(substeps=2, externals=ext, algebraic="stage")
        for kernel in ("wave", "tile", "mfma", "wide"):
            assert not S.solver("RK4Classic", 1, ext, "stage", "auto", kernel)._generic_only_ok("integrate_DAE", (None, None))          # walks, with the warning
            with pytest.raises(_lib.UnsupportedShapeError, match="generic kernels"):          # (names the first option: the tableau)
                S.solver("RK4Classic", 1, ext, "stage", "require", kernel)._generic_only_ok("integrate_DAE", (None, None))
            with pytest.raises(_lib.UnsupportedShapeError, match="externals"):
                S.solver("rk4", 1, ext, "stage", "require", kernel)._generic_only_ok("integrate_DAE", (None, None))
        # segments and per-trajectory events: the walk under "auto", a refusal under "require"
        seg = nd.RK4Classic(externals=ext, algebraic="stage", segment=2)
        seg.fused = "auto"
        assert not seg._generic_only_ok("integrate_DAE", (None, None))
        seg.fused = "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
            seg._generic_only_ok("integrate_DAE", (None, None))
        pt = S.solver("RK4Classic", 1, ext, "stage", "auto")
        assert not pt._generic_only_ok("integrate_DAE", (None, None), True)
        pt.fused = "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
            pt._generic_only_ok("integrate_DAE", (None, None), True)
        m = models.DAE_Model(8, 2, 2, 2, 64, direct_encode=True, solver=nd.RK4Classic(externals=ext, algebraic="stage"))
        assert m._forward_encoded(*(None,) * 6, None, None, None) is None          # rows + solver route


# ----------------------------------------------------------------------------- 8. the precondition of the GPU forward test
@pytest.mark.parametrize("shape", list(S.FWD_SHAPES))
def test_gpu_forward_cases_hold_stage_and_step_apart(shape):
    """On every forward case of tests/test_gpu_stage_heads.py the fp64 "stage" walk differs from the fp64 "step" walk by more than
    100 x TOL_GPU (trajectory-relative, xs): a kernel that never runs a stage head cannot pass there.  Asserted here, on the CPU, so that a
    drifting case fails loudly."""
    for n in (1, 2):
        case = _c64(S.forward_case(shape, n))
        for name in S.METHODS:
            for ext in S.INTERP:
                a, b = _walk(S.solver(name, n, ext, "stage"), case), _walk(S.solver(name, n, ext, "step"), case)
                gap = traj_rel_err(a[0], b[0])
                print(shape, n, name, ext, f"stage vs step {gap:.3e}")
                assert gap > 100 * TOL_GPU, (shape, n, name, ext, gap)
