"""Per-trajectory events (ODE_Event / DAE_Event with per_trajectory=True), host side (no GPU): the callback walk against the CPU oracle run
one trajectory at a time (tests/pev_cases.py: there a trajectory's own clock and list decide), the sensitivity of the cases shown with the
oracle alone, per_trajectory=False and a per-trajectory object whose rows share their steps against the walk as it was, the mask and the
merged rows of the event classes, and the additive C ABI (the _pev entry points: argument checks from the dims alone) with the routing.

The walk-vs-oracle gate is helpers.TOL_ORACLE on the per-trajectory relative error (helpers.traj_rel_err, the metric the sensitivity
condition is stated in): the oracle evaluates a one-row batch, the walk all 33 rows at once, and ATen's fp32 GEMM blocks the two
differently -- measured 3.4e-7 at most over every case below, against 2e-6."""
import ctypes
import functools

import pytest
import torch

import capi_args as A
import generic_cases as C
import pev_cases as P
from capi_args import R
from capi_args import sub as _sub
from helpers import TOL_GPU, TOL_ORACLE, traj_rel_err
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4}
PEV_EXPORTS = ("psnode_event_table_pt_f32", "psnode_ode_integrate_pev_supported", "psnode_ode_integrate_pev_f32",
               "psnode_dae_integrate_pev_supported", "psnode_dae_integrate_pev_f32", "psnode_ode_backward_pev_supported",
               "psnode_ode_backward_pev_f32", "psnode_dae_backward_pev_supported", "psnode_dae_backward_pev_f32")


def _solver(name, n=1):
    s = SOLVERS[name](substeps=n)
    s.fused = "off"
    return s


@functools.lru_cache(maxsize=None)
def _ode_case(pattern):
    return P.sensitive_ode_case(C.ode_case(6, 2, (32, 32), P.B0, P.T0, seed=5, t=P.clock()), pattern)


@functools.lru_cache(maxsize=None)
def _dae_case(pattern):
    return P.sensitive_dae_case(C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), P.B0, P.T0, seed=7, t=P.clock(), perturb_x_init=True), pattern)


# ----------------------------------------------------------------------------- 1. the walk vs the oracle, one trajectory at a time
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_ode_walk_equals_the_oracle_per_trajectory(pattern, name, n):
    case, _ = _ode_case(pattern)
    de, t, x, z, ev, zj = case
    with torch.no_grad():
        got = P.run_ode(_solver(name, n), de, t, x, z, torch.cat((x[0], z[0]), -1), ev, zj)
    e = traj_rel_err(got, P.oracle_ode(name, case, n))
    print(pattern, name, n, f"{e:.3e}")
    assert got.shape == x.shape and e <= TOL_ORACLE


@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_ode_walk_teacher_forced_equals_the_oracle_per_trajectory(pattern, name):
    case, _ = _ode_case(pattern)
    de, t, x, z, ev, zj = case
    with torch.no_grad():
        got = P.run_ode(_solver(name), de, t, x, z, torch.cat((x[0], z[0]), -1), ev, zj, tx=True)
    assert traj_rel_err(got, P.oracle_ode(name, case, 1, True)) <= TOL_ORACLE


@pytest.mark.parametrize("tx,ti", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_dae_walk_equals_the_oracle_per_trajectory(pattern, name, tx, ti):
    case, _ = _dae_case(pattern)
    with torch.no_grad():
        gx, gi = P.run_dae(_solver(name), *case, tx, ti)
    rx, ri = P.oracle_dae(name, case, 1, tx, ti)
    ex, ei = traj_rel_err(gx, rx), traj_rel_err(gi, ri)
    print(pattern, name, tx, ti, f"{ex:.3e} {ei:.3e}")
    assert ex <= TOL_ORACLE and ei <= TOL_ORACLE


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_dae_walk_with_substeps_and_without_dataset_x(pattern, n):
    case, _ = _dae_case(pattern)
    for name in SOLVERS:
        with torch.no_grad():
            gx, gi = P.run_dae(_solver(name, n), *case)
        rx, ri = P.oracle_dae(name, case, n)
        assert traj_rel_err(gx, rx) <= TOL_ORACLE and traj_rel_err(gi, ri) <= TOL_ORACLE, name
    no_x = C.without_x(case)
    with torch.no_grad():
        gx, gi = P.run_dae(_solver("rk4"), *no_x)
    rx, ri = P.oracle_dae("rk4", no_x)
    assert gx.shape == (P.T0, P.B0, 5) and traj_rel_err(gx, rx) <= TOL_ORACLE and traj_rel_err(gi, ri) <= TOL_ORACLE


# ----------------------------------------------------------------------------- 2. sensitivity, with the oracle alone
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_the_cases_tell_the_two_rules_apart(pattern):
    """Every trajectory whose event steps differ from trajectory 0's lies at least 100 x TOL_GPU from the shared-rule result on the same
    batch; the others are the shared rule's, to the GEMM blocking -- a condition on the cases, shown with the oracle alone.  The two
    walks then stand in the same relation: the per-trajectory event object's next to the default one's on the same batch."""
    case, differ = _ode_case(pattern)
    assert int(differ.sum()) == {"mixed": 26, "blocks": 17, "only_zero": 32}[pattern]
    for name in SOLVERS:
        gap = P.per_traj_err(P.oracle_ode(name, case), P.oracle_ode_shared(name, case))
        assert bool((gap[differ] >= 100 * TOL_GPU).all()) and bool((gap[~differ] <= TOL_ORACLE).all()), (name, gap)
    dcase, ddiffer = _dae_case(pattern)
    gap = P.per_traj_err(P.oracle_dae("rk4", dcase)[0], P.oracle_dae_shared("rk4", dcase)[0])
    assert bool((gap[ddiffer] >= 100 * TOL_GPU).all()) and bool((gap[~ddiffer] <= TOL_ORACLE).all()), gap
    de, t, x, z, ev, zj = case
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        own = P.run_ode(_solver("rk4"), de, t, x, z, a0, ev, zj, per_trajectory=True)
        shared = P.run_ode(_solver("rk4"), de, t, x, z, a0, ev, zj, per_trajectory=False)
        dx, _ = P.run_dae(_solver("rk4"), *dcase, per_trajectory=True)
        sx, _ = P.run_dae(_solver("rk4"), *dcase, per_trajectory=False)
    assert traj_rel_err(shared, P.oracle_ode_shared("rk4", case)) <= TOL_ORACLE          # the default rule is the oracle's, on the whole batch
    for gap, d in ((P.per_traj_err(own, shared), differ), (P.per_traj_err(dx, sx), ddiffer)):
        assert bool((gap[d] >= 100 * TOL_GPU).all()) and bool((gap[~d] == 0).all()), gap


# ----------------------------------------------------------------------------- 3. the default rule and shared steps: the walk as it was, bit for bit
@pytest.mark.parametrize("n", [1, 3])
def test_default_rule_and_shared_steps_are_the_walk_as_it_was(n):
    """G2 / G3-style batches: every trajectory has its events at the steps of trajectory 0 (on its own clock).  per_trajectory=False runs
    the statements it ran; per_trajectory=True computes the same numbers bit for bit, because every trajectory then hits where 0 does."""
    de, t, x, z, ev, zj = C.ode_case(6, 2, (32, 32), 7, P.T0, seed=8, ev_rows=(0, 3))
    a0 = torch.cat((x[0], z[0]), -1)
    s = _solver("rk4", n)
    for tx in (False, True):
        old = nd.ODE_Event()
        old.set_event(ev, zj)
        with torch.no_grad():
            ref = C.walk_ode_hold(s, de, t, x, z, a0, old.event_fn, old.jump_change_fn, tx)
            assert torch.equal(P.run_ode(s, de, t, x, z, a0, ev, zj, tx, per_trajectory=False), ref)
            assert torch.equal(P.run_ode(s, de, t, x, z, a0, ev, zj, tx, per_trajectory=True), ref)
    dc = C.dae_case(5, 2, 3, 2, (32, 32), (24, 24), 7, P.T0, seed=9, ev_rows=(0, 3), perturb_x_init=True)
    de, ae, t, x, z, v, i, xi, a0, ev, zj, vj = dc
    for tx, ti in ((False, False), (True, False), (False, True), (True, True)):
        old = nd.DAE_Event()
        old.set_event(ev, zj, vj)
        with torch.no_grad():
            ref = C.walk_dae_hold(s, xi, de, ae, t, x, z, v, i, a0, old.event_fn, old.jump_change_fn, tx, ti)
            for pt in (False, True):
                got = P.run_dae(s, *dc, tx, ti, per_trajectory=pt)
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (tx, ti, pt)


# ----------------------------------------------------------------------------- 4. the event classes
def test_mask_and_merged_rows_of_the_event_classes():
    t = P.clock()
    ev = P.event_times("mixed", t)
    zj, vj = torch.randn(P.B0, P.NE, 2), torch.randn(P.B0, P.NE, 3)
    zj[0] = vj[0] = float("nan")          # trajectory 0 never fires: its rows are never taken
    tab = P.step_table("mixed", P.T0, P.B0)
    e = nd.DAE_Event(per_trajectory=True)
    assert e.per_trajectory is True and nd.ODE_Event().per_trajectory is False and nd.DAE_Event().per_trajectory is False
    assert e.event_fn(t[0]) is False and not bool(e.hit_mask(t[0]).any())          # no events set
    e.set_event(ev, zj, vj)
    for k in range(P.T0 - 1):
        mask = e.hit_mask(t[k])
        assert mask.dtype == torch.bool and tuple(mask.shape) == (P.B0,) and torch.equal(mask, tab[k] >= 0)
        assert e.event_fn(t[k]) is bool(mask.any())
        z0, v0 = torch.randn(P.B0, 2), torch.randn(P.B0, 3)
        z1, v1 = e.jump_change_fn(t[k], z0, v0)
        for b in range(P.B0):
            col = int(tab[k, b])
            assert torch.equal(z1[b], zj[b, col] if col >= 0 else z0[b]) and torch.equal(v1[b], vj[b, col] if col >= 0 else v0[b])
    assert e.event_fn(t[1]) is False and e.event_fn(t[-1]) is False          # steps 1 and the last grid point carry nothing in "mixed"
    # NaN never hits, not even a NaN clock
    assert not bool(e.hit_mask(torch.full((P.B0, 1), float("nan"))).any())
    # the flag is a plain attribute: the same object under the default rule answers for trajectory 0
    e.per_trajectory = False
    assert e.event_fn(t[0]) is False and not bool(e.hit_mask(t[0]).any())          # trajectory 0 has no events
    m = models.ODE_Model(8, 2, 16, solver=nd.RK4())
    assert m.event.per_trajectory is False
    m.event.per_trajectory = True
    assert fused.per_trajectory_events(m.event.event_fn) is False          # ... no events set: the event-less call
    m.event.set_event(ev, zj)
    assert fused.per_trajectory_events(m.event.event_fn) is True
    # two entries of one trajectory at one step: the duplicate the default rule reports for trajectory 0, for every trajectory
    dup = ev.clone()
    dup[17, 0, 0] = dup[17, 1, 0] = t[1, 17, 0]
    o = nd.ODE_Event(per_trajectory=True)
    o.set_event(dup, zj)
    with pytest.raises(RuntimeError, match="one trajectory"):
        o.jump_change_fn(t[1], torch.zeros(P.B0, 2))
    assert "per_trajectory" in nd.ODE_Event.__doc__


# ----------------------------------------------------------------------------- 5. C ABI, dims only
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))
_supported, _call = functools.partial(A.supported, family="pev"), functools.partial(A.call, family="pev")


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    for name in PEV_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    sub_p = ctypes.POINTER(_lib.SubstepsF32)
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_pev_supported").argtypes == getattr(lib, f"psnode_{stem}_sub_supported").argtypes
        assert getattr(lib, f"psnode_{stem}_pev_f32").argtypes == getattr(lib, f"psnode_{stem}_sub_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_pev_f32").argtypes[2 + n_act] == sub_p
    assert lib.psnode_dae_backward_pev_f32.argtypes[0] == ctypes.POINTER(_lib.DaeBwdTfArgsF32)
    assert len(lib.psnode_event_table_pt_f32.argtypes) == 12
    # the table entry point's own checks: nothing to do, NULL pointers, a negative count
    assert lib.psnode_event_table_pt_f32(0, 5, None, 0, 0, None, 0, 0, 2, None, None, None) == 0
    assert lib.psnode_event_table_pt_f32(4, 5, None, 5, 1, None, 2, 1, 2, None, None, None) == -1
    assert lib.psnode_event_table_pt_f32(4, 5, 256, 5, 1, None, 2, 1, 2, 256, None, None) == -1
    assert lib.psnode_event_table_pt_f32(4, 5, 256, 5, 1, 256, 2, 1, -1, 256, None, None) == -2


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_pev_argument_checks_and_status_order(stem, make, n_act):
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
    for sub in (None, _sub(1), _sub(2)):                 # a NULL tableau needs a valid method; a tableau makes the method unread
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
    # order: the sub-steps struct before the act pair before the NULL args before the tableau before the route
    assert _call(lib, stem, make(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(0), R(unknown)) == -2
    assert _call(lib, stem, make(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2), R(unknown)) == -3
    assert _call(lib, stem, None, n_act, R(bad), _sub(2)) == -1
    assert _call(lib, stem, make(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2)) == -3
    assert _call(lib, stem, make(kernel=_lib.KERNEL_MFMA), n_act, tab, _sub(2)) == -5


def _fill_ode_bwd(b):
    for l in range(4):
        b.de.weight[l] = b.de.bias[l] = 256
    b.t.ptr = b.z.ptr = b.all_initial = b.xs = b.grad_xs = b.grad_x0 = b.grad_all_initial = b.grad_params = 256


def _fill_dae_bwd(q):
    for m in (q.de, q.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
    q.grad_params_de = q.grad_params_ae = 256


def test_a_missing_event_table_side_outputs_teacher_forcing_and_x_sub():
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
    # forward calls with every pointer in place but the event table: PSNODE_ERR_NULL; with it: as far as the workspace check
    a = _ode_args()
    for l in range(4):
        a.de.weight[l] = a.de.bias[l] = 256
    a.t.ptr = a.x.ptr = a.z.ptr = a.all_initial = a.x_out = 256
    assert _call(lib, "ode_integrate", a, 1, None, None) == -1 and _call(lib, "ode_integrate", a, 1, None, _sub(2)) == -1
    a.event_idx = 256
    assert _call(lib, "ode_integrate", a, 1, None, None) == -1          # ... an event table wants the jump rows
    a.z_jump = 256
    assert _call(lib, "ode_integrate", a, 1, None, None) == -4 and _call(lib, "ode_integrate", a, 1, None, _sub(2)) == -4
    d = _dae_args()
    for m in (d.de, d.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    d.t.ptr = d.z.ptr = d.v.ptr = d.x_init = d.all_initial = d.x_out = d.i_out = 256
    assert _call(lib, "dae_integrate", d, 2, None, None) == -1
    d.event_idx = d.z_jump = d.v_jump = 256
    assert _call(lib, "dae_integrate", d, 2, None, None) == -4
    # backward calls: the event table, then x_sub where there are sub-steps, then the workspace
    b = _ode_bwd_args()
    _fill_ode_bwd(b)
    assert _call(lib, "ode_backward", b, 1, None, None) == -1          # no event table
    b.event_idx = b.z_jump = 256
    assert _call(lib, "ode_backward", b, 1, None, _sub(2)) == -1       # no x_sub
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256)) == -4
    assert _call(lib, "ode_backward", b, 1, None, _sub(1)) == -4 and _call(lib, "ode_backward", b, 1, None, None) == -4
    e = _dae_bwd_args()
    _fill_dae_bwd(e.base)
    assert _call(lib, "dae_backward", e, 2, None, None) == -1
    e.base.event_idx = e.base.z_jump = e.base.v_jump = 256
    assert _call(lib, "dae_backward", e, 2, None, _sub(2)) == -1
    assert _call(lib, "dae_backward", e, 2, None, _sub(2, 256)) == -4 and _call(lib, "dae_backward", e, 2, None, None) == -4


def test_the_lds_fit_is_the_sub_build_s():
    """This build keeps no LDS of its own (the event index of a column lives in a register of the threads that own the column): its
    _supported answers are the _sub build's along a growing z_dim, for K0 and for K5."""
    lib = _lib.load()
    for stem, make in (("ode_integrate", _ode_args), ("ode_backward", _ode_bwd_args)):
        answers = []
        for zd in range(64, 660, 4):
            a = make(kernel=_lib.KERNEL_GENERIC, xd=8, zd=zd, hidden=32)
            pev, sub = _supported(lib, stem, a, 1, None, _sub(2)), _supported(lib, stem, a, 1, None, _sub(2), family="sub")
            assert pev == sub, (stem, zd)
            answers.append(pev)
        assert 0 in answers and 1 in answers, stem


# ----------------------------------------------------------------------------- 6. routing
_layers = A.hip_layers


def test_python_predicates_and_refusals():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    pt = dict(per_trajectory=True)
    for method in ("euler", "rk4", nd.Kutta3().method):
        for sub in (1, 2, 7):
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, substeps=sub, **pt)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", act=tanh, substeps=sub, **pt)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, substeps=sub, **pt)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, act=tanh, input_true_x=True, substeps=sub, **pt)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, substeps=sub, **pt)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), substeps=sub, **pt)
            for tx, ti in ((True, False), (False, True), (True, True)):
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **pt)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 1, 33, input_true_x=tx, input_true_i=ti, substeps=sub, **pt)
            for kernel in ("wave", "tile", "mfma", "wide"):          # the specialised kernels are refused
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, substeps=sub, **pt)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel, substeps=sub, **pt)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, substeps=sub, **pt)
            assert fused.ode_backward_supported(method, ode01, 8, 2, "generic", substeps=sub, **pt)
            assert fused.dae_backward_supported(method, de, ae, 8, 2, 2, 2, kernel="generic", substeps=sub, **pt)
            # linear externals together with per-trajectory events: no kernel
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, substeps=sub, externals="linear", **pt)
            assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, substeps=sub, externals="linear", **pt)
            assert not fused.ode_backward_supported(method, ode01, 8, 2, "generic", substeps=sub, externals="linear", **pt)
    opts = lambda substeps=1, externals="hold", act=None, method="rk4": fused.GenericOpts.of(method, (act,), substeps, externals, True)
    assert opts().family == "pev" and opts(5).family == "pev" and opts(1, "linear").family == "none"
    assert fused.GenericOpts.of("rk4", (None,)).family == "plain" and fused.GenericOpts.of("rk4", (None,)).per_trajectory is False
    one = opts().c_args()
    assert one[0] is None and one[1] is None and one[2]._obj.substeps == 1 and not one[2]._obj.x_sub
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
        opts().require_plain("a specialised entry")
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        opts(1, "linear").require_generic("x", "generic", False)
    for kernel, save in (("wave", False), ("mfma", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
            opts().require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="substeps"):          # the fifth option in the naming order
            opts(3).require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="activation"):
            opts(3, act=tanh).require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="tableau"):
            opts(3, method=nd.Kutta3().method).require_generic("x", kernel, save)
    opts().require_generic("x", "generic", False)
    with pytest.raises(ValueError):
        fused.GenericOpts.of("rk4", (None,), 1, "hold", 1)
    # specialised entries refuse the flag; event-less calls are unchanged
    with pytest.raises(_lib.UnsupportedShapeError):
        fused.GenericOpts.of("rk4", (None, None), 1, "hold", True).require_plain("dae_backward_wide")
    t = torch.zeros(3, 4, 1)
    assert not fused.has_events(t, None) and not fused.has_events(t[:1], torch.zeros(4, 2, 1)) and not fused.has_events(t, torch.zeros(4, 0, 1))
    assert fused.has_events(t, torch.zeros(4, 2, 1)) and fused.has_events(t, None, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        fused.check_event_idx(torch.zeros(2, dtype=torch.int32), 3, 4, True, torch.device("cpu"))
    fused.check_event_idx(torch.zeros(2, 4, dtype=torch.int32), 3, 4, True, torch.device("cpu"))
    fused.check_event_idx(torch.zeros(2, dtype=torch.int32), 3, 4, False, torch.device("cpu"))


def test_routing_of_per_trajectory_events_in_the_solver():
    for cls in (nd.RK4, nd.Kutta3):
        for kernel in ("auto", "generic"):
            for n in (1, 3):
                s = cls(substeps=n)
                s.kernel, s.fused = kernel, "require"
                assert s._generic_only_ok("integrate_ODE", (None,), True)
                assert s._generic_kwargs(True) == dict(per_trajectory=True, **({"substeps": n} if n > 1 else {}))
                assert "per_trajectory" not in s._generic_kwargs() and "per_trajectory" not in s._generic_kwargs(False)
        for kernel in ("wave", "tile", "mfma", "wide"):
            s = cls()
            s.kernel, s.fused = kernel, "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,), True)          # walks, with the warning
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory" if cls is nd.RK4 else "tableau"):
                s._generic_only_ok("integrate_ODE", (None,), True)
            if cls is nd.RK4:
                assert s._generic_only_ok("integrate_ODE", (None,), False)       # event-less calls and the default rule: unchanged
        s = cls(externals="linear")
        s.kernel, s.fused = "auto", "auto"
        assert s._generic_only_ok("integrate_ODE", (None,), False) and not s._generic_only_ok("integrate_ODE", (None,), True)
        s.fused = "require"
        with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
            s._generic_only_ok("integrate_ODE", (None,), True)
    # the one-launch encoded forwards are not taken by a call with events whose model's event object is per-trajectory; the answer comes
    # before any tensor is looked at (an event-less call of such a model takes the route it took: tests/test_gpu_events_per_trajectory.py)
    for m, args in ((models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4()), (torch.zeros(3, 4, 1), torch.zeros(3, 4, 8), torch.zeros(3, 4, 2))),
                    (models.DAE_Model(8, 2, 2, 2, 64, direct_encode=True, solver=nd.RK4()), (None,) * 6)):
        m.event.per_trajectory = True
        ev = torch.zeros(4, 2, 1)
        assert m._forward_encoded(*args, ev, None) is None if len(args) == 3 else m._forward_encoded(*args, ev, None, None) is None
    assert "per_trajectory" in nd.FixedGridODESolver._note_walk.__code__.co_consts.__repr__()
