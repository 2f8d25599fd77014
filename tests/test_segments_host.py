"""Multiple-shooting segments (solver.segment), host side (no GPU): the callback walk with segment = w against its own free runs on the
slices (bitwise) and against the fp32 CPU oracle on the slices, the limits w = 1 / w >= T - 1 / None, the visibility of a restart, the
gradients the definition promises (fp64 autograd through the walk), the refusals, the additive C ABI (psnode_segments_f32 and its eight
entry points: argument checks from the dims alone), the LDS fit and the routing.  Cases: tests/segment_cases.py."""
import ctypes
from copy import deepcopy

import pytest
import torch

import capi_args as A
import generic_cases as C
import segment_cases as S
from capi_args import R
from capi_args import sub as _sub
from helpers import TOL_GPU, TOL_ORACLE, rel_err
from oracle import psnode_oracle as O
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

MS_EXPORTS = tuple(f"psnode_{s}_ms_{k}" for s in ("ode_integrate", "dae_integrate", "ode_backward", "dae_backward") for k in ("supported", "f32"))
B0, T0 = 5, 8          # (the host cases need no tiles; the GPU file runs B = 33)
ODE_DIMS = (6, 2, (32, 32))
DAE_DIMS = (5, 2, 3, 2, (32, 32), (24, 24))


def _ode(seed=0, events=True, Tn=T0, B=B0):
    return S.ode_case(*ODE_DIMS, B=B, Tn=Tn, seed=seed, events=events)


def _dae(seed=0, events=True, Tn=T0, B=B0):
    return S.dae_case(*DAE_DIMS, B=B, Tn=Tn, seed=seed, events=events)


# ----------------------------------------------------------------------------- 1. the walk is its own free runs on the slices
@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
@pytest.mark.parametrize("w", S.WS)
def test_ode_walk_is_bitwise_the_free_runs_on_the_slices(w, name, n, events):
    case = _ode(3 + n, events)
    for dtype in (torch.float32, torch.float64):
        got, ref = S.walk_ode(name, n, w, *case, dtype=dtype), S.walk_sliced_ode(name, n, w, *case, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, ref), (w, name, n, events, dtype)


@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4", "Kutta3"])
@pytest.mark.parametrize("w", S.WS)
def test_dae_walk_is_bitwise_the_free_runs_on_the_slices(w, name, n, events):
    case = _dae(5 + n, events)
    for dtype in (torch.float32, torch.float64):
        (gx, gi), (rx, ri) = S.walk_dae(name, n, w, case, dtype=dtype), S.walk_sliced_dae(name, n, w, case, dtype=dtype)
        assert torch.equal(gx, rx) and torch.equal(gi, ri), (w, name, n, events, dtype)


@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("name", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("w", S.WS)
def test_walk_equals_the_oracle_on_the_slices(w, name, events):
    de, t, x, z, ev, zj = _ode(11, events)
    a0 = torch.cat((x[0], z[0]), -1)
    L = C.layers_of(de.x_dot)
    with torch.no_grad():
        ref = S.sliced_ode(S.Free(w, lambda ts, xs, zs, start: O.integrate_ode(name, L, ts, torch.cat((start[None], xs[1:])), zs, a0, ev, zj)), t, x, z)
    e = rel_err(S.walk_ode(name, 1, w, de, t, x, z, ev, zj, dtype=torch.float32), ref)
    case = _dae(12, events)
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    Ld, La = C.layers_of(de.x_dot), C.layers_of(ae.i_calculator)
    with torch.no_grad():
        rx, ri = S.sliced_dae(S.Free(w, lambda ts, xs, zs, vs, is_, start: O.integrate_dae(name, Ld, La, start, ts, xs, zs, vs, is_, a0, ev, zj, vj)),
                              t, x, z, v, i, x_init)
    gx, gi = S.walk_dae(name, 1, w, case, dtype=torch.float32)
    ex, ei = rel_err(gx, rx), rel_err(gi, ri)
    print(w, name, events, f"ode {e:.3e} dae x {ex:.3e} i {ei:.3e}")
    assert max(e, ex, ei) <= TOL_ORACLE


# ----------------------------------------------------------------------------- 2. the limits
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
def test_w_1_is_teacher_forcing_and_long_segments_are_the_free_walk(name, n):
    de, t, x, z, ev, zj = _ode(20)
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        free = C.run_ode(S.solver(name, None, n), de, t, x, z, a0, ev, zj)
        as_it_was = C.walk_ode_hold(S.solver(name, None, n), de, t, x, z, a0, *_callbacks(nd.ODE_Event(), ev, zj), False)
        assert torch.equal(free, as_it_was)
        assert torch.equal(C.run_ode(S.solver(name, 1, n), de, t, x, z, a0, ev, zj), C.run_ode(S.solver(name, None, n), de, t, x, z, a0, ev, zj, tx=True))
        for w in (7, 100):
            assert torch.equal(C.run_ode(S.solver(name, w, n), de, t, x, z, a0, ev, zj), free)
        case = _dae(21)
        fx, fi = C.run_dae(S.solver(name, None, n), *case)
        de_, ae_, t_, x_, z_, v_, i_, xi_, a0_, ev_, zj_, vj_ = case
        wx, wi = C.walk_dae_hold(S.solver(name, None, n), xi_, de_, ae_, t_, x_, z_, v_, i_, a0_, *_callbacks(nd.DAE_Event(), ev_, zj_, vj_), False, False)
        assert torch.equal(fx, wx) and torch.equal(fi, wi)
        for w in (7, 100):
            gx, gi = C.run_dae(S.solver(name, w, n), *case)
            assert torch.equal(gx, fx) and torch.equal(gi, fi)


def _callbacks(event, ev, *jumps):
    if ev is None:
        return None, None
    event.set_event(ev, *jumps)
    return event.event_fn, event.jump_change_fn


def test_a_restart_is_visible():
    """w = 3: row 4 of every trajectory is more than 100 x TOL_GPU away from the free run's -- the cases tell the two apart"""
    de, t, x, z, ev, zj = _ode(30, B=S.B0)
    gap = S.row_gap(S.walk_ode("rk4", 1, 3, de, t, x, z, ev, zj), S.walk_ode("rk4", 1, None, de, t, x, z, ev, zj), 4)
    case = _dae(31, B=S.B0)
    (sx, si), (fx, fi) = S.walk_dae("rk4", 1, 3, case), S.walk_dae("rk4", 1, None, case)
    gx, gi = S.row_gap(sx, fx, 4), S.row_gap(si, fi, 4)
    print(f"smallest ratio to TOL_GPU over the trajectories: ode {float(gap.min()) / TOL_GPU:.1f}, dae x {float(gx.min()) / TOL_GPU:.1f}, "
          f"dae i {float(gi.min()) / TOL_GPU:.1f}")
    assert float(gap.min()) > 100 * TOL_GPU and float(gx.min()) > 100 * TOL_GPU
    # rows 1 .. 3 are segment 0: the free run itself
    assert torch.equal(sx[:4], fx[:4]) and torch.equal(si[:4], fi[:4])


# ----------------------------------------------------------------------------- 3. gradients through the walk (fp64)
def _leaf(a):
    return None if a is None else a.double().clone().requires_grad_(True)


def _ode_walk_grads(w, loss_rows, case, x_leaf=True):
    de, t, x, z, ev, zj = case
    m = deepcopy(de).double()
    xg, zg, zjg = _leaf(x), _leaf(z), _leaf(zj)
    if not x_leaf:
        xg = xg.detach()
    a0 = torch.cat((x[0], z[0]), -1).double().requires_grad_(True)
    xs = C.run_ode(S.solver("rk4", w), m, t.double(), xg, zg, a0, None if ev is None else ev.double(), zjg)
    xs[loss_rows].sum().backward()
    return dict(x=xg.grad, z=zg.grad, zj=None if zjg is None else zjg.grad, a0=a0.grad)


def test_the_dataset_rows_get_no_gradient_and_a_segment_s_loss_stays_in_its_rows():
    case = _ode(40)
    g = _ode_walk_grads(3, slice(None), case)
    assert g["x"][0].abs().sum() > 0 and not g["x"][1:].any()          # x[0] is the start of the call; every other row is data
    g = _ode_walk_grads(3, slice(4, 7), case)                          # segment 1 alone: rows 4 .. 6, inputs of rows 3 .. 5
    assert not g["x"].any() and not g["z"][:3].any() and not g["z"][6:].any() and g["z"][3:6].abs().sum() > 0
    g = _ode_walk_grads(3, slice(1, 4), case)                          # segment 0 alone: nothing beyond row (0 + 1) w
    S.rows_beyond_are_zero(g, ("z",), 3, "ode segment 0")
    assert not g["z"][3:].any() and g["x"][0].abs().sum() > 0
    # the loss on row 3 -- a restart point's output -- travels back into segment 0
    g = _ode_walk_grads(3, slice(3, 4), case)
    assert g["z"][:3].abs().sum() > 0 and not g["z"][3:].any()


def _dae_walk(w, case, x_init=None):
    de, ae, t, x, z, v, i, xi, a0, ev, zj, vj = case
    lv = dict(z=_leaf(z), v=_leaf(v), x_init=_leaf(xi if x_init is None else x_init), a0=_leaf(a0), zj=_leaf(zj), vj=_leaf(vj), x=_leaf(x))
    mde, mae = deepcopy(de).double(), deepcopy(ae).double()
    xs, is_ = C.run_dae(S.solver("rk4", w), mde, mae, t.double(), lv["x"], lv["z"], lv["v"], i.double(), lv["x_init"], lv["a0"],
                        None if ev is None else ev.double(), lv["zj"], lv["vj"])
    return xs, is_, lv, (mde, mae)


@pytest.mark.parametrize("events", [False, True])
def test_dae_gradients_of_a_restart(events):
    """a loss on xs[4] with w = 3: only the step 3 -> 4 is in play.  Its DE read the restart head g(x[3]; z_3 | v_3 -- the jumped rows
    with an event at step 3): grad z[3] (or the jump row's) must be what autograd gives through the sliced call, the dataset x gets
    nothing, and no row beyond 3 or before it gets anything."""
    case = _dae(41, events)
    xs, is_, lv, _ = _dae_walk(3, case)
    xs[4].sum().backward()
    assert lv["x"].grad is None or not lv["x"].grad.any()
    assert lv["x_init"].grad is None or not lv["x_init"].grad.any()          # segment 0 took no part
    # the sliced call: the free run on rows 3 .. 6 from x[3]
    de, ae, t, x, z, v, i, xi, a0, ev, zj, vj = case
    sl = case[:2] + tuple(q[3:7] for q in (t, x, z, v, i)) + (x[3], a0, ev, zj, vj)
    xs2, _, lv2, _ = _dae_walk(None, sl)
    xs2[1].sum().backward()
    for k in ("z", "v"):
        g, g2 = lv[k].grad, lv2[k].grad
        assert not g[:3].any() and not g[4:].any()
        assert torch.equal(g[3], g2[0]), k
    if events:      # step 3 carries event 1: the restart head read the jump rows, row 3 of z | v nothing
        assert not lv["z"].grad[3].any() and lv["zj"].grad[:, 1].abs().sum() > 0
        assert torch.equal(lv["zj"].grad, lv2["zj"].grad) and torch.equal(lv["vj"].grad, lv2["vj"].grad)
    else:
        assert lv["z"].grad[3].abs().sum() > 0
    assert torch.equal(lv["a0"].grad, lv2["a0"].grad)
    # a loss on segment 0 alone: exact zeros beyond row w
    xs, is_, lv, _ = _dae_walk(3, case)
    (xs[1:4].sum() + is_[:4].sum()).backward()
    S.rows_beyond_are_zero({k: lv[k].grad for k in ("z", "v")}, ("z", "v"), 3, "dae segment 0")
    assert lv["x_init"].grad.abs().sum() > 0 and (lv["x"].grad is None or not lv["x"].grad.any())


# ----------------------------------------------------------------------------- 4. refusals
def test_constructor_and_call_refusals():
    assert nd.Euler().segment is None and nd.RK4(segment=3).segment == 3 and nd.Kutta3(segment=1, substeps=2).segment == 1
    for bad in (0, -1, True, False, 2.0, "3"):
        for cls in (nd.Euler, nd.Midpoint, nd.RK4, nd.Kutta3, nd.RK4Classic):
            with pytest.raises(ValueError, match="segment"):
                cls(segment=bad)
    with pytest.raises(ValueError, match="segment"):
        nd.AB2(segment=3)
    assert nd.AB2(segment=None).segment is None
    de, t, x, z, ev, zj = _ode(50)
    a0 = torch.cat((x[0], z[0]), -1)
    s = S.solver("rk4", 3)
    with pytest.raises(ValueError, match="segment"):
        C.run_ode(s, de, t, x, z, a0, ev, zj, tx=True)
    with pytest.raises(ValueError, match="segment"):
        s._walk_ode(de, t, x, z, a0, None, None, True)
    case = _dae(51)
    for tx, ti in ((True, False), (False, True), (True, True)):
        with pytest.raises(ValueError, match="segment"):
            C.run_dae(s, *case, tx=tx, ti=ti)
        with pytest.raises(ValueError, match="segment"):
            s._walk_dae(case[7], case[0], case[1], *case[2:7], case[8], None, None, tx, ti)
    with pytest.raises(ValueError, match="segment"):
        C.run_dae(s, *C.without_x(case))
    with pytest.raises(ValueError, match="segment"):
        fused.GenericOpts.of("ab2", (None,), 1, "hold", False, 3)
    for bad in (0, True, 2.5):
        with pytest.raises(ValueError, match="segment"):
            fused.GenericOpts.of("rk4", (None,), 1, "hold", False, bad)


# ----------------------------------------------------------------------------- 5. the C ABI
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))


def _seg(every, x_true=None):
    g = _lib.SegmentsF32()
    g.every, g.x_true = every, x_true
    return g


def _tail(n_act, tab, sub, seg, act):
    return [act] * n_act + [tab, R(sub) if sub is not None else None, R(seg) if seg is not None else None]


def _supported(lib, stem, a, n_act, tab=None, sub=None, seg=None, act=None):
    return getattr(lib, f"psnode_{stem}_ms_supported")(R(a) if a is not None else None, *_tail(n_act, tab, sub, seg, act))


def _call(lib, stem, a, n_act, tab=None, sub=None, seg=None, act=None):
    return getattr(lib, f"psnode_{stem}_ms_f32")(R(a) if a is not None else None, *_tail(n_act, tab, sub, seg, act), None, 0, None)


def _with_x(a, stem):
    if stem == "dae_integrate":
        a.x.ptr = 256          # (a DAE forward without dataset rows is refused: the restarts read them)
    return a


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    seg_p = ctypes.POINTER(_lib.SegmentsF32)
    for name in MS_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert not name.endswith("_workspace_bytes") and not any(f in name for f in ("_act_", "_tf_", "_rk_", "_sub_", "_lin_"))
    for stem, _, n_act in ENTRIES:
        assert getattr(lib, f"psnode_{stem}_ms_supported").argtypes == getattr(lib, f"psnode_{stem}_sub_supported").argtypes + [seg_p]
        sub_f = getattr(lib, f"psnode_{stem}_sub_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_ms_f32").argtypes == sub_f[:-3] + [seg_p] + sub_f[-3:]
    assert [f[0] for f in _lib.SegmentsF32._fields_] == ["every", "x_true"] and ctypes.sizeof(_lib.SegmentsF32) == 16


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_ms_argument_checks_and_status_order(stem, make, n_act):
    lib = _lib.load()
    mk = lambda **kw: _with_x(make(**kw), stem)
    tab = R(nd.Kutta3().method.abi())
    ok = _seg(3, 256)
    # the segments struct comes first: NULL, then every < 1 -- whatever else is wrong with the call
    for a in (mk(), None, mk(kernel=_lib.KERNEL_MFMA), mk(method=77)):
        assert _call(lib, stem, a, n_act, None, _sub(0), None) == -1 and _supported(lib, stem, a, n_act, None, _sub(0), None) == 0
        for every in (0, -4):
            assert _call(lib, stem, a, n_act, None, _sub(0), _seg(every)) == -2 and _supported(lib, stem, a, n_act, None, _sub(0), _seg(every)) == 0
    for tb in (None, tab):
        # a NULL sub-steps struct is one sub-step: supported, and the call gets as far as the pointer checks
        assert _supported(lib, stem, mk(), n_act, tb, None, ok) == 1 and _call(lib, stem, mk(), n_act, tb, None, ok) == -1
        for n in (0, -3, 1025):
            assert _call(lib, stem, mk(), n_act, tb, _sub(n), ok) == -2 and _supported(lib, stem, mk(), n_act, tb, _sub(n), ok) == 0
        for n in (1, 2, 3, 1024):
            for every in (1, 3, 11, 1000, 0x7fffffff):
                assert _supported(lib, stem, mk(), n_act, tb, _sub(n), _seg(every)) == 1
            assert _supported(lib, stem, mk(kernel=_lib.KERNEL_GENERIC), n_act, tb, _sub(n), ok) == 1
            assert _call(lib, stem, mk(), n_act, tb, _sub(n), ok) == -1
            for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                assert _supported(lib, stem, mk(kernel=kernel), n_act, tb, _sub(n), ok) == 0
                assert _call(lib, stem, mk(kernel=kernel), n_act, tb, _sub(n), ok) == -5
        assert _call(lib, stem, None, n_act, tb, _sub(2), ok) == -1
    for sub in (None, _sub(1), _sub(2)):                 # a NULL tableau needs a valid method; a tableau makes the method unread
        assert _call(lib, stem, mk(method=77), n_act, None, sub, ok) == -3 and _supported(lib, stem, mk(method=77), n_act, None, sub, ok) == 0
        assert _supported(lib, stem, mk(method=77), n_act, tab, sub, ok) == 1
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _call(lib, stem, mk(), n_act, R(bad), _sub(2), ok) == -3
    assert _call(lib, stem, mk(), n_act, tab, _sub(2), ok, R(unknown)) == -3 and _supported(lib, stem, mk(), n_act, tab, _sub(2), ok, R(unknown)) == 0
    tanh, silu = R(fused.Act(_lib.ACT_TANH).abi()), R(fused.Act(_lib.ACT_SILU).abi())
    assert _supported(lib, stem, mk(), n_act, None, _sub(2), ok, tanh) == 1 and _supported(lib, stem, mk(), n_act, tab, None, ok, silu) == 1
    # order: segments | sub-steps | act pair | NULL args | tableau | route
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(0), _seg(0), R(unknown)) == -2
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2), ok, R(unknown)) == -3
    assert _call(lib, stem, None, n_act, R(bad), _sub(2), ok) == -1
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2), ok) == -3
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, tab, _sub(2), ok) == -5


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


def test_side_outputs_teacher_forcing_the_dataset_rows_and_x_true():
    lib = _lib.load()
    sub, ok = _sub(3), _seg(3, 256)
    a = _ode_args()
    a.save_act = a.save_xstage = 256
    assert _supported(lib, "ode_integrate", a, 1, None, sub, ok) == 0 and _call(lib, "ode_integrate", a, 1, None, sub, ok) == -5
    d = _with_x(_dae_args(), "dae_integrate")
    d.save_act = d.save_xstage = d.save_ae_act = 256
    assert _supported(lib, "dae_integrate", d, 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", d, 2, None, sub, ok) == -5
    b = _ode_bwd_args()
    b.saved_act = b.saved_xstage = 256
    assert _supported(lib, "ode_backward", b, 1, None, sub, ok) == 0 and _call(lib, "ode_backward", b, 1, None, sub, ok) == -5
    e = _dae_bwd_args()
    e.base.saved_act = 256
    assert _supported(lib, "dae_backward", e, 2, None, sub, ok) == 0 and _call(lib, "dae_backward", e, 2, None, sub, ok) == -5
    # every teacher-forcing flag
    fa = _ode_args()
    fa.flags = _lib.FLAG_INPUT_TRUE_X
    assert _supported(lib, "ode_integrate", fa, 1, None, sub, ok) == 0 and _call(lib, "ode_integrate", fa, 1, None, sub, ok) == -5
    for flags in (1, 2, 3):
        fd = _with_x(_dae_args(), "dae_integrate")
        fd.flags = flags
        assert _supported(lib, "dae_integrate", fd, 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", fd, 2, None, sub, ok) == -5
        tfd = _dae_bwd_args(flags=flags)
        assert _supported(lib, "dae_backward", tfd, 2, None, sub, ok) == 0 and _call(lib, "dae_backward", tfd, 2, None, sub, ok) == -5
    tfo = _ode_bwd_args(flags=_lib.FLAG_INPUT_TRUE_X)
    assert _supported(lib, "ode_backward", tfo, 1, None, sub, ok) == 0 and _call(lib, "ode_backward", tfo, 1, None, sub, ok) == -5
    # a DAE forward whose x view is empty
    assert _supported(lib, "dae_integrate", _dae_args(), 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", _dae_args(), 2, None, sub, ok) == -5
    # forward calls with every pointer in place get as far as the workspace check
    a = _ode_args()
    for l in range(4):
        a.de.weight[l] = a.de.bias[l] = 256
    a.t.ptr = a.x.ptr = a.z.ptr = a.all_initial = a.x_out = 256
    assert _call(lib, "ode_integrate", a, 1, None, None, ok) == -4 and _call(lib, "ode_integrate", a, 1, None, _sub(2), _seg(1)) == -4
    d = _with_x(_dae_args(), "dae_integrate")
    for m in (d.de, d.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    d.t.ptr = d.z.ptr = d.v.ptr = d.x_init = d.all_initial = d.x_out = d.i_out = 256
    assert _call(lib, "dae_integrate", d, 2, None, None, ok) == -4
    # backward calls: x_sub where there are sub-steps, x_true where a step restarts (T - 1 = 11 > every), then the workspace
    b = _ode_bwd_args()
    _fill_ode_bwd(b)
    assert _call(lib, "ode_backward", b, 1, None, _sub(2), ok) == -1               # no x_sub
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), _seg(3)) == -1     # no x_true, and 11 > 3
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), _seg(10)) == -1
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), _seg(11)) == -4    # no restart: x_true may be NULL
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), ok) == -4 and _call(lib, "ode_backward", b, 1, None, None, ok) == -4
    e = _dae_bwd_args()
    _fill_dae_bwd(e.base)
    assert _call(lib, "dae_backward", e, 2, None, _sub(2), ok) == -1
    assert _call(lib, "dae_backward", e, 2, None, None, _seg(3)) == -1 and _call(lib, "dae_backward", e, 2, None, None, _seg(100)) == -4
    assert _call(lib, "dae_backward", e, 2, None, _sub(2, 256), ok) == -4


def test_the_lds_fit_is_the_sub_build_s():
    """the build keeps no LDS of its own (the restart is a countdown in a scalar register): its _supported answers are the _sub build's
    along a growing z_dim, for K0 and for K5"""
    lib = _lib.load()
    for stem, make, n_act in ENTRIES:
        answers = []
        for zd in range(64, 660, 4):
            a = _with_x(make(kernel=_lib.KERNEL_GENERIC, xd=8, zd=zd, hidden=32), stem)
            ms, sub = _supported(lib, stem, a, n_act, None, _sub(2), _seg(3)), A.supported(lib, stem, a, n_act, None, _sub(2), family="sub")
            assert ms == sub, (stem, zd)
            answers.append(ms)
        assert 0 in answers and 1 in answers, stem          # (the DAE stems too: the AE input and the head are in their fit)


# ----------------------------------------------------------------------------- 6. routing
_layers = A.hip_layers


def test_python_predicates_options_and_refusals():
    ode01 = _layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    tanh = fused.Act(_lib.ACT_TANH, name="Tanh")
    n = 8 + 2 + 2 + 2
    de = _layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = _layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    for method in ("euler", "rk4", nd.Kutta3().method):
        for sub in (1, 2, 7):
            for w in (1, 3, 1000):
                ms = dict(substeps=sub, segment=w)
                assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, **ms)
                assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel="generic", act=tanh, **ms)
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, **ms)
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, **ms)
                assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, act=(tanh, None), **ms)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_x=True, **ms)
                for kernel in ("wave", "tile", "mfma", "wide"):
                    assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, **ms)
                    assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, kernel=kernel, **ms)
                    assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, **ms)
                assert fused.ode_backward_supported(method, ode01, 8, 2, "generic", **ms)
                assert fused.dae_backward_supported(method, de, ae, 8, 2, 2, 2, kernel="generic", **ms)
                # the two combinations without a kernel
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, externals="linear", **ms)
                assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, per_trajectory=True, **ms)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, "generic", per_trajectory=True, **ms)
    opts = lambda substeps=1, externals="hold", act=None, method="rk4", pt=False, w=3: fused.GenericOpts.of(method, (act,), substeps, externals, pt, w)
    assert opts().family == "ms" and opts(5).family == "ms" and opts(1, "linear").family == "none" and opts(pt=True).family == "none"
    assert fused.GenericOpts.of("rk4", (None,)).family == "plain" and fused.GenericOpts.of("rk4", (None,)).segment is None
    assert fused.GenericOpts.of("rk4", (None,), segment=4).family == "ms"
    c = opts(2, w=7).c_args(x_true=torch.zeros(2, 2, 2))
    assert c[0] is None and c[1] is None and c[2]._obj.substeps == 2 and c[3]._obj.every == 7 and c[3]._obj.x_true
    assert opts(w=10 ** 12).c_args()[3]._obj.every == 0x7fffffff and not opts().c_args()[3]._obj.x_true
    with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
        opts().require_plain("a specialised entry")
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        opts(1, "linear").require_generic("x", "generic", False)
    with pytest.raises(_lib.UnsupportedShapeError, match="per-trajectory"):
        opts(pt=True).require_generic("x", "generic", False)
    with pytest.raises(ValueError, match="segment"):
        opts().require_generic("x", "generic", False, teacher_forced=True)
    for kernel, save in (("wave", False), ("mfma", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="segment=3"):          # the sixth option in the naming order
            opts().require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="substeps"):
            opts(3).require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="activation"):
            opts(3, act=tanh).require_generic("x", kernel, save)
        with pytest.raises(_lib.UnsupportedShapeError, match="tableau"):
            opts(method=nd.Kutta3().method).require_generic("x", kernel, save)
    opts().require_generic("x", "generic", False)
    with pytest.raises(ValueError, match="x_true"):
        fused._ms_rows("x", 3, None, 8, 5, 6, torch.device("cpu"))
    with pytest.raises(ValueError, match="x_true"):
        fused._ms_rows("x", 3, torch.zeros(7, 5, 6), 8, 5, 6, torch.device("cpu"))
    assert fused._ms_rows("x", 7, None, 8, 5, 6, torch.device("cpu")) is None and fused._ms_rows("x", None, None, 8, 5, 6, torch.device("cpu")) is None


def test_routing_of_segments_in_the_solver():
    for cls in (nd.RK4, nd.Kutta3):
        for kernel in ("auto", "generic"):
            for n in (1, 3):
                s = cls(substeps=n, segment=4)
                s.kernel, s.fused = kernel, "require"
                assert s._generic_only_ok("integrate_ODE", (None,))
                assert s._generic_kwargs() == dict(segment=4, **({"substeps": n} if n > 1 else {}))
        assert "segment" not in cls()._generic_kwargs()
        for kernel in ("wave", "tile", "mfma", "wide"):
            s = cls(segment=4)
            s.kernel, s.fused = kernel, "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,))          # walks, with the warning
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match="segment" if cls is nd.RK4 else "tableau"):
                s._generic_only_ok("integrate_ODE", (None,))
        for kw, pt, word in ((dict(externals="linear"), False, "externals='linear'"), ({}, True, "per-trajectory")):
            s = cls(segment=4, **kw)
            s.kernel, s.fused = "auto", "auto"
            assert not s._generic_only_ok("integrate_ODE", (None,), pt)
            s.fused = "require"
            with pytest.raises(_lib.UnsupportedShapeError, match=word):
                s._generic_only_ok("integrate_ODE", (None,), pt)
    # the walk carries the two combinations: externals='linear' next to segments is the sliced free run too
    de, t, x, z, ev, zj = _ode(60)
    a0 = torch.cat((x[0], z[0]), -1)
    with torch.no_grad():
        lin = nd.RK4(segment=3, externals="linear", substeps=2)
        lin.fused = "off"
        free = nd.RK4(externals="linear", substeps=2)
        free.fused = "off"
        got = C.run_ode(lin, de, t, x, z, a0, ev, zj)
        assert torch.equal(got[:4], C.run_ode(free, de, t, x, z, a0, ev, zj)[:4])
        ev_ = nd.ODE_Event()
        ev_.set_event(ev, zj)
        tail = free.integrate_ODE(x_func=de, t=t[3:7], x=x[3:7], z=z[3:7], all_initial=a0, event_fn=ev_.event_fn, jump_change_fn=ev_.jump_change_fn)
        assert torch.equal(got[4:7], tail[1:])
    # a dataset x that requires grad and has a restart is not fused; a short record is
    s = nd.RK4(segment=3)
    s.fused = "require"
    xg = x.clone().requires_grad_(True)
    with pytest.raises(nd.NotFusableError, match="segment"):
        C.run_ode(s, de, t, xg, z, a0, ev, zj)
    # the one-launch encoded forwards decline a solver with segments before any tensor is looked at
    for m, args in ((models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.RK4(segment=5)), (torch.zeros(3, 4, 1), torch.zeros(3, 4, 8), torch.zeros(3, 4, 2))),
                    (models.DAE_Model(8, 2, 2, 2, 64, direct_encode=True, solver=nd.RK4(segment=5)), (None,) * 6)):
        assert m._forward_encoded(*args, None, None) is None if len(args) == 3 else m._forward_encoded(*args, None, None, None) is None
    assert "segment" in nd.FixedGridODESolver._note_walk.__code__.co_consts.__repr__()


def test_the_time_chunked_launches_refuse_segments():
    """a chunk has neither the dataset rows nor the restarts' phase: `segment=` must not be dropped or restarted per chunk"""
    from py_psnode_amd import sharded
    z = torch.zeros(9, 4, 2)
    for w in (1, 3, 100):
        with pytest.raises(ValueError, match="segment"):
            sharded.integrate_ode_pipelined("rk4", [], z[:, :, :1], z, z, z[0], chunks=4, gather=False, segment=w)
        with pytest.raises(ValueError, match="segment"):
            sharded.integrate_dae_pipelined("rk4", [], [], z[0], z[:, :, :1], z, z, z, z[0], chunks=4, gather=False, segment=w)
