"""Teacher-forced training (integrate_ODE(input_true_x=True), integrate_DAE(input_true_x / input_true_i)) on the generic backward K5:
every call here runs under solver.fused = "require".  References: the reference's own gradients (golden set G8) where they exist, else
this package's walk of the SAME modules in float64 on the CPU with gradients from torch autograd (the method of test_gpu_activations.py).
Gates: test_grad_goldens.TOL_GPU (1e-5 of each tensor's max) against G8 and across kernels, 2e-4 of the tensor's max against the fp64 walk."""
import copy
import functools
import warnings

import pytest
import torch

import generic_cases as C
from helpers import T, load
from py_psnode_amd import autograd as pag
from py_psnode_amd import fused, models
from py_psnode_amd import neural_dae as nd
from test_grad_goldens import SOLVERS, TOL_GPU, _close

pytestmark = pytest.mark.gpu

TOL_WALK = 2e-4     # gradient gate of tests/test_gpu_backward.py / test_gpu_activations.py (max abs error <= TOL x the tensor's max)
# against the fp64 walk: a gradient the fused run leaves None stands for zeros
_close_walk = functools.partial(C.close, tol=TOL_WALK, none_is_zero=True)
METHODS = ["euler", "midpoint", "rk4"]
P = lambda a: a.permute(1, 0, 2)
ODE_FLAGS = [(True, False)]
DAE_FLAGS = [(True, False), (False, True), (True, True)]


# ----------------------------------------------------------------------------- 1. the reference's gradients (G8), 3. K5 vs K4f / K7f
def _g8(tag, method, tx, ti, kernel):
    """test_tf_goldens._run with solver.kernel = `kernel`; returns what it compares instead of comparing"""
    d = load(f"g8_tf_grad_{tag}.npz")
    H = int(tag.split("_h")[1]) if "_h" in tag else 64
    m = models.ODE_Model(8, 2, H) if tag.startswith("ode") else models.DAE_Model(8, 2, 2, 2, H)
    sd = {k[4:].replace("__", "."): T(v) for k, v in d.items() if k.startswith("sd__")}
    assert set(sd) == set(m.state_dict())
    m.load_state_dict(sd)
    m = m.cuda()
    m.solver = SOLVERS[method]()
    m.solver.fused = "require"
    m.solver.kernel = kernel
    c = lambda k: T(d[k]).cuda()
    leaves = {k: c(k).requires_grad_(True) for k in ("z", "v", "z_jump", "v_jump")}
    x, i, t, ev = c("x"), c("i"), c("t"), c("event_t")
    if tag.startswith("dae"):
        res = m(t=t, x=x, z=leaves["z"], v=leaves["v"], i=i, event_t=ev, z_jump=leaves["z_jump"], v_jump=leaves["v_jump"],
                input_true_x=tx, input_true_i=ti)
    else:
        m.event.set_event(t=ev, z=leaves["z_jump"])
        a0 = torch.cat((P(x)[0], P(leaves["z"])[0]), dim=-1)
        res = (P(m.solver.integrate_ODE(x_func=m.de_func, t=P(t), x=P(x), z=P(leaves["z"]), all_initial=a0, event_fn=m.event.event_fn,
                                        jump_change_fn=m.event.jump_change_fn, input_true_x=True)),)
    sum((r * c(f"G{k}")).sum() for k, r in enumerate(res)).backward()
    got = {f"out{k}": r.detach() for k, r in enumerate(res)}
    got.update({"gp__" + name.replace(".", "__"): (p.grad if p.grad is not None else torch.zeros_like(p)) for name, p in m.named_parameters()})
    got.update({f"g_{k}": (a.grad if a.grad is not None else torch.zeros_like(a)) for k, a in leaves.items()})
    return d, got


def _generic_takes(tag):
    d = load(f"g8_tf_grad_{tag}.npz")
    lay = lambda prefix: [(w.cuda(), b.cuda()) for w, b in __import__("helpers").layers(d, prefix)]
    if tag.startswith("ode"):
        return fused.ode_backward_supported("rk4", lay("sd__de_func__x_dot"), 8, 2, kernel="generic")
    return fused.dae_backward_supported("rk4", lay("sd__de_func__x_dot"), lay("sd__ae_func__i_calculator"), 8, 2, 2, 2, kernel="generic")


@pytest.mark.parametrize("tag", ["ode01", "dae01", "ode01_h128", "dae01_h128"])
@pytest.mark.parametrize("method", METHODS)
def test_k5_reproduces_the_reference_teacher_forced_gradients(tag, method):
    if "_h128" in tag and not _generic_takes(tag):
        pytest.skip(f"{tag}: *_backward_supported(kernel='generic') is False -- the generic backward K5 does not fit this shape into LDS")
    seen = []
    orig_o, orig_d, orig_w = fused.ode_backward, fused.dae_backward_tf, fused.dae_backward_wide
    fused.ode_backward = lambda *a, **k: (seen.append(("ode", k.get("kernel"))), orig_o(*a, **k))[1]
    fused.dae_backward_tf = lambda *a, **k: (seen.append(("tf", k.get("kernel"))), orig_d(*a, **k))[1]
    fused.dae_backward_wide = lambda *a, **k: (seen.append(("k7f", None)), orig_w(*a, **k))[1]
    try:
        for tx, ti in (ODE_FLAGS if tag.startswith("ode") else DAE_FLAGS):
            d, got = _g8(tag, method, tx, ti, "generic")
            key = f"{method}_tx{int(tx)}_ti{int(ti)}"
            worst = 0.0
            for k, g in got.items():
                if f"{key}_{k}" in d:
                    ref = torch.as_tensor(d[f"{key}_{k}"], dtype=torch.float64)
                    worst = max(worst, float((g.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6))
            print(f"{tag} {key} kernel=generic: worst error / tensor max = {worst:.3e}")
            for k, g in got.items():
                if f"{key}_{k}" in d:
                    _close(g, d[f"{key}_{k}"], f"{tag} {key} {k}", TOL_GPU)
    finally:
        fused.ode_backward, fused.dae_backward_tf, fused.dae_backward_wide = orig_o, orig_d, orig_w
    assert seen and all(s == (("ode" if tag.startswith("ode") else "tf"), "generic") for s in seen), seen      # K5 ran, not K4f / K7f


@pytest.mark.parametrize("tag", ["ode01", "dae01"])
@pytest.mark.parametrize("method", METHODS)
def test_k5_equals_k4f_k7f(tag, method):
    for tx, ti in (ODE_FLAGS if tag.startswith("ode") else DAE_FLAGS):
        _, a = _g8(tag, method, tx, ti, "generic")
        _, b = _g8(tag, method, tx, ti, "mfma")
        for k in a:
            _close(a[k], b[k].double().cpu(), f"{tag} {method} tx{int(tx)} ti{int(ti)} {k}: K5 vs the MFMA backward", TOL_GPU)


# ----------------------------------------------------------------------------- 2. shapes only K5 covers, vs the fp64 walk
def _solver(method, fused_mode, kernel="auto"):
    s = SOLVERS[method]()
    s.fused, s.kernel = fused_mode, kernel
    return s


def _event_steps(events, Tn):
    return {"none": [], "mid": [Tn // 2], "first": [0], "two": [1, Tn // 2 + 1]}[events]


def _ode_case(xd, zd, hidden, B, Tn, seed, events):
    return C.ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=_event_steps(events, Tn))


def _train_ode(method, case, G, dev, kernel="auto", x_grad=False):
    """teacher-forced throughout; the dataset x is a leaf only where a test asks what that raises"""
    return C.ode_train(functools.partial(_solver, method, kernel=kernel), case, G, dev, tx=True, x_leaf=x_grad, copy=True)


ODE_SHAPES = {"x20_h96x2": (20, 3, (96, 96)), "one_hidden": (6, 2, (48,)), "five_hidden": (5, 1, (40, 32, 40, 32, 40)),
              "h160_streamed": (8, 2, (160, 160, 160))}


@pytest.mark.parametrize("events", ["none", "mid", "first"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", list(ODE_SHAPES))
def test_ode_shapes_only_k5_covers(shape, method, events):
    xd, zd, hidden = ODE_SHAPES[shape]
    case = _ode_case(xd, zd, hidden, 19, 9, seed=3 + len(shape), events=events)          # B = 19: not a multiple of 16
    G = torch.randn(case[2].shape, generator=torch.Generator().manual_seed(3))
    _, ref = _train_ode(method, case, G, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _train_ode(method, case, G, "cuda")
    C.judge_ode_training(ref, got, None, xs, None, "_FusedOde", TOL_WALK, f"{shape} {method} {events}", none_is_zero=True)


def _dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, events):
    return C.dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, ev_rows=_event_steps(events, Tn), perturb_x_init=True)


def _train_dae(method, case, G, Hi, tx, ti, dev, kernel="auto", i_grad=False):
    xs, _, g = C.dae_train(functools.partial(_solver, method, kernel=kernel), case, G, Hi, dev, tx, ti, i_leaf=i_grad, copy=True)
    return xs, g


DAE_SHAPES = {"z4_v6_i6": (8, 4, 6, 6, (64, 64, 64), (64, 64, 64)), "z0": (5, 0, 3, 2, (48, 48), (32, 32)),
              "ae_depth_differs": (4, 2, 1, 2, (48, 48, 48), (32,))}


def _dae_check(shape, method, tx, ti, events, Tn=9, B=19):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES[shape]
    case = _dae_case(xd, zd, vd, idim, dh, ah, B, Tn, seed=5 + len(shape), events=events)
    G = torch.randn(case[3].shape, generator=torch.Generator().manual_seed(6))
    Hi = torch.randn(case[6].shape, generator=torch.Generator().manual_seed(7))
    _, ref = _train_dae(method, case, G, Hi, tx, ti, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = _train_dae(method, case, G, Hi, tx, ti, "cuda")
    C.judge_dae_training(ref, got, None, (xs, None), None, "_FusedDaeTeacherForced", TOL_WALK,
                         f"{shape} {method} tx{int(tx)} ti{int(ti)} {events}", none_is_zero=True)


@pytest.mark.parametrize("events", ["none", "mid", "first"])
@pytest.mark.parametrize("tx,ti", DAE_FLAGS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", list(DAE_SHAPES))
def test_dae_shapes_only_k5_covers(shape, method, tx, ti, events):
    _dae_check(shape, method, tx, ti, events)


@pytest.mark.parametrize("tx,ti", DAE_FLAGS)
@pytest.mark.parametrize("method", METHODS)
def test_two_grid_points(method, tx, ti):
    """T = 2: one step, with and without an event at it"""
    for events in ("none", "first"):
        _dae_check("z4_v6_i6", method, tx, ti, events, Tn=2)
        if tx and not ti:
            case = _ode_case(20, 3, (96, 96), 19, 2, seed=8, events=events)
            G = torch.randn(case[2].shape, generator=torch.Generator().manual_seed(3))
            _, ref = _train_ode(method, case, G, "cpu")
            _, got = _train_ode(method, case, G, "cuda")
            for k, r in ref.items():
                _close_walk(got[k], r, f"ode T=2 {method} {events} grad {k}")


def _ode_raw_gx0(method, case, G, kernel):
    """psnode_ode_backward_f32's grad_x0 through the raw-tensor API (the autograd function discards it: the dataset x gets no gradient)"""
    import torch.nn as nn
    de, t, x, z, ev, zj = case
    lay = [(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in de.x_dot if isinstance(m, nn.Linear)]
    c = lambda q: None if q is None else q.cuda()
    t, x, z, ev, zj = c(t), c(x), c(z), c(ev), c(zj)
    idx = fused.event_table(t, ev) if ev is not None else None
    return fused.ode_backward(method, lay, t, z, torch.cat((x[0], z[0]), -1), x, c(G), event_idx=idx, z_jump=zj, kernel=kernel,
                              input_true_x=True)[0]


@pytest.mark.parametrize("events", ["none", "first"])
@pytest.mark.parametrize("method", METHODS)
def test_ode_grad_x0_is_grad_xs0_plus_the_start_adjoint_of_step_0(method, events):
    """grad_x0 of the C ABI under INPUT_TRUE_X: x[0] is both xs[0] and the start of step 0, and no other step reaches it.  Reference at
    x_dim 20: the fp64 walk with x[0] a leaf of its own; on the ode01 shape also K4f's grad_x0."""
    case = _ode_case(20, 3, (96, 96), 19, 9, seed=21, events=events)
    de, t, x, z, ev, zj = case
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    d = lambda q: None if q is None else q.double()
    x0 = d(x)[0].clone().requires_grad_(True)
    xd_ = torch.cat((x0.unsqueeze(0), d(x)[1:]), 0)
    event = nd.ODE_Event()
    if ev is not None:
        event.set_event(d(ev), d(zj))
    xs = _solver(method, "off").integrate_ODE(x_func=copy.deepcopy(de).double(), t=d(t), x=xd_, z=d(z), all_initial=torch.cat((d(x)[0], d(z)[0]), -1),
                                              event_fn=event.event_fn if ev is not None else None,
                                              jump_change_fn=event.jump_change_fn if ev is not None else None, input_true_x=True)
    (xs * d(G)).sum().backward()
    got = _ode_raw_gx0(method, case, G, "generic")
    assert float((x0.grad - d(G)[0]).abs().max()) > 0          # the start adjoint of step 0 is part of it
    _close_walk(got, x0.grad, f"{method} {events} grad_x0 (x_dim 20)")
    case8 = _ode_case(8, 2, (64, 64, 64), 19, 9, seed=22, events=events)
    G8 = torch.randn(case8[2].shape, generator=torch.Generator().manual_seed(4))
    _close(_ode_raw_gx0(method, case8, G8, "generic"), _ode_raw_gx0(method, case8, G8, "wide").double().cpu(), f"{method} {events} grad_x0: K5 vs K4f", TOL_GPU)


# ----------------------------------------------------------------------------- 4. the carry is cut
@pytest.mark.parametrize("method", METHODS)
def test_ode_no_adjoint_travels_from_step_to_step(method):
    Tn, k = 10, 6
    case = _ode_case(20, 3, (96, 96), 19, Tn, seed=11, events="none")
    G = torch.zeros(case[2].shape)
    G[k + 1] = torch.randn(G[k + 1].shape, generator=torch.Generator().manual_seed(1))
    _, got = _train_ode(method, case, G, "cuda")
    gz = got["z"]
    assert float(gz[k].abs().max()) > 0
    assert torch.equal(gz[:k], torch.zeros_like(gz[:k])) and torch.equal(gz[k + 1:], torch.zeros_like(gz[k + 1:]))


@pytest.mark.parametrize("method", METHODS)
def test_dae_no_adjoint_travels_through_x_without_events(method):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    Tn, k = 10, 6
    case = _dae_case(xd, zd, vd, idim, dh, ah, 19, Tn, seed=12, events="none")
    G = torch.zeros(case[3].shape)
    G[k + 1] = torch.randn(G[k + 1].shape, generator=torch.Generator().manual_seed(1))
    Hi = torch.zeros(case[6].shape)
    _, got = _train_dae(method, case, G, Hi, True, False, "cuda")
    for name in ("z", "v"):
        g = got[name]
        assert float(g[k].abs().max()) > 0, name
        assert torch.equal(g[:k], torch.zeros_like(g[:k])) and torch.equal(g[k + 1:], torch.zeros_like(g[k + 1:])), name


@pytest.mark.parametrize("ahead", [0, 2])
@pytest.mark.parametrize("method", METHODS)
def test_dae_event_head_is_the_one_link_through_x(method, ahead):
    """input_true_x only, one event at step e, grad_xs non-zero at grid point e + 1 + ahead alone.  ahead = 0: the DE of step e hands its
    algebraic adjoint to the recomputed head, which reads the RUNNING state xs[e] -- so step e - 1 (and no earlier one) receives an
    adjoint.  ahead = 2: the steps after the event start from dataset rows; nothing reaches the event.
    (The issue words this case as "an event at step e < k": that is ahead = 2, where grad_z_jump is exactly zero.  The link through the
    recomputed head exists for k = e only, so that case is checked too.)"""
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    Tn = 10
    e = Tn // 2
    case = _dae_case(xd, zd, vd, idim, dh, ah, 19, Tn, seed=13, events="mid")
    G = torch.zeros(case[3].shape)
    G[e + 1 + ahead] = torch.randn(G[0].shape, generator=torch.Generator().manual_seed(1))
    Hi = torch.zeros(case[6].shape)
    _, ref = _train_dae(method, case, G, Hi, True, False, "cpu")
    _, got = _train_dae(method, case, G, Hi, True, False, "cuda")
    for k, r in ref.items():
        _close_walk(got[k], r, f"{method} ahead {ahead} grad {k}")
    gz = got["z"]
    if ahead == 0:
        assert float(got["zj"].abs().max()) > 0 and float(gz[e - 1].abs().max()) > 0
        assert torch.equal(gz[:e - 1], torch.zeros_like(gz[:e - 1]))
    else:
        assert torch.equal(got["zj"], torch.zeros_like(got["zj"])) and torch.equal(gz[:e + ahead], torch.zeros_like(gz[:e + ahead]))


@pytest.mark.parametrize("events", ["none", "mid"])
@pytest.mark.parametrize("method", METHODS)
def test_true_i_cuts_the_head_from_the_de(method, events):
    """grad_xs = 0.  With both flags nothing reaches the DE (its algebraic adjoint is dropped and the heads read dataset rows): its parameter
    gradient is exactly zero, and the AE's is the sum of the heads' own VJPs of grad_is.  With input_true_i alone the heads read the
    running state, so the DE does receive an adjoint -- through x, never through i: it matches the walk."""
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    case = _dae_case(xd, zd, vd, idim, dh, ah, 19, 9, seed=14, events=events)
    G = torch.zeros(case[3].shape)
    Hi = torch.randn(case[6].shape, generator=torch.Generator().manual_seed(7))
    _, ref = _train_dae(method, case, G, Hi, True, True, "cpu")
    _, got = _train_dae(method, case, G, Hi, True, True, "cuda")
    for k, g in got.items():
        if k.startswith("de"):
            assert torch.equal(g, torch.zeros_like(g)), k
        elif k.startswith("ae"):
            assert float(g.abs().max()) > 0, k
            _close_walk(g, ref[k], f"{method} {events} grad {k}")
    _, got0 = _train_dae(method, case, G, torch.zeros_like(Hi), True, True, "cuda")
    for k, g in got0.items():
        if k.startswith("ae") or k.startswith("de"):
            assert torch.equal(g, torch.zeros_like(g)), k               # no grad_is, no AE gradient: it depends on grad_is alone
    _, ref1 = _train_dae(method, case, G, Hi, False, True, "cpu")
    _, got1 = _train_dae(method, case, G, Hi, False, True, "cuda")
    for k, r in ref1.items():
        if r is not None or got1[k] is not None:
            _close_walk(got1[k], r, f"{method} {events} true_i alone grad {k}")


# ----------------------------------------------------------------------------- 5. bitwise-repeatable
@pytest.mark.parametrize("tx,ti", DAE_FLAGS)
def test_backward_is_bitwise_repeatable(tx, ti):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    case = _dae_case(xd, zd, vd, idim, dh, ah, 200, 12, seed=15, events="two")
    G = torch.randn(case[3].shape, generator=torch.Generator().manual_seed(6))
    Hi = torch.randn(case[6].shape, generator=torch.Generator().manual_seed(7))
    _, g1 = _train_dae("rk4", case, G, Hi, tx, ti, "cuda")
    _, g2 = _train_dae("rk4", case, G, Hi, tx, ti, "cuda")
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    if tx and not ti:
        oc = _ode_case(20, 3, (96, 96), 200, 12, seed=16, events="two")
        Go = torch.randn(oc[2].shape, generator=torch.Generator().manual_seed(5))
        _, o1 = _train_ode("rk4", oc, Go, "cuda")
        _, o2 = _train_ode("rk4", oc, Go, "cuda")
        for k in o1:
            assert (o1[k] is None and o2[k] is None) or torch.equal(o1[k], o2[k]), k


# ----------------------------------------------------------------------------- 6. routing
def test_x20_teacher_forced_training_runs_under_require():
    """Before this feature: NotFusableError (no backward kernel with teacher forcing outside K4f's class)."""
    case = _ode_case(20, 3, (64, 64, 64), 19, 8, seed=17, events="mid")
    G = torch.randn(case[2].shape, generator=torch.Generator().manual_seed(3))
    for kernel in ("auto", "generic"):
        xs, got = _train_ode("rk4", case, G, "cuda", kernel=kernel)
        assert type(xs.grad_fn).__name__.startswith("_FusedOde") and all(torch.isfinite(g).all() for g in got.values() if g is not None)
    with pytest.raises(nd.NotFusableError):
        _train_ode("rk4", case, G, "cuda", kernel="mfma")          # no K4f at x_dim 20, and "mfma" excludes K5


def test_dataset_rows_with_grad_still_raise():
    case = _ode_case(20, 3, (64, 64, 64), 19, 8, seed=17, events="none")
    G = torch.randn(case[2].shape, generator=torch.Generator().manual_seed(3))
    with pytest.raises(nd.NotFusableError):
        _train_ode("rk4", case, G, "cuda", x_grad=True)
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    dc = _dae_case(xd, zd, vd, idim, dh, ah, 19, 8, seed=18, events="none")
    Gd, Hi = torch.zeros(dc[3].shape), torch.ones(dc[6].shape)
    with pytest.raises(nd.NotFusableError):
        _train_dae("rk4", dc, Gd, Hi, False, True, "cuda", i_grad=True)


def test_a_tanh_de_still_raises():
    import torch.nn as nn
    de = models.DE_Func(23, (64, 64, 64), 20, activation=nn.Tanh)
    case = (de,) + _ode_case(20, 3, (64, 64, 64), 19, 8, seed=17, events="none")[1:]
    G = torch.randn(case[2].shape, generator=torch.Generator().manual_seed(3))
    with pytest.raises(nd.NotFusableError):
        _train_ode("rk4", case, G, "cuda")


# ----------------------------------------------------------------------------- 7. dataset rows at the end of their allocation
def _at_end(a, pad=1000):
    """the same values as a view that ends at the last byte of its buffer"""
    buf = torch.empty(pad + a.numel(), dtype=a.dtype, device=a.device)
    view = buf[pad:].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() + view.numel() * 4 == buf.data_ptr() + buf.numel() * 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("tx,ti", DAE_FLAGS)
def test_dataset_rows_at_the_end_of_their_buffers(tx, ti):
    xd, zd, vd, idim, dh, ah = DAE_SHAPES["z4_v6_i6"]
    de_m, ae_m, t, x, z, v, i, x_init, a0, ev, zj, vj = (None if q is None else (q.cuda() if torch.is_tensor(q) else q)
                                                         for q in _dae_case(xd, zd, vd, idim, dh, ah, 21, 9, seed=19, events="mid"))
    import torch.nn as nn
    de = [(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in de_m.x_dot if isinstance(m, nn.Linear)]
    ae = [(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in ae_m.i_calculator if isinstance(m, nn.Linear)]
    idx = fused.event_table(t, ev)
    xs, is_ = fused.dae_integrate("rk4", de, ae, x_init, t, x, z, v, i, a0, z_jump=zj, v_jump=vj, event_idx=idx, input_true_x=tx,
                                  input_true_i=ti, kernel="generic")[:2]
    gxs, gis = torch.randn_like(xs), torch.randn_like(is_)
    call = lambda xs_, x_, i_: fused.dae_backward_tf("rk4", de, ae, t, z, v, a0, xs_, is_, gxs, gis, event_idx=idx, z_jump=zj, v_jump=vj,
                                                     kernel="generic", x_true=x_ if tx else None, i_true=i_ if ti else None)
    a, b = call(xs, x, i), call(_at_end(xs), _at_end(x), _at_end(i))
    for k in a:
        if k in ("de", "ae"):
            assert all(torch.equal(p, q) for p, q in zip(a[k], b[k])), k
        else:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    if tx and not ti:
        oc = _ode_case(20, 3, (96, 96), 21, 9, seed=20, events="mid")
        lay = [(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in oc[0].x_dot if isinstance(m, nn.Linear)]
        to, xo, zo, evo, zjo = (q.cuda() for q in oc[1:])
        a0o = torch.cat((xo[0], zo[0]), -1)
        io = fused.event_table(to, evo)
        go = torch.randn_like(xo)
        oc_ = lambda x_: fused.ode_backward("rk4", lay, to, zo, a0o, x_, go, event_idx=io, z_jump=zjo, kernel="generic", input_true_x=True)
        p, q = oc_(xo), oc_(_at_end(xo))
        assert all(torch.equal(u, w) for u, w in zip(p[:4], q[:4])) and all(torch.equal(u, w) for u, w in zip(p[4], q[4]))


def test_predicates_on_the_device():
    """what the host test asks with stand-in tensors, asked with real ones"""
    de = models.DE_Func(23, (64, 64, 64), 20).cuda()
    import torch.nn as nn
    lay = [(m.weight.detach(), m.bias.detach()) for m in de.x_dot if isinstance(m, nn.Linear)]
    assert pag.ode_training_supported("rk4", lay, 20, 3, 50, 33, input_true_x=True)
    assert pag.ode_training_supported("rk4", lay, 20, 3, 50, 33, kernel="generic", input_true_x=True)
    assert not pag.ode_training_supported("rk4", lay, 20, 3, 50, 33, act=fused.Act(fused._lib.ACT_TANH, name="Tanh"), input_true_x=True)
