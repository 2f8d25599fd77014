"""The instrument, not the kernels (no GPU, nothing launched): the gate, the training judges and the case builders of
tests/generic_cases.py, which the tests of the K0 / K5 option families share.  The judges get synthetic results -- CPU tensors and a
stand-in trajectory whose grad_fn carries the expected name -- and must pass the accepted set and reject each mutant with the assertion
that names it."""
import pytest
import torch

import generic_cases as C
from helpers import TOL_GPU

TOLS = [2e-4, TOL_GPU]          # the two gradient tolerances in use


# ----------------------------------------------------------------------------- close
def _ref_and_unit(seed=0):
    """a float64 reference with max |ref| = 3 at one element, and the unit tensor of that element"""
    ref = torch.rand(4, 5, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    ref[2, 3] = -3.0
    unit = torch.zeros_like(ref)
    unit[1, 1] = 1.0
    return ref, unit


@pytest.mark.parametrize("tol", TOLS)
def test_close_accepts_half_the_tolerance_and_rejects_twice(tol):
    ref, unit = _ref_and_unit()
    C.close(ref + 0.5 * tol * 3.0 * unit, ref, "inside", tol)
    C.close((ref - 0.5 * tol * 3.0 * unit).float(), ref, "inside, in float32", tol)
    for sign in (1.0, -1.0):
        with pytest.raises(AssertionError, match="outside: err"):
            C.close(ref + sign * 2.0 * tol * 3.0 * unit, ref, "outside", tol)
    # the scale is the reference's max, floored at 1e-6
    C.close(torch.full((3,), 0.5e-6 * tol, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), "zeros", tol)
    with pytest.raises(AssertionError):
        C.close(torch.full((3,), 2e-6 * tol, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), "zeros", tol)


@pytest.mark.parametrize("tol", TOLS)
def test_close_none_and_empty(tol):
    ref, _ = _ref_and_unit()
    C.close(None, None, "neither side has one", tol)
    with pytest.raises(AssertionError, match="missing: no value"):
        C.close(None, ref, "missing", tol)
    # a None reference stands for zeros
    C.close(torch.zeros(4, 5), None, "zeros for None", tol)
    with pytest.raises(AssertionError):
        C.close(torch.full((4, 5), 1e-3), None, "not zeros", tol)
    # the teacher-forced file's arm: a None candidate read as zeros, on request only
    C.close(None, torch.zeros(4, 5, dtype=torch.float64), "None for zeros", tol, none_is_zero=True)
    with pytest.raises(AssertionError, match="err"):
        C.close(None, ref, "None for values", tol, none_is_zero=True)
    # an empty tensor has a shape to get right
    C.close(torch.zeros(7, 3, 0), torch.zeros(7, 3, 0, dtype=torch.float64), "empty", tol)
    with pytest.raises(AssertionError, match="shape"):
        C.close(torch.zeros(7, 2, 0), torch.zeros(7, 3, 0, dtype=torch.float64), "empty", tol)
    with pytest.raises(AssertionError, match="shape"):
        C.close(torch.zeros(5, 4), ref, "transposed", tol)


# ----------------------------------------------------------------------------- the judges
class _FusedOdeStandIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        return a.clone()

    @staticmethod
    def backward(ctx, g):
        return g


class _FusedDaeStandIn(_FusedOdeStandIn):
    pass


def _results(dae, seed=1):
    """ref, got, again, xs, ref_xs of a run that passes: gradients by name (one of them None on both sides, as without events),
    trajectories [T,B,D] whose stand-in grad_fn is named as the fused functions'"""
    g = torch.Generator().manual_seed(seed)
    names = ("x_init", "z", "v", "a0", "zj", "vj", "de0", "ae0") if dae else ("z", "a0", "zj", "x", "p0", "p1")
    ref = {k: torch.randn(3, 4, generator=g, dtype=torch.float64) for k in names}
    ref["zj"] = None
    got = {k: None if r is None else r.float() for k, r in ref.items()}
    again = {k: None if q is None else q.clone() for k, q in got.items()}
    fn = _FusedDaeStandIn if dae else _FusedOdeStandIn
    ref_xs = [torch.randn(6, 5, 3, generator=g, dtype=torch.float64) for _ in range(2 if dae else 1)]
    xs = [fn.apply(r.float().requires_grad_(True)) for r in ref_xs]
    return (ref, got, again, tuple(xs), tuple(ref_xs)) if dae else (ref, got, again, xs[0], ref_xs[0])


def _judge(dae, res, prefix=None, tol=2e-4, **kw):
    judge = C.judge_dae_training if dae else C.judge_ode_training
    judge(*res, ("_FusedDae" if dae else "_FusedOde") if prefix is None else prefix, tol, "case", **kw)


def _off(a, factor, tol):
    """a, with its largest element moved by factor x tol x max |a|"""
    a = a.clone()
    k = int(a.abs().argmax())
    a.view(-1)[k] += factor * tol * float(a.abs().max())
    return a


@pytest.mark.parametrize("dae", [False, True])
@pytest.mark.parametrize("tol", TOLS)
def test_judges_accept_the_accepted_set(dae, tol):
    res = _results(dae)
    _judge(dae, res, tol=tol)
    _judge(dae, res, tol=tol, ref_float=True)
    ref, got, again, xs, ref_xs = res
    got["z"] = again["z"] = _off(ref["z"], 0.5, tol)
    _judge(dae, (ref, got, again, xs, ref_xs), tol=tol)
    # what a file does not check is left out by None
    judge = C.judge_dae_training if dae else C.judge_ode_training
    judge(ref, got, None, xs, None, None, tol)


@pytest.mark.parametrize("dae", [False, True])
@pytest.mark.parametrize("tol", TOLS)
def test_judges_reject_each_mutant_by_name(dae, tol):
    def mutant(edit, match, **kw):
        res = list(_results(dae))
        res[1] = dict(res[0])          # (the candidate starts as the float64 reference itself: only the mutation is off)
        res[2] = dict(res[0])
        edit(*res)
        with pytest.raises(AssertionError, match=match):
            _judge(dae, tuple(res), tol=tol, **kw)
        return res

    def both(key, value):
        def edit(ref, got, again, xs, ref_xs):
            got[key] = again[key] = value(ref[key])
        return edit

    mutant(both("z", lambda r: _off(r, 2.0, tol)), "case grad z: err")
    mutant(both("a0", lambda r: None), "case grad a0: no value")
    with pytest.raises(AssertionError, match="err"):          # ... and the teacher-forced arm does not wave it through either
        res = list(_results(dae))
        res[1]["a0"] = res[2]["a0"] = None
        _judge(dae, tuple(res), tol=tol, none_is_zero=True)

    def one_bit(ref, got, again, xs, ref_xs):
        again["z"] = got["z"].clone()
        again["z"].view(torch.int64).view(-1)[5] ^= 1          # one bit of one element
    mutant(one_bit, "backward not repeatable: z")

    def none_once(ref, got, again, xs, ref_xs):
        ref["zj"] = None
        got["zj"], again["zj"] = None, torch.zeros(3, 4)
    mutant(none_once, "backward not repeatable: zj")
    mutant(lambda ref, got, again, xs, ref_xs: got.pop("z"), "no gradient z")

    res = list(_results(dae))
    walked = res[4][0].float().requires_grad_(True) * 1.0 if dae else res[4].float().requires_grad_(True) * 1.0
    res[3] = (walked, res[3][1]) if dae else walked
    with pytest.raises(AssertionError, match="grad_fn"):
        _judge(dae, tuple(res), tol=tol)
    with pytest.raises(AssertionError, match="grad_fn"):
        _judge(dae, _results(dae), prefix="_FusedOdeSub" if not dae else "_FusedDaeLin", tol=tol)

    for which in range(2 if dae else 1):
        res = list(_results(dae))
        r = res[4][which] if dae else res[4]
        moved = r.clone()
        moved[3, 2] += 2.0 * TOL_GPU * float(r[:, 2].abs().max())          # trajectory 2, by twice the gate
        fn = _FusedDaeStandIn if dae else _FusedOdeStandIn
        out = fn.apply(moved.requires_grad_(True))
        res[3] = tuple(out if k == which else q for k, q in enumerate(res[3])) if dae else out
        with pytest.raises(AssertionError, match=f"trajectory {'xi'[which]} off"):
            _judge(dae, tuple(res), tol=tol)
        inside = r.clone()
        inside[3, 2] += 0.5 * TOL_GPU * float(r[:, 2].abs().max())
        out = fn.apply(inside.requires_grad_(True))
        res[3] = tuple(out if k == which else q for k, q in enumerate(res[3])) if dae else out
        res[1], res[2] = dict(res[0]), dict(res[0])
        _judge(dae, tuple(res), tol=tol)


# ----------------------------------------------------------------------------- the case builders
def _same(a, b):
    if torch.is_tensor(a) or a is None:
        return (a is None and b is None) or torch.equal(a, b)
    pa, pb = list(a.parameters()), list(b.parameters())
    return len(pa) == len(pb) and all(torch.equal(p, q) for p, q in zip(pa, pb)) and str(a) == str(b)


@pytest.mark.parametrize("given_clock", [False, True])
def test_two_calls_with_the_same_arguments_are_equal_throughout(given_clock):
    t = C.dyadic_clock(7, 5, 2) if given_clock else None
    for make in (lambda: C.ode_case(6, 2, (16, 8), 5, 7, seed=11, ev_rows=(1, 3), t=t, pad=True, act=torch.nn.Tanh),
                 lambda: C.dae_case(4, 2, 3, 2, (16,), (8, 8), 5, 7, seed=12, ev_rows=(0, 3), t=t, perturb_x_init=True),
                 lambda: C.dae_case(4, 0, 3, 2, (16,), (8, 8), 5, 7, seed=12, ev_rows=(2,), t=t)):
        a, b = make(), make()
        assert len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    assert all(torch.equal(p, q) for p, q in zip(C.cotangents(4, (3, 2), (5,)), C.cotangents(4, (3, 2), (5,))))
    G, Gi = C.cotangents(4, (3, 2), (5,))
    assert torch.equal(G, torch.randn(3, 2, generator=torch.Generator().manual_seed(4))) and not torch.equal(Gi, C.cotangents(4, (5,))[0])
    # the seed decides, and the perturbed x_init is a draw of its own between i and the jump rows
    assert not _same(C.ode_case(6, 2, (16, 8), 5, 7, seed=11)[0], C.ode_case(6, 2, (16, 8), 5, 7, seed=13)[0])
    plain, moved = (C.dae_case(4, 2, 3, 2, (16,), (8, 8), 5, 7, seed=12, ev_rows=(0, 3), perturb_x_init=p) for p in (False, True))
    assert all(_same(p, q) for p, q in zip(plain[:7], moved[:7])) and torch.equal(plain[7], plain[3][0])
    assert not torch.equal(moved[7], moved[3][0]) and not torch.equal(plain[10], moved[10])


def test_pad_leaves_trajectory_zero_whole():
    g = lambda: torch.Generator().manual_seed(5)
    whole, pad = C.ragged_clock(9, 7, g()), C.ragged_clock(9, 7, g(), pad=True)
    assert (whole >= 0).all() and torch.equal(pad[:, 0], whole[:, 0]) and torch.equal(pad[:-2], whole[:-2])
    assert (pad[-2:, 2::3] == -1.0).all() and torch.equal(pad[-2:, [0, 1, 3, 4, 6]], whole[-2:, [0, 1, 3, 4, 6]])
    assert torch.equal(C.padded(whole), pad) and (whole >= 0).all()          # (padded copies)
    de, t, x, z, ev, zj = C.ode_case(6, 2, (16,), 7, 9, seed=3, ev_rows=(1, 4), pad=True)
    assert (t[:, 0] >= 0).all() and (t[-2:, 2::3] == -1.0).all() and torch.equal(ev[:, :, 0], t[[1, 4], :, 0].t())
    # too short or too narrow to pad: the clock stays whole
    assert (C.ragged_clock(3, 7, g(), pad=True) >= 0).all() and (C.ragged_clock(9, 2, g(), pad=True) >= 0).all()


def test_event_rows_outside_the_grid_are_dropped_and_z_dim_zero_has_none():
    t = C.dyadic_clock(6, 4, 2)
    de, _, x, z, ev, zj = C.ode_case(6, 2, (16,), 4, 6, seed=7, t=t, ev_rows=(0, 3, 5, 9))          # rows 5 (the last) and 9 start no step
    assert ev.shape == (4, 2, 1) and zj.shape == (4, 2, 2) and torch.equal(ev, t[[0, 3]].permute(1, 0, 2))
    assert _same(zj, C.ode_case(6, 2, (16,), 4, 6, seed=7, t=t, ev_rows=(0, 3))[5])
    for rows in ((), (5,), (7, 8)):
        assert C.ode_case(6, 2, (16,), 4, 6, seed=7, t=t, ev_rows=rows)[4:] == (None, None)
        assert C.dae_case(4, 2, 3, 2, (16,), (8,), 4, 6, seed=7, t=t, ev_rows=rows)[9:] == (None, None, None)
    assert C.ode_case(6, 2, (16,), 4, 2, seed=7, ev_rows=(1, 1))[4:] == (None, None)          # T = 2: row 1 is the last
    assert C.ode_case(6, 2, (16,), 4, 1, seed=7, ev_rows=(1, 0))[4:] == (None, None)          # T = 1: no step at all
    # z_dim 0: an ODE has nothing to jump; a DAE keeps its events (v jumps)
    assert C.ode_case(6, 0, (16,), 4, 6, seed=7, t=t, ev_rows=(0, 3))[4:] == (None, None)
    ev, zj, vj = C.dae_case(4, 0, 3, 2, (16,), (8,), 4, 6, seed=7, t=t, ev_rows=(0, 3))[9:]
    assert ev.shape == (4, 2, 1) and zj.shape == (4, 2, 0) and vj.shape == (4, 2, 3)
    assert C.without_x(C.dae_case(4, 2, 3, 2, (16,), (8,), 4, 6, seed=7))[3].shape == (6, 4, 0)
