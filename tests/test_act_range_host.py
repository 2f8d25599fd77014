"""The instrument of the activation range tests checked on the CPU, before any kernel (cases, references, gates: act_range_cases.py).

  - the fp64 closed forms act64 / act_grad64 (and their chains) equal torch.autograd in fp64, kinks included;
  - the constants the bounds use (Lipschitz constants, sup |act''|) hold, and the derived bounds stay inside the budget the header of
    csrc/psnode_act.h promises (`budget_bound`);
  - the probe sets contain every knee they claim to;
  - ATen's fp32 walk of the same modules passes every gate, for every entry of ACTS: the reference alone stays within its bounds
    (`reference_candidate`: ATen, but for the four forms of ATen's that are themselves among the mutants);
  - every mutant of ACT_MUTANTS is rejected by at least one gate on the probe set the GPU file uses;
  - the wide-range trajectory case is well posed for the kinked activations: ATen's fp32 walk takes no branch the other way;
  - the Softplus-from-output rule is rejected at thresholds 5, 1 and 0 and accepted at 20: the cut the kernels' routing relies on.
"""
import functools
import math
import types

import pytest
import torch

import act_range_cases as A
import elu_range_cases as E

KEYS = list(A.ACTS)
DEPTHS = (1, 3, 5)          # hidden layers of the GPU file's shapes


@functools.lru_cache(maxsize=None)
def _u(key):
    return A.act_probe_magnitudes(A.ACTS[key])


def _grid64():
    return torch.cat((torch.linspace(-40.0, 40.0, 80001, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-300, -1e-300], dtype=torch.float64),
                      A.EXTREMES.double()))


@pytest.mark.parametrize("key", KEYS)
def test_closed_forms_equal_autograd_fp64(key):
    a = A.ACTS[key]
    a = types.SimpleNamespace(**{**vars(a), "alpha": a.act.alpha, "beta": a.act.beta, "thr": a.act.threshold})     # the module's own doubles
    x = torch.cat((_grid64(), _u(key).double())).requires_grad_(True)
    if a.kind == "softplus":
        x = torch.cat((x.detach(), torch.tensor([a.thr / a.beta], dtype=torch.float64))).requires_grad_(True)     # exactly at the threshold
    m = a.module().double()
    y = m(x)
    g, = torch.autograd.grad(y.sum(), x)
    xd = x.detach()
    sel = torch.isfinite(y.detach()) & torch.isfinite(g)       # (ATen's own fp64 forms overflow on part of the extremes)
    assert bool(sel[xd.abs() <= 40].all())
    ev = (A.act64(a, xd) - y.detach()).abs()[sel]
    eg = (A.act_grad64(a, xd) - g).abs()[sel]
    assert float((ev / y.detach()[sel].abs().clamp_min(1.0)).max()) <= 1e-13, float(ev.max())
    assert float((eg / g[sel].abs().clamp_min(1.0)).max()) <= 1e-13, float(eg.max())      # (ATen's own fp64 forms cancel a little)
    assert bool(torch.isfinite(A.act64(a, xd)).all()) and bool(torch.isfinite(A.act_grad64(a, xd)).all())
    # the chain
    x3 = torch.linspace(-30.0, 30.0, 4001, dtype=torch.float64).requires_grad_(True)
    y3 = m(m(m(x3)))
    g3, = torch.autograd.grad(y3.sum(), x3)
    assert float((A.act_n64(a, x3.detach(), 3) - y3.detach()).abs().max()) <= 1e-13
    assert float((A.act_grad_n64(a, x3.detach(), 3) - g3).abs().max()) <= 1e-13


def test_kink_rules_are_torchs():
    z = torch.zeros(1, dtype=torch.float64)
    assert float(A.act_grad64(A.ACTS["ReLU"], z)) == 0.0
    assert float(A.act_grad64(A.ACTS["LeakyReLU(0.1)"], z)) == pytest.approx(0.1, abs=1e-7)
    assert float(A.act_grad64(A.ACTS["ELU(2.0)"], z)) == 2.0 and float(A.act_grad64(A.ACTS["ELU(0.5)"], z)) == 0.5
    sp = A.ACTS["Softplus(2,5)"]
    at = torch.tensor([2.5, math.nextafter(2.5, 3.0)], dtype=torch.float64)
    g = A.act_grad64(sp, at)
    assert float(g[0]) == pytest.approx(1 / (1 + math.exp(-5.0)), abs=1e-15) and float(g[1]) == 1.0
    v = A.act64(sp, at)
    assert float(v[0]) == pytest.approx(math.log1p(math.exp(5.0)) / 2, abs=1e-15) and float(v[1]) == float(at[1])


@pytest.mark.parametrize("key", KEYS)
def test_lipschitz_and_curvature_constants(key):
    a = A.ACTS[key]
    x = torch.linspace(-40.0, 40.0, 160001, dtype=torch.float64)
    g = A.act_grad64(a, x)
    assert float(g.abs().max()) <= A.lipschitz(a) * (1 + 1e-12)
    if a.kind in A.CURV:
        assert float(((g[1:] - g[:-1]) / (x[1] - x[0])).abs().max()) <= A.CURV[a.kind]


@pytest.mark.parametrize("key", [k for k in KEYS if A.ACTS[k].kind in A.BUDGET_COUNT])
def test_derived_bounds_keep_the_headers_budget(key):
    """ELU_ABS per layer (chained) + the stated count of roundings x 2^-24 x |ref|: the running error analysis of each value form never
    exceeds it on the probe set."""
    a = A.ACTS[key]
    u = _u(key).double()
    for n in DEPTHS:
        derived, _ = A.value_bound(a, u, n)
        budget = A.budget_bound(a, u, n)
        k = int((derived - budget).argmax())
        assert bool((derived <= budget).all()), (key, n, float(u[k]), float(derived[k]), float(budget[k]))


@pytest.mark.parametrize("key", KEYS)
def test_probe_sets_contain_their_knees(key):
    a = A.ACTS[key]
    u = _u(key)
    have = set(u.tolist())
    inf = torch.tensor(math.inf)
    for c in A.act_knees(a):
        c32 = torch.tensor(float(c), dtype=torch.float32)
        for v in (c32, torch.nextafter(c32, inf), torch.nextafter(c32, -inf)):
            assert float(v) in have, (key, c, float(v))
    band = A.act_band(a).float()
    assert band.numel() == 512 and all(float(v) in have for v in band)
    for v in (0.0, 2.0 ** -149, -2.0 ** -149, 1e4, -1e4, 88.0, -88.0, 104.0, -104.0):
        assert float(torch.tensor(v, dtype=torch.float32)) in have, v
    assert bool((u == 0).any()) and bool(torch.signbit(u[u == 0]).any())       # -0.0 too
    if a.kind == "softplus":
        assert 80.0 / a.beta in have and a.thr / a.beta in have
    if a.kind == "mish":
        assert 20.0 in have
    assert u.numel() <= 2 * 5200          # two values per trajectory of the T = 2 probe: "a few thousand trajectories"
    assert sorted(A.EXTREMES.abs().tolist()) == sorted(torch.tensor([1e19, 3e19, 1e30, 3e38] * 2, dtype=torch.float32).tolist())


def _gates(a, cand, u, n):
    out, g = A.candidate_run(cand, u, n)
    v = A.value_gate(a, out, u, n)
    d = A.grad_gate(a, g, u, n)
    return v, d


@pytest.mark.parametrize("key", KEYS)
def test_aten_fp32_passes_every_gate(key):
    a = A.ACTS[key]
    u = _u(key)
    for n in DEPTHS:
        v, d = _gates(a, A.reference_candidate(a), u, n)
        assert v[0], (key, n, "value", v)
        assert d[0], (key, n, "derivative", d)


# ATen's own fp32 forms that are not finite over the fp32 range (x^3 overflows in GELU(tanh)'s backward): the kernels' forms are asked
# for more than ATen delivers there, so ATen is not held to the extremes gate for them
ATEN_NOT_FINITE_AT_EXTREMES = ("GELU(tanh)",)


@pytest.mark.parametrize("key", [k for k in KEYS if k not in ATEN_NOT_FINITE_AT_EXTREMES])
def test_aten_fp32_passes_the_extremes_gate(key):
    a = A.ACTS[key]
    for n in (1, 3):
        out, g = A.candidate_run(A.reference_candidate(a), A.EXTREMES, n)
        ok, ev, eg = A.extremes_gate(a, out, g, A.EXTREMES, n)
        assert ok, (key, n, ev, eg, out, g)


@pytest.mark.parametrize("key", KEYS)
def test_fp32_walk_of_the_probe_passes_every_gate(key):
    """The whole instrument on the CPU: the T = 2 identity probe through the oracle's fp32 loop with this module as its activation, values
    against act_n64, dL/dz[0] under a one-hot dL/dxs against act_grad_n64."""
    a = A.ACTS[key]
    u = _u(key)
    xd, zd, H, nh = 8, 2, 64, 3
    c = E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=False, u=u)
    assert set(c.u_of.reshape(-1).tolist()) >= set(u.tolist())
    m = A.reference_candidate(a)
    z = c.z.clone().requires_grad_(True)
    with E.oracle_elu(m):
        xs = E.ode_walk64("euler", c.layers, c.t, c.x[0], z, c.a0)
    v = A.value_gate(a, xs[1:].detach(), c.u_of, nh)
    assert v[0], (key, v)
    nr = min(xd, zd)
    G = torch.zeros_like(xs)
    G[1, :, :nr] = 1.0
    g, = torch.autograd.grad((xs * G).sum(), z)
    d = A.grad_gate(a, g[0, :, :nr], c.z[0, :, :nr], nh)
    assert d[0], (key, d)


def _rejected(a, cand, u):
    why = []
    for n in (1, 3):
        v, d = _gates(a, cand, u, n)
        why += ([f"value n={n}"] if not v[0] else []) + ([f"derivative n={n}"] if not d[0] else [])
        out, g = A.candidate_run(cand, A.EXTREMES, n)
        why += [f"extremes n={n}"] if not A.extremes_gate(a, out, g, A.EXTREMES, n)[0] else []
    return why


@pytest.mark.parametrize("mutant", A.ACT_MUTANTS, ids=[m[0].replace(" ", "_") for m in A.ACT_MUTANTS])
def test_every_mutant_is_rejected(mutant):
    name, key, cand = mutant
    why = _rejected(A.ACTS[key], cand, _u(key))
    assert why, f"{name}: no gate rejects it"


def test_softplus_from_output_is_rejected_below_the_cut_and_accepted_above():
    """The rule of the act build (beta h > thr ? 1 : 1 - e^(-beta h)) against the derivative gate: wrong by up to e^-thr below
    thr = 24 ln 2, torch's rule to fp32 precision above.  K5 routes a Softplus below the cut to its pre build (csrc/psnode_act.h)."""
    worst = {}
    for key in ("Softplus(2,5)", "Softplus(1,1)", "Softplus(1,0)", "Softplus(1,20)"):
        a = A.ACTS[key]
        for n in (1, 3):
            _, g = A.candidate_run(A.softplus_grad_from_output(a), _u(key), n)
            ok, err, bound, at, *_ = A.grad_gate(a, g, _u(key), n)
            worst[key, n] = (ok, float((g.double() - A.act_grad_n64(a, _u(key), n)).abs().max()))
            assert ok == (a.thr >= A.SOFTPLUS_CUT), (key, n, err, bound, at)
    assert worst["Softplus(2,5)", 1][1] > 6e-3 and worst["Softplus(1,1)", 1][1] > 0.3 and worst["Softplus(1,0)", 1][1] > 0.99
    assert A.ACTS["Softplus(1,20)"].thr >= A.SOFTPLUS_CUT > 16.6


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("key", A.DISCONTINUOUS)
def test_wide_case_is_well_posed_in_fp32(key, method):
    """ATen's fp32 autograd walk of the wide-range case against the fp64 walk, at a tenth of the GPU file's gates: no hidden pre-activation
    of the run sits within rounding of a kink of this activation (a flipped branch shows as 1e-3 or more)."""
    a = A.ACTS[key]
    c = A.wide_act_case()
    G = torch.randn(A.T_WIDE, A.B_WIDE, 8, generator=torch.Generator().manual_seed(11))
    x64, named64 = A.ode_grads64(c, method, a, G)
    x32, named32 = A.ode_grads(c, method, a, G, torch.float32)
    with E.oracle_elu(a.module()):
        o32 = E.run_ode(c, method)
    assert E.traj_rel_err(x32, x64) <= 3e-6 and E.traj_rel_err(o32, x64) <= 3e-6
    worst = max(A.close_gate(g, r, what)[2] for (what, r), (_, g) in zip(named64, named32))
    assert worst <= 2e-5, worst


def test_softplus_below_the_cut_answers_for_the_pre_builds_fit():
    """K5 keeps u for a Softplus whose threshold is below 24 ln 2, so such a call fits where the pre build fits: the pinned boundary of
    test_activations_pre_host.py (hidden 160 x 3, z 2: x 24 fits, x 32 does not), while the default threshold keeps the act build's fit
    and the forward, which keeps no u, fits either way."""
    import ctypes

    from py_psnode_amd import _lib
    from test_activations_pre_host import _act, _ode_args, _ode_bwd
    lib = _lib.load()
    R = ctypes.byref
    inside, outside = _ode_bwd(xd=24, hidden=(160, 160, 160)), _ode_bwd(xd=32, hidden=(160, 160, 160))
    for thr, fits_outside in ((20.0, 1), (16.64, 1), (16.63, 0), (5.0, 0), (1.0, 0), (0.0, 0), (-3.0, 0)):
        sp = _act(_lib.ACT_SOFTPLUS, beta=1.0, threshold=thr)
        assert lib.psnode_ode_backward_act_supported(R(inside), R(sp)) == 1, thr
        assert lib.psnode_ode_backward_act_supported(R(outside), R(sp)) == fits_outside, thr
        assert lib.psnode_ode_integrate_act_supported(R(_ode_args(xd=32, hidden=(160, 160, 160))), R(sp)) == 1, thr
