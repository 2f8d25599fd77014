"""Cases, references and gates for the activation range tests (test_act_range_host.py on the CPU, test_gpu_act_range.py on the GPU): the
identity-probe instrument of elu_range_cases.py, generalised from ELU(1) to the ten kinds of csrc/psnode_act.h.

The probes are elu_range_cases' (`identity_probe_ode` / `_dae`, `random_probe_*`, `wide_*_case`): with weights of zeros and ones and dt = 1
each grid point of a probe's result IS act^n(u) of a chosen u, and dL/dz[0] under a one-hot output gradient IS prod_k act'(p_k) along the
chain p_0 = u, p_{k+1} = act(p_k).  New here:

  ACTS                      the kinds and parameters under test, each with its nn.Module factory and its fused.Act;
  act64 / act_grad64        fp64 closed forms of act and act' with torch's rules at the kinks;  act_n64 / act_grad_n64: along the chain;
  act_probe_magnitudes      probe_magnitudes() plus, per kind, a dense band and the one-ulp neighbours of the form's own knees;  EXTREMES;
  value_gate / grad_gate    |out - act_n64| and |got - act_grad_n64| against bounds DERIVED from the forms of psnode_act.h (below);
  ACT_MUTANTS               wrong forms, each of which at least one gate must reject (test_act_range_host.py).

How the bounds are derived.  U = 2^-24 is one fp32 rounding (relative).  v_exp_f32, v_rcp_f32 and v_log_f32 are taken at 1 ulp = 2 U.  The
exponential e^x is exp2(x * log2e): the product and the constant round once each, which moves the result by 2 |x| U relative, so
rel(e^x) = (2 + 2 |x|) U (`_relexp`).  Every form is then walked operation by operation at the fp64 value of its operands (a first-order
running error analysis; `_value_err` and `_grad_err` hold one paragraph per kind, with the operation counts), which gives a bound per u,
not one per kind: a global count x |ref| cannot tell `1 - s` by subtraction from `e^-u s` (both are a few U of a quantity near 1).
Chains: a layer's input error e_k passes through the layer with the activation's Lipschitz constant, e_{k+1} = L e_k + (this layer's
bound); act' of a perturbed input moves by sup |act''| e_k (u-forms) or |d act' / d h| e_{k+1} (h-forms); the product of the n factors
moves by sum_k (factor k's bound x the other factors, each taken with its own bound added) plus one rounding per multiplication.
Results below 2^-126 may be flushed to zero (v_exp_f32 and v_rcp_f32 do not return denormals): every bound of a rounded branch carries
2^-126, times (1 + |u|) where the form multiplies such a factor by u.
  erfcf is the device library's and v_log_f32's accuracy near 1 is not documented, so for GELU and for Softplus' log branch the
derivation does not close on its own.  There the rule of `traj_gates` applies: no further from fp64 than 3 x ATen's own fp32 CPU error at
that u (taken as the largest relative error among the 33 probe values around u, so that one value ATen happens to hit exactly does not
set a bound of zero), plus the absolute part ELU_ABS = 1.2e-7 per layer that psnode_act.h and DESIGN.md promise.  GELU's value also has
to meet the derivation with erfc at the OpenCL limit of 16 ulp, which the device library is written to: it is the smaller of the two
for u < 0, where ATen's own `1 + erf` cancels.  Softplus' log branch adds the counted roundings AROUND v_log_f32, (9 + 2 |beta u|) U |ref|
(`_value_err`): ATen evaluates u + log1p(e^-u), which from u = 17 up is u to far below an ulp, so that its error alone would ask the log
form for more than one rounding of its result (the first GPU run showed exactly that: errors of one ulp of 16 .. 32, 1.9e-6, against
3 x ATen's 1e-10 relative -- the relative part of an unbounded branch had been left out of this one bound).
  Trajectory checks of a kinked activation are well posed only away from the kinks: see WIDE_SEED.
  `budget_bound` is the promise itself -- ELU_ABS per layer plus a stated count of roundings x U x |ref| -- and the host file asserts that
the derived bound never exceeds it on the probe sets: the forms keep the budget the header states.
No bound was tuned on what a kernel returns; the host file applies every gate to an fp32 CPU walk of the same modules first
(`reference_candidate`: ATen's kernels, but for four forms of ATen's that cancel where psnode_act.h's do not and are mutants themselves).
"""
import functools
import math
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

import elu_range_cases as E
from elu_range_cases import ELU_ABS, _worst, probe_magnitudes
from py_psnode_amd import fused

U = 2.0 ** -24
TINY = 2.0 ** -126                  # smallest normal fp32: results below it may be flushed
SOFTPLUS_CUT = 24 * math.log(2)     # csrc/psnode_act.h, kSoftplusCut: from here the act build's rule on h is torch's to fp32 precision
GELU_C, GELU_K = math.sqrt(2 / math.pi), 0.044715


# ------------------------------------------------------------------------------------------------------------------ the kinds under test
def _entry(key, factory):
    m = factory()
    a = fused.act_of_module(m)
    if a is False:
        a = fused.pre_act_of_module(m)
    assert isinstance(a, fused.Act), key
    kind = type(m).__name__.lower() + ("_tanh" if getattr(m, "approximate", "none") == "tanh" else "")
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))         # the parameters as the kernels receive them (psnode_act_f32)
    return types.SimpleNamespace(key=key, kind=kind, module=factory, act=a, alpha=f32(a.alpha), beta=f32(a.beta), thr=f32(a.threshold))


ACTS = {e.key: e for e in (
    _entry("ELU(0.5)", lambda: nn.ELU(0.5)), _entry("ELU(2.0)", lambda: nn.ELU(2.0)),
    _entry("Tanh", nn.Tanh), _entry("Sigmoid", nn.Sigmoid), _entry("ReLU", nn.ReLU),
    _entry("LeakyReLU(0.1)", lambda: nn.LeakyReLU(0.1)), _entry("LeakyReLU(0.0)", lambda: nn.LeakyReLU(0.0)),
    _entry("Softplus(1,20)", lambda: nn.Softplus(1, 20)), _entry("Softplus(2,5)", lambda: nn.Softplus(2, 5)),
    _entry("Softplus(1,1)", lambda: nn.Softplus(1, 1)), _entry("Softplus(1,0)", lambda: nn.Softplus(1, 0)),
    _entry("SiLU", nn.SiLU), _entry("GELU", nn.GELU), _entry("GELU(tanh)", lambda: nn.GELU(approximate="tanh")), _entry("Mish", nn.Mish))}
KINKED = ("elu", "relu", "leakyrelu")       # act' jumps at 0
# Lipschitz constants sup |act'| and sup |act''| (checked numerically by the host file)
LIP = {"elu": None, "tanh": 1.0, "sigmoid": 0.25, "relu": 1.0, "leakyrelu": None, "softplus": 1.0, "silu": 1.1, "gelu": 1.13, "gelu_tanh": 1.13,
       "mish": 1.09}
CURV = {"silu": 0.5, "gelu": 0.8, "gelu_tanh": 0.81, "mish": 0.65}


def lipschitz(a):
    return max(1.0, a.alpha) if a.kind in ("elu", "leakyrelu") else LIP[a.kind]


# ------------------------------------------------------------------------------------------------------------------ fp64 closed forms
def _t64(y):
    return torch.as_tensor(y, dtype=torch.float64)


def _mish_parts(y):
    w = torch.exp(y.clamp(max=300.0))
    n = w * (w + 2)
    return w, n, n / (n + 2)


def _gelu_tanh_z(y):
    return GELU_C * (y + GELU_K * y * y * y)


def act64(a, y):
    """act(y) in fp64, torch's rules at the kinks (Softplus decided on beta y > thr)."""
    y = _t64(y)
    k = a.kind
    if k == "elu":
        return torch.where(y > 0, y, a.alpha * torch.expm1(y.clamp(max=0.0)))
    if k == "tanh":
        return torch.tanh(y)
    if k == "sigmoid":
        return torch.sigmoid(y)
    if k == "relu":
        return y.clamp(min=0.0)
    if k == "leakyrelu":
        return torch.where(y > 0, y, a.alpha * y)
    if k == "softplus":
        by = a.beta * y
        return torch.where(by > a.thr, y, (torch.log1p(torch.exp(-by.abs())) + by.clamp(min=0.0)) / a.beta)
    if k == "silu":
        return y * torch.sigmoid(y)
    if k == "gelu":
        return y * 0.5 * torch.erfc(-y * math.sqrt(0.5))
    if k == "gelu_tanh":
        return y * torch.sigmoid(2 * _gelu_tanh_z(y))              # (1 + tanh z) / 2 = sigmoid(2 z)
    assert k == "mish", k
    return y * _mish_parts(y)[2]


def act_grad64(a, y):
    """act'(y) in fp64: ReLU'(0) = 0, LeakyReLU'(0) = s, ELU(alpha)'(0) = alpha, Softplus' = beta y > thr ? 1 : sigmoid(beta y)."""
    y = _t64(y)
    k = a.kind
    one = torch.ones_like(y)
    if k == "elu":
        return torch.where(y > 0, one, a.alpha * torch.exp(y.clamp(max=0.0)))
    if k == "tanh":
        return 4 * torch.sigmoid(2 * y) * torch.sigmoid(-2 * y)        # 1 - tanh^2 without cancellation
    if k == "sigmoid":
        return torch.sigmoid(y) * torch.sigmoid(-y)
    if k == "relu":
        return torch.where(y > 0, one, 0 * one)
    if k == "leakyrelu":
        return torch.where(y > 0, one, a.alpha * one)
    if k == "softplus":
        return torch.where(a.beta * y > a.thr, one, torch.sigmoid(a.beta * y))
    if k == "silu":
        s = torch.sigmoid(y)
        return s + y * s * torch.sigmoid(-y)
    if k == "gelu":
        return 0.5 * torch.erfc(-y * math.sqrt(0.5)) + y * torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)
    if k == "gelu_tanh":
        z2 = 2 * _gelu_tanh_z(y)
        return torch.sigmoid(z2) + y * 2 * torch.sigmoid(z2) * torch.sigmoid(-z2) * GELU_C * (1 + 3 * GELU_K * y * y)
    assert k == "mish", k
    w, n, T = _mish_parts(y)
    return T + y * (4 * (n + 1) / (n + 2) ** 2) * torch.sigmoid(y)


def chain64(a, u, n):
    """[p_0 = u, p_1 = act(u), ..., p_n] in fp64."""
    ps = [_t64(u)]
    for _ in range(n):
        ps.append(act64(a, ps[-1]))
    return ps


def act_n64(a, u, n):
    return chain64(a, u, n)[-1]


def act_grad_n64(a, u, n):
    ps = chain64(a, u, n)
    g = torch.ones_like(ps[0])
    for p in ps[:-1]:
        g = g * act_grad64(a, p)
    return g


# ------------------------------------------------------------------------------------------------------------------ probe values
EXTREMES = torch.tensor([s * m for m in (1e19, 3e19, 1e30, 3e38) for s in (1.0, -1.0)], dtype=torch.float32)


def _ulps(c):
    """c as fp32 with its two neighbours on either side."""
    c = torch.tensor(float(c), dtype=torch.float32)
    out = [c]
    lo = hi = c
    for _ in range(2):
        lo, hi = torch.nextafter(lo, torch.tensor(-math.inf)), torch.nextafter(hi, torch.tensor(math.inf))
        out += [lo, hi]
    return torch.stack(out).double()


def act_knees(a):
    """The u at which this kind's form changes branch or saturates (csrc/psnode_act.h)."""
    k = a.kind
    if k == "softplus":
        kn = [a.thr / a.beta, 80.0 / a.beta]
        if a.thr > 0:
            kn.append(math.log(math.expm1(a.thr)) / a.beta)        # below it beta h <= thr: the lower end of the band the rule on h gets wrong
        return kn
    if k == "mish":
        return [20.0]
    if k == "gelu_tanh":
        return [9.0, -9.0]
    if k in KINKED:
        return [0.0, TINY, -TINY]
    if k == "tanh":
        return [8.0, -8.0, 12.5 * math.log(2), 18.0, -18.0]      # 1 - t rounds to 1 from |u| = 12.5 ln 2
    if k == "sigmoid":
        return [8.0, -8.0, 18.0, -18.0, 25 * math.log(2), -88.0, -89.0]
    return []


def act_band(a, n=512):
    """The dense band of this kind, 512 points: where its derivative form is nearest to cancellation or to a change of branch."""
    k = a.kind
    lin = lambda lo, hi, m=n: torch.linspace(lo, hi, m, dtype=torch.float64)
    if k == "softplus":
        hi = a.thr / a.beta
        lo = (math.log(math.expm1(a.thr)) if a.thr > 0.05 else a.thr - 4.0) / a.beta
        return lin(lo - 0.5, hi + 0.25)
    if k == "mish":
        return lin(19.5, 20.5)
    if k == "gelu_tanh":
        return torch.cat((lin(8.5, 9.5, n // 2), lin(-9.5, -8.5, n // 2)))
    if k in KINKED:
        return lin(-0.01, 0.01)
    if k in ("tanh", "sigmoid"):
        return torch.cat((lin(8.0, 18.0, n // 2), lin(-18.0, -8.0, n // 2)))
    if k == "silu":
        return lin(8.0, 18.0)           # 1 - s by subtraction loses its last bits here
    return lin(-7.0, -3.0)              # gelu: 1 + erf cancels here


def act_probe_magnitudes(a):
    """probe_magnitudes() (both signs, the specials) + the dense band + the knees with two fp32 neighbours on either side, + -0.0 and the
    smallest denormals; fp32, fixed shuffled order."""
    extra = [act_band(a)] + [_ulps(c) for c in act_knees(a)] + [torch.tensor([2.0 ** -149, -2.0 ** -149, 1e-40, -1e-40, -0.0], dtype=torch.float64)]
    u = torch.cat([probe_magnitudes().double()] + extra).float()
    return u[torch.randperm(u.numel(), generator=torch.Generator().manual_seed(9))]


# ------------------------------------------------------------------------------------------------------------------ ATen in fp32
def aten32(a, p):
    """(act, act') of ATen's fp32 CPU kernels at fp32(p), as fp64."""
    x = _t64(p).float().requires_grad_(True)
    y = a.module()(x)
    g, = torch.autograd.grad(y.sum(), x)
    return y.detach().double(), g.double()


def _smooth_rel(err, ref, p, width=33):
    """Largest err / |ref| among the `width` probe values nearest (in order) to each p."""
    rel = (err / ref.abs().clamp_min(TINY)).reshape(-1)
    rel = torch.where(torch.isfinite(rel), rel, torch.zeros_like(rel))
    order = torch.argsort(p.reshape(-1))
    sm = F.max_pool1d(rel[order].view(1, 1, -1), width, 1, width // 2).view(-1)
    out = torch.empty_like(sm)
    out[order] = sm
    return out.view(ref.shape)


# ------------------------------------------------------------------------------------------------------------------ derived bounds, one layer
def _relexp(x):
    return (2 + 2 * x.abs()) * U


def _sig_parts(p):
    """s = rcp(1 + e), e = e^-p: (e, s, absolute error of e, relative error of s).  [exp | sum 1 | rcp 2]"""
    e = torch.exp((-p).clamp(max=700.0))
    de = e * _relexp(p)
    D = 1 + e
    return e, 1 / D, de, (de + U * D) / D + 2 * U


def _gelu_tanh_parts(p):
    """z = c (p + k p p p) [3 products, the constant k, the sum, the product with c and c itself: 4 U on the cubic term, 3 U on z];
    e = exp2(-2 log2e |z|) [the folded constant and the product: 4 |z| U; exp2 2; and 2 dz from z's own error]; r = rcp(1 + e).
    -> (z, e, r, d e, relative error of r)"""
    z = _gelu_tanh_z(p)
    dz = 4 * U * GELU_C * GELU_K * p.abs() ** 3 + 3 * U * z.abs()
    e = torch.exp(-2 * z.abs())
    de = e * ((2 + 4 * z.abs()) * U + 2 * dz)
    D = 1 + e
    return z, e, 1 / D, de, (de + U * D) / D + 2 * U


def _mish_err(p):
    """w = e^min(p, 20), n = w (w + 2) [sum 1, product 1], q = rcp(n + 2) [sum 1, rcp 2], T = n q [1]: d T = 2 d n / (n + 2)^2 + 4 U T.
    -> (w, n, T, d w, d n, d T, relative error of q)"""
    w, n, T = _mish_parts(p.clamp(max=20.0))
    dw = w * _relexp(p.clamp(max=20.0))
    dn = dw * (2 * w + 2) + 2 * U * n
    D = n + 2
    return w, n, T, dw, dn, 2 * dn / D ** 2 + 4 * U * T, (dn + U * D) / D + 2 * U


def _value_err(a, p, use_aten=True):
    """First-order bound of |form(p) - act64(p)| for the value form of psnode_act.h at an exact fp32 input p (fp64 tensor).
    -> (bound, ATen's smoothed relative error where the 3 x ATen rule was used, else None)"""
    k = a.kind
    r = act64(a, p)
    zero = torch.zeros_like(p)
    if k == "elu":          # max(x, 0) + alpha (med3(e^x, 0, 1) - 1): x > 0 exact.  t = e^x; t - 1 exact from t >= 0.5 (Sterbenz), else 1; alpha * 1
        t = torch.exp(p.clamp(max=0.0))
        return torch.where(p > 0, zero, a.alpha * t * _relexp(p) + (t < 0.5) * a.alpha * U * (1 - t) + U * r.abs()), None
    if k == "tanh":         # t = exp2(-2 log2e |x|): (2 + 4 |x|) U; N = 1 - t (exact from t >= 0.5), D = 1 + t [1], rcp [2], product [1]
        t = torch.exp(-2 * p.abs())
        dt = t * (2 + 4 * p.abs()) * U
        return 2 * dt / (1 + t) ** 2 + (t < 0.5) * U * (1 - t) / (1 + t) + 4 * U * r.abs(), None
    if k == "sigmoid":
        e, s, de, rs = _sig_parts(p)
        return s * rs + TINY, None
    if k == "relu":
        return zero, None
    if k == "leakyrelu":    # x > 0 ? x : x * s [1]
        return torch.where(p > 0, zero, U * r.abs() + TINY), None
    if k == "softplus":     # beta x > thr (or > 80): x itself; else log2(w) ln2 (t rcp(w - 1)) / beta, w = 1 + t, t = e^y
        # The operations around v_log_f32 are counted -- ln2 as a constant 1 and its product 1, rcp 2, the two products 2, the product with
        # 1 / beta 1, and t's own error, which moves log1p(t) by at most rel(t) t / ((1 + t) log1p(t)) <= rel(t) = (2 + 2 |y|) U relative
        # (w - 1 is exact or t itself; the rounding of w cancels between log(w) and w - 1, the point of the form): (9 + 2 |y|) U |ref|.
        # v_log_f32 itself is covered by the rule of traj_gates, 3 x ATen's own error there, + ELU_ABS.  (ATen returns u + log1p(e^-u),
        # which from u = 17 up is u to far below an ulp: its error alone would ask the log form for more than a rounding of the result.)
        y = a.beta * p
        exact = (y > a.thr) | (y > 80.0)
        v32, _ = aten32(a, p)
        sm = _smooth_rel((v32 - act64(a, p.float().double())).abs(), r, p)
        return torch.where(exact, zero, 3 * sm * r.abs() + ELU_ABS + (9 + 2 * y.abs().clamp(max=88.0)) * U * r.abs()), sm
    if k == "silu":         # u * rcp(1 + e^-u): s, product [1]
        e, s, de, rs = _sig_parts(p)
        return r.abs() * (rs + U) + TINY * (1 + p.abs()), None
    if k == "gelu":         # u * (0.5 * erfc(-u sqrt(1/2))): the argument [product 1, constant 1] moves erfc by |erfc'(a)| |a| 2 U, erfc itself
        arg = -p * math.sqrt(0.5)           # <= 16 ulp = 32 U (OpenCL), * 0.5 exact, product [1]
        derived = p.abs() * 0.5 * (2 / math.sqrt(math.pi)) * torch.exp(-arg * arg) * arg.abs() * 2 * U + 33 * U * r.abs() + TINY * (1 + p.abs())
        if not use_aten:
            return derived, None
        v32, _ = aten32(a, p)
        sm = _smooth_rel((v32 - act64(a, p.float().double())).abs(), r, p)
        return torch.minimum(derived, 3 * sm * r.abs() + ELU_ABS), sm
    if k == "gelu_tanh":    # u * (r * (z < 0 ? e : 1)): g = 1 / (1 + e) or e / (1 + e), d g = d e / (1 + e)^2 + g (3 | 4) U; product [1]
        z, e, rr, de, relr = _gelu_tanh_parts(p)
        g = torch.where(z < 0, e * rr, rr)
        return p.abs() * (de * rr * rr + 4 * U * g) + U * r.abs() + TINY * (1 + p.abs()), None
    assert k == "mish", k   # u * (u > 20 ? 1 : n q): T(20) = 1 - 2 e^-40
    w, n, T, dw, dn, dT, relq = _mish_err(p)
    return torch.where(p > 20.0, U * r.abs(), p.abs() * dT + U * r.abs()) + TINY * (1 + p.abs()), None


# rounding counts of `budget_bound`: the operations of each value form (see _value_err), hardware transcendentals counted twice
BUDGET_COUNT = {"elu": 6, "tanh": 5, "sigmoid": 5, "relu": 0, "leakyrelu": 1, "silu": 8, "gelu_tanh": 16, "mish": 12}


def budget_bound(a, u, n):
    """The promise of psnode_act.h / DESIGN.md "Activations": ELU_ABS per layer, chained with the Lipschitz constant, plus BUDGET_COUNT
    roundings x U x |ref| for the unbounded branches.  (ELU(alpha) scales its exponential by alpha: ELU_ABS x max(1, alpha).)  Plus the flush
    floor of the derived bounds."""
    ps = chain64(a, u, n)
    e = torch.zeros_like(ps[0])
    for p1 in ps[1:]:
        e = lipschitz(a) * e + ELU_ABS * max(1.0, a.alpha if a.kind == "elu" else 1.0) + BUDGET_COUNT[a.kind] * U * p1.abs() + TINY * (1 + p1.abs() + ps[0].abs())
    return e


def _softplus_jump(a, p, e):
    """A later layer's input within its error of the threshold may take the other branch: the forward jumps by log1p(e^thr) / beta - thr / beta
    there, the derivative by 1 - sigmoid(thr)."""
    near = (a.beta * p - a.thr).abs() <= a.beta * e
    return near * ((math.log1p(math.exp(-abs(a.thr))) + max(a.thr, 0.0) - a.thr) / a.beta), near * (1 - 1 / (1 + math.exp(-a.thr)))


def value_bound(a, u, n):
    """-> (bound of |out - act_n64(u)| after n layers, [ATen's smoothed relative error per layer] or [])"""
    ps = chain64(a, u, n)
    e = torch.zeros_like(ps[0])
    atens = []
    for k in range(n):
        b, sm = _value_err(a, ps[k])
        if sm is not None:
            atens.append(sm)
        e = lipschitz(a) * e + b
        if a.kind == "softplus" and k > 0:
            e = e + _softplus_jump(a, ps[k], e)[0]
    return e, atens


def _grad_err(a, p, e_u, e_h):
    """First-order bound of |form - act_grad64(p)| for the derivative form(s) K5 applies, at a layer whose input carries the error e_u and
    whose output h the error e_h.  -> (bound, ATen's smoothed relative error or None)"""
    k = a.kind
    d = act_grad64(a, p)
    h = act64(a, p)
    zero = torch.zeros_like(p)
    if k == "elu":          # h > 0 ? 1 : h + alpha [1]
        return torch.where(p > 0, zero, e_h + U * d.abs()), None
    if k == "tanh":         # 1 - h h [product 1, difference 1]
        return 2 * h.abs() * e_h + U * h * h + U * d, None
    if k == "sigmoid":      # h (1 - h) [difference 1, product 1]
        return (1 - 2 * h).abs() * e_h + 2 * U * d + TINY, None
    if k in ("relu", "leakyrelu"):
        return zero, None
    if k == "softplus":
        y = a.beta * p
        # from u (the pre build, and every build that keeps u): beta u > thr ? 1 : rcp(1 + e^-y); sigmoid' <= 1/4 on the input's error
        e, s, de, rs = _sig_parts(y)
        b = torch.where(y > a.thr, zero, s * rs + a.beta * 0.25 * e_u)
        if a.thr >= SOFTPLUS_CUT:   # from h (the act build): beta h > thr ? 1 : 1 - e^(-beta h) [exp | difference 1]; the two rules differ by e^-thr
            bh = (1 - d) * (a.beta * e_h + _relexp(a.beta * h)) + U * d + math.exp(-a.thr)
            b = torch.maximum(b, torch.where(y > a.thr + 1, zero, bh))
        return b + TINY, None
    cu = CURV[k] * e_u
    if k == "silu":         # s (1 + u oms), oms = u >= 0 ? e s [1] : 1 - s [1]; u oms [1], 1 + [1], s * [1]
        e, s, de, rs = _sig_parts(p)
        oms = 1 - s
        doms = torch.where(p >= 0, oms * (de / e.clamp_min(1e-300) + rs + U), s * rs + U * oms)
        X = p * torch.sigmoid(-p)
        dY = p.abs() * doms + U * X.abs() + U * (1 + X).abs()
        return d.abs() * (rs + U) + s * dY + cu + TINY * (1 + p.abs()), None
    if k == "gelu":         # 0.5 erfc(.) + u (c e^(-u u / 2)): 3 x ATen + ELU_ABS
        _, g32 = aten32(a, p)
        sm = _smooth_rel((g32 - act_grad64(a, p.float().double())).abs(), d, p)
        return 3 * sm * d.abs() + ELU_ABS + cu, sm
    if k == "gelu_tanh":    # g + (u (2 e r r)) (c (1 + 3 k u2)): B = u 2 e r r [3 products], C [u2 1, 3k u2 1 + constant 1, sum 1, c 1 + constant 1]
        z, e, rr, de, relr = _gelu_tanh_parts(p)
        g = torch.where(z < 0, e * rr, rr)
        BC = (d - g).abs()
        relB = de / e.clamp_min(1e-300) + 2 * relr + 3 * U
        C = GELU_C * (1 + 3 * GELU_K * p * p)        # (an e below 2^-126 is flushed, and B C = u 2 e r r C loses up to 2^-126 x 2 |u| C with it)
        return de * rr * rr + 4 * U * g + BC * (relB + 6 * U + U) + U * d.abs() + cu + TINY * (1 + 2 * p.abs() * C), None
    assert k == "mish", k   # u > 20 ? 1 : n q + u sech2 sg, sech2 = 4 (n + 1) q q [sum 1, 3 products], sg = w rcp(1 + w) [sum 1, rcp 2, product 1]
    w, n, T, dw, dn, dT, relq = _mish_err(p)
    rel_s2 = (dn + U * (n + 1)) / (n + 1) + 2 * relq + 3 * U
    sg = w / (1 + w)
    dsg = dw / (1 + w) ** 2 + 4 * U * sg
    X = (d - T).abs()
    return torch.where(p > 20.0, U + zero, dT + X * (rel_s2 + dsg / sg.clamp_min(1e-300) + 2 * U) + U * d.abs()) + cu + TINY * (1 + p.abs()), None


def grad_bound(a, u, n):
    """-> (bound of |got - act_grad_n64(u)|, [ATen's smoothed relative error per layer] or [])"""
    ps = chain64(a, u, n)
    ds = [act_grad64(a, p) for p in ps[:-1]]
    e = torch.zeros_like(ps[0])
    errs, atens = [], []
    for k in range(n):
        e_u = e
        b, _ = _value_err(a, ps[k])
        e = lipschitz(a) * e + b
        jump = torch.zeros_like(e)
        if a.kind == "softplus" and k > 0:
            jv, jump = _softplus_jump(a, ps[k], e_u)
            e = e + jv
        g, sm = _grad_err(a, ps[k], e_u, e)
        if sm is not None:
            atens.append(sm)
        errs.append(g + jump)
    total = torch.zeros_like(e)
    ref = torch.ones_like(e)
    for k in range(n):
        others = torch.ones_like(e)
        for j in range(n):
            if j != k:
                others = others * (ds[j].abs() + errs[j])
        total = total + errs[k] * others
        ref = ref * ds[k]
    return total + (n - 1) * U * ref.abs(), atens


# ------------------------------------------------------------------------------------------------------------------ gates
def _saturated(a, u):
    """Where the form's first layer is exactly -1 / +1 (Tanh: 1 - t and 1 + t round to 1 from |u| = 12.5 ln 2 = 8.67; taken from 10) or
    0 / 1 (Sigmoid: 1 + e^-u rounds to 1 from u = 25 ln 2 = 17.33, taken from 18; e^-u overflows from u = -88.73 down, taken from -89).
    -> [(mask, the first layer's exact value)]"""
    if a.kind == "tanh":
        return [(u >= 10.0, 1.0), (u <= -10.0, -1.0)]
    if a.kind == "sigmoid":
        return [(u >= 18.0, 1.0), (u <= -89.0, 0.0)]
    return []


def _largest(err, u):
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err).reshape(-1)
    k = int(err.argmax())
    return float(err[k]), float(u.reshape(-1)[k])


def value_gate(a, out, u, n, rel_slack=0.0):
    """|out - act_n64(u)| <= value_bound + rel_slack |ref|, every value finite, and the exactness clauses the forms guarantee:
      ReLU / LeakyReLU / ELU(alpha): u > 0 returns u bit for bit (the bound is 0 there);  Softplus: u itself from beta u > thr up (bound 0);
      Tanh / Sigmoid: the saturated first layer is exactly -1 / +1 / 0 / 1, so that all saturated u of one side share ONE output, which for
      n = 1 is that value.
    rel_slack: the stage weights' rounding of Midpoint / RK4 on a T = 2 probe (STAGE_SLACK), 0 for Euler.
    -> (ok, worst error [by error / bound], bound there, u there, ATen's smoothed relative error there or None,
        (largest absolute error, u there))"""
    out, u = _t64(out), _t64(u)
    ref = act_n64(a, u, n)
    bound, atens = value_bound(a, u, n)
    bound = bound + rel_slack * ref.abs()
    err = (out - ref).abs()
    ok, e, b, at = _worst(err, bound, u)
    ok = ok and bool(torch.isfinite(out).all())
    for mask, val in _saturated(a, u):
        if bool(mask.any()):
            sat = out[mask]
            ok = ok and float((sat - sat.reshape(-1)[0]).abs().max()) <= rel_slack * float(sat.abs().max())
            if n == 1 and rel_slack == 0.0:
                ok = ok and float((sat - val).abs().max()) == 0.0
    aten_at = None
    if atens:
        k = int((u.reshape(-1) == at).nonzero()[0]) if at == at else 0
        aten_at = float(max(s.reshape(-1)[k] for s in atens))
    return ok, e, b, at, aten_at, _largest(err, u)


def grad_gate(a, got, u, n, rel_slack=0.0):
    """|got - act_grad_n64(u)| <= grad_bound + rel_slack |ref|; every value finite.  The side of a kink (ELU(alpha), ReLU, LeakyReLU at 0)
    is torch's for every |u| >= 2^-126 and for u == 0; for a denormal u either one-sided derivative passes (the product along the chain
    from u, or from 0), and `side` says which the candidate returned: "own" (u's), "zero" (that of 0), "" (no denormal probe decides).
    -> (ok, worst error [by error / bound], bound there, u there, ATen's smoothed relative error there or None, side,
        (largest absolute error, u there))"""
    got, u = _t64(got), _t64(u)
    ref = act_grad_n64(a, u, n)
    bound, atens = grad_bound(a, u, n)
    bound = bound + rel_slack * ref.abs()
    err = (got - ref).abs()
    side = ""
    if a.kind in KINKED:
        den = (u != 0) & (u.abs() < TINY)
        if bool(den.any()):
            ref0 = act_grad_n64(a, torch.zeros_like(u), n)
            err0 = (got - ref0).abs()
            differ = den & ((ref - ref0).abs() > 0)
            if bool(differ.any()):
                own = bool((err[differ] <= err0[differ]).all())
                zer = bool((err0[differ] <= err[differ]).all())
                side = "own" if own else "zero" if zer else "mixed"
            err = torch.where(den, torch.minimum(err, err0), err)
    ok, e, b, at = _worst(err, bound, u)
    ok = ok and bool(torch.isfinite(got).all())
    aten_at = None
    if atens:
        k = int((u.reshape(-1) == at).nonzero()[0]) if at == at else 0
        aten_at = float(max(s.reshape(-1)[k] for s in atens))
    return ok, e, b, at, aten_at, side, _largest(err, u)


EXTREME_REL = 4 * U


def extremes_gate(a, out, got, u, n):
    """The extremes set (|u| from 1e19 to 3e38): outputs and gradients finite and within 4 x 2^-24 relative (+ 2^-126) of the fp64 limit.
    -> (ok, worst value error, worst gradient error)"""
    out, got, u = _t64(out), _t64(got), _t64(u)
    rv, rg = act_n64(a, u, n), act_grad_n64(a, u, n)
    ev, eg = (out - rv).abs(), (got - rg).abs()
    ok = bool(torch.isfinite(out).all()) and bool(torch.isfinite(got).all())
    ok = ok and bool((ev <= EXTREME_REL * rv.abs() + TINY).all()) and bool((eg <= EXTREME_REL * rg.abs() + TINY).all())
    return ok, float(ev.max()), float(eg.max())


# ------------------------------------------------------------------------------------------------------------------ wide-range trajectories
B_WIDE, T_WIDE = 70, 40
# A trajectory check of a kinked activation (ELU(alpha != 1), ReLU, LeakyReLU: act' jumps at 0; Softplus below the cut: act itself jumps at
# the threshold) is well posed only where no hidden pre-activation of the run lies within fp32 rounding of the kink: a branch taken the
# other way moves a gradient by far more than 2e-4 of its max, in ATen's fp32 walk as in any kernel (of the seeds 37 .. 43, ATen's walk
# flips at 37, 39, 40 and 41).  The seed is one at which ATen's fp32 walk itself passes both gates with a decade to spare
# (test_act_range_host.py: test_wide_case_is_well_posed_in_fp32).
WIDE_SEED = 43
DISCONTINUOUS = ("ELU(0.5)", "ELU(2.0)", "ReLU", "LeakyReLU(0.1)", "LeakyReLU(0.0)", "Softplus(2,5)", "Softplus(1,1)", "Softplus(1,0)")


@functools.lru_cache(maxsize=None)
def wide_act_case(seed=WIDE_SEED):
    """wide_ode_case(70, 40, 8, 2, 64) with three trajectories' z at +1e4 and two at -1e4 (every exponential of the forms overflows there)."""
    c = E.wide_ode_case(B_WIDE, T_WIDE, 8, 2, 64, seed=seed)
    c.z[:, 5:8] = 1e4
    c.z[:, 9:11] = -1e4
    c.a0 = torch.cat((c.x[0], c.z[0]), -1)
    return c


def close_gate(a, b, what, tol=2e-4):
    """`_close` of test_gpu_backward.py: 2e-4 of each tensor's max.  -> (ok, text, ratio)"""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    r = err / max(scale, 1e-6)
    return bool(torch.isfinite(a).all()) and err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs max {scale:.3e} ({r:.1e})", r


def ode_grads(c, method, a, G, dtype=torch.float64):
    """Autograd through the oracle's loop with the module as its activation, on leaves of `dtype` (fp64: the truth of the backward tests).
    -> (xs, [(name, gradient)]) in the order of ode_backward's outputs: x0, z, z_jump, all_initial, the parameters."""
    ls = [(w.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True)) for w, b in c.layers]
    req = lambda q: None if q is None else q.detach().to(dtype).clone().requires_grad_(True)
    x0, z, a0, zj = req(c.x[0]), req(c.z), req(c.a0), req(c.zj)
    with E.oracle_elu(a.module()):
        xs = E.ode_walk64(method, ls, c.t.to(dtype), x0, z, a0, None if c.ev is None else c.ev.to(dtype), zj)
    (xs * G.to(dtype)).sum().backward()
    named = [("grad x0", x0.grad), ("grad z", z.grad), ("grad z_jump", None if zj is None else zj.grad), ("grad all_initial", a0.grad)]
    return xs.detach(), named + [(f"grad param {k}", p.grad) for k, p in enumerate(q for wb in ls for q in wb)]


def ode_grads64(c, method, a, G):
    return ode_grads(c, method, a, G, torch.float64)


# ------------------------------------------------------------------------------------------------------------------ candidates and mutants
def torch_candidate(a):
    """ATen's fp32 kernels of the same module: u -> act(u), differentiable."""
    m = a.module()
    return lambda x: m(x)


def reference_candidate(a):
    """The fp32 stand-in for a correct kernel on the CPU: ATen's kernels of the same module, except where ATen's own form cancels and the
    kernels' (psnode_act.h) does not -- there ATen IS one of the mutants the gates have to reject, and the form of psnode_act.h is written
    out in fp32 torch instead:
      GELU         value   ATen u (1 + erf) / 2            here u erfc(-u / sqrt 2) / 2
      GELU(tanh)   value   ATen u (1 + tanh z) / 2         here u r (z < 0 ? e : 1), e = e^(-2|z|), r = 1 / (1 + e);  its derivative likewise
      SiLU         deriv.  ATen s (1 + u (1 - s))          here 1 - s = e^-u s for u >= 0
      Mish         deriv.  ATen through 1 - tanh^2         here 1 - T^2 = 4 (n + 1) / (n + 2)^2"""
    one = torch.ones_like
    if a.kind == "gelu":
        return form(lambda x: x * (0.5 * torch.erfc(-x * math.sqrt(0.5))), _g32(a))
    if a.kind == "gelu_tanh":
        def fwd(x):
            z = GELU_C * (x + GELU_K * x * x * x)
            e = torch.exp(-2 * z.abs())
            return x * ((1 / (1 + e)) * torch.where(z < 0, e, one(e)))
        return form(fwd, lambda x, h: _gelu_tanh_grad(x, clamp=True))
    if a.kind == "silu":
        def bwd(x, h):
            e = torch.exp(-x)
            s = 1 / (1 + e)
            return s * (1 + x * torch.where(x >= 0, e * s, 1 - s))
        return form(F.silu, bwd)
    if a.kind == "mish":
        def bwd(x, h):
            w = torch.exp(x.clamp(max=20.0))
            n = w * (w + 2)
            q = 1 / (n + 2)
            return torch.where(x > 20.0, one(x), n * q + x * (4 * (n + 1) * q * q) * (w / (1 + w)))
        return form(F.mish, bwd)
    return torch_candidate(a)


def form(fwd, bwd):
    """A candidate from a value form fwd(u) and a derivative form bwd(u, h): u -> act(u) with that derivative under autograd (fp32)."""
    class _Form(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            h = fwd(x)
            ctx.save_for_backward(x, h)
            return h

        @staticmethod
        def backward(ctx, g):
            x, h = ctx.saved_tensors
            return g * bwd(x, h)
    return _Form.apply


def candidate_run(cand, u, n):
    """(act^n(u), prod act') of a candidate in fp32: the host stand-in for a kernel on the identity probe."""
    x = torch.as_tensor(u, dtype=torch.float32).clone().requires_grad_(True)
    y = x
    for _ in range(n):
        y = cand(y)
    g, = torch.autograd.grad(y.sum(), x)
    return y.detach(), g


def _g32(a):
    """ATen's derivative as a bwd(u, h) form."""
    def bwd(x, h):
        with torch.enable_grad():
            xx = x.detach().requires_grad_(True)
            g, = torch.autograd.grad(a.module()(xx).sum(), xx)
        return g
    return bwd


def _f32(a):
    m = a.module()
    return lambda x: m(x)


def softplus_grad_from_output(a):
    """The rule of the act build: beta h > thr ? 1 : 1 - e^(-beta h).  Torch's to fp32 precision from thr = 24 ln 2 only."""
    return form(_f32(a), lambda x, h: torch.where(a.beta * h > a.thr, torch.ones_like(h), 1 - torch.exp(-a.beta * h)))


def _rel_branch(a, sel):
    return form(lambda x: torch.where(sel(x), _f32(a)(x) * (1 + 2e-6), _f32(a)(x)), _g32(a))


def _softplus_no_guard(a):
    def fwd(x):
        y = a.beta * x
        t = torch.exp(y)
        w = 1 + t
        return torch.where(y > a.thr, x, torch.log(w) * (t / (w - 1)) / a.beta)         # 0 / 0 where 1 + t rounds to 1
    return form(fwd, _g32(a))


def _mutants():
    A = ACTS
    one = torch.ones_like
    out = []
    for key in ("Softplus(2,5)", "Softplus(1,1)", "Softplus(1,0)"):
        out.append((f"{key}' decided on the output", key, softplus_grad_from_output(A[key])))
    sp, sp2 = A["Softplus(1,20)"], A["Softplus(2,5)"]
    out.append(("Softplus without the u == 1 guard of log1p", sp.key, _softplus_no_guard(sp)))
    out.append(("Softplus threshold compared on x instead of beta x", sp2.key,
                form(lambda x: torch.where(x > sp2.thr, x, torch.log1p(torch.exp(sp2.beta * x)) / sp2.beta), _g32(sp2))))
    out.append(("Softplus' threshold compared on x instead of beta x", sp2.key,
                form(_f32(sp2), lambda x, h: torch.where(x > sp2.thr, one(x), torch.sigmoid(sp2.beta * x)))))
    out.append(("tanh as 2 sigmoid(2x) - 1", "Tanh", form(lambda x: 2 * torch.sigmoid(2 * x) - 1, lambda x, h: 1 - h * h)))
    out.append(("sigmoid' as h (1 - h) with h clamped at 1 - 2^-12", "Sigmoid",
                form(torch.sigmoid, lambda x, h: h.clamp(max=1 - 2.0 ** -12) * (1 - h.clamp(max=1 - 2.0 ** -12)))))
    out.append(("SiLU' with 1 - s by subtraction on the positive side", "SiLU",
                form(F.silu, lambda x, h: torch.sigmoid(x) * (1 + x * (1 - torch.sigmoid(x))))))
    out.append(("GELU via 1 + erf", "GELU", form(lambda x: x * (0.5 * (1 + torch.erf(x * math.sqrt(0.5)))), _g32(A["GELU"]))))
    out.append(("Mish via tanh(log1p(e^u))", "Mish", form(lambda x: x * torch.tanh(torch.log1p(torch.exp(x))), _g32(A["Mish"]))))
    out.append(("GELU(tanh)' with u^2 unclamped (0 x inf beyond 1.8e19)", "GELU(tanh)",
                form(_f32(A["GELU(tanh)"]), lambda x, h: _gelu_tanh_grad(x, clamp=False))))
    for key in ("LeakyReLU(0.1)", "LeakyReLU(0.0)"):
        s = A[key].alpha
        out.append((f"{key} slope applied at u >= 0 only from below: derivative 1 at u == 0", key,
                    form(_f32(A[key]), lambda x, h, s=s: torch.where(x >= 0, one(x), s * one(x)))))
    out.append(("ReLU' = 1 at u == 0", "ReLU", form(F.relu, lambda x, h: (x >= 0).float())))
    for key in ("ELU(0.5)", "ELU(2.0)"):
        al = A[key].alpha
        out.append((f"{key}' = h + 1 (alpha forgotten)", key, form(_f32(A[key]), lambda x, h: torch.where(h > 0, one(h), h + 1))))
        out.append((f"{key}' = alpha e^u from u >= 0 down: alpha at u == 0 is right, 1 at u > 0 lost below 1e-3", key,
                    form(_f32(A[key]), lambda x, h, al=al: torch.where(x > 1e-3, one(x), al * torch.exp(x.clamp(max=0.0))))))
    branch = {"elu": lambda x: x < -0.5, "tanh": lambda x: x > 0.5, "sigmoid": lambda x: x > 0.5, "relu": lambda x: x > 0.5,
              "leakyrelu": lambda x: x > 0.5, "softplus": lambda x: (x > -1.0) & (x < -0.25), "silu": lambda x: x > 0.5, "gelu": lambda x: x > 0.5,
              "gelu_tanh": lambda x: x > 0.5, "mish": lambda x: x > 0.5}
    for key, a in A.items():
        out.append((f"{key}: relative 2e-6 on one branch", key, _rel_branch(a, branch[a.kind])))
    return out


def _gelu_tanh_grad(x, clamp):
    u2 = (x * x).clamp(max=1e4) if clamp else x * x
    z = GELU_C * (x + GELU_K * u2 * x)
    e = torch.exp(-2 * z.abs())
    r = 1 / (1 + e)
    return r * torch.where(z < 0, e, torch.ones_like(e)) + (x * (2 * e * r * r)) * (GELU_C * (1 + 3 * GELU_K * u2))


ACT_MUTANTS = _mutants()        # [(name, key of ACTS, candidate)]
