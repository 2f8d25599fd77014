"""Cases, references and gates for the ELU range tests (test_elu_range_host.py on the CPU, test_gpu_elu_range.py on the GPU).

The suite's other inputs (0.1 randn states, default nn.Linear initialisation) keep every hidden pre-activation inside about [-0.4, +0.4],
where ELU is almost the identity and ELU' almost 1.  This module builds inputs that reach the whole activation range:

  wide_ode_case / wide_dae_case    whole trajectories whose hidden pre-activations spread from below -17 to above +5 in every hidden layer;
  identity_probe_ode / _dae        weights of zeros and ones and a clock with dt = 1, so that each grid point of the result IS ELU^n(u) of
                                   a chosen u (n = number of hidden layers): products with 1.0 and sums with 0.0 are exact;
  random_probe_ode / _dae          the same one-evaluation construction with the wide recipe's random weights.

References are fp64 evaluations of the same algorithm (the oracle run on float64 tensors, or the closed form ELU^n).  The gates are plain
functions that return their figures, so that the host file can apply them to the fp32 oracle (which must pass every one) and to mutants of
the oracle's ELU (each of which at least one gate must reject) before the GPU file applies them to the HIP kernels.
"""
import contextlib
import math
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import TOL_GPU, traj_rel_err
from oracle import psnode_oracle as O

ELU_ABS = 1.2e-7            # the inline ELU's contract: absolute error vs fp64 expm1 (test_inline_elu_accuracy_contract, DESIGN.md "ELU")
EPS32 = 2.0 ** -23
PROBE_TOL = 2e-6            # one-evaluation tolerance of the row-kernel tests (test_gpu_parity.py: test_row_mlp_kernel*)
# Midpoint / RK4 on a T = 2 probe: f does not depend on x, every stage returns the same k, and x1 = dt * sum(b_s k).  The update
# (k + 3 (k + k) + k) * dt * 0.125 rounds at most four times (3 * 2k, two sums, and a kernel's fused forms no more): 4 * 2^-24 relative;
# doubled for kernels that weight the stages in another order.
STAGE_SLACK = 8 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ weights and cases
def _hidden_list(H, n_hidden):
    return list(H) if isinstance(H, (tuple, list)) else [H] * n_hidden


def _linears(dims, seed):
    torch.manual_seed(seed)
    return [nn.Linear(dims[k], dims[k + 1]) for k in range(len(dims) - 1)]


def wide_mlp(dims, seed, gain, bias_amp):
    """Default nn.Linear initialisation; every hidden layer's weight x gain, its bias + bias_amp * randn; the output layer untouched."""
    g = torch.Generator().manual_seed(seed + 7919)
    out = []
    lin = _linears(dims, seed)
    for k, l in enumerate(lin):
        w, b = l.weight.detach().clone(), l.bias.detach().clone()
        if k + 1 < len(lin):
            w = w * gain
            b = b + bias_amp * torch.randn(b.shape, generator=g)
        out.append((w, b))
    return out


def _amps(B, amp_hi):
    """Per-trajectory amplitude of the external inputs, log-spaced 0.1 .. amp_hi over the batch: the low-amplitude trajectories keep a
    small error scale while some of their units already saturate."""
    return torch.logspace(math.log10(0.1), math.log10(amp_hi), B).view(1, B, 1) if B > 1 else torch.full((1, 1, 1), amp_hi)


def _clock(Tn, B, dt):
    return (torch.arange(Tn, dtype=torch.float32) * dt).view(Tn, 1, 1).repeat(1, B, 1)


def wide_ode_case(B, Tn, xd, zd, H, seed, gain=3.0, bias_amp=1.0, amp_hi=30.0, n_hidden=3, events=True):
    """-> namespace(layers, t, x, z, a0, ev, zj).  Uniform clock, dt 0.01; two events (grid points 2 and Tn - 3) when z exists."""
    g = torch.Generator().manual_seed(seed)
    layers = wide_mlp([3 * (xd + zd)] + _hidden_list(H, n_hidden) + [xd], seed, gain, bias_amp)
    amp = _amps(B, amp_hi)
    t = _clock(Tn, B, 0.01)
    x = torch.zeros(Tn, B, xd)
    x[0] = 0.1 * torch.randn(B, xd, generator=g)
    z = amp * torch.randn(Tn, B, zd, generator=g)
    a0 = torch.cat((x[0], z[0]), -1)
    ev = zj = None
    if events and zd and Tn > 6:
        ev = torch.stack([t[2, :, :], t[Tn - 3, :, :]], dim=1).contiguous()
        zj = amp.view(B, 1, 1) * torch.randn(B, 2, zd, generator=g)
    return types.SimpleNamespace(layers=layers, t=t, x=x, z=z, a0=a0, ev=ev, zj=zj, xd=xd, zd=zd)


def wide_dae_case(B, Tn, xd, zd, vd, idim, H, seed, gain=3.0, bias_amp=1.0, amp_hi=30.0, n_hidden=3, events=True):
    """The DAE twin: DE and AE both widened.  -> namespace(de, ae, t, x, z, v, i, xi, a0, ev, zj, vj)."""
    g = torch.Generator().manual_seed(seed)
    n = xd + zd + vd + idim
    hid = _hidden_list(H, n_hidden)
    de = wide_mlp([3 * n] + hid + [xd], seed, gain, bias_amp)
    ae = wide_mlp([n + xd + zd + vd] + hid + [idim], seed + 1, gain, bias_amp)
    amp = _amps(B, amp_hi)
    t = _clock(Tn, B, 0.01)
    r = lambda *s: torch.randn(*s, generator=g)
    xi = 0.1 * r(B, xd)
    x = torch.zeros(Tn, B, xd)
    x[0] = xi
    z, v, i = amp * r(Tn, B, zd), amp * r(Tn, B, vd), amp * r(Tn, B, idim)
    a0 = torch.cat((xi, z[0], v[0], i[0]), -1)
    ev = zj = vj = None
    if events and Tn > 6:
        ev = torch.stack([t[2, :, :], t[Tn - 3, :, :]], dim=1).contiguous()
        zj, vj = amp.view(B, 1, 1) * r(B, 2, zd), amp.view(B, 1, 1) * r(B, 2, vd)
    return types.SimpleNamespace(de=de, ae=ae, t=t, x=x, z=z, v=v, i=i, xi=xi, a0=a0, ev=ev, zj=zj, vj=vj, xd=xd, zd=zd, vd=vd, idim=idim)


def to64(ls):
    return [(w.double(), b.double()) for w, b in ls]


def _d(a):
    return None if a is None else a.double()


def run_ode(c, method, dtype=torch.float32, layers=None):
    """The oracle on a wide_ode_case in fp32 or (the same code on float64 tensors) fp64."""
    ls = c.layers if layers is None else layers
    if dtype == torch.float64:
        return O.integrate_ode(method, to64(ls), _d(c.t), _d(c.x), _d(c.z), _d(c.a0), _d(c.ev), _d(c.zj))
    return O.integrate_ode(method, ls, c.t, c.x, c.z, c.a0, c.ev, c.zj)


def run_dae(c, method, dtype=torch.float32):
    if dtype == torch.float64:
        return O.integrate_dae(method, to64(c.de), to64(c.ae), _d(c.xi), _d(c.t), _d(c.x), _d(c.z), _d(c.v), _d(c.i), _d(c.a0), _d(c.ev),
                               _d(c.zj), _d(c.vj))
    return O.integrate_dae(method, c.de, c.ae, c.xi, c.t, c.x, c.z, c.v, c.i, c.a0, c.ev, c.zj, c.vj)


def _hidden_pre(layers, inp):
    pre = []
    u = inp
    for w, b in layers[:-1]:
        u = F.linear(u, w, b)
        pre.append(u)
        u = F.elu(u)
    return pre


def _held(c, ext, jump, j):
    """External input of step j -> j + 1 (zero-order hold of row j, replaced by the event's jump when the clock hits one)."""
    e0 = ext[j]
    if c.ev is not None and jump is not None and O._event_hit(c.ev, c.t[j]):
        e0 = O._jump(c.ev, jump, c.t[j], e0)
    return e0


def preactivation_stats(c, method="rk4"):
    """Hidden pre-activations of the first stage of every step along the fp32 oracle's solution of a wide case.
    -> (per hidden layer: 1-D tensor of all pre-activations of the DE [followed by the AE's for a DAE case], max |x| of the run)."""
    dae = hasattr(c, "de")
    if not dae:
        xs = run_ode(c, method)
        pre = [[] for _ in c.layers[:-1]]
        for j in range(c.t.shape[0] - 1):
            s = torch.cat((xs[j], _held(c, c.z, c.zj, j)), -1)
            for k, p in enumerate(_hidden_pre(c.layers, torch.cat((c.a0, s - c.a0, s), -1))):
                pre[k].append(p.reshape(-1))
        return [torch.cat(p) for p in pre], float(xs.abs().max())
    xs, is_ = run_dae(c, method)
    pre = [[] for _ in c.de[:-1]] + [[] for _ in c.ae[:-1]]
    nde = len(c.de) - 1
    for j in range(c.t.shape[0] - 1):
        s = torch.cat((xs[j], _held(c, c.z, c.zj, j), _held(c, c.v, c.vj, j), is_[j]), -1)
        for k, p in enumerate(_hidden_pre(c.de, torch.cat((c.a0, s - c.a0, s), -1))):
            pre[k].append(p.reshape(-1))
        for k, p in enumerate(_hidden_pre(c.ae, torch.cat((c.a0, xs[j + 1], c.z[j + 1], c.v[j + 1]), -1))):
            pre[nde + k].append(p.reshape(-1))
    return [torch.cat(p) for p in pre], float(xs.abs().max())


COVERAGE = ((lambda p: p < -0.25, 0.30, "< -0.25"), (lambda p: p < -5.0, 0.05, "< -5"), (lambda p: p < -17.0, 0.01, "< -17"),
            (lambda p: p > 5.0, 0.05, "> +5"))


def coverage_shares(pre):
    """Share of one layer's pre-activations in each band of COVERAGE."""
    return [float(sel(pre).float().mean()) for sel, _, _ in COVERAGE]


# ------------------------------------------------------------------------------------------------------------------ probes
def probe_magnitudes(n_log=4096, n_band=512):
    """The magnitude set of test_inline_elu_accuracy_contract (logspace 1e-38 .. 1e2, the dense band 0.2 .. 0.3 around the polynomial
    form's knee, the specials), both signs, as fp32 values in a fixed shuffled order."""
    mags = torch.cat((torch.logspace(-38, 2, n_log, dtype=torch.float64), torch.linspace(0.2, 0.3, n_band, dtype=torch.float64),
                      torch.tensor([0.25, 0.2500001, 0.2499999, 17.0, 88.0, 104.0, 1e4, 0.0], dtype=torch.float64)))
    u = torch.cat((-mags, mags)).float()
    return u[torch.randperm(u.numel(), generator=torch.Generator().manual_seed(5))]


def _fill(shape, u, need_all=True):
    """A tensor of `shape` filled with u repeated cyclically (need_all: it must hold every value of u at least once)."""
    n = 1
    for s in shape:
        n *= s
    assert n >= u.numel() or not need_all, (shape, u.numel())
    return u.repeat((n + u.numel() - 1) // u.numel())[:n].view(*shape).clone()


def _select(rows, cols, col0, ncol):
    """W[rows, cols] with W[k, col0 + k % ncol] = 1: unit k reads column k % ncol of the block that starts at col0."""
    w = torch.zeros(rows, cols)
    for k in range(rows):
        w[k, col0 + k % ncol] = 1.0
    return w


def _identity_mlp(in_dim, col0, ncol, hidden, out_dim):
    """First layer: unit k reads input column col0 + k % ncol; hidden layers: identity on the common units; last: output d = unit d.
    All biases 0.  Every output d < m reads ELU^n(input column col0 + d % ncol), m = the narrowest width."""
    dims = [in_dim] + list(hidden) + [out_dim]
    ls = [(_select(dims[1], in_dim, col0, ncol), torch.zeros(dims[1]))]
    for k in range(1, len(dims) - 1):
        w = torch.zeros(dims[k + 1], dims[k])
        m = min(dims[k], dims[k + 1])
        w[:m, :m] = torch.eye(m)
        ls.append((w, torch.zeros(dims[k + 1])))
    return ls


def _probe_grid(B, n_read, u, teacher):
    """Grid length so that [Tn - 1, B, n_read] holds every probe value once (teacher forcing: one evaluation per step), or 2."""
    return (u.numel() + B * n_read - 1) // (B * n_read) + 1 if teacher else 2


def identity_probe_ode(xd, zd, H, B=70, n_hidden=3, teacher=True, u=None):
    """ODE identity probe.  Teacher-forced over a dataset x == 0 with the clock t = 0, 1, 2, ...: xs[j] = 0 + 1 * f(z[j-1]), and
    f = ELU^n of the z columns.  teacher=False: T = 2 from x[0] = 0 (one step; B is raised so that one step holds every probe value).
    -> namespace(layers, t, x, z, a0, teacher, u_of): u_of[j, b, d] = the u that xs[j + 1, b, d] evaluates."""
    u = probe_magnitudes() if u is None else u
    hid = _hidden_list(H, n_hidden)
    assert zd >= 1 and min(hid) >= xd
    n_read = min(xd, zd)
    if not teacher:
        B = max(B, (u.numel() + n_read - 1) // n_read)
    Tn = _probe_grid(B, n_read, u, teacher)
    n = xd + zd
    layers = _identity_mlp(3 * n, 2 * n + xd, zd, hid, xd)
    z = torch.zeros(Tn, B, zd)
    z[:Tn - 1, :, :n_read] = _fill((Tn - 1, B, n_read), u)
    if zd > n_read:
        z[:Tn - 1, :, n_read:] = _fill((Tn - 1, B, zd - n_read), u.flip(0), need_all=False)
    z[Tn - 1] = z[0]
    x = torch.zeros(Tn, B, xd)
    a0 = torch.cat((x[0], z[0]), -1)
    u_of = z[:Tn - 1][..., [d % zd for d in range(xd)]]
    return types.SimpleNamespace(layers=layers, t=_clock(Tn, B, 1.0), x=x, z=z, a0=a0, ev=None, zj=None, teacher=teacher, u_of=u_of,
                                 n=len(hid), xd=xd, zd=zd)


def identity_carry_probe_ode(xd, zd, H, Tn=8, row=3, n_hidden=3, u=None):
    """Multi-step identity probe WITHOUT teacher forcing: z is non-zero at the one interior grid row `row`, zero elsewhere, x[0] = 0.
    f does not depend on x and f(0) = 0 (all biases 0, ELU(0) = 0), so xs[1 .. row] = 0 exactly, xs[row + 1] = 0 + 1 * ELU^n(u), and the
    later steps add exact zeros: xs[row + 1 ..] all carry ELU^n(u).  The probed evaluation sits inside the time loop's steady-state body
    (K1x's prefetching FAST loop, the ring steps of its saving forward), not in a first or peeled last step.
    -> namespace(..., row, u_of [B, xd])"""
    c = identity_probe_ode(xd, zd, H, n_hidden=n_hidden, teacher=False, u=u)
    B = c.t.shape[1]
    assert 1 <= row < Tn - 2
    z = torch.zeros(Tn, B, zd)
    z[row] = c.z[0]
    x = torch.zeros(Tn, B, xd)
    return types.SimpleNamespace(layers=c.layers, t=_clock(Tn, B, 1.0), x=x, z=z, a0=torch.zeros(B, xd + zd), ev=None, zj=None, teacher=False,
                                 u_of=c.u_of[0], row=row, n=c.n, xd=xd, zd=zd)


def identity_probe_dae(xd, zd, vd, idim, H, B=70, n_hidden=3, teacher=True, u=None):
    """DAE identity probe: the DE reads the (z, v) columns of its s block (xs[j] = ELU^n(e[j-1]), e = cat(z, v)), the AE head the (z, v)
    columns of its tail (is[j] = ELU^n(e[j]), no clock involved).  -> namespace(..., u_x [T-1,B,xd], u_i [T,B,idim])."""
    u = probe_magnitudes() if u is None else u
    hid = _hidden_list(H, n_hidden)
    ne = zd + vd
    assert ne >= 1 and min(hid) >= max(xd, idim)
    n_read = min(max(xd, idim), ne)
    if not teacher:
        B = max(B, (u.numel() + n_read - 1) // n_read)
    Tn = _probe_grid(B, n_read, u, teacher)
    n = xd + ne + idim
    de = _identity_mlp(3 * n, 2 * n + xd, ne, hid, xd)
    ae = _identity_mlp(n + xd + ne, n + xd, ne, hid, idim)
    e = torch.zeros(Tn, B, ne)
    e[:Tn - 1, :, :n_read] = _fill((Tn - 1, B, n_read), u)
    if ne > n_read:
        e[:Tn - 1, :, n_read:] = _fill((Tn - 1, B, ne - n_read), u.flip(0), need_all=False)
    e[Tn - 1] = e[0]
    z, v = e[..., :zd].contiguous(), e[..., zd:].contiguous()
    x, i, xi = torch.zeros(Tn, B, xd), torch.zeros(Tn, B, idim), torch.zeros(B, xd)
    a0 = torch.cat((xi, z[0], v[0], i[0]), -1)
    u_x = e[:Tn - 1][..., [d % ne for d in range(xd)]]
    u_i = e[..., [d % ne for d in range(idim)]]
    return types.SimpleNamespace(de=de, ae=ae, t=_clock(Tn, B, 1.0), x=x, z=z, v=v, i=i, xi=xi, a0=a0, ev=None, zj=None, vj=None,
                                 teacher=teacher, u_x=u_x, u_i=u_i, n=len(hid), xd=xd, zd=zd, vd=vd, idim=idim)


def random_probe_ode(B, Tn, xd, zd, H, seed, n_hidden=3, teacher=True, **kw):
    """One visible MLP evaluation per grid point (dataset x == 0, dt = 1, teacher forcing; or T = 2 from x[0] = 0) with the wide recipe's
    random weights: zero padding, split-K folds and every unit take part.  The reference is `probe_ref_ode`."""
    c = wide_ode_case(B, Tn if teacher else 2, xd, zd, H, seed, n_hidden=n_hidden, events=False, **kw)
    c.x = torch.zeros_like(c.x)
    c.t = _clock(c.t.shape[0], B, 1.0)
    c.a0 = torch.cat((c.x[0], c.z[0]), -1)
    c.teacher = teacher
    return c


def random_probe_dae(B, Tn, xd, zd, vd, idim, H, seed, n_hidden=3, teacher=True, **kw):
    c = wide_dae_case(B, Tn if teacher else 2, xd, zd, vd, idim, H, seed, n_hidden=n_hidden, events=False, **kw)
    c.x, c.xi = torch.zeros_like(c.x), torch.zeros_like(c.xi)
    c.t = _clock(c.t.shape[0], B, 1.0)
    c.a0 = torch.cat((c.xi, c.z[0], c.v[0], c.i[0]), -1)
    c.teacher = teacher
    return c


def probe_run_ode(c, method="euler", dtype=torch.float32):
    """A probe case on the oracle (fp32, or fp64 = the reference of the random probes)."""
    k = (lambda a: _d(a)) if dtype == torch.float64 else (lambda a: a)
    ls = to64(c.layers) if dtype == torch.float64 else c.layers
    return O.integrate_ode(method, ls, k(c.t), k(c.x), k(c.z), k(c.a0), input_true_x=c.teacher)


def probe_run_dae(c, method="euler", dtype=torch.float32):
    """Teacher forcing of a DAE probe: x AND i from the dataset (i == 0), so that the DE's input does not carry the head's output."""
    k = (lambda a: _d(a)) if dtype == torch.float64 else (lambda a: a)
    de, ae = (to64(c.de), to64(c.ae)) if dtype == torch.float64 else (c.de, c.ae)
    return O.integrate_dae(method, de, ae, k(c.xi), k(c.t), k(c.x), k(c.z), k(c.v), k(c.i), k(c.a0), input_true_x=c.teacher,
                           input_true_i=c.teacher)


def elu_n64(u, n):
    """ELU^n(u) in fp64: the closed-form reference of the identity probes."""
    y = torch.as_tensor(u, dtype=torch.float64)
    for _ in range(n):
        y = torch.where(y > 0, y, torch.expm1(y))
    return y


# ------------------------------------------------------------------------------------------------------------------ gates
def traj_gates(cand, oracle32, truth64, factor=3):
    """The two trajectory gates of the wide-range tests.
      e32 = traj_rel_err(cand, oracle fp32) <= TOL_GPU                       (the project's gate)
      e64 = traj_rel_err(cand, fp64 truth)  <= factor * eo + 1e-7, eo = traj_rel_err(oracle fp32, fp64 truth)
    (the rule of test_accuracy_equivalent_to_reference_vs_fp64: no further from the truth than the reference's own fp32 noise allows).
    -> (ok, e32, e64, eo)"""
    assert bool(torch.isfinite(torch.as_tensor(truth64)).all()), "the fp64 reference must be finite"
    e32, e64, eo = traj_rel_err(cand, oracle32), traj_rel_err(cand, truth64), traj_rel_err(oracle32, truth64)
    ok = bool(torch.isfinite(torch.as_tensor(cand)).all()) and e32 <= TOL_GPU and e64 <= factor * eo + 1e-7
    return ok, e32, e64, eo


def _worst(err, bound, u):
    """(all within bound, worst error, bound there, u there): worst = the largest error / bound ratio (or error where the bound is 0)."""
    err, bound, u = err.reshape(-1), bound.reshape(-1), torch.as_tensor(u, dtype=torch.float64).reshape(-1)
    if err.numel() == 0:
        return True, 0.0, 0.0, float("nan")
    bad = ~(err <= bound)                   # NaN counts as bad
    k = int(torch.where(bad, torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300)).argmax()) if bool(bad.any()) \
        else int((err / bound.clamp_min(1e-300)).argmax())
    return not bool(bad.any()), float(err[k]), float(bound[k]), float(u[k])


worst = _worst


def elu_grad_bound(n):
    """The kernels form ELU' = med3(h, -2, 0) + 1 from the stored (or recomputed) activation h.  Layer k's h carries the absolute error of
    k chained ELUs (each <= 1.2e-7 and 1-Lipschitz: k * 1.2e-7) and the sum h + 1 <= 1 rounds once (2^-24).  The product of n factors in
    [0, 1] moves by at most the sum of the factors' errors, plus one rounding (2^-24) per multiplication; the weight path of the probe
    (transposed zeros-and-ones matrices, dt = 1) is exact.  n = 3: 6 * 1.2e-7 + 5 * 2^-24 = 1.02e-6 (below the first estimate
    3 * 1.2e-7 * 4 = 1.44e-6)."""
    return ELU_ABS * n * (n + 1) / 2 + (2 * n - 1) * 2.0 ** -24


def elu_grad_gate(got, u, n, rel_slack=0.0, exact_zero=True):
    """Gate of the ELU' probes: got = dL/du through n chained ELUs with a one-hot output gradient, i.e. prod_k ELU'(p_k) along
    u -> ELU(u) -> ...  Exactly 1 for u >= 0 (torch's rule: ELU'(0) = 1), exactly 0 from -88 down (fp64 e^u is 1e-39 there, not 0: the
    exact value is asserted on its own), within `elu_grad_bound` of the fp64 product between.
    exact_zero=False: for a candidate that forms ELU' as e^u (ATen's autograd: 6e-39 at -88) instead of h + 1; then |got| <= 1e-38 there.
    -> (ok, worst error, bound there, u there)"""
    got, u = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(u, dtype=torch.float64)
    ref, h = torch.ones_like(u), u
    for _ in range(n):
        ref = ref * torch.where(h > 0, torch.ones_like(h), torch.exp(h))
        h = elu_n64(h, 1)
    bound = torch.where(u >= 0, torch.zeros_like(u), torch.full_like(u, elu_grad_bound(n))) + rel_slack * ref
    ok, err, b, at = _worst((got - ref).abs(), bound, u)
    deep = u <= -88.0
    if bool(deep.any()):
        ok = ok and float(got[deep].abs().max()) <= (0.0 if exact_zero else 1e-38)
    return ok, err, b, at


def identity_gate_plain(out, u, n, rel_slack=0.0):
    """The contract of test_inline_elu_accuracy_contract applied n times (plain-domain kernels: products with 1.0 and sums with 0.0 are
    exact, so out IS the kernel's ELU^n(u)):
      u > 0: exactly u;   u == 0: exactly 0;   u <= 0: |out - ELU^n_fp64(u)| <= n * 1.2e-7 (each ELU is 1-Lipschitz, so the n errors
      add), out in [-1, 0];   u <= -88: exactly -1 at the first ELU, i.e. exactly ELU^(n-1)(-1) -- asserted as: equal for every u <= -88.
    rel_slack: relative allowance for the stage weights' rounding of Midpoint / RK4 on the T = 2 probes (0 for Euler).
    -> (ok, worst error, bound there, u there)"""
    out = torch.as_tensor(out, dtype=torch.float64)
    u = torch.as_tensor(u, dtype=torch.float64)
    ref = elu_n64(u, n)
    err = (out - ref).abs()
    bound = torch.where(u > 0, torch.zeros_like(u), torch.full_like(u, n * ELU_ABS)) + rel_slack * ref.abs()
    bound = torch.where(u == 0, torch.zeros_like(u), bound)
    ok, e, b, at = _worst(err, bound, u)
    neg = u < 0
    if bool(neg.any()):
        ok = ok and float(out[neg].max()) <= 0.0 and float(out[neg].min()) >= -1.0 * (1 + rel_slack)
    deep = u <= -88.0
    if bool(deep.any()):
        ok = ok and float((out[deep] - out[deep][0]).abs().max()) == 0.0        # saturated: one value, whatever u
        if n == 1 and rel_slack == 0.0:
            ok = ok and float((out[deep] + 1.0).abs().max()) == 0.0
    return ok, e, b, at


def scaled_bound(u, n):
    """Bound of the scaled-domain (inference) instances on the identity probe: the first layer's ones are stored as fp32(log2e), the last
    layer's as fp32(1 / log2e) (two rounded weights), and the two products with them round (two rounded products): 4 * 2^-23 relative
    to ELU^n(u), on top of the n absolute ELU errors."""
    ref = elu_n64(u, n)
    return n * ELU_ABS + 4 * EPS32 * ref.abs()


def identity_gate_scaled(out, u, n, rel_slack=0.0):
    """-> (ok, worst error, bound there, u there); every value finite (no inf from exp2 before the clamp, no NaN from 0 * inf)."""
    out = torch.as_tensor(out, dtype=torch.float64)
    u = torch.as_tensor(u, dtype=torch.float64)
    ref = elu_n64(u, n)
    ok, e, b, at = _worst((out - ref).abs(), scaled_bound(u, n) + rel_slack * ref.abs(), u)
    return ok and bool(torch.isfinite(out).all()), e, b, at


def random_probe_gate(out, ref64, bdim=1):
    """Per trajectory: max_{t,d} |out - ref64| <= 2e-6 * max(1, max_{t,d} |ref64|).  -> (ok, worst ratio error / scale, trajectory)"""
    out, ref = torch.as_tensor(out, dtype=torch.float64), torch.as_tensor(ref64, dtype=torch.float64)
    other = [k for k in range(ref.dim()) if k != bdim]
    err = (out - ref).abs().amax(other)
    scale = ref.abs().amax(other).clamp_min(1.0)
    ratio = err / scale
    ok = bool(torch.isfinite(out).all()) and bool((ratio <= PROBE_TOL).all())
    return ok, float(ratio.max()), int(ratio.argmax())


# ------------------------------------------------------------------------------------------------------------------ mutants
def _elu(u):
    return F.elu(u)


ELU_MUTANTS = {
    # saturates early: -1 below -9 (absolute error up to e^-9 = 1.2e-4)
    "saturate_at_-9": lambda u: torch.where(u < -9, torch.full_like(u, -1.0), _elu(u)),
    # loses accuracy on the deep-negative branch: e^u (1 + 2e-5) - 1 below -2
    "deep_branch_2e-5": lambda u: torch.where(u < -2, torch.exp(u) * (1 + 2e-5) - 1, _elu(u)),
    # clamps large positives
    "clamp_at_32": lambda u: _elu(u.clamp(max=32.0)),
    "clamp_at_88": lambda u: _elu(u.clamp(max=88.0)),
    # flushes the shallow negative side
    "zero_above_-1e-3": lambda u: torch.where((u > -1e-3) & (u < 0), torch.zeros_like(u), _elu(u)),
    # relative error 2e-6 on the whole negative branch
    "negative_rel_2e-6": lambda u: torch.where(u < 0, _elu(u) * (1 + 2e-6), _elu(u)),
}


@contextlib.contextmanager
def oracle_elu(fn):
    """Run the oracle with its ELU replaced (the oracle module's `F` is swapped for a two-function stand-in; torch itself is untouched)."""
    saved = O.F
    O.F = types.SimpleNamespace(linear=F.linear, elu=fn)
    try:
        yield
    finally:
        O.F = saved


# ------------------------------------------------------------------------------------------------------------------ fp64 autograd walks
def ode_walk64(method, layers, t, x0, z, a0, ev=None, zj=None):
    """The oracle's ODE loop under autograd on fp64 LEAVES (layers' tensors, x0, z, a0, zj): the truth of the backward tests.  all_initial
    is a leaf of its own, so each returned gradient of the kernels has its own counterpart."""
    xs = [x0]
    xc = x0
    for j in range(1, t.shape[0]):
        t0, z0 = t[j - 1], z[j - 1]
        if ev is not None and zj is not None and O._event_hit(ev, t0):
            sel = (ev[0] == t0[0][0]).view(-1)
            z0 = zj[:, sel].view(z0.shape)
        xc, _ = O.step(method, lambda xx: O.de_rhs(layers, xx, (z0,), a0), t0, t[j] - t0, t[j], xc)
        xs.append(xc)
    return torch.stack(xs)


def dae_walk64(method, de, ae, xi, t, z, v, a0, ev=None, zj=None, vj=None):
    xs, xc = [xi], xi
    i0 = O.ae_rhs(ae, xi, z[0], v[0], a0)
    is_ = [i0]
    for j in range(1, t.shape[0]):
        t0, z0, v0 = t[j - 1], z[j - 1], v[j - 1]
        if ev is not None and O._event_hit(ev, t0):
            sel = (ev[0] == t0[0][0]).view(-1)
            z0, v0 = zj[:, sel].view(z0.shape), vj[:, sel].view(v0.shape)
            i0 = O.ae_rhs(ae, xc, z0, v0, a0)
        i_in = i0
        xc, _ = O.step(method, lambda xx: O.de_rhs(de, xx, (z0, v0, i_in), a0), t0, t[j] - t0, t[j], xc)
        i0 = O.ae_rhs(ae, xc, z[j], v[j], a0)
        xs.append(xc)
        is_.append(i0)
    return torch.stack(xs), torch.stack(is_)
