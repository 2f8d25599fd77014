"""Shared by tests/test_externals_linear_host.py and tests/test_gpu_externals_linear.py (not a conftest).

1. `refine_rows_linear`: the n-times refined problem on which the one-step-per-interval Euler call -- the CPU oracle's -- is what Euler with
   `substeps = n` and `externals = "linear"` computes on the coarse problem (no teacher forcing): clock t'[kn + j] = t[k] + j h
   (generic_cases.refine_clock), rows z'[kn + j] = w_L + (j / n) (w_R - w_L) with w_R = z[k + 1] and w_L = z[k], or the jumped values on an
   interval that starts with an event; there row kn keeps the dataset value, which the event replaces.

2. A stand-alone restatement of an explicit Runge-Kutta step with linearly interpolated externals, for an arbitrary tableau:
       k_s = f(x + h sum_{q<s} a[s][q] k_q ;  w_L + theta_s (w_R - w_L)),   theta_s = (j + sum_{q<s} a[s][q]) / n
   It shares no code with the package."""
import torch

TABLEAUS = {      # name -> (a, b): the strictly lower triangle row by row, and the weights
    "euler": (((),), (1.0,)),
    "midpoint": (((), (0.5,)), (0.0, 1.0)),
    "rk4": (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125)),
    "Heun2": (((), (1.0,)), (0.5, 0.5)),
    "Kutta3": (((), (0.5,), (-1.0, 2.0)), (1 / 6, 2 / 3, 1 / 6)),
    "RK4Classic": (((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
}


def refine_rows_linear(a, n, t=None, event_t=None, jump=None):
    """a [T,B,D] -> [(T-1) n + 1, B, D]: row kn + j = w_L + (j / n) (a[k + 1] - w_L), in a's dtype.  w_L = a[k], or jump[:, e] on an interval
    that starts with event e (event_t [B,nE,1], jump [B,nE,D]); row kn itself always keeps a[k]."""
    Tn = a.shape[0]
    rows = []
    for k in range(Tn - 1):
        left = a[k]
        if event_t is not None and jump is not None and a.shape[-1] > 0:
            hit = (event_t[0, :, 0] == t[k, 0, 0]).nonzero().view(-1)
            if hit.numel():
                left = jump[:, int(hit[0])]
        rows.append(a[k])
        for j in range(1, n):
            rows.append(left + (j / n) * (a[k + 1] - left))
    rows.append(a[-1])
    return torch.stack(rows, 0)


def rk_step_linear(f, a, b, h, x0, w_left, w_right, j, n):
    """One sub-step j of n: f(x, w) -> dx/dt with w a tuple of external tensors; w_left / w_right the tuples at the interval's two ends."""
    ks = []
    for s in range(len(b)):
        c = 0.0
        arg = x0
        if s:
            inc = 0.0
            for q in range(s):
                c = c + a[s][q]
                inc = inc + a[s][q] * ks[q]
            arg = x0 + h * inc
        theta = (j + c) / n
        ks.append(f(arg, tuple(l + theta * (r - l) for l, r in zip(w_left, w_right))))
    out = 0.0
    for s in range(len(b)):
        out = out + b[s] * ks[s]
    return x0 + h * out


def ode_linear_reference(f, a, b, t, x0, z, n, event_steps=(), z_jump=None):
    """The whole ODE: t [T,B,1], z [T,B,zd], x0 [B,xd]; event e fires at grid step event_steps[e] and replaces z[k] by z_jump[:, e] as the
    interval's left value.  Returns xs [T,B,xd]."""
    xs = [x0]
    cur = x0
    for k in range(t.shape[0] - 1):
        left = z[k]
        if k in event_steps:
            left = z_jump[:, list(event_steps).index(k)]
        h = (t[k + 1] - t[k]) / n
        for j in range(n):
            cur = rk_step_linear(f, a, b, h, cur, (left,), (z[k + 1],), j, n)
        xs.append(cur)
    return torch.stack(xs, 0)
