"""Shared by tests/test_externals_lagrange_host.py and tests/test_gpu_externals_lagrange.py (not a conftest).

1. `stencils_brute`: the stencil table of externals="lagrange" restated with loops -- per trajectory, the pieces (maximal runs of intervals
   with t[k+1] > t[k] and no event step inside; an interval with t[k+1] <= t[k] is a piece of its own), and per interval k of piece [a, e]
   q = min(4, e - a + 1), s = clamp(k - 1, a, e - q + 1), code = (k - s) | (q << 2).

2. A stand-alone restatement of an explicit Runge-Kutta step whose stage at theta reads the polynomial through the stencil's nodes, for an
   arbitrary tableau, and of the whole ODE with events (node s is the jumped row where step s has an event).  It shares no code with the
   package.

3. The argument lists of the nine _lag entry points (the _lin family's plus the stencil table)."""
import torch

from capi_args import R
from externals_linear_cases import TABLEAUS  # noqa: F401  (name -> (a, b))

EV_ROWS = (0, 2, 3, 6)      # on 12 grid points: pieces of 3, 2, 4 and 6 nodes


def pieces_brute(tcol, ev_steps):
    """[(a, e), ...] of one trajectory's clock (a list of floats): nodes a .. e, intervals a .. e - 1"""
    Tn = len(tcol)
    out, k = [], 0
    while k < Tn - 1:
        if not tcol[k + 1] - tcol[k] > 0:
            out.append((k, k + 1))
            k += 1
            continue
        e = k + 1
        while e <= Tn - 2 and tcol[e + 1] - tcol[e] > 0 and e not in ev_steps:
            e += 1
        out.append((k, e))
        k = e
    return out


def stencils_brute(t, ev_steps=()):
    """t [T, B(, 1)] -> codes [T-1][B] (lists of ints) and the pieces per trajectory"""
    t2 = t.reshape(t.shape[0], -1)
    Tn, B = t2.shape
    codes = [[0] * B for _ in range(Tn - 1)]
    all_pieces = []
    for b in range(B):
        ps = pieces_brute([float(v) for v in t2[:, b]], set(ev_steps))
        all_pieces.append(ps)
        for a, e in ps:
            q = min(4, e - a + 1)
            for k in range(a, e):
                s = min(max(k - 1, a), e - q + 1)
                codes[k][b] = (k - s) | (q << 2)
    return codes, all_pieces


def lagrange_value(nodes, off, theta):
    """sum_m l_m(off + theta) nodes[m], l_m(u) = prod_{r != m} (u - r) / (m - r): nodes a list of q tensors (or floats)"""
    q, u = len(nodes), off + theta
    out = 0.0
    for m in range(q):
        w = 1.0
        for r in range(q):
            if r != m:
                w = w * (u - r) / (m - r)
        out = out + w * nodes[m]
    return out


def interval_nodes(rows, jumps, ev_steps, codes, k):
    """per external tensor of `rows` ([T,B,D]; jumps: [B,nE,D] or None): off [B] and the node rows [4][B,D] of interval k (rows beyond q: 0)"""
    B = rows[0].shape[1]
    offs = [codes[k][b] & 3 for b in range(B)]
    qs = [(codes[k][b] >> 2) & 7 for b in range(B)]
    out = []
    for w, wj in zip(rows, jumps):
        per_m = []
        for m in range(4):
            col = []
            for b in range(B):
                s = k - offs[b]
                if m >= qs[b]:
                    col.append(torch.zeros_like(w[0, b]))
                elif m == 0 and s in ev_steps and wj is not None:
                    col.append(wj[b, list(ev_steps).index(s)])
                else:
                    col.append(w[s + m, b])
            per_m.append(torch.stack(col))
        out.append(per_m)
    return offs, qs, out


def ext_at_theta(offs, qs, nodes, theta):
    """the tuple of externals [B,D] at theta, column by column"""
    out = []
    for per_m in nodes:
        cols = [lagrange_value([per_m[m][b] for m in range(qs[b])], offs[b], theta) for b in range(len(offs))]
        out.append(torch.stack(cols))
    return tuple(out)


def rk_step_lagrange(f, a, b, h, x0, ext, j, n):
    """One sub-step j of n: f(x, w) -> dx/dt; ext(theta) -> the tuple of externals"""
    ks = []
    for s in range(len(b)):
        c, arg = 0.0, x0
        if s:
            inc = 0.0
            for q in range(s):
                c = c + a[s][q]
                inc = inc + a[s][q] * ks[q]
            arg = x0 + h * inc
        ks.append(f(arg, ext((j + c) / n)))
    out = 0.0
    for s in range(len(b)):
        out = out + b[s] * ks[s]
    return x0 + h * out


def ode_lagrange_reference(f, a, b, t, x0, z, n, ev_steps=(), z_jump=None, x_true=None):
    """The whole ODE: t [T,B,1], z [T,B,zd], x0 [B,xd]; event e fires at grid step ev_steps[e].  x_true: teacher forcing from its rows."""
    codes, _ = stencils_brute(t, ev_steps)
    xs, cur = [x0], x0
    for k in range(t.shape[0] - 1):
        offs, qs, nodes = interval_nodes((z,), (z_jump,), ev_steps, codes, k)
        h = (t[k + 1] - t[k]) / n
        if x_true is not None:
            cur = x_true[k]
        for j in range(n):
            cur = rk_step_lagrange(f, a, b, h, cur, lambda th: ext_at_theta(offs, qs, nodes, th), j, n)
        xs.append(cur)
    return torch.stack(xs, 0)


# ----------------------------------------------------------------------------- the C entry points
def options(n_act, tab, sub_, act_, stencil):
    return [act_] * n_act + [tab, R(sub_) if sub_ is not None else None, stencil]


def supported(lib, stem, a, n_act, tab=None, sub=None, act=None, stencil=None):
    return getattr(lib, f"psnode_{stem}_lag_supported")(R(a), *options(n_act, tab, sub, act, stencil))


def call(lib, stem, a, n_act, tab=None, sub=None, act=None, stencil=None):
    """psnode_<stem>_lag_f32 without workspace or stream: with every pointer of the args NULL a call that got past its checks would have
    nothing to launch on"""
    return getattr(lib, f"psnode_{stem}_lag_f32")(R(a) if a is not None else None, *options(n_act, tab, sub, act, stencil), None, 0, None)
