"""Cases of the Adams-Bashforth 3 tests and a stand-alone fp64 restatement of the method, written without the package's solver classes; a
plain module on top of ab2_cases.py / pev_cases.py / generic_cases.py, whose shapes, clocks, event patterns and runners it reuses.

The method (issue "Adams-Bashforth 3 on the generic kernels K0 / K5"): step k, per trajectory, h_k = t[k+1] - t[k], f_k the DE at the inputs
AB2's stage reads.  R_k: k == 0, an event of the trajectory at step k, or h_{k-1} == 0.  Depth d_k: 0 if R_k; 1 if R_{k-1} or
h_{k-1} + h_{k-2} == 0; else 2.  Depth 2 / 1: the Adams-Bashforth step through the last three / two slopes.  Depth 0: the restart step,
    x~ = x_k + h f_k;  f~ = DE(x~; rows k + 1 of z | v, never jumped; a DAE: i~ = AE(x~; z[k+1], v[k+1]));  x_{k+1} = x_k + (h / 2)(f_k + f~)
and the slope kept for the history is f_k.  The restatement does not copy the issue's coefficient formulas: it integrates the Lagrange basis
of the interpolation nodes 0, -h1, -h1 - h2 over [0, h0] (`_weights`), which is what an Adams-Bashforth method is.

Base shape B = 33 (three workgroups, the last with one live column), T = 8 (two events leave too few depth-2 steps on AB2's six points), the
seven event patterns of ab2_cases, clocks "ragged", "ratio" (2 : 1) and "padded", parameters scaled by W_SCALE = 1.5."""
from copy import deepcopy

import torch
import torch.nn as nn

import ab2_cases as A
import generic_cases as C
from py_psnode_amd import neural_dae as nd

B0, T0 = A.B0, 8
PATTERNS = A.PATTERNS
SHARED, PER_TRAJ = A.SHARED, A.PER_TRAJ
W_SCALE = A.W_SCALE
CLOCKS = ("ragged", "ratio", "padded")
clock, valid_len, shared_table, _scaled = A.clock, A.valid_len, A.shared_table, A._scaled
run_ode, run_dae, ode_train, dae_train, grads_close = A.run_ode, A.run_dae, A.ode_train, A.dae_train, A.grads_close


def ode_case(pattern, shape="reg", B=B0, Tn=T0, kind="ragged", act=nn.ELU, seed=21):
    """(de, t, x, z, ev, zj, table, per_trajectory): ab2_cases.ode_case on eight grid points"""
    return A.ode_case(pattern, shape, B, Tn, kind, act, seed)


def dae_case(pattern, shape="x8z2v2i2", B=B0, Tn=T0, kind="ragged", de_act=nn.ELU, ae_act=nn.ELU, seed=22, shapes=C.DAE_SHAPES):
    """(de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, table, per_trajectory)"""
    return A.dae_case(pattern, shape, B, Tn, kind, de_act, ae_act, seed, shapes)


def solver(mode="off", kernel="auto", cls=None):
    return A.solver(mode, kernel, cls or nd.AB3)


# ----------------------------------------------------------------------------- the restatement
def _basis_integral(h, a, b, node):
    """int_0^h (tau - a)(tau - b) dtau / ((node - a)(node - b))"""
    return (h ** 3 / 3 - (a + b) * h ** 2 / 2 + a * b * h) / ((node - a) * (node - b))


def _weights(h0, h1, h2, depth):
    """(c0, c1, c2) [B, 1]: the integrals over [0, h0] of the Lagrange basis of the nodes 0, -h1, -h1 - h2 (depth 2), 0, -h1 (depth 1) or of
    1 (depth 0), per trajectory by `depth` (int [B, 1]).  Steps that a depth does not read are replaced by 1 before they divide."""
    one, zero = torch.ones_like(h0), torch.zeros_like(h0)
    s1 = torch.where(depth >= 1, h1, one)
    s2 = torch.where(depth >= 2, h2, one)
    n1, n2 = -s1, -s1 - s2
    deep = (_basis_integral(h0, n1, n2, zero), _basis_integral(h0, zero, n2, n1), _basis_integral(h0, zero, n1, n2))
    two = (h0 + h0 ** 2 / (2 * s1), -h0 ** 2 / (2 * s1), zero)
    flat = (h0, zero, zero)
    return tuple(torch.where(depth == 2, d, torch.where(depth == 1, w, f)) for d, w, f in zip(deep, two, flat))


def _depth(k, h_hist, hit, r_prev):
    """(R_k bool [B, 1], d_k int [B, 1]) from the previous steps h_hist = (h_{k-1}, h_{k-2}) (None where they do not exist)"""
    h1, h2 = h_hist
    restart = torch.ones_like(hit) if k == 0 else hit | (h1 == 0)
    shallow = torch.ones_like(hit) if k < 2 else restart | r_prev | ((h1 + h2) == 0)
    return restart, torch.where(restart, 0, torch.where(shallow, 1, 2))


def _advance(x, f, hist, h, restart, depth, corrector, variant):
    """x_{k+1}; hist = [(f_{k-1}, h_{k-1}), (f_{k-2}, h_{k-2})]; corrector: () -> f~ of the restart step"""
    zero = torch.zeros_like(f)
    (f1, h1), (f2, h2) = [(q if q[0] is not None else (zero, torch.ones_like(h))) for q in hist]
    c0, c1, c2 = _weights(h, h1, h2, depth)
    out = x + c0 * f + c1 * f1 + c2 * f2
    if variant != "euler_restart" and bool(restart.any()):
        out = torch.where(restart, x + h / 2 * (f + corrector()), out)
    return out


def _flags(k, hist, col, r_prev, variant):
    hit = (col >= 0).view(-1, 1)
    if variant == "no_event_restart":
        hit = torch.zeros_like(hit)
    return _depth(k, (hist[0][1], hist[1][1]), hit, r_prev)


def restate_ode(de, t, x0, z, a0, table, zj, variant="ab3"):
    """xs [T, B, xd] in the dtype of the inputs; `de` a DE_Func-style module called with the package's keyword convention.  variant:
    "ab3"; "euler_restart" (the Euler / AB2 / AB3 ramp: a restart step is Euler's); "no_event_restart" (the history runs through the
    events); "ab2" (ab2_cases.restate_ode) -- the neighbours the sensitivity check measures the distance to."""
    if variant == "ab2":
        return A.restate_ode(de, t, x0, z, a0, table, zj)
    xs, cur, hist = [x0], x0, [(None, None), (None, None)]
    r_prev = torch.ones(x0.shape[0], 1, dtype=torch.bool)
    for k in range(t.shape[0] - 1):
        col = table[k]
        f = de(t0=t[k], xt=cur, zt=A._jumped(z[k], zj, col), all_initial=a0)
        h = t[k + 1] - t[k]
        restart, depth = _flags(k, hist, col, r_prev, variant)
        corrector = lambda: de(t0=t[k + 1], xt=cur + h * f, zt=z[k + 1], all_initial=a0)
        cur = _advance(cur, f, hist, h, restart, depth, corrector, variant)
        hist, r_prev = [(f, h), hist[0]], restart
        xs.append(cur)
    return torch.stack(xs)


def restate_dae(de, ae, t, x_init, z, v, a0, table, zj, vj, variant="ab3"):
    """(xs [T, B, xd], is [T, B, id])"""
    if variant == "ab2":
        return A.restate_dae(de, ae, t, x_init, z, v, a0, table, zj, vj)
    cur = x_init
    i_cur = ae(xt=cur, zt=z[0], vt=v[0], all_initial=a0)
    xs, is_, hist = [cur], [i_cur], [(None, None), (None, None)]
    r_prev = torch.ones(cur.shape[0], 1, dtype=torch.bool)
    for k in range(t.shape[0] - 1):
        col = table[k]
        zk, vk = A._jumped(z[k], zj, col), A._jumped(v[k], vj, col)
        if bool((col >= 0).any()):
            i_cur = torch.where((col >= 0).view(-1, 1), ae(xt=cur, zt=zk, vt=vk, all_initial=a0), i_cur)
        f = de(t0=t[k], xt=cur, zt=zk, vt=vk, it=i_cur, all_initial=a0)
        h = t[k + 1] - t[k]
        restart, depth = _flags(k, hist, col, r_prev, variant)

        def corrector():
            xp = cur + h * f
            return de(t0=t[k + 1], xt=xp, zt=z[k + 1], vt=v[k + 1], it=ae(xt=xp, zt=z[k + 1], vt=v[k + 1], all_initial=a0), all_initial=a0)
        cur = _advance(cur, f, hist, h, restart, depth, corrector, variant)
        hist, r_prev = [(f, h), hist[0]], restart
        i_cur = ae(xt=cur, zt=z[k + 1], vt=v[k + 1], all_initial=a0)
        xs.append(cur)
        is_.append(i_cur)
    return torch.stack(xs), torch.stack(is_)


def restate_ode64(case, **kw):
    de, t, x, z, ev, zj, table, _ = case
    with torch.no_grad():
        x64, z64 = x.double(), z.double()
        return restate_ode(deepcopy(de).double(), t.double(), x64[0], z64, torch.cat((x64[0], z64[0]), -1), table, C.to64(zj), **kw)


def restate_dae64(case, **kw):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, table, _ = case
    with torch.no_grad():
        return restate_dae(deepcopy(de).double(), deepcopy(ae).double(), t.double(), x_init.double(), z.double(), v.double(), a0.double(),
                           table, C.to64(zj), C.to64(vj), **kw)
