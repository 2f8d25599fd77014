"""Cases of the Adams-Bashforth 2 tests and a stand-alone fp64 restatement of the method, written without the package's solver classes; a
plain module, imported like generic_cases.py / pev_cases.py, whose shapes, clocks and event patterns it reuses.

The method (issue "Adams-Bashforth 2 on the generic kernels K0 / K5"): step k, per trajectory, h_k = t[k+1] - t[k], f_k the DE at the inputs
Euler's stage reads (x_k; row k of z | v or the jumped rows; for a DAE the carried head or the event-time head):
    x_{k+1} = x_k + c0 f_k + c1 f_{k-1};  restart (k = 0, an event of the trajectory at step k, h_{k-1} == 0): c0 = h_k, c1 = 0;
    otherwise rho = h_k / h_{k-1}, c0 = h_k (1 + rho / 2), c1 = -h_k (rho / 2).
Both event rules are one table here, int [T-1, B] (-1 = none): the shared rule is the table whose columns all equal trajectory 0's.

Base shape B = 33 (three workgroups, the last with one live column), T = 6, grid step 0.1.  Event patterns: "none"; shared "s03" (steps 0
and 3), "s1" (a restart right after the start), "s23" (consecutive); the three per-trajectory patterns of pev_cases.  The parameters of
every case's MLPs are scaled by W_SCALE, so that on a six-point grid AB2 lies more than 100 x TOL_GPU from Euler and from AB2 without the
restart at the events (tests/test_adams_bashforth_host.py asserts it: without it the GPU tests would prove nothing)."""
from copy import deepcopy

import torch
import torch.nn as nn

import generic_cases as C
import pev_cases as P
from py_psnode_amd import neural_dae as nd

B0, T0 = P.B0, P.T0
SHARED = {"none": (), "s03": (0, 3), "s1": (1,), "s23": (2, 3)}
PER_TRAJ = P.PATTERNS
PATTERNS = tuple(SHARED) + PER_TRAJ
W_SCALE = 1.5


def clock(kind="ragged", Tn=T0, B=B0):
    """"ragged": pev_cases.clock (per-trajectory step sizes around 0.1, constant inside a trajectory); "ratio": steps alternate 2 : 1 inside
    every trajectory; "padded": the ragged one with -1 padding that starts at grid point T - (b % 3) of trajectory b (b % 3 == 0: whole;
    trajectory 0, whose clock decides the shared events, among them)."""
    t = P.clock(Tn, B)
    if kind == "ratio":
        w = torch.tensor([2.0 if k % 2 == 0 else 1.0 for k in range(Tn - 1)])
        steps = (t[1:2] - t[0:1]) * (w / 1.5).view(-1, 1, 1)
        t = torch.cat((t[0:1], t[0:1] + torch.cumsum(steps, 0)), 0)
    elif kind == "padded":
        t = t.clone()
        for b in range(B):
            if b % 3:
                t[Tn - (b % 3):, b] = -1.0
    return t


def valid_len(Tn, b):
    """grid points of trajectory b in front of the "padded" clock's padding"""
    return Tn - (b % 3)


def _scaled(m):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(W_SCALE)
    return m


def ode_case(pattern, shape="reg", B=B0, Tn=T0, kind="ragged", act=nn.ELU, seed=21):
    """(de, t, x, z, ev, zj, table, per_trajectory)"""
    xd, zd, hidden = C.ODE_FWD_SHAPES[shape] if isinstance(shape, str) else shape
    t = clock(kind, Tn, B)
    case = C.ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=SHARED.get(pattern, ()), t=t, act=act)
    _scaled(case[0])
    if pattern in PER_TRAJ:
        case = P.with_pattern(case, pattern, 2.0)
        return case + (P.step_table(pattern, Tn, B), True)
    return case + (shared_table(SHARED[pattern], Tn, B), False)


def dae_case(pattern, shape="x8z2v2i2", B=B0, Tn=T0, kind="ragged", de_act=nn.ELU, ae_act=nn.ELU, seed=22, shapes=C.DAE_SHAPES):
    """(de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, table, per_trajectory)"""
    t = clock(kind, Tn, B)
    case = C.dae_case(*shapes[shape], B, Tn, seed, ev_rows=SHARED.get(pattern, ()), t=t, de_act=de_act, ae_act=ae_act, perturb_x_init=True)
    _scaled(case[0])
    _scaled(case[1])
    if pattern in PER_TRAJ:
        case = P.with_pattern(case, pattern, 2.0, dae=True)
        return case + (P.step_table(pattern, Tn, B), True)
    return case + (shared_table(SHARED[pattern], Tn, B), False)


def shared_table(rows, Tn, B):
    tab = torch.full((max(Tn - 1, 0), B), -1, dtype=torch.int32)
    for col, k in enumerate(r for r in rows if r < Tn - 1):
        tab[k] = col
    return tab


# ----------------------------------------------------------------------------- the restatement
def _coef(h, h_prev, restart):
    """(c0, c1) [B, 1] of one step; h_prev None at k = 0"""
    if h_prev is None:
        return h, torch.zeros_like(h)
    restart = restart | (h_prev == 0)
    rho = h / torch.where(restart, torch.ones_like(h_prev), h_prev)
    return torch.where(restart, h, h * (1 + rho / 2)), torch.where(restart, torch.zeros_like(h), -h * (rho / 2))


def _jumped(rows, jump, col):
    """rows [B, D] with trajectory b's replaced by jump[b, col[b]] where col[b] >= 0"""
    if jump is None or not bool((col >= 0).any()):
        return rows
    pick = jump[torch.arange(jump.shape[0]), col.clamp_min(0).long()]
    return torch.where((col >= 0).view(-1, 1), pick, rows)


def restate_ode(de, t, x0, z, a0, table, zj, restart_at_events=True, euler=False):
    """xs [T, B, xd] in the dtype of the inputs; `de` a DE_Func-style module called with the package's keyword convention.
    restart_at_events=False / euler=True: the two neighbours the sensitivity check measures the distance to."""
    xs, cur, f_prev, h_prev = [x0], x0, None, None
    for k in range(t.shape[0] - 1):
        col = table[k]
        f = de(t0=t[k], xt=cur, zt=_jumped(z[k], zj, col), all_initial=a0)
        h = t[k + 1] - t[k]
        hit = (col >= 0).view(-1, 1) if restart_at_events else torch.zeros(h.shape, dtype=torch.bool)
        c0, c1 = (h, torch.zeros_like(h)) if euler else _coef(h, h_prev, hit)
        cur = cur + c0 * f + (c1 * f_prev if f_prev is not None else 0)
        f_prev, h_prev = f, h
        xs.append(cur)
    return torch.stack(xs)


def restate_dae(de, ae, t, x_init, z, v, a0, table, zj, vj, restart_at_events=True, euler=False):
    """(xs [T, B, xd], is [T, B, id])"""
    cur = x_init
    i_cur = ae(xt=cur, zt=z[0], vt=v[0], all_initial=a0)
    xs, is_, f_prev, h_prev = [cur], [i_cur], None, None
    for k in range(t.shape[0] - 1):
        col = table[k]
        zk, vk = _jumped(z[k], zj, col), _jumped(v[k], vj, col)
        if bool((col >= 0).any()):
            i_cur = torch.where((col >= 0).view(-1, 1), ae(xt=cur, zt=zk, vt=vk, all_initial=a0), i_cur)
        f = de(t0=t[k], xt=cur, zt=zk, vt=vk, it=i_cur, all_initial=a0)
        h = t[k + 1] - t[k]
        hit = (col >= 0).view(-1, 1) if restart_at_events else torch.zeros(h.shape, dtype=torch.bool)
        c0, c1 = (h, torch.zeros_like(h)) if euler else _coef(h, h_prev, hit)
        cur = cur + c0 * f + (c1 * f_prev if f_prev is not None else 0)
        f_prev, h_prev = f, h
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


# ----------------------------------------------------------------------------- runners through the package
def solver(mode="off", kernel="auto", cls=None):
    s = (cls or nd.AB2)()
    s.fused, s.kernel = mode, kernel
    return s


def run_ode(s, case, dev="cpu", dtype=torch.float32):
    de, t, x, z, ev, zj, _, pt = case
    cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
    xc, zc = cv(x), cv(z)
    with torch.no_grad():
        return P.run_ode(s, deepcopy(de).to(device=dev, dtype=dtype), cv(t), xc, zc, torch.cat((xc[0], zc[0]), -1), cv(ev), cv(zj),
                         per_trajectory=pt)


def run_dae(s, case, dev="cpu", dtype=torch.float32):
    cv = lambda a: None if a is None else a.to(device=dev, dtype=dtype)
    with torch.no_grad():
        return P.run_dae(s, deepcopy(case[0]).to(device=dev, dtype=dtype), deepcopy(case[1]).to(device=dev, dtype=dtype),
                         *(cv(q) for q in case[2:12]), per_trajectory=case[13])


def ode_train(s, case, G, dev):
    """one forward + backward of sum(xs * G): fp32 on "cuda", fp64 on "cpu" -> xs, {name: grad}"""
    de, t, x, z, ev, zj, _, pt = case
    dtype, cv = C._cv(dev)
    m = deepcopy(de).to(device=dev, dtype=dtype)
    xg, zg = cv(x).requires_grad_(True), cv(z).requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = None if zj is None else cv(zj).requires_grad_(True)
    xs = P.run_ode(s, m, cv(t), xg, zg, a0, None if ev is None else cv(ev), zjg, per_trajectory=pt)
    (xs * cv(G)).sum().backward()
    grads = {"x": xg.grad, "z": zg.grad, "a0": a0.grad}
    if zjg is not None:
        grads["zj"] = zjg.grad
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def dae_train(s, case, G, Gi, dev):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, _, pt = case
    dtype, cv = C._cv(dev)
    de, ae = deepcopy(de).to(device=dev, dtype=dtype), deepcopy(ae).to(device=dev, dtype=dtype)
    leaf = lambda a: None if a is None else cv(a).requires_grad_(True)
    xi, zg, vg, a0g, zjg, vjg = leaf(x_init), leaf(z), leaf(v), leaf(a0), leaf(zj), leaf(vj)
    xs, is_ = P.run_dae(s, de, ae, cv(t), cv(x), zg, vg, cv(i), xi, a0g, None if ev is None else cv(ev), zjg, vjg, per_trajectory=pt)
    ((xs * cv(G)).sum() + (is_ * cv(Gi)).sum()).backward()
    grads = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad}
    if zjg is not None:
        grads.update(zj=zjg.grad, vj=vjg.grad)
    grads.update({f"de{k}": p.grad for k, p in enumerate(de.parameters())})
    grads.update({f"ae{k}": p.grad for k, p in enumerate(ae.parameters())})
    return xs, is_, grads


def grads_close(ref, got, tol, what=""):
    """every gradient within tol of its tensor's max (a gradient that is None counts as zero)"""
    worst = {}
    for name, r in ref.items():
        g = got[name]
        if (g if g is not None else r).numel() == 0:          # (z_dim 0: an empty gradient)
            continue
        r = torch.zeros_like(g.detach().double().cpu()) if r is None else r.detach().double().cpu()
        g = torch.zeros_like(r) if g is None else g.detach().double().cpu()
        worst[name] = float((g - r).abs().max() / r.abs().max().clamp_min(1e-30))
    print(what, {k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (what, bad)
