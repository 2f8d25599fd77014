"""Cases and references shared by the tests of multiple-shooting segments (solver.segment); a plain module, imported like generic_cases.py.

The definition under test: with segment = w, output rows m w + 1 .. min((m + 1) w, T - 1) are what the free-running call returns in its
rows 1 .. on the slices [m w : (m + 1) w + 1] of t, z[, v, i], started from the dataset row x[m w] (m = 0: from the call's own start),
with the same all_initial, event list and jumps.  `sliced_ode` / `sliced_dae` assemble exactly that from any free-running integrator.

The dataset x of a case is the free run (float64 walk, Euler) plus a perturbation of 0.05 per element, so that a restart is visible: a
segment that starts from x[k] and one that runs on from the prediction differ by about the perturbation, four orders above TOL_GPU.
Shapes: B = 33 (two full tiles of 16 trajectories and one column), T = 8 (seven intervals), w in {1, 3, 7, 100}; shared events at steps
0, 3 and 4 -- step 3 is a restart point for w = 3, step 4 lies inside a segment."""
import warnings
from copy import deepcopy

import torch

import generic_cases as C
from py_psnode_amd import neural_dae as nd

B0, T0 = 33, 8
WS = (1, 3, 7, 100)
EV = (0, 3, 4)
SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4, "Kutta3": nd.Kutta3, "Heun2": nd.Heun2, "RK4Classic": nd.RK4Classic}


def solver(name, w=None, n=1, mode="off", kernel="auto"):
    s = SOLVERS[name](substeps=n, segment=w)
    s.fused, s.kernel = mode, kernel
    return s


def _perturbed(x, free, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    out = x.clone()
    out[1:] = free[1:].to(x.dtype) + 0.05 * torch.randn(free[1:].shape, generator=g)
    return out


def ode_case(xd, zd, hidden, B=B0, Tn=T0, seed=0, events=True, t=None, pad=False, act=None):
    """generic_cases.ode_case whose rows x[1:] are the free Euler run (float64 walk) + 0.05 randn"""
    kw = {} if act is None else dict(act=act)
    de, t, x, z, ev, zj = C.ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=EV if events else (), t=t, pad=pad, **kw)
    free = C.ode_walk64(solver("euler"), de, t, x, z, ev, zj)
    return de, t, _perturbed(x, free, seed), z, ev, zj


def dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B=B0, Tn=T0, seed=0, events=True, t=None, pad=False, de_act=None, ae_act=None):
    """generic_cases.dae_case (x_init perturbed: not the dataset row) whose rows x[1:] are the free Euler run + 0.05 randn"""
    kw = {k: a for k, a in (("de_act", de_act), ("ae_act", ae_act)) if a is not None}
    case = C.dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, ev_rows=EV if events else (), t=t, pad=pad, perturb_x_init=True, **kw)
    free = C.dae_walk64(solver("euler"), case)[0]
    return case[:3] + (_perturbed(case[3], free, seed),) + case[4:]


def slices(Tn, w):
    """[(first grid point, last grid point)] of the segments of a record of Tn points"""
    return [(s, min(s + w, Tn - 1)) for s in range(0, max(Tn - 1, 1), w)] if Tn > 1 else []


def sliced_ode(free, t, x, z, x_start=None):
    """free(t_s, x_s, z_s, start [B, xd]) -> xs of the free run on a slice; -> the assembled [T, B, xd]"""
    out = torch.zeros(x.shape, dtype=x.dtype)
    out[0] = x[0] if x_start is None else x_start
    for a, b in slices(t.shape[0], free.w):
        out[a + 1:b + 1] = free(t[a:b + 1], x[a:b + 1], z[a:b + 1], out[0] if a == 0 else x[a])[1:]
    return out


def sliced_dae(free, t, x, z, v, i, x_init):
    """free(t_s, x_s, z_s, v_s, i_s, start) -> (xs, is) of the free run on a slice; -> the assembled pair.  Row 0 is the first slice's."""
    xs = torch.zeros(x.shape, dtype=x.dtype)
    is_ = torch.zeros(i.shape, dtype=i.dtype)
    for a, b in slices(t.shape[0], free.w):
        sx, si = free(t[a:b + 1], x[a:b + 1], z[a:b + 1], v[a:b + 1], i[a:b + 1], x_init if a == 0 else x[a])
        if a == 0:
            xs[0], is_[0] = sx[0], si[0]
        xs[a + 1:b + 1], is_[a + 1:b + 1] = sx[1:], si[1:]
    if t.shape[0] == 1:
        sx, si = free(t, x, z, v, i, x_init)
        xs[0], is_[0] = sx[0], si[0]
    return xs, is_


class Free:
    """a free-running integrator with the segment length it is sliced at"""
    def __init__(self, w, fn):
        self.w, self.fn = w, fn

    def __call__(self, *a):
        return self.fn(*a)


def walk_sliced_ode(name, n, w, de, t, x, z, ev, zj, dtype=torch.float64):
    """the package's own free walk (segment=None), slice by slice, in `dtype`"""
    m = deepcopy(de).to(dtype)
    cv = lambda a: None if a is None else a.to(dtype)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1)
    s = solver(name, None, n)

    def free(ts, xs_, zs, start):
        event = nd.ODE_Event()
        if ev is not None:
            event.set_event(cv(ev), cv(zj))
        return s.integrate_ODE(x_func=m, t=ts, x=xs_, z=zs, all_initial=a0, event_fn=event.event_fn if ev is not None else None,
                               jump_change_fn=event.jump_change_fn if ev is not None else None, x_init=start)
    with torch.no_grad():
        return sliced_ode(Free(w, free), cv(t), cv(x), cv(z))


def walk_sliced_dae(name, n, w, case, dtype=torch.float64):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    de, ae = deepcopy(de).to(dtype), deepcopy(ae).to(dtype)
    cv = lambda a: None if a is None else a.to(dtype)
    s = solver(name, None, n)

    def free(ts, xs_, zs, vs, is__, start):
        return C.run_dae(s, de, ae, ts, xs_, zs, vs, is__, start, cv(a0), cv(ev), cv(zj), cv(vj))
    with torch.no_grad():
        return sliced_dae(Free(w, free), cv(t), cv(x), cv(z), cv(v), cv(i), cv(x_init))


def walk_ode(name, n, w, de, t, x, z, ev, zj, dtype=torch.float64):
    """the walk with segment = w, in `dtype`"""
    cv = lambda a: None if a is None else a.to(dtype)
    with torch.no_grad():
        return C.run_ode(solver(name, w, n), deepcopy(de).to(dtype), cv(t), cv(x), cv(z), torch.cat((cv(x)[0], cv(z)[0]), -1), cv(ev), cv(zj))


def walk_dae(name, n, w, case, dtype=torch.float64):
    cv = lambda a: None if a is None else a.to(dtype)
    with torch.no_grad():
        return C.run_dae(solver(name, w, n), deepcopy(case[0]).to(dtype), deepcopy(case[1]).to(dtype), *(cv(q) for q in case[2:]))


def row_gap(a, b, row):
    """per trajectory: max |a[row] - b[row]| over the columns, relative to the trajectory's max |b| (floor 1e-3) -- traj_rel_err at one row"""
    scale = b.abs().amax((0, 2)).clamp_min(1e-3)
    return (a[row] - b[row]).abs().amax(-1) / scale


# ----------------------------------------------------------------------------- training
def ode_train(mk, case, G, dev):
    """loss = sum(xs * G) through integrate_ODE(..., x_init=leaf): the dataset x is no leaf (it gets no gradient; a leaf x with a restart
    walks).  Leaves: x_init, z, all_initial, the jump rows, the parameters.  mk(mode) -> solver.  -> xs, {name: grad}"""
    de, t, x, z, ev, zj = case
    dtype, cv = C._cv(dev)
    m = deepcopy(de).to(device=dev, dtype=dtype)
    x0 = cv(x)[0].clone().requires_grad_(True)
    zg = cv(z).requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = cv(zj).requires_grad_(True) if zj is not None else None
    event = nd.ODE_Event()
    if ev is not None:
        event.set_event(cv(ev), zjg)
    xs = mk("require" if dev == "cuda" else "off").integrate_ODE(
        x_func=m, t=cv(t), x=cv(x), z=zg, all_initial=a0, event_fn=event.event_fn if ev is not None else None,
        jump_change_fn=event.jump_change_fn if ev is not None else None, x_init=x0)
    (xs * cv(G)).sum().backward()
    grads = {"x_init": x0.grad, "z": zg.grad, "a0": a0.grad, "zj": zjg.grad if zjg is not None else None}
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def check_ode_training(mk, case, G, tol, what=""):
    """the float64 walk, the fused run twice (a RuntimeWarning -- a walk under "auto" -- is an error), the judge of generic_cases"""
    ref_xs, ref = ode_train(mk, case, G, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = ode_train(mk, case, G, "cuda")
        _, again = ode_train(mk, case, G, "cuda")
    C.judge_ode_training(ref, got, again, xs, ref_xs, "_FusedOdeMs", tol, what)
    return got, ref


def check_dae_training(mk, case, G, Gi, tol, what=""):
    return C.check_dae_training(mk, case, G, Gi, "_FusedDaeMs", tol, what=what)


def rows_beyond_are_zero(grads, names, last_row, what):
    """a loss on the segments up to grid point `last_row` leaves the input gradients of every later row exactly zero"""
    for k in names:
        g = grads.get(k)
        if g is not None and g.shape[0] > last_row + 1:
            assert not g[last_row + 1:].any(), f"{what}: grad {k} is not zero beyond row {last_row}"

