"""Cases, runners and yardsticks of the per-trajectory event tests (ODE_Event / DAE_Event with per_trajectory=True; the _pev builds of
K0 / K5); a plain module, imported like generic_cases.py, whose shapes, cases and gates it reuses.  generic_cases.run_ode / run_dae build
the shared-rule event objects themselves, so the runners here are this module's own.

Event patterns (B = 33, T = 6, nE = 2, NaN = "no event in this column"), by the step(s) at which trajectory b jumps:
  mixed      b % 5 == 0: none (trajectory 0 among them) | 1: step 0 | 2: step 3 | 3: steps 0 and 3, stored in reversed column order |
             4: step 2, in column 1 with column 0 NaN
  blocks     trajectories 0-15 none, 16-31 step 1, trajectory 32 step 4: a workgroup without a hit at a step where another has one, the
             ragged workgroup's lone trajectory, the last step
  only_zero  trajectory 0 alone has an event, at step 2 (the shared rule would jump everyone)

The yardstick of trajectory b: the fp32 CPU oracle (oracle/psnode_oracle.py, which knows the shared rule only) on the one-trajectory batch
[b : b + 1] -- there b's own clock and list decide; with sub-steps on the refined one-trajectory problem (generic_cases.refine_*)."""
from copy import deepcopy

import torch

import generic_cases as C
from helpers import REL_FLOOR, TOL_GPU
from oracle import psnode_oracle as O
from py_psnode_amd import neural_dae as nd

B0, T0, NE = 33, 6, 2
PATTERNS = ("mixed", "blocks", "only_zero")
ORACLE_NAME = {"Euler": "euler", "Midpoint": "midpoint", "RK4": "rk4"}


def clock(Tn=T0, B=B0, pad=False, seed=77):
    """generic_cases.ragged_clock on a grid of dt = 0.1 (times 0.5 .. 1.5 per trajectory): one interval's jump has to move a trajectory by
    100 x TOL_GPU of its size (`sensitive_ode_case`), which the 0.01 grid of the other families' cases does not give"""
    return C.ragged_clock(Tn, B, torch.Generator().manual_seed(seed), pad, dt=0.1)


def hits(pattern, b):
    """[(column, step), ...] of trajectory b"""
    if pattern == "mixed":
        return [[], [(0, 0)], [(0, 3)], [(0, 3), (1, 0)], [(1, 2)]][b % 5]
    if pattern == "blocks":
        return [] if b < 16 else ([(0, 1)] if b < 32 else [(0, 4)])
    if pattern == "only_zero":
        return [(0, 2)] if b == 0 else []
    raise KeyError(pattern)


def event_times(pattern, t):
    """ev [B, nE, 1]: t[step, b] in the columns `hits` names (steps beyond the grid dropped), NaN elsewhere"""
    Tn, B = t.shape[0], t.shape[1]
    ev = torch.full((B, NE, 1), float("nan"), dtype=t.dtype)
    for b in range(B):
        for col, step in hits(pattern, b):
            if step < Tn - 1:
                ev[b, col, 0] = t[step, b, 0]
    return ev


def step_table(pattern, Tn, B):
    """int [T-1, B]: the column that fires, -1 = none -- `hits` restated as the table the kernels read"""
    tab = torch.full((max(Tn - 1, 0), B), -1, dtype=torch.int32)
    for b in range(B):
        for col, step in hits(pattern, b):
            if step < Tn - 1:
                tab[step, b] = col
    return tab


def differs_from_trajectory_0(pattern, Tn, B):
    """bool[B]: trajectory b's event steps are not trajectory 0's (the shared rule computes something else for it)"""
    steps = lambda b: sorted(s for _, s in hits(pattern, b) if s < Tn - 1)
    return torch.tensor([steps(b) != steps(0) for b in range(B)])


def per_traj_err(y, ref):
    """[B]: max abs error of trajectory b / max abs value of the reference trajectory (helpers.traj_rel_err before its max)"""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    return (y - ref).abs().amax((0, 2)) / ref.abs().amax((0, 2)).clamp_min(REL_FLOOR)


def with_pattern(case, pattern, scale=1.0, dae=False):
    """the case with the pattern's event times on its own clock and jump rows for nE columns, drawn from a generator of their own"""
    g = torch.Generator().manual_seed(1234)
    t = case[2] if dae else case[1]
    B = t.shape[1]
    ev = event_times(pattern, t)
    if dae:
        zd, vd = case[4].shape[-1], case[5].shape[-1]
        return case[:9] + (ev, scale * torch.randn(B, NE, zd, generator=g), scale * torch.randn(B, NE, vd, generator=g))
    zd = case[3].shape[-1]
    return case[:4] + (ev, scale * torch.randn(B, NE, zd, generator=g))


# ----------------------------------------------------------------------------- runners
def run_ode(solver, de, t, x, z, a0, ev, zj, tx=False, per_trajectory=True):
    event = nd.ODE_Event(per_trajectory=per_trajectory)
    if ev is not None:
        event.set_event(ev, zj)
    return solver.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0, event_fn=event.event_fn, jump_change_fn=event.jump_change_fn,
                                input_true_x=tx)


def run_dae(solver, de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, tx=False, ti=False, per_trajectory=True):
    event = nd.DAE_Event(per_trajectory=per_trajectory)
    if ev is not None:
        event.set_event(ev, zj, vj)
    return solver.integrate_DAE(x_init=x_init, x_func=de, i_func=ae, t=t, x=x, z=z, v=v, i=i, all_initial=a0, event_fn=event.event_fn,
                                jump_change_fn=event.jump_change_fn, input_true_x=tx, input_true_i=ti)


def ode_walk64(solver, case, tx=False):
    de, t, x, z, ev, zj = case
    with torch.no_grad():
        return run_ode(solver, deepcopy(de).double(), C.to64(t), C.to64(x), C.to64(z), torch.cat((C.to64(x)[0], C.to64(z)[0]), -1),
                       C.to64(ev), C.to64(zj), tx)


def ode_gpu(solver, case, tx=False, per_trajectory=True):
    de, t, x, z, ev, zj = case
    xc, zc = x.cuda(), z.cuda()
    with torch.no_grad():
        return run_ode(solver, deepcopy(de).cuda(), t.cuda(), xc, zc, torch.cat((xc[0], zc[0]), -1), C.to_cuda(ev), C.to_cuda(zj), tx,
                       per_trajectory)


def dae_walk64(solver, case, tx=False, ti=False):
    with torch.no_grad():
        return run_dae(solver, deepcopy(case[0]).double(), deepcopy(case[1]).double(), *(C.to64(q) for q in case[2:]), tx, ti)


def dae_gpu(solver, case, tx=False, ti=False, per_trajectory=True):
    with torch.no_grad():
        return run_dae(solver, deepcopy(case[0]).cuda(), deepcopy(case[1]).cuda(), *(C.to_cuda(q) for q in case[2:]), tx, ti, per_trajectory)


# ----------------------------------------------------------------------------- the yardstick: the oracle, one trajectory at a time
def oracle_ode(method, case, n=1, tx=False):
    """[T, B, xd]: trajectory b from O.integrate_ode on the batch [b : b + 1] (n > 1: on its n-times refined problem, read at rows ::n)"""
    de, t, x, z, ev, zj = case
    layers = C.layers_of(de.x_dot)
    outs = []
    with torch.no_grad():
        for b in range(t.shape[1]):
            s = slice(b, b + 1)
            tb, xb, zb, evb, zjb = t[:, s], x[:, s], z[:, s], ev[s], zj[s]
            a0 = torch.cat((xb[0], zb[0]), -1)
            if n == 1:
                outs.append(O.integrate_ode(method, layers, tb, xb, zb, a0, evb, zjb, tx))
            else:
                assert not tx, "the refined problem has no dataset rows between the grid points"
                tf, zf = C.refine_clock(tb, n), C.refine_rows(zb, n, tb, evb, zjb)
                xf = torch.zeros(tf.shape[0], 1, x.shape[-1])
                xf[0] = xb[0]
                outs.append(O.integrate_ode(method, layers, tf, xf, zf, a0, evb, zjb)[::n])
    return torch.cat(outs, 1)


def oracle_ode_shared(method, case, tx=False):
    """the shared rule on the same batch: trajectory 0's clock and list decide for everyone"""
    de, t, x, z, ev, zj = case
    with torch.no_grad():
        return O.integrate_ode(method, C.layers_of(de.x_dot), t, x, z, torch.cat((x[0], z[0]), -1), ev, zj, tx)


def oracle_dae(method, case, n=1, tx=False, ti=False):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    dl, al = C.layers_of(de.x_dot), C.layers_of(ae.i_calculator)
    xs, is_ = [], []
    with torch.no_grad():
        for b in range(t.shape[1]):
            s = slice(b, b + 1)
            tb, xb, zb, vb, ib, evb, zjb, vjb = t[:, s], x[:, s], z[:, s], v[:, s], i[:, s], ev[s], zj[s], vj[s]
            if n == 1:
                ox, oi = O.integrate_dae(method, dl, al, x_init[s], tb, xb, zb, vb, ib, a0[s], evb, zjb, vjb, tx, ti)
            else:
                assert not (tx or ti)
                tf = C.refine_clock(tb, n)
                zf, vf = C.refine_rows(zb, n, tb, evb, zjb), C.refine_rows(vb, n, tb, evb, vjb)
                xf, i_f = torch.zeros(tf.shape[0], 1, x.shape[-1]), torch.zeros(tf.shape[0], 1, i.shape[-1])
                ox, oi = O.integrate_dae(method, dl, al, x_init[s], tf, xf, zf, vf, i_f, a0[s], evb, zjb, vjb)
                ox, oi = ox[::n], oi[::n]
            xs.append(ox)
            is_.append(oi)
    return torch.cat(xs, 1), torch.cat(is_, 1)


def oracle_dae_shared(method, case, tx=False, ti=False):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    with torch.no_grad():
        return O.integrate_dae(method, C.layers_of(de.x_dot), C.layers_of(ae.i_calculator), x_init, t, x, z, v, i, a0, ev, zj, vj, tx, ti)


def sensitive_ode_case(case, pattern, method="euler"):
    """`with_pattern` with the jump rows scaled up until, by the ORACLE alone, every trajectory whose event steps differ from trajectory 0's
    lies at least 100 x TOL_GPU from the shared-rule result -- a condition on the case, asserted here.  -> (case, the differing mask)"""
    Tn, B = case[1].shape[0], case[1].shape[1]
    differ = differs_from_trajectory_0(pattern, Tn, B)
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0):
        c = with_pattern(case, pattern, scale)
        gap = per_traj_err(oracle_ode(method, c), oracle_ode_shared(method, c))
        if bool((gap[differ] >= 100 * TOL_GPU).all()):
            return c, differ
    raise AssertionError(f"{pattern}: no jump scale separates the two rules: {gap[differ].min():.3e}")


def sensitive_dae_case(case, pattern, method="euler"):
    Tn, B = case[2].shape[0], case[2].shape[1]
    differ = differs_from_trajectory_0(pattern, Tn, B)
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0):
        c = with_pattern(case, pattern, scale, dae=True)
        gap = per_traj_err(oracle_dae(method, c)[0], oracle_dae_shared(method, c)[0])
        if bool((gap[differ] >= 100 * TOL_GPU).all()):
            return c, differ
    raise AssertionError(f"{pattern}: no jump scale separates the two rules: {gap[differ].min():.3e}")


# ----------------------------------------------------------------------------- training (generic_cases.ode_train / dae_train with this module's runners)
def ode_train(solver, case, G, dev, tx=False):
    """One forward + backward of loss = sum(xs * G): float32 under solver("require") on "cuda", float64 under solver("off") on "cpu".
    Leaves: z, all_initial, the jump rows, the parameters, and x unless teacher-forced.  -> xs, {name: grad}"""
    de, t, x, z, ev, zj = case
    dtype, cv = C._cv(dev)
    m = deepcopy(de).to(device=dev, dtype=dtype)
    xg, zg = cv(x), cv(z).requires_grad_(True)
    if not tx:
        xg.requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = cv(zj).requires_grad_(True)
    xs = run_ode(solver("require" if dev == "cuda" else "off"), m, cv(t), xg, zg, a0, cv(ev), zjg, tx)
    (xs * cv(G)).sum().backward()
    grads = {"z": zg.grad, "a0": a0.grad, "zj": zjg.grad}
    if not tx:
        grads["x"] = xg.grad
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def dae_train(solver, case, G, Gi, dev, tx=False, ti=False):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    dtype, cv = C._cv(dev)
    de, ae = deepcopy(de).to(device=dev, dtype=dtype), deepcopy(ae).to(device=dev, dtype=dtype)
    leaf = lambda a: cv(a).requires_grad_(True)
    xi, zg, vg, a0g, zjg, vjg = leaf(x_init), leaf(z), leaf(v), leaf(a0), leaf(zj), leaf(vj)
    xs, is_ = run_dae(solver("require" if dev == "cuda" else "off"), de, ae, cv(t), cv(x), zg, vg, cv(i), xi, a0g, cv(ev), zjg, vjg, tx, ti)
    ((xs * cv(G)).sum() + (is_ * cv(Gi)).sum()).backward()
    grads = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad, "zj": zjg.grad, "vj": vjg.grad}
    grads.update({f"de{k}": p.grad for k, p in enumerate(de.parameters())})
    grads.update({f"ae{k}": p.grad for k, p in enumerate(ae.parameters())})
    return xs, is_, grads
