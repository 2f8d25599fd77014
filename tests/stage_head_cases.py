"""Cases and yardsticks of the stage-wise algebraic heads (solver.algebraic = "stage"), shared by tests/test_stage_heads_host.py and
tests/test_gpu_stage_heads.py; a plain module, imported like helpers.py (not a conftest).

The semantics (neural_dae.FixedGridODESolver, `algebraic`): stage s >= 1 of sub-step j evaluates i_s = g(X_s, z_s, v_s) at its own argument
and at the externals of theta_s = (j + c_s) / n, and k_s = f(X_s, z_s, v_s, i_s); stage 0 reads the i the "step" walk reads.  `restate_dae`
says that once more without the package's step functions; `adjoint_by_hand` is the reverse recursion of DESIGN.md, "Stage-wise algebraic
heads on K0 / K5"; `order_problem` is the smooth forced DAE of the order gates; `forward_case` builds the GPU test's forward cases, whose
"stage" and "step" solutions the host test holds apart."""
import functools
import math

import torch
import torch.nn as nn

import generic_cases as C
from py_psnode_amd import models
from py_psnode_amd import neural_dae as nd
from py_psnode_amd.neural_dae.my_solvers import _LagWalk

SOLVERS = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4, "Heun2": nd.Heun2, "Kutta3": nd.Kutta3, "RK4Classic": nd.RK4Classic}
# the tableaus, written out: a[s][j] (j < s), b[s]
TABLEAUS = {
    "euler": (((),), (1.0,)),
    "midpoint": (((), (0.5,)), (0.0, 1.0)),
    "rk4": (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125)),
    "Heun2": (((), (1.0,)), (0.5, 0.5)),
    "Kutta3": (((), (0.5,), (-1.0, 2.0)), (1 / 6, 2 / 3, 1 / 6)),
    "RK4Classic": (((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
}
B0, T0 = 33, 6
EV = (0, 3)          # the grid rows that carry the events
METHODS = ("midpoint", "rk4", "Kutta3", "RK4Classic")
INTERP = ("linear", "lagrange")
# every form of K0 that has a DAE instance: register with QM 4 and (a leading block beyond 64 columns) QM 8, every image resident, some
# streamed, and the eight-layer loop
FWD_SHAPES = {"reg": (8, 2, 2, 2, (64, 64, 64), (64, 64, 64)), "reg_wide": (40, 2, 2, 2, (64, 64), (64, 64)),
              "resident": (8, 2, 2, 2, (96, 96), (96, 96)), "streamed": (8, 2, 2, 2, (128, 128, 128), (128, 128, 128)),
              "deep": (4, 2, 1, 2, (32,) * 5, (24,) * 5)}
# Eight times the builders' clock and externals, after tests/test_gpu_externals_linear.py::test_ode_forward: at the builders' own scale
# (h ~ n / 64) a frozen and a stage-wise head differ by about 1e-4, at four times by 1e-3 -- what the GPU test asks as a minimum of a kernel
# that does run the heads.  The five-layer MLPs of 32 / 24 units react to i an order of magnitude less than the others (3e-4 at this scale):
# the last layer of that case's head is multiplied by GAIN, which makes i, and with it the difference, that much larger.
SCALE = 8.0
GAIN = {"deep": 8.0}


def solver(name, n=1, externals="linear", algebraic="stage", mode="off", kernel="auto"):
    s = SOLVERS[name](substeps=n, externals=externals, algebraic=algebraic)
    s.fused, s.kernel = mode, kernel
    return s


@functools.lru_cache(maxsize=None)
def forward_case(shape, n, no_x=False, Tn=T0, B=B0, pad=False, events=True, scale=SCALE, seed=0):
    xd, zd, vd, idim, dh, ah = FWD_SHAPES[shape]
    t = C.dyadic_clock(Tn, B, n) * scale
    if pad:
        t = C.padded(t)
    case = C.dae_case(xd, zd, vd, idim, dh, ah, B, Tn, seed=23 + xd + n + seed, t=t, ev_rows=EV if events else (), perturb_x_init=True)
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    if shape in GAIN:
        last = [m for m in ae.modules() if isinstance(m, nn.Linear)][-1]
        with torch.no_grad():
            last.weight *= GAIN[shape]
            last.bias *= GAIN[shape]
    sc = lambda q: None if q is None else scale * q
    case = (de, ae, t, x, sc(z), sc(v), i, x_init, a0, ev, sc(zj), sc(vj))
    return C.without_x(case) if no_x else case


# ----------------------------------------------------------------------------- the stand-alone restatement
def _events_of(t, ev):
    """{step k: event column e} on trajectory 0's clock (the shared table)"""
    if ev is None:
        return {}
    out = {}
    for k in range(t.shape[0] - 1):
        hit = (ev[0, :, 0] == t[k, 0, 0]).nonzero().view(-1)
        if hit.numel():
            out[k] = int(hit[0])
    return out


def restate_dae(name, n, externals, case, tx=False):
    """The tableau step on x' = f(x, w(theta), g(x, w(theta))) with the package's interpolants (`_lin_ext`'s expression, `_LagWalk`), in the
    tensors' dtype.  Stage 0 of sub-step 0 reads the carried head of grid point k (which saw the dataset row x[k] under tx) or the
    event-time head at the running state; every other evaluation its own head."""
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    a, b = TABLEAUS[name]
    c = [sum(row) for row in a]
    f = lambda xx, zz, vv, ii: de(t0=None, xt=xx, zt=zz, vt=vv, it=ii, all_initial=a0)
    g = lambda xx, zz, vv: ae(xt=xx, zt=zz, vt=vv, all_initial=a0)
    hits = _events_of(t, ev)
    lag = None
    if externals == "lagrange":
        event = nd.DAE_Event()
        if ev is not None:
            event.set_event(ev, zj, vj)
        lag = _LagWalk(t, event.event_fn if ev is not None else None, event.jump_change_fn if ev is not None else None, (z, v))
    Tn = t.shape[0]
    cur = x_init
    cur_i = g(x[0] if tx else cur, z[0], v[0])
    xs, is_ = [cur], [cur_i]
    for k in range(Tn - 1):
        zl, vl = z[k], v[k]
        if k in hits:
            zl, vl = zj[:, hits[k]], vj[:, hits[k]]
            cur_i = g(cur, zl, vl)
        h = (t[k + 1] - t[k]) / n
        y = x[k] if tx else cur
        for j in range(n):
            if lag is not None:
                w = lag.ext_at(k, j, n)
            else:
                w = lambda cc, j=j: (zl + ((j + cc) / n) * (z[k + 1] - zl), vl + ((j + cc) / n) * (v[k + 1] - vl))
            ks = []
            for s in range(len(b)):
                X = y
                if s:
                    acc = None
                    for jj in range(s):
                        if a[s][jj] != 0.0:
                            acc = a[s][jj] * ks[jj] if acc is None else acc + a[s][jj] * ks[jj]
                    X = y + h * acc
                zs, vs = w(c[s])
                i_s = cur_i if (s == 0 and j == 0) else g(X, zs, vs)
                ks.append(f(X, zs, vs, i_s))
            acc = None
            for s in range(len(b)):
                if b[s] != 0.0:
                    acc = b[s] * ks[s] if acc is None else acc + b[s] * ks[s]
            y = y + h * acc
        cur = y
        cur_i = g(x[k + 1] if tx else cur, z[k + 1], v[k + 1])
        xs.append(cur)
        is_.append(cur_i)
    return torch.stack(xs), torch.stack(is_)


# ----------------------------------------------------------------------------- the reverse recursion, by hand (linear externals)
def adjoint_by_hand(name, n, case, Gx, Gi):
    """Gradients of sum(xs Gx) + sum(is Gi) w.r.t. x_init, z, v, the jump rows and all_initial under externals="linear",
    algebraic="stage": the forward sweep keeps every stage's (X_s, theta_s, i_s), the reverse sweep is written out -- only the VJPs of the two
    MLPs themselves come from autograd.  With lam the adjoint of a (sub-)step's result and h its step:
        gk_s = h b_s lam;   for s = S - 1 .. 0:   (dX, dw, di, da0) = VJP_f(X_s, w(theta_s), i_s; gk_s),
            s >= 1: (dX', dw', da0') = VJP_g(X_s, w(theta_s); di) joins dX, dw, da0;   s = 0: di is the adjoint of the i the step read,
            the left rows get (1 - theta_s) dw, the right rows theta_s dw, the start state dX, and gk_j += h a[s][j] dX for j < s."""
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    a, b = TABLEAUS[name]
    S = len(b)
    c = [sum(row) for row in a]
    hits = _events_of(t, ev)
    Tn = t.shape[0]

    def vjp_f(X, zz, vv, ii, gk):
        leaves = [q.detach().requires_grad_(True) for q in (X, zz, vv, ii, a0)]
        with torch.enable_grad():
            out = de(t0=None, xt=leaves[0], zt=leaves[1], vt=leaves[2], it=leaves[3], all_initial=leaves[4])
        return torch.autograd.grad(out, leaves, gk)

    def vjp_g(X, zz, vv, gi):
        leaves = [q.detach().requires_grad_(True) for q in (X, zz, vv, a0)]
        with torch.enable_grad():
            out = ae(xt=leaves[0], zt=leaves[1], vt=leaves[2], all_initial=leaves[3])
        return torch.autograd.grad(out, leaves, gi)

    with torch.no_grad():
        # forward sweep
        g = lambda xx, zz, vv: ae(xt=xx, zt=zz, vt=vv, all_initial=a0)
        f = lambda xx, zz, vv, ii: de(t0=None, xt=xx, zt=zz, vt=vv, it=ii, all_initial=a0)
        cur, cur_i = x_init, g(x_init, z[0], v[0])
        tape = []          # per interval: (zl, vl, h, [per sub-step: (y, [(X_s, theta_s, i_s)])], state the event head saw)
        for k in range(Tn - 1):
            zl, vl = (zj[:, hits[k]], vj[:, hits[k]]) if k in hits else (z[k], v[k])
            x_head = cur
            if k in hits:
                cur_i = g(cur, zl, vl)
            h = (t[k + 1] - t[k]) / n
            y, subs = cur, []
            for j in range(n):
                ks, stages = [], []
                for s in range(S):
                    X = y
                    for jj in range(s):
                        if a[s][jj] != 0.0:
                            X = X + h * a[s][jj] * ks[jj]
                    th = (j + c[s]) / n
                    zs, vs = zl + th * (z[k + 1] - zl), vl + th * (v[k + 1] - vl)
                    i_s = cur_i if (s == 0 and j == 0) else g(X, zs, vs)
                    ks.append(f(X, zs, vs, i_s))
                    stages.append((X, th, i_s))
                subs.append((y, stages))
                for s in range(S):
                    if b[s] != 0.0:
                        y = y + h * b[s] * ks[s]
            tape.append((zl, vl, h, subs, x_head))
            cur, cur_i = y, g(y, z[k + 1], v[k + 1])
        xs_last = cur
        # reverse sweep
        gz, gv, ga0 = torch.zeros_like(z), torch.zeros_like(v), torch.zeros_like(a0)
        gzj = torch.zeros_like(zj) if zj is not None else None
        gvj = torch.zeros_like(vj) if vj is not None else None
        lam, gi_c = Gx[Tn - 1].clone(), Gi[Tn - 1].clone()
        x_next = xs_last
        for k in range(Tn - 2, -1, -1):
            zl, vl, h, subs, x_head = tape[k]
            dX, dz, dv, da = vjp_g(x_next, z[k + 1], v[k + 1], gi_c)          # the head at grid point k + 1
            lam = lam + dX
            gz[k + 1] += dz
            gv[k + 1] += dv
            ga0 += da
            gzl, gvl = torch.zeros_like(zl), torch.zeros_like(vl)
            gi0 = None
            for j in range(n - 1, -1, -1):
                y, stages = subs[j]
                gk = [h * b[s] * lam for s in range(S)]
                gy = lam.clone()
                for s in range(S - 1, -1, -1):
                    X, th, i_s = stages[s]
                    zs, vs = zl + th * (z[k + 1] - zl), vl + th * (v[k + 1] - vl)
                    dX, dz, dv, di, da = vjp_f(X, zs, vs, i_s, gk[s])
                    ga0 += da
                    if s >= 1 or j >= 1:          # this evaluation's own head (s = 0, j >= 1: the in-interval head in front of the sub-step)
                        hX, hz, hv, ha = vjp_g(X, zs, vs, di)
                        dX, dz, dv = dX + hX, dz + hz, dv + hv
                        ga0 += ha
                    else:
                        gi0 = di
                    gzl += (1.0 - th) * dz
                    gvl += (1.0 - th) * dv
                    gz[k + 1] += th * dz
                    gv[k + 1] += th * dv
                    gy = gy + dX
                    for jj in range(s):
                        if a[s][jj] != 0.0:
                            gk[jj] = gk[jj] + h * a[s][jj] * dX
                lam = gy
            if k in hits:          # the step read the event-time head at the running state and the jumped rows
                hX, hz, hv, ha = vjp_g(x_head, zl, vl, gi0)
                lam = lam + hX
                ga0 += ha
                gzj[:, hits[k]] += gzl + hz
                gvj[:, hits[k]] += gvl + hv
                gi_c = Gi[k].clone()
            else:
                gz[k] += gzl
                gv[k] += gvl
                gi_c = Gi[k] + gi0
            lam = lam + Gx[k]
            x_next = subs[0][0]
        dX, dz, dv, da = vjp_g(x_init, z[0], v[0], gi_c)
        gz[0] += dz
        gv[0] += dv
        ga0 += da
        return {"x_init": lam + dX, "z": gz, "v": gv, "a0": ga0, "zj": gzj, "vj": gvj}


# ----------------------------------------------------------------------------- the order gates: a smooth forced DAE
def order_problem(points, B=3):
    """Tanh DE / AE, x 3 / z 2 / v 2 / i 2, hidden 16 x 16; z(t) = 0.5 sin(3 t + phi), v(t) = 0.5 cos(2 t + psi) sampled on `points` points of
    [0, 1] (the forcing of tests/test_externals_lagrange_host.py, for z and v)."""
    torch.manual_seed(5)
    n = 3 + 2 + 2 + 2
    de = models.DAE_DE_Func(n, (16, 16), 3, activation=nn.Tanh).double()
    ae = models.AE_Func(n + 3 + 2 + 2, (16, 16), 2, activation=nn.Tanh).double()
    g = torch.Generator().manual_seed(6)
    x0 = 0.5 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    phi = torch.rand(B, 2, generator=g, dtype=torch.float64) * 3.0
    psi = torch.rand(B, 2, generator=g, dtype=torch.float64) * 3.0
    t = torch.linspace(0.0, 1.0, points, dtype=torch.float64).view(-1, 1, 1).repeat(1, B, 1)
    z = 0.5 * torch.sin(3.0 * t + phi.unsqueeze(0))
    v = 0.5 * torch.cos(2.0 * t + psi.unsqueeze(0))
    x = torch.zeros(points, B, 0, dtype=torch.float64)
    i = torch.zeros(points, B, 2, dtype=torch.float64)
    a0 = torch.cat((x0, z[0], v[0], i[0]), -1)
    return de, ae, t, x, z, v, i, x0, a0, None, None, None


def order_run(s, points):
    s.fused = "off"
    with torch.no_grad():
        return C.run_dae(s, *order_problem(points))[0]


def observed_orders(make, grids=(9, 17, 33, 65), fine=1025):
    """(errors, orders per doubling) of the solver `make()` on `grids` against the same solver on `fine` points (16 x the finest grid)."""
    ref = order_run(make(), fine)
    errs = [float((order_run(make(), p) - ref[::(fine - 1) // (p - 1)]).abs().max()) for p in grids]
    return errs, [math.log2(errs[k] / errs[k + 1]) for k in range(len(errs) - 1)]
