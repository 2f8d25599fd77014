"""Cases and the stand-alone restatement for the Runge-Kutta-Chebyshev tests (tests/test_rkc_host.py, tests/test_gpu_rkc.py); a plain
module, imported like helpers.py.

The restatement (`table_loop`, `ref_ode`, `ref_dae`) is written from the formulas alone and shares no code with the package: the host
suite pins the package's walk to it within 1e-12, the GPU suite reads the stage rows Y_j from it.

The GPU cases are built here so that the host suite can measure their rounding floor d -- the distance, on the same case, between the
package's fp32 walk on the CPU and its fp64 walk -- and assert 4 d <= helpers.TOL_GPU for every case of s <= 5: the plain TOL_GPU gate is
then the one that binds on the device.  Grid step 0.1 (times 1/2, 1 or 2 per trajectory), B = 33, T = 6, events at steps 0 and 3."""
import numpy as np
import torch

import generic_cases as C
from py_psnode_amd import neural_dae as nd

B0, T0 = 33, 6
EV = (0, 3)
METHODS = [(1, 1), (1, 2), (1, 3), (1, 5), (2, 2), (2, 3), (2, 5)]      # (order, stages) of the forward cases
TRAIN_METHODS = [(1, 2), (1, 5), (2, 3)]
# K5's register, streamed (LDS and global accumulators), staged (132 input columns) and wide-input paths
K5_ODE_SHAPES = [(8, 2, 64, 3), (8, 2, 96, 2), (8, 2, 128, 3), (44, 0, 40, 2), (32, 4, 48, 2)]
WIDE = [(1, 8), (1, 16)]      # the two cases that may use the widened gate max(TOL_GPU, 4 d)


# The seeds of the cases whose first draw rounded above the floor the plain gate needs (4 d <= TOL_GPU with d the package's own fp32 walk
# against its fp64 walk on the CPU, tests/test_rkc_host.py): the draw is part of the case, so those cases take a later one.  (The floor is
# the recurrence's own rounding and does not move with the weights or the step: scaling the weights of the RKC2(stages=5) forward cases
# by 0.25 / 0.05 leaves d at 1.9e-6 .. 2.5e-6 / 2.4e-6 .. 3.2e-6.  The search kept draws of d <= 2.0e-6, a fifth under the bound, and the
# host assertion fails loudly if a change of generic_cases' builders moves a draw.)
SEED_BUMP = {("ode_fwd", "streamed", 1, 5): 1, ("dae_fwd", "x5z4v6i6", 1, 5): 2, ("ode_fwd", "reg", 2, 5): 3, ("ode_fwd", "streamed", 2, 5): 3,
             ("ode_fwd", "wide", 2, 5): 9, ("ode_fwd", "deep", 2, 5): 2, ("dae_fwd", "x8z2v2i2", 2, 5): 1, ("dae_train", "deep", 1, 2): 4,
             ("dae_train", "deep", 1, 5): 1, ("ode_train", 8, 96, 2, 3): 1}


def _seed(base, *key):
    return base + 1000 * SEED_BUMP.get(key, 0)


def solver(order, stages, mode="require", kernel="auto", damping=None):
    s = (nd.RKC1 if order == 1 else nd.RKC2)(stages, damping)
    s.fused, s.kernel = mode, kernel
    return s


def clock(Tn=T0, B=B0, dtype=torch.float32):
    """t[k] = 0.1 k, scaled per trajectory by 1/2, 1 or 2 (trajectory 0, whose clock decides the events: 1)"""
    t = (torch.arange(Tn, dtype=dtype) * 0.1).view(Tn, 1, 1).repeat(1, B, 1)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=dtype)[torch.arange(B) % 3].view(1, B, 1)
    scale[0, 0, 0] = 1.0
    return t * scale


def ode_fwd_case(shape, order, stages, B=B0, Tn=T0, pad=False, act=None):
    xd, zd, hidden = C.ODE_FWD_SHAPES[shape]
    t = clock(Tn, B)
    if pad:
        t = C.padded(t)
    kw = {} if act is None else dict(act=act)
    return C.ode_case(xd, zd, hidden, B, Tn, seed=_seed(100 + 7 * xd + len(hidden) + 10 * order + stages, "ode_fwd", shape, order, stages), t=t, ev_rows=EV, **kw)


def dae_fwd_case(shape, order, stages, no_x=False):
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES[shape]
    case = C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=_seed(200 + xd + 10 * order + stages, "dae_fwd", shape, order, stages), t=clock(), ev_rows=EV)
    return C.without_x(case) if no_x else case


def ode_train_case(xd, zd, H, nh, order, stages, events=True, act=None):
    kw = {} if act is None else dict(act=act)
    return C.ode_case(xd, zd, (H,) * nh, B0, T0, seed=_seed(300 + xd + 10 * order + stages, "ode_train", xd, H, order, stages), t=clock(), ev_rows=EV if events else (), **kw)


def dae_train_case(shape, order, stages, events=True, **kw):
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES[shape]
    return C.dae_case(xd, zd, vd, idim, dh, ah, B0, T0, seed=_seed(400 + xd + 10 * order + stages, "dae_train", shape, order, stages), t=clock(), ev_rows=EV if events else (), **kw)


def floor_d(got32, ref64):
    """d of one tensor: max |fp32 walk - fp64 walk| over the tensor max of the fp64 walk (the scale of generic_cases.close)"""
    ref64 = ref64.detach().double()
    return float((got32.detach().double() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-6)


def ode_floor(order, stages, case, tx=False):
    """d of xs on an ODE case: the package's fp32 walk on the CPU against its fp64 walk"""
    de, t, x, z, ev, zj = case
    with torch.no_grad():
        got = C.run_ode(solver(order, stages, "off"), de, t, x, z, torch.cat((x[0], z[0]), -1), ev, zj, tx)
    return floor_d(got, C.ode_walk64(solver(order, stages, "off"), de, t, x, z, ev, zj, tx))


def dae_floor(order, stages, case, tx=False, ti=False):
    with torch.no_grad():
        got = C.run_dae(solver(order, stages, "off"), *case, tx, ti)
    ref = C.dae_walk64(solver(order, stages, "off"), case, tx, ti)
    return max(floor_d(got[0], ref[0]), floor_d(got[1], ref[1]))


# ----------------------------------------------------------------------------- the restatement
def table_loop(s, order, eps=None, consistent=True):
    """The coefficients from the Chebyshev three-term recurrences, looped with numpy scalars: dict of lists indexed by the stage j (1-based;
    entry 0 unused), rounded to fp32 except c and beta."""
    f = np.float64
    eps = f(0.05 if order == 1 else 2.0 / 13.0) if eps is None else f(eps)
    w0 = f(1.0) + eps / f(s * s)
    T, D, E = [f(1.0), w0], [f(0.0), f(1.0)], [f(0.0), f(0.0)]
    for j in range(2, s + 1):
        T.append(f(2.0) * w0 * T[-1] - T[-2])
        D.append(f(2.0) * T[j - 1] + f(2.0) * w0 * D[-1] - D[-2])
        E.append(f(4.0) * D[j - 1] + f(2.0) * w0 * E[-1] - E[-2])
    out = {k: [0.0] * (s + 1) for k in ("kappa", "mu", "nu", "mu_t", "gamma_t", "c")}
    if order == 1:
        w1 = T[s] / D[s]
        out["mu_t"][1] = w1 / w0
        for j in range(2, s + 1):
            out["mu"][j] = f(2.0) * w0 * T[j - 1] / T[j]
            out["nu"][j] = -T[j - 2] / T[j]
            out["mu_t"][j] = f(2.0) * w1 * T[j - 1] / T[j]
        for j in range(1, s + 1):
            out["c"][j] = T[s] * D[j] / (D[s] * T[j])
        out["beta"] = (f(1.0) + w0) * D[s] / T[s]
    else:
        w1 = D[s] / E[s]
        b = [None, None] + [E[j] / (D[j] * D[j]) for j in range(2, s + 1)]
        b[0] = b[1] = b[2]
        out["mu_t"][1] = b[1] * w1
        for j in range(2, s + 1):
            out["mu"][j] = f(2.0) * b[j] * w0 / b[j - 1]
            out["nu"][j] = -b[j] / b[j - 2]
            out["mu_t"][j] = f(2.0) * b[j] * w1 / b[j - 1]
            out["gamma_t"][j] = -(f(1.0) - b[j - 1] * T[j - 1]) * out["mu_t"][j]
            out["kappa"][j] = f(1.0) - out["mu"][j] - out["nu"][j]
            out["c"][j] = D[s] * E[j] / (E[s] * D[j])
        out["c"][1] = out["c"][2] / D[2]
        out["beta"] = (f(1.0) + w0) * E[s] / D[s]
    for k in ("kappa", "mu", "nu", "mu_t", "gamma_t"):
        out[k] = [float(np.float32(q)) for q in out[k]]
    # consistency of the rounded method, kappa_j + mu_j + nu_j = 1 exactly: the last of the three from the rounded others
    for j in range(2, s + 1 if consistent else 0):
        if order == 1:
            out["nu"][j] = 1.0 - out["mu"][j]
        else:
            out["kappa"][j] = 1.0 - out["mu"][j] - out["nu"][j]
    out["c"] = [float(q) for q in out["c"]]
    out["beta"] = float(out["beta"])
    return out


def ref_step(tab, s, F, head, y0, h, i0, stages_out=None):
    """One step from y0: F(y, i) the right-hand side, head(y) -> i or None (i0 for every stage).  Appends Y_1 .. Y_{s-1} to stages_out."""
    f0 = F(y0, i0)
    ys = [y0, y0 + (tab["mu_t"][1] * h) * f0]
    for j in range(2, s + 1):
        i_j = i0 if head is None else head(ys[j - 1])
        terms = [(tab["kappa"][j], ys[0]), (tab["mu"][j], ys[j - 1]), (tab["nu"][j], ys[j - 2])]
        acc = None
        for cf, y in terms:
            if cf != 0.0:
                acc = cf * y if acc is None else acc + cf * y
        acc = acc + (tab["mu_t"][j] * h) * F(ys[j - 1], i_j)
        if tab["gamma_t"][j] != 0.0:
            acc = acc + (tab["gamma_t"][j] * h) * f0
        ys.append(acc)
    if stages_out is not None:
        stages_out.append(ys[1:s])
    return ys[s]


def _event_of(t, ev, k):
    """the index of the event at step k (trajectory 0's clock), or None"""
    if ev is None:
        return None
    hit = (ev[0, :, 0] == t[k, 0, 0]).nonzero().view(-1)
    return int(hit[0]) if hit.numel() else None


def ref_ode(order, s, de, t, x, z, ev, zj, tx=False, stages_out=None):
    tab = table_loop(s, order)
    a0 = torch.cat((x[0], z[0]), -1)
    xs, cur = [x[0]], x[0]
    for k in range(t.shape[0] - 1):
        e = _event_of(t, ev, k)
        zk = z[k] if e is None else zj[:, e]
        F = lambda y, i, zk=zk, k=k: de(t0=t[k], xt=y, zt=zk, all_initial=a0)
        cur = ref_step(tab, s, F, None, x[k] if tx else cur, t[k + 1] - t[k], None, stages_out)
        xs.append(cur)
    return torch.stack(xs)


def ref_dae(order, s, case, tx=False, ti=False, stages_out=None):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    tab = table_loop(s, order)
    g = lambda y, zz, vv: ae(xt=y, zt=zz, vt=vv, all_initial=a0)
    cur_x, cur_i = x_init, g(x[0] if tx else x_init, z[0], v[0])
    xs, is_ = [cur_x], [cur_i]
    for k in range(t.shape[0] - 1):
        e = _event_of(t, ev, k)
        zk, vk = (z[k], v[k]) if e is None else (zj[:, e], vj[:, e])
        if e is not None:
            cur_i = g(cur_x, zk, vk)
        F = lambda y, ii, zk=zk, vk=vk, k=k: de(t0=t[k], xt=y, zt=zk, vt=vk, it=ii, all_initial=a0)
        head = None if ti else (lambda y, zk=zk, vk=vk: g(y, zk, vk))
        cur_x = ref_step(tab, s, F, head, x[k] if tx else cur_x, t[k + 1] - t[k], i[k] if ti else cur_i, stages_out)
        cur_i = g(x[k + 1] if tx else cur_x, z[k + 1], v[k + 1])
        xs.append(cur_x)
        is_.append(cur_i)
    return torch.stack(xs), torch.stack(is_)


# ----------------------------------------------------------------------------- training on the CPU in a given dtype (the floor of the gradients)
def ode_train_dtype(solver, case, G, dtype, tx=False):
    """generic_cases.ode_train on the CPU through the walk (solver("off")) in `dtype`: -> xs, {name: grad}"""
    de, t, x, z, ev, zj = case
    cv = lambda a: None if a is None else a.to(dtype)
    m = C.deepcopy(de).to(dtype)
    xg, zg = cv(x).clone(), cv(z).clone().requires_grad_(True)
    if not tx:
        xg.requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = cv(zj).clone().requires_grad_(True) if zj is not None else None
    xs = C.run_ode(solver("off"), m, cv(t), xg, zg, a0, cv(ev), zjg, tx)
    (xs * cv(G)).sum().backward()
    grads = {"z": zg.grad, "a0": a0.grad, "zj": zjg.grad if zjg is not None else None}
    if not tx:
        grads["x"] = xg.grad
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def dae_train_dtype(solver, case, G, Gi, dtype, tx=False, ti=False):
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    cv = lambda a: None if a is None else a.to(dtype)
    de, ae = C.deepcopy(de).to(dtype), C.deepcopy(ae).to(dtype)
    leaf = lambda a: None if a is None else cv(a).clone().requires_grad_(True)
    xi, zg, vg, a0g, zjg, vjg = leaf(x_init), leaf(z), leaf(v), leaf(a0), leaf(zj), leaf(vj)
    xs, is_ = C.run_dae(solver("off"), de, ae, cv(t), cv(x), zg, vg, cv(i), xi, a0g, cv(ev), zjg, vjg, tx, ti)
    ((xs * cv(G)).sum() + (is_ * cv(Gi)).sum()).backward()
    grads = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad, "zj": zjg.grad if zjg is not None else None,
             "vj": vjg.grad if vjg is not None else None}
    grads.update({f"de{k}": p.grad for k, p in enumerate(de.parameters())})
    grads.update({f"ae{k}": p.grad for k, p in enumerate(ae.parameters())})
    return xs, is_, grads


def grad_floors(g32, g64):
    """{name: d} of the gradients both runs have"""
    return {k: floor_d(g32[k], g64[k]) for k in g64 if g64[k] is not None and g64[k].numel()}
