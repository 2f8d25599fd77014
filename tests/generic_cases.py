"""Cases, runs, training checks and gates shared by the tests of the K0 / K5 option families (activations, pre-activation kinds, tableaus,
sub-steps, linear externals, teacher forcing); a plain module, imported like helpers.py (not a conftest).  Each test file keeps what is its
own -- solver factory, event rows, cotangent seeds, tolerance, grad_fn prefix -- and passes it in; nothing here has a per-file default.

Time-major throughout: t [T,B,1], x [T,B,xd], events ev [B,nE,1] with jump rows zj [B,nE,zd] (vj [B,nE,vd]).  An ODE case is
(de, t, x, z, ev, zj), a DAE case (de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj).

Refinement of a problem (sub-steps): clock t'[kn + j] = t[k] + j h, h = (t[k+1] - t[k]) / n in the clock's own dtype; externals
z'[kn + j] = z[k]; on an interval that starts with an event the rows j >= 1 carry the jumped values (the event itself fires at row kn only:
the refined clock meets an event time nowhere else).  The n-times refined problem's one-step-per-interval solution, read at rows ::n, is
what `substeps = n` computes on the coarse problem (no teacher forcing)."""
import warnings
from copy import deepcopy

import torch
import torch.nn as nn

from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import models
from py_psnode_amd import neural_dae as nd

# ----------------------------------------------------------------------------- shapes
# every form of K0: register, streamed, wide register, the eight-layer instances
ODE_FWD_SHAPES = {"reg": (8, 2, (64, 64, 64)), "streamed": (20, 3, (96, 96)), "wide": (20, 3, (128, 128)), "deep": (8, 2, (32,) * 7)}
DAE_SHAPES = {"x8z2v2i2": (8, 2, 2, 2, (64, 64, 64), (64, 64, 64)), "x5z4v6i6": (5, 4, 6, 6, (64, 64, 64), (64, 64, 64))}
# the shape list of tests/test_gpu_backward.py::test_generic_backward_kernel_ode: K5's register path and its edges, the streamed path with
# LDS and (hidden 128) global accumulators, the staged path (132 input columns)
K5_ODE_SHAPES = [(8, 2, 64, 3), (16, 16, 16, 1), (5, 3, 24, 2), (8, 2, 128, 3), (8, 2, 32, 3), (20, 2, 64, 3), (32, 4, 48, 2), (17, 0, 33, 3),
                 (40, 2, 64, 1), (8, 2, (33, 17, 64), 3), (5, 3, (16, 64, 16), 3), (44, 0, 40, 2), (8, 2, 64, 4)]
# K5's DAE paths: register DE + streamed head, everything streamed (hidden 96; hidden 128: global accumulators), a five-layer staged MLP
K5_DAE_SHAPES = {"reg": (8, 2, 2, 2, (64, 64, 64), (64, 64, 64)), "zvi16": (5, 4, 6, 6, (64, 64, 64), (64, 64, 64)),
                 "streamed": (8, 2, 2, 2, (96, 96), (96, 96)), "h128": (8, 2, 2, 2, (128, 128, 128), (128, 128, 128)),
                 "deep": (4, 2, 1, 2, (32,) * 5, (24,) * 5)}


# ----------------------------------------------------------------------------- clocks
def ragged_clock(Tn, B, g, pad=False, dt=0.01):
    """per-trajectory step sizes (ragged), drawn from g; pad: the last grid points of some trajectories are -1, as the datasets pad short
    curves.  Trajectory 0 (whose clock decides the events) stays whole."""
    t = (torch.arange(Tn, dtype=torch.float32) * dt).view(Tn, 1, 1).repeat(1, B, 1)
    if B > 1:
        t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, B - 1, 1, generator=g))
    return padded(t) if pad and Tn > 3 and B > 2 else t


def padded(t):
    """a copy of t with the last two grid points of trajectories 2, 5, 8, ... at -1"""
    t = t.clone()
    t[-2:, 2::3] = -1.0
    return t


def dyadic_clock(Tn, B, n, dtype=torch.float32):
    """t[k] = k n / 64 scaled per trajectory by 1/2, 1 or 2: every sub-step is h = 1/64 (times the scale) exactly, in fp32 too."""
    t = (torch.arange(Tn, dtype=dtype) * (n / 64.0)).view(Tn, 1, 1).repeat(1, B, 1)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=dtype)[torch.arange(B) % 3].view(1, B, 1)
    scale[0, 0, 0] = 1.0
    return t * scale


def refine_clock(t, n):
    h = (t[1:] - t[:-1]) / n
    rows = [t[:-1] + j * h for j in range(n)]                      # each [T-1, B, 1]
    fine = torch.stack(rows, 1).reshape(-1, *t.shape[1:])          # [(T-1) n, B, 1]
    return torch.cat((fine, t[-1:]), 0)


def refine_rows(a, n, t=None, event_t=None, jump=None):
    """a [T,B,D] -> [(T-1) n + 1, B, D]; with events (event_t [B,nE,1], jump [B,nE,D]) the rows j >= 1 of an event interval hold jump[:, e]."""
    Tn = a.shape[0]
    out = a[:-1].unsqueeze(1).repeat(1, n, 1, 1)                   # [T-1, n, B, D]
    if event_t is not None and jump is not None and a.shape[-1] > 0:
        for k in range(Tn - 1):
            hit = (event_t[0, :, 0] == t[k, 0, 0]).nonzero().view(-1)
            if hit.numel():
                out[k, 1:] = jump[:, int(hit[0])]
    return torch.cat((out.reshape(-1, *a.shape[1:]), a[-1:]), 0)


# ----------------------------------------------------------------------------- cases
# The order of the draws is part of a case: torch.manual_seed(seed) before the modules are made; one generator draws the clock (unless
# given), x, z, [v, i], [the perturbation of x_init], then the jump rows.
def ode_case(xd, zd, hidden, B, Tn, seed, ev_rows=(), t=None, pad=False, act=nn.ELU):
    """(de, t, x, z, ev, zj).  ev_rows: the grid rows whose times (on trajectory 0's clock) carry an event; rows outside [0, T - 2] are
    dropped, and z_dim 0 has no events.  t: a given clock, else the ragged one (with `pad`)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    de = models.DE_Func(xd + zd, hidden, xd, activation=act)
    if t is None:
        t = ragged_clock(Tn, B, g, pad)
    x = 0.5 * torch.randn(Tn, B, xd, generator=g)
    z = 0.5 * torch.randn(Tn, B, zd, generator=g)
    ev = zj = None
    rows = [k for k in ev_rows if k < Tn - 1]
    if rows and zd > 0:
        ev = t[rows].permute(1, 0, 2).contiguous()                 # [B, nE, 1]
        zj = 0.5 * torch.randn(B, len(rows), zd, generator=g)
    return de, t, x, z, ev, zj


def dae_case(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, ev_rows=(), t=None, pad=False, de_act=nn.ELU, ae_act=nn.ELU,
             perturb_x_init=False):
    """(de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj); ev_rows, t, pad as ode_case (z_dim 0 keeps its events: v jumps).  perturb_x_init:
    x_init is not the dataset row x[0] -- the two are different inputs of the call."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd + vd + idim
    de = models.DAE_DE_Func(n, de_hidden, xd, activation=de_act)
    ae = models.AE_Func(n + xd + zd + vd, ae_hidden, idim, activation=ae_act)
    if t is None:
        t = ragged_clock(Tn, B, g, pad)
    x, z, v, i = (0.5 * torch.randn(Tn, B, w, generator=g) for w in (xd, zd, vd, idim))
    x_init = x[0] + 0.1 * torch.randn(B, xd, generator=g) if perturb_x_init else x[0].clone()
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1)
    ev = zj = vj = None
    rows = [k for k in ev_rows if k < Tn - 1]
    if rows:
        ev = t[rows].permute(1, 0, 2).contiguous()
        zj = 0.5 * torch.randn(B, len(rows), zd, generator=g)
        vj = 0.5 * torch.randn(B, len(rows), vd, generator=g)
    return de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj


def without_x(case):
    """a DAE case whose dataset x has no columns: x is not read without teacher forcing, and this is what the models pass then"""
    return case[:3] + (case[3][:, :, :0],) + case[4:]


def cotangents(seed, *shapes):
    """one generator seeded `seed` draws a standard-normal tensor per shape, in order"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


# ----------------------------------------------------------------------------- runs
def layers_of(seq):
    return [(m.weight.detach(), m.bias.detach()) for m in seq if isinstance(m, nn.Linear)]


def to64(a):
    return None if a is None else a.double()


def to_cuda(a):
    return None if a is None else a.cuda()


def run_ode(solver, de, t, x, z, a0, ev, zj, tx=False):
    event = nd.ODE_Event()
    if ev is not None:
        event.set_event(ev, zj)
    return solver.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0, event_fn=event.event_fn if ev is not None else None,
                                jump_change_fn=event.jump_change_fn if ev is not None else None, input_true_x=tx)


def run_dae(solver, de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj, tx=False, ti=False):
    event = nd.DAE_Event()
    if ev is not None:
        event.set_event(ev, zj, vj)
    return solver.integrate_DAE(x_init=x_init, x_func=de, i_func=ae, t=t, x=x, z=z, v=v, i=i, all_initial=a0,
                                event_fn=event.event_fn if ev is not None else None,
                                jump_change_fn=event.jump_change_fn if ev is not None else None, input_true_x=tx, input_true_i=ti)


def ode_walk64(solver, de, t, x, z, ev, zj, tx=False):
    """the callback walk of a float64 copy of `de` on the CPU (solver: one with fused = "off"), all_initial = x[0] | z[0]"""
    with torch.no_grad():
        return run_ode(solver, deepcopy(de).double(), to64(t), to64(x), to64(z), torch.cat((to64(x)[0], to64(z)[0]), -1), to64(ev),
                       to64(zj), tx)


def ode_gpu(solver, de, t, x, z, ev, zj, tx=False):
    xc, zc = to_cuda(x), to_cuda(z)
    with torch.no_grad():
        return run_ode(solver, deepcopy(de).cuda(), to_cuda(t), xc, zc, torch.cat((xc[0], zc[0]), -1), to_cuda(ev), to_cuda(zj), tx)


def ode_forward_pair(walk_solver, gpu_solver, de, t, x, z, ev, zj, tx=False):
    """(the GPU run, the fp64 walk) of one ODE case; the walk runs first"""
    ref = ode_walk64(walk_solver, de, t, x, z, ev, zj, tx)
    return ode_gpu(gpu_solver, de, t, x, z, ev, zj, tx), ref


def dae_walk64(solver, case, tx=False, ti=False):
    with torch.no_grad():
        return run_dae(solver, deepcopy(case[0]).double(), deepcopy(case[1]).double(), *(to64(q) for q in case[2:]), tx, ti)


def dae_gpu(solver, case, tx=False, ti=False):
    with torch.no_grad():
        return run_dae(solver, deepcopy(case[0]).cuda(), deepcopy(case[1]).cuda(), *(to_cuda(q) for q in case[2:]), tx, ti)


def dae_forward_pair(walk_solver, gpu_solver, case, tx=False, ti=False):
    ref = dae_walk64(walk_solver, case, tx, ti)
    return dae_gpu(gpu_solver, case, tx, ti), ref


# ----------------------------------------------------------------------------- the walk as it was
def walk_ode_hold(s, x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x):
    """FixedGridODESolver._walk_ode as it stood before `externals` existed (x_init None); with s.substeps == 1, as it stood before
    sub-steps did."""
    xs = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
    cur = x[0]
    xs[0] = cur
    for k in range(t.shape[0] - 1):
        t0, t1, zk = t[k], t[k + 1], z[k]
        if event_fn is not None and event_fn(t0) == True:  # noqa: E712
            zk = jump_change_fn(t0, zk)
        start = x[k] if input_true_x else cur
        if s.substeps == 1:
            cur, _ = s.step_integrate(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, all_initial=all_initial)
        else:
            h = (t1 - t0) / s.substeps
            cur = start
            for j in range(s.substeps):
                cur, _ = s.step_integrate(func=x_func, t0=t0 + j * h, dt=h, t1=t0 + (j + 1) * h, x0=cur, z0=zk, all_initial=all_initial)
        xs[k + 1] = cur
    return xs


def walk_dae_hold(s, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i):
    """FixedGridODESolver._walk_dae as it stood before `externals` existed; with s.substeps == 1, as it stood before sub-steps did."""
    cur_x = x_init
    cur_i = i_func(xt=x[0] if input_true_x else cur_x, zt=z[0], vt=v[0], all_initial=all_initial)
    xs = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
    is_ = torch.zeros(i.shape, dtype=i.dtype, device=i.device)
    xs[0], is_[0] = cur_x, cur_i
    for k in range(t.shape[0] - 1):
        t0, t1, zk, vk = t[k], t[k + 1], z[k], v[k]
        if event_fn is not None and event_fn(t0) == True:  # noqa: E712
            zk, vk = jump_change_fn(t0, zk, vk)
            cur_i = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
        start = x[k] if input_true_x else cur_x
        i_in = i[k] if input_true_i else cur_i
        if s.substeps == 1:
            cur_x, _ = s.step_integrate(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, v0=vk, i0=i_in, all_initial=all_initial)
        else:
            h = (t1 - t0) / s.substeps
            cur_x = start
            for j in range(s.substeps):
                if j > 0 and not input_true_i:
                    i_in = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
                cur_x, _ = s.step_integrate(func=x_func, t0=t0 + j * h, dt=h, t1=t0 + (j + 1) * h, x0=cur_x, z0=zk, v0=vk, i0=i_in,
                                            all_initial=all_initial)
        cur_i = i_func(xt=x[k + 1] if input_true_x else cur_x, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
        xs[k + 1], is_[k + 1] = cur_x, cur_i
    return xs, is_


# ----------------------------------------------------------------------------- gates
def close(a, b, what, tol, none_is_zero=False):
    """max |a - b| <= tol x max |b| (floor 1e-6), a on any device against the float64 reference b.  Both None passes (a call without
    events has no jump gradient on either side); a None reference stands for zeros; a None candidate against a reference fails, unless
    none_is_zero asks for it to be read as zeros too; shapes must agree, which is all there is to compare on an empty tensor."""
    if a is None and b is None:
        return
    if b is None:
        b = torch.zeros(a.shape, dtype=torch.float64)
    if a is None and none_is_zero:
        a = torch.zeros(b.shape)
    assert a is not None, f"{what}: no value where the reference has one"
    assert tuple(a.shape) == tuple(b.shape), f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if b.numel() == 0:          # (z_dim 0: nothing to compare but the shape)
        return
    b = b.detach().double().cpu()
    scale = float(b.abs().max())
    err = float((a.detach().double().cpu() - b).abs().max())
    print(f"{what}: max abs err {err:.3e}, tensor max {scale:.3e}, ratio {err / max(scale, 1e-6):.3e}")
    assert err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _same_bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _judge(ref, got, again, pairs, grad_fn_of, grad_fn_prefix, tol, what, ref_float, none_is_zero):
    if grad_fn_prefix is not None:
        assert type(grad_fn_of.grad_fn).__name__.startswith(grad_fn_prefix), f"{what}: grad_fn {grad_fn_of.grad_fn} is no {grad_fn_prefix}"
    for name, out, ref_out in pairs:
        r = ref_out.detach().float() if ref_float else ref_out.detach()
        e = traj_rel_err(out.detach().cpu(), r)
        assert e <= TOL_GPU, f"{what}: trajectory {name} off by {e:.3e}"
    for k in ref:
        assert k in got, f"{what}: no gradient {k}"
        close(got[k], ref[k], f"{what} grad {k}".strip(), tol, none_is_zero)
        if again is not None:
            assert _same_bits(got[k], again[k]), f"{what}: backward not repeatable: {k}"


def judge_ode_training(ref, got, again, xs, ref_xs, grad_fn_prefix, tol, what="", ref_float=False, none_is_zero=False):
    """The verdict on one ODE training run, from its results alone (no GPU is touched: CPU tensors do).  ref / got / again: gradients by
    name of the float64 walk, the fused run and its repetition; xs / ref_xs: the two trajectories.
      - xs.grad_fn's class name starts with grad_fn_prefix (the fused autograd function ran, not a walk);
      - xs within helpers.TOL_GPU of ref_xs on traj_rel_err (ref_float: the reference rounded to float32 first, the externals tests' form);
      - every gradient the reference has: close(got, ref, tol);
      - got and again bit for bit the same.
    A check a file does not make is left out by passing None for what it needs: again, ref_xs, grad_fn_prefix."""
    pairs = [("x", xs, ref_xs)] if ref_xs is not None else []
    _judge(ref, got, again, pairs, xs, grad_fn_prefix, tol, what, ref_float, none_is_zero)


def judge_dae_training(ref, got, again, xs, ref_xs, grad_fn_prefix, tol, what="", ref_float=False, none_is_zero=False):
    """judge_ode_training for a DAE: xs = (xs, is_) and ref_xs = (ref xs, ref is_), both trajectories under the gate"""
    pairs = [("x", xs[0], ref_xs[0]), ("i", xs[1], ref_xs[1])] if ref_xs is not None else []
    _judge(ref, got, again, pairs, xs[0], grad_fn_prefix, tol, what, ref_float, none_is_zero)


# ----------------------------------------------------------------------------- training
def _cv(dev, copy=False):
    dtype = torch.float32 if dev == "cuda" else torch.float64
    kw = dict(copy=True) if copy else {}
    return dtype, (lambda a: None if a is None else a.to(device=dev, dtype=dtype, **kw))


def ode_train(solver, case, G, dev, tx=False, x_leaf=None, copy=False):
    """One forward + backward of loss = sum(xs * G): float32 under solver("require") on "cuda", float64 under solver("off") on "cpu".
    Leaves: z, all_initial (built from x[0] | z[0], a leaf of its own), the jump rows, the parameters, and x unless teacher-forced
    (x_leaf overrides; the dataset rows get no gradient).  -> xs, {name: grad}; "x" is reported when not teacher-forced."""
    de, t, x, z, ev, zj = case
    dtype, cv = _cv(dev, copy)
    m = deepcopy(de).to(device=dev, dtype=dtype)
    xg, zg = cv(x), cv(z).requires_grad_(True)
    if (not tx) if x_leaf is None else x_leaf:
        xg.requires_grad_(True)
    a0 = torch.cat((cv(x)[0], cv(z)[0]), -1).requires_grad_(True)
    zjg = cv(zj).requires_grad_(True) if zj is not None else None
    xs = run_ode(solver("require" if dev == "cuda" else "off"), m, cv(t), xg, zg, a0, cv(ev), zjg, tx)
    (xs * cv(G)).sum().backward()
    grads = {"z": zg.grad, "a0": a0.grad, "zj": zjg.grad if zjg is not None else None}
    if not tx:
        grads["x"] = xg.grad                                    # (x0: the only row of x the integration reads)
    grads.update({f"p{k}": p.grad for k, p in enumerate(m.parameters())})
    return xs, grads


def dae_train(solver, case, G, Gi, dev, tx=False, ti=False, i_leaf=False, no_x=False, copy=False):
    """ode_train for a DAE, loss = sum(xs * G) + sum(is_ * Gi).  Leaves: x_init, z, v, all_initial, the jump rows, both MLPs' parameters
    (and the dataset i with i_leaf).  no_x: the call gets the converted x without its columns.  -> xs, is_, {name: grad}."""
    de, ae, t, x, z, v, i, x_init, a0, ev, zj, vj = case
    dtype, cv = _cv(dev, copy)
    de, ae = deepcopy(de).to(device=dev, dtype=dtype), deepcopy(ae).to(device=dev, dtype=dtype)
    leaf = lambda a: None if a is None else cv(a).requires_grad_(True)
    xi, zg, vg, a0g, zjg, vjg = leaf(x_init), leaf(z), leaf(v), leaf(a0), leaf(zj), leaf(vj)
    ic = leaf(i) if i_leaf else cv(i)
    xc = cv(x)[:, :, :0] if no_x else cv(x)
    xs, is_ = run_dae(solver("require" if dev == "cuda" else "off"), de, ae, cv(t), xc, zg, vg, ic, xi, a0g, cv(ev), zjg, vjg, tx, ti)
    ((xs * cv(G)).sum() + (is_ * cv(Gi)).sum()).backward()
    grads = {"x_init": xi.grad, "z": zg.grad, "v": vg.grad, "a0": a0g.grad, "zj": zjg.grad if zjg is not None else None,
             "vj": vjg.grad if vjg is not None else None}
    grads.update({f"de{k}": p.grad for k, p in enumerate(de.parameters())})
    grads.update({f"ae{k}": p.grad for k, p in enumerate(ae.parameters())})
    return xs, is_, grads


def check_ode_training(solver, case, G, grad_fn_prefix, tol, tx=False, what="", ref_float=False):
    """The float64 walk, then the fused run twice with RuntimeWarning an error (a walk under "auto" warns), then the judge.  -> got, ref"""
    ref_xs, ref = ode_train(solver, case, G, "cpu", tx)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = ode_train(solver, case, G, "cuda", tx)
        _, again = ode_train(solver, case, G, "cuda", tx)
    judge_ode_training(ref, got, again, xs, ref_xs, grad_fn_prefix, tol, what, ref_float)
    return got, ref


def check_dae_training(solver, case, G, Gi, grad_fn_prefix, tol, tx=False, ti=False, what="", ref_float=False):
    rx, ri, ref = dae_train(solver, case, G, Gi, "cpu", tx, ti)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, is_, got = dae_train(solver, case, G, Gi, "cuda", tx, ti)
        _, _, again = dae_train(solver, case, G, Gi, "cuda", tx, ti)
    judge_dae_training(ref, got, again, (xs, is_), (rx, ri), grad_fn_prefix, tol, what, ref_float)
    return got, ref
