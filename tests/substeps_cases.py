"""Shared by tests/test_substeps_host.py and tests/test_gpu_substeps.py: the n-times refined problem whose one-step-per-interval solution,
read at rows ::n, is what `substeps = n` computes on the coarse problem (no teacher forcing), and small problem builders.

Refinement of a time-major problem: clock t'[kn + j] = t[k] + j h, h = (t[k+1] - t[k]) / n in the clock's own dtype; externals
z'[kn + j] = z[k]; on an interval that starts with an event the rows j >= 1 carry the jumped values (the event itself fires at row kn only:
the refined clock meets an event time nowhere else)."""
import torch
import torch.nn as nn

from py_psnode_amd import models
from py_psnode_amd import neural_dae as nd


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


def dyadic_clock(Tn, B, n, dtype=torch.float32):
    """t[k] = k n / 64 scaled per trajectory by 1/2, 1 or 2: every sub-step is h = 1/64 (times the scale) exactly, in fp32 too."""
    t = (torch.arange(Tn, dtype=dtype) * (n / 64.0)).view(Tn, 1, 1).repeat(1, B, 1)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=dtype)[torch.arange(B) % 3].view(1, B, 1)
    scale[0, 0, 0] = 1.0
    return t * scale


def ode_problem(xd, zd, hidden, B, Tn, seed, t, ev_steps=(0, 3), act=nn.ELU):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    de = models.DE_Func(xd + zd, hidden, xd, activation=act)
    x = 0.5 * torch.randn(Tn, B, xd, generator=g)
    z = 0.5 * torch.randn(Tn, B, zd, generator=g)
    ev = zj = None
    steps = [k for k in ev_steps if k < Tn - 1]
    if steps and zd > 0:
        ev = t[steps].permute(1, 0, 2).contiguous()                # [B, nE, 1]
        zj = 0.5 * torch.randn(B, len(steps), zd, generator=g)
    return de, x, z, ev, zj


def dae_problem(xd, zd, vd, idim, de_hidden, ae_hidden, B, Tn, seed, t, ev_steps=(0, 3), de_act=nn.ELU, ae_act=nn.ELU):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd + vd + idim
    de = models.DAE_DE_Func(n, de_hidden, xd, activation=de_act)
    ae = models.AE_Func(n + xd + zd + vd, ae_hidden, idim, activation=ae_act)
    x, z, v, i = (0.5 * torch.randn(Tn, B, w, generator=g) for w in (xd, zd, vd, idim))
    x_init = x[0].clone()
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1)
    ev = zj = vj = None
    steps = [k for k in ev_steps if k < Tn - 1]
    if steps:
        ev = t[steps].permute(1, 0, 2).contiguous()
        zj = 0.5 * torch.randn(B, len(steps), zd, generator=g)
        vj = 0.5 * torch.randn(B, len(steps), vd, generator=g)
    return de, ae, x, z, v, i, x_init, a0, ev, zj, vj


def layers_of(seq):
    return [(m.weight.detach(), m.bias.detach()) for m in seq if isinstance(m, nn.Linear)]


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
