"""Host-side builders for the tests that ask the library's C ABI from the dims alone (no GPU, no torch modules, no oracle): argument
structs of the K0 / K5 entry points with every pointer NULL, the option structs, and the `supported` / call pair of an entry-point
family.  A plain module, imported like helpers.py.  What differs between the test files -- `method`, T, B -- is an argument that each
file binds once (functools.partial)."""
import ctypes
import functools

import torch
import torch.nn as nn

from helpers import T
from py_psnode_amd import _lib

R = ctypes.byref


def mlp(m, in_dim, hidden, out):
    """hidden: an int (three equal hidden layers) or the tuple of widths"""
    widths = ((hidden,) * 3 if isinstance(hidden, int) else tuple(hidden)) + (out,)
    m.n_layers, m.in_dim = len(widths), in_dim
    for k, o in enumerate(widths):
        m.out_dim[k] = o


def _ode(a, kernel, xd, zd, hidden, method, Tn, B):
    a.method, a.kernel, a.x_dim, a.z_dim, a.T, a.B = method, kernel, xd, zd, Tn, B
    mlp(a.de, 3 * (xd + zd), hidden, xd)
    return a


def _dae(a, kernel, xd, zd, vd, idim, hidden, ae_hidden, method, Tn, B):
    a.method, a.kernel, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = method, kernel, xd, zd, vd, idim, Tn, B
    n = xd + zd + vd + idim
    mlp(a.de, 3 * n, hidden, xd)
    mlp(a.ae, n + xd + zd + vd, hidden if ae_hidden is None else ae_hidden, idim)
    return a


def ode_args(kernel=_lib.KERNEL_AUTO, xd=8, zd=2, hidden=64, *, method, T, B):
    return _ode(_lib.OdeArgsF32(), kernel, xd, zd, hidden, method, T, B)


def dae_args(kernel=_lib.KERNEL_AUTO, xd=8, zd=2, vd=2, idim=2, hidden=64, ae_hidden=None, *, method, T, B):
    return _dae(_lib.DaeArgsF32(), kernel, xd, zd, vd, idim, hidden, ae_hidden, method, T, B)


def ode_bwd_args(kernel=_lib.KERNEL_AUTO, xd=8, zd=2, hidden=64, flags=0, *, method, T, B):
    a = _ode(_lib.OdeBwdArgsF32(), kernel, xd, zd, hidden, method, T, B)
    a.flags = flags
    return a


def dae_bwd_args(kernel=_lib.KERNEL_AUTO, xd=8, zd=2, vd=2, idim=2, hidden=64, ae_hidden=None, flags=0, *, method, T, B):
    """the teacher-forcing form (DaeBwdTfArgsF32); `.base` is the DaeBwdArgsF32 of the entry points without flags"""
    a = _lib.DaeBwdTfArgsF32()
    _dae(a.base, kernel, xd, zd, vd, idim, hidden, ae_hidden, method, T, B)
    a.flags = flags
    return a


def bound(**dims):
    """(ode_args, dae_args, ode_bwd_args, dae_bwd_args) with `dims` bound, under the names the parametrised test ids carry"""
    out = []
    for fn in (ode_args, dae_args, ode_bwd_args, dae_bwd_args):
        p = functools.partial(fn, **dims)
        p.__name__ = "_" + fn.__name__
        out.append(p)
    return out


def act(kind, alpha=0.0, beta=1.0, threshold=20.0):
    a = _lib.ActF32()
    a.kind, a.alpha, a.beta, a.threshold = kind, alpha, beta, threshold
    return a


def sub(n, x_sub=None):
    s = _lib.SubstepsF32()
    s.substeps, s.x_sub = n, x_sub
    return s


def state_dict_of(d, prefix):
    """the state dict stored in a golden set under '<prefix><name with __ for .>'"""
    return {k[len(prefix):].replace("__", "."): T(v) for k, v in d.items() if k.startswith(prefix)}


class OnHip(torch.Tensor):
    """A host tensor that reports a HIP device: the predicates refuse other devices before they ask the library, and the library's
    answer to a `supported` query depends on the dims alone (no pointer is followed)."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def hip_layers(seq):
    hip = lambda q: torch.Tensor._make_subclass(OnHip, q.detach())
    return [(hip(m.weight), hip(m.bias)) for m in seq if isinstance(m, nn.Linear)]


# what follows the args struct: one activation per MLP, the tableau and -- in the families "sub" and "lin", not in "rk" -- the sub-steps struct
def _options(family, n_act, tab, sub_, act_):
    tail = [act_] * n_act + [tab]
    if family != "rk":
        tail.append(R(sub_) if sub_ is not None else None)
    return tail


def _symbol(lib, stem, family, what):
    return getattr(lib, f"psnode_{stem}_{family}_{what}")


def supported(lib, stem, a, n_act, tab=None, sub=None, act=None, *, family):
    """psnode_<stem>_<family>_supported; tab / act: byref'd structs or None, sub: the struct itself or None"""
    return _symbol(lib, stem, family, "supported")(R(a), *_options(family, n_act, tab, sub, act))


def call(lib, stem, a, n_act, tab=None, sub=None, act=None, *, family):
    """psnode_<stem>_<family>_f32 without workspace or stream: with every pointer of the args NULL, a call that got past its checks would
    have nothing to launch on"""
    return _symbol(lib, stem, family, "f32")(R(a) if a is not None else None, *_options(family, n_act, tab, sub, act), None, 0, None)
