"""Shared host-side plumbing of the fused HIP integrator: recognising the reference's MLP right-hand sides, marshalling tensors into the
C ABI structs (include/psnode_hip.h), the device-side event table, workspaces.  Nothing here computes on the CPU and nothing here
imports oracle/."""
import collections
import ctypes
import dataclasses
import functools
import math
import os
import struct
import weakref
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import _lib

Layers = Sequence[Tuple[torch.Tensor, torch.Tensor]]


METHOD_ID = {"euler": _lib.EULER, "midpoint": _lib.MIDPOINT, "rk4": _lib.RK4_38}
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}      # right-hand-side evaluations per step


@dataclasses.dataclass(frozen=True)
class Tableau:
    """An explicit Runge-Kutta method of 1..4 stages as a `method` of the generic route (K0 forward, K5 backward; psnode_rk_tableau_f32,
    include/psnode_hip.h): a[s][j], j < s, is the coefficient of slope k_j in the argument of stage s, b[s] the weight of k_s in the update.
    One step:  argument of stage s = x0 + h * sum_{j<s} a[s][j] k_j,  new state = x0 + h * sum_s b[s] k_s  (sums in increasing index, a
    coefficient that is exactly 0 skipped).  `a` may be given as S rows of any length up to S (missing entries are zeros) and must be
    strictly lower triangular.  Frozen and hashable; `order` is informative."""
    name: str
    a: tuple
    b: tuple
    order: int

    def __post_init__(self):
        try:
            b = tuple(float(q) for q in self.b)
            S = len(b)
            rows = [tuple(float(q) for q in r) for r in self.a]
        except TypeError as e:
            raise ValueError(f"Tableau: a must be a sequence of rows and b a sequence of numbers ({e})") from e
        if not 1 <= S <= 4:
            raise ValueError(f"Tableau: {S} stages, supported 1..4")
        if len(rows) != S or any(len(r) > S for r in rows):
            raise ValueError(f"Tableau: a must have {S} rows of at most {S} entries, as b has {S}")
        rows = [r + (0.0,) * (S - len(r)) for r in rows]
        if not all(math.isfinite(q) for r in rows for q in r) or not all(math.isfinite(q) for q in b):
            raise ValueError("Tableau: coefficients must be finite")
        if any(rows[s][j] != 0.0 for s in range(S) for j in range(s, S)):
            raise ValueError("Tableau: a must be strictly lower triangular (an explicit method)")
        if abs(sum(b) - 1.0) > 1e-6:
            raise ValueError(f"Tableau: sum(b) = {sum(b)!r}, must be 1 within 1e-6")
        object.__setattr__(self, "a", tuple(rows))
        object.__setattr__(self, "b", b)
        object.__setattr__(self, "name", str(self.name))
        object.__setattr__(self, "order", int(self.order))
        object.__setattr__(self, "_c", tuple(sum(r) for r in rows))

    @property
    def stages(self) -> int:
        return len(self.b)

    @property
    def c(self) -> tuple:
        """The nodes c_s = sum_j a[s][j] (the callback walk evaluates stage s at t0 + c_s dt)."""
        return self._c

    def abi(self) -> "_lib.RkTableauF32":
        t = _lib.RkTableauF32()
        t.stages = self.stages
        for s, r in enumerate(self.a):
            for j, q in enumerate(r):
                t.a[s][j] = q
        for s, q in enumerate(self.b):
            t.b[s] = q
        return t

    def __str__(self):
        return self.name


@dataclasses.dataclass(frozen=True)
class Recurrence:
    """A stabilised explicit step given by a three-term recurrence (Runge-Kutta-Chebyshev), the `method` of neural_dae.RKC1 / RKC2 and a
    sibling of Tableau: one step of `stages` right-hand-side evaluations per grid interval,
        Y_1 = Y_0 + (mu_t[0] h) F_0;   Y_j = kappa[j-1] Y_0 + mu[j-1] Y_{j-1} + nu[j-1] Y_{j-2} + (mu_t[j-1] h) F(Y_{j-1}) + (gamma_t[j-1] h) F_0
    summed in the order written, a coefficient that is exactly 0 skipped.  `table` is `rkc_table`'s dict: the fp32-rounded coefficients (as
    Python floats; THEY are the method, the walk and the kernels read the same values), the nodes c and the real stability boundary beta.
    Frozen and hashable (by name, stages, order and the coefficient tuples)."""
    name: str
    stages: int
    order: int
    kappa: tuple
    mu: tuple
    nu: tuple
    mu_t: tuple
    gamma_t: tuple
    c: tuple = dataclasses.field(compare=False, default=())
    beta: float = dataclasses.field(compare=False, default=0.0)

    def abi(self, x_stage=None) -> "_lib.RkcF32":
        r = _lib.RkcF32()
        r.stages = self.stages
        for j in range(self.stages):
            r.kappa[j], r.mu[j], r.nu[j], r.mu_t[j], r.gamma_t[j] = self.kappa[j], self.mu[j], self.nu[j], self.mu_t[j], self.gamma_t[j]
        r.x_stage = x_stage
        return r

    def __str__(self):
        return self.name


def _f32(q: float) -> float:
    """q rounded once to fp32, as a Python float."""
    return struct.unpack("f", struct.pack("f", q))[0]


def rkc_table(stages, order, damping=None) -> Recurrence:
    """The Runge-Kutta-Chebyshev method of `stages` stages (1..32; order 2: 2..32) and `order` 1 or 2 with damping eps (default 0.05 /
    2/13): the coefficients from the Chebyshev recurrences T_j, T_j', T_j'' at w0 = 1 + eps / s^2 in fp64, rounded once to fp32.
    order 1: w1 = T_s / T_s', mu_t_1 = w1 / w0, mu_j = 2 w0 T_{j-1} / T_j, nu_j = -T_{j-2} / T_j, mu_t_j = 2 w1 T_{j-1} / T_j, gamma_t = kappa = 0,
    c_j = T_s T_j' / (T_s' T_j), beta = (1 + w0) T_s' / T_s.   order 2: w1 = T_s' / T_s'', b_j = T_j'' / T_j'^2 (b_0 = b_1 = b_2),
    a_j = 1 - b_j T_j, mu_t_1 = b_1 w1, mu_j = 2 b_j w0 / b_{j-1}, nu_j = -b_j / b_{j-2}, mu_t_j = 2 b_j w1 / b_{j-1}, gamma_t_j = -a_{j-1} mu_t_j,
    kappa_j = 1 - mu_j - nu_j, c_1 = c_2 / T_2', c_j = T_s' T_j'' / (T_s'' T_j'), beta = (1 + w0) T_s'' / T_s'.  Entry j - 1 of a tuple is
    stage j; entry 0 of kappa / mu / nu / gamma_t is 0 and never read.  kappa_j + mu_j + nu_j = 1 holds exactly for the ROUNDED values: the
    last of the three is taken from the rounded others (nu_j = 1 - mu_j at order 1, kappa_j = 1 - mu_j - nu_j at order 2)."""
    if isinstance(stages, bool) or not isinstance(stages, int):
        raise ValueError(f"stages must be an int, got {stages!r}")
    if order not in (1, 2) or isinstance(order, bool):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    if not (1 if order == 1 else 2) <= stages <= _lib.RKC_MAX_STAGES:
        raise ValueError(f"RKC{order}: stages must be in {1 if order == 1 else 2}..{_lib.RKC_MAX_STAGES}, got {stages!r}")
    if damping is not None and (isinstance(damping, bool) or not isinstance(damping, (int, float))):
        raise ValueError(f"damping must be a finite number > 0, got {damping!r}")
    eps = (0.05 if order == 1 else 2.0 / 13.0) if damping is None else float(damping)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"damping must be a finite number > 0, got {damping!r}")
    return _rkc_table(stages, order, eps)      # (validated first: the cache hashes its arguments)


@functools.lru_cache(maxsize=128)
def _rkc_table(s: int, order: int, eps: float) -> Recurrence:
    w0 = 1.0 + eps / (s * s)
    T, dT, ddT = [1.0, w0], [0.0, 1.0], [0.0, 0.0]
    for j in range(2, s + 1):
        T.append(2.0 * w0 * T[j - 1] - T[j - 2])
        dT.append(2.0 * T[j - 1] + 2.0 * w0 * dT[j - 1] - dT[j - 2])
        ddT.append(4.0 * dT[j - 1] + 2.0 * w0 * ddT[j - 1] - ddT[j - 2])
    kappa, mu, nu, mu_t, gamma_t, c = [0.0] * s, [0.0] * s, [0.0] * s, [0.0] * s, [0.0] * s, [0.0] * s
    if order == 1:
        w1 = T[s] / dT[s]
        mu_t[0] = w1 / w0
        for j in range(2, s + 1):
            mu[j - 1] = 2.0 * w0 * T[j - 1] / T[j]
            nu[j - 1] = -T[j - 2] / T[j]
            mu_t[j - 1] = 2.0 * w1 * T[j - 1] / T[j]
        for j in range(1, s + 1):
            c[j - 1] = T[s] * dT[j] / (dT[s] * T[j])
        beta = (1.0 + w0) * dT[s] / T[s]
    else:
        w1 = dT[s] / ddT[s]
        b = [0.0, 0.0] + [ddT[j] / (dT[j] * dT[j]) for j in range(2, s + 1)]
        b[0] = b[1] = b[2]
        a = [1.0 - b[j] * T[j] for j in range(s + 1)]
        mu_t[0] = b[1] * w1
        for j in range(2, s + 1):
            mu[j - 1] = 2.0 * b[j] * w0 / b[j - 1]
            nu[j - 1] = -b[j] / b[j - 2]
            mu_t[j - 1] = 2.0 * b[j] * w1 / b[j - 1]
            gamma_t[j - 1] = -a[j - 1] * mu_t[j - 1]
            kappa[j - 1] = 1.0 - mu[j - 1] - nu[j - 1]
            c[j - 1] = dT[s] * ddT[j] / (ddT[s] * dT[j])
        c[0] = c[1] / dT[2]
        beta = (1.0 + w0) * ddT[s] / dT[s]
    # The rounded values are the method, so the consistency condition kappa_j + mu_j + nu_j = 1 (a constant state stays constant: R(0) = 1,
    # not 1 + 6e-8) is made to hold FOR them: the last of the three is 1 minus the rounded others -- nu_j at order 1, where kappa_j is 0 by
    # definition, kappa_j at order 2 -- which is exact in fp32 (a multiple of 2^-24 below 1 in magnitude) and moves it by a rounding error.
    mu = [_f32(q) for q in mu]
    if order == 1:
        nu = [0.0] + [1.0 - mu[j] for j in range(1, s)]
    else:
        nu = [_f32(q) for q in nu]
        kappa = [0.0] + [1.0 - mu[j] - nu[j] for j in range(1, s)]
    r32 = lambda q: tuple(_f32(v) for v in q)
    return Recurrence(f"RKC{order}(stages={s})", s, order, r32(kappa), r32(mu), r32(nu), r32(mu_t), r32(gamma_t), tuple(c), beta)


AB2 = "ab2"      # the `method` value of two-step Adams-Bashforth (neural_dae.AB2): the _ab entry points of K0 / K5, no other kernel


AB3 = "ab3"      # three-step Adams-Bashforth with a predictor-corrector restart step (neural_dae.AB3): the _ab3 entry points of K0 / K5


def is_ab(method) -> bool:
    return isinstance(method, str) and method in (AB2, AB3)


def ab_order(method) -> int:
    """2 for "ab2", 3 for "ab3" (and 2 for every method that is no Adams-Bashforth method, where nothing reads it)."""
    return 3 if isinstance(method, str) and method == AB3 else 2


def method_info(method):
    """(method id for the args struct, right-hand-side evaluations per step, Tableau | None) of a `method` of the generic route: one of the
    built-in names, a Tableau (whose calls go to the _rk entry points, which do not read the id) or "ab2" (two-step Adams-Bashforth: one
    evaluation per step; its calls go to the _ab entry points, which do not read the id either)."""
    if isinstance(method, Tableau):
        return _lib.EULER, method.stages, method
    if isinstance(method, Recurrence):      # (one evaluation per stage pass; the stage count travels in the sub-steps' place: GenericOpts.of)
        return _lib.EULER, 1, method
    if is_ab(method):
        return _lib.EULER, 1, None
    return METHOD_ID[method], STAGES[method], None


def builtin_method(method, what: str):
    """(method id, stages) for the specialised kernels, which carry the three built-in formulas only: a Tableau is refused."""
    if isinstance(method, Recurrence):
        raise _lib.UnsupportedShapeError(f"{what}: a Runge-Kutta-Chebyshev recurrence ({method.name}) runs on the generic kernels K0 / K5 only "
                                         "(kernel 'auto' / 'generic', no saved rows); this entry point carries euler / midpoint / rk4")
    if isinstance(method, Tableau):
        raise _lib.UnsupportedShapeError(f"{what}: a Runge-Kutta tableau ({method.name}) runs on the generic kernels K0 / K5 only "
                                         "(kernel 'auto' / 'generic', no saved rows); this entry point carries euler / midpoint / rk4")
    return METHOD_ID[method], STAGES[method]


# z | v inside a grid interval: the left grid point's rows held (the reference), interpolated linearly to the right one's, or by the
# polynomial through the up to four neighbouring dataset rows of the interval's piece (four-point Lagrange, `lagrange_stencils`)
EXTERNALS = ("hold", "linear", "lagrange")
# Where a DAE's algebraic variable is evaluated: "step" (once per (sub-)step, frozen over its stages: the reference's rule) or "stage" (in
# front of every stage s >= 1 at that stage's argument and interpolated externals: neural_dae.FixedGridODESolver)
ALGEBRAIC = ("step", "stage")


def is_linear(externals: str) -> bool:
    """True for the interpolated externals ("linear", "lagrange"), False for "hold"; ValueError for anything else."""
    if not isinstance(externals, str) or externals not in EXTERNALS:
        raise ValueError(f"externals must be one of {EXTERNALS}, got {externals!r}")
    return externals != "hold"


def is_lagrange(externals: str) -> bool:
    """True for externals="lagrange", False for "hold" / "linear"; ValueError for anything else."""
    return is_linear(externals) and externals == "lagrange"


def _externals_text(externals: str) -> str:
    """The option as the subject of a refusal."""
    return ("four-point Lagrange interpolated external inputs (externals='lagrange')" if externals == "lagrange"
            else "linearly interpolated external inputs (externals='linear')")


def stencil_code(off: int, q: int) -> int:
    """The code byte of a stencil (PSNODE_STENCIL_CODE, include/psnode_hip.h): off = k - s in bits 0-1, the node count q in bits 2-4."""
    return off | (q << 2)


def lagrange_stencils(t: torch.Tensor, event_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The stencil table of externals="lagrange": int8 [T-1, B], one code byte (`stencil_code`) per grid interval and trajectory.
    t: the clocks [T, B] (or [T, B, 1]; [T, 1] / [T] is one shared clock, B = 1); event_idx: None or the shared event table, int [T-1]
    (an entry >= 0: an event step).  Interval k is valid if t[k+1] - t[k] > 0.  A piece is a maximal run of consecutive valid intervals
    with no event step in its interior; an invalid interval is a two-node piece of its own.  Interval k of piece [a, e] reads
    q = min(4, e - a + 1) nodes from s = clamp(k - 1, a, e - q + 1) on; off = k - s.  Tensor ops on t's device, no host synchronisation."""
    if t.dim() == 3:
        t = t[..., 0]
    if t.dim() == 1:
        t = t[:, None]
    T, B = t.shape
    dev = t.device
    if T < 2:
        return torch.empty((0, B), dtype=torch.int8, device=dev)
    valid = (t[1:] - t[:-1]) > 0                                             # [T-1, B]
    k = torch.arange(T - 1, device=dev)[:, None]                             # interval index = its left node
    start = ~valid                                                           # node k starts a piece: an invalid interval, ...
    start[1:] |= ~valid[:-1]                                                 # ... the interval behind one, ...
    start[0] = True                                                          # ... the first, ...
    if event_idx is not None:
        start |= (event_idx.to(dev).reshape(T - 1, 1) >= 0)                  # ... an event step
    a = torch.cummax(torch.where(start, k, torch.zeros_like(k)), 0).values   # the piece's first node
    # the piece's last node: the next piece start behind k, else T - 1; an invalid interval ends at k + 1
    nxt = torch.where(start, k, torch.full_like(k, T - 1)).expand(T - 1, B)
    nxt = torch.cat((nxt[1:], torch.full((1, B), T - 1, device=dev, dtype=nxt.dtype)), 0)
    e = torch.flip(torch.cummin(torch.flip(nxt, (0,)), 0).values, (0,))
    q = (e - a + 1).clamp(max=4)
    s = torch.minimum(torch.maximum(k - 1, a), e - q + 1)
    return ((k - s) | (q << 2)).to(torch.int8)


KERNEL_ID = {"auto": _lib.KERNEL_AUTO, "generic": _lib.KERNEL_GENERIC, "mfma": _lib.KERNEL_MFMA, "wide": _lib.KERNEL_MFMA_WIDE,
             "tile": _lib.KERNEL_MFMA_TILE, "wave": _lib.KERNEL_MFMA_WAVE}      # forward ODE calls: K1 (4-wave tile) / K1x (one wave per 4 trajectories)


# PSNODE_POISON=1 (debug / `pytest -m gpu` leg of tests/test_gpu_fuzz.py): every buffer this module hands a kernel uninitialised --
# outputs, stored rows, workspaces -- is filled with NaN bit patterns first, so that a kernel (or a host-side contraction) that consumes
# memory nobody wrote shows up as NaN instead of as whatever the caching allocator happened to recycle.
_POISON = os.environ.get("PSNODE_POISON", "0") == "1"


def _empty(*size, **kw) -> torch.Tensor:
    t = torch.empty(*size, **kw)
    if _POISON and t.numel():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(0xFF)            # 0xFFFFFFFF read as fp32 is a NaN
        else:
            t.fill_(-(1 << 30))
    return t


# ----------------------------------------------------------------------------- recognition
class Act:
    """A hidden-layer activation other than ELU(alpha=1) that the generic kernels K0 / K5 apply (psnode_act_f32, include/psnode_hip.h).
    Everywhere in this package `act=None` means ELU(1), the activation of every specialised kernel.  Calling it applies the activation
    with torch (the recipe probe)."""
    __slots__ = ("kind", "alpha", "beta", "threshold", "name")

    def __init__(self, kind: int, alpha: float = 0.0, beta: float = 1.0, threshold: float = 20.0, name: str = ""):
        self.kind, self.alpha, self.beta, self.threshold, self.name = int(kind), float(alpha), float(beta), float(threshold), name

    def abi(self) -> "_lib.ActF32":
        a = _lib.ActF32()
        a.kind, a.alpha, a.beta, a.threshold = self.kind, self.alpha, self.beta, self.threshold
        return a

    def __call__(self, u: torch.Tensor) -> torch.Tensor:
        return _ACT_TORCH[self.kind](self, u)

    def _key(self):
        return (self.kind, self.alpha, self.beta, self.threshold)

    def __eq__(self, other):
        return isinstance(other, Act) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Act({self.name})"


_F = nn.functional
_ACT_TORCH = {
    _lib.ACT_ELU: lambda a, u: _F.elu(u, a.alpha),
    _lib.ACT_TANH: lambda a, u: torch.tanh(u),
    _lib.ACT_SIGMOID: lambda a, u: torch.sigmoid(u),
    _lib.ACT_RELU: lambda a, u: _F.relu(u),
    _lib.ACT_LEAKY_RELU: lambda a, u: _F.leaky_relu(u, a.alpha),
    _lib.ACT_SOFTPLUS: lambda a, u: _F.softplus(u, a.beta, a.threshold),
    _lib.ACT_SILU: lambda a, u: _F.silu(u),
    _lib.ACT_GELU: lambda a, u: _F.gelu(u),
    _lib.ACT_GELU_TANH: lambda a, u: _F.gelu(u, approximate="tanh"),
    _lib.ACT_MISH: lambda a, u: _F.mish(u),
}


def dae_acts(act):
    """The public `act=` of a DAE call -- None (both MLPs ELU(1)) or (de_act, ae_act) -- as the tuple of Act | None every call carries
    inside this package (an ODE call's is `(act,)`)."""
    return (None, None) if act is None else tuple(act)


def _act_ptrs(acts):
    """One ctypes pointer to a psnode_act_f32 per act, NULL for None = ELU(1).  (A pointer made by ctypes.byref holds on to its struct.)"""
    return [ctypes.byref(a.abi()) if a is not None else None for a in acts]


# What the entry points psnode_<stem>_<family>_* take behind the args struct, in this order: one psnode_act_f32 per MLP (acts), the tableau (tab),
# the sub-steps struct (sub), the segments struct (seg) and -- the _f32 call alone -- the per_trajectory int (pt).  tf_args: its dae_backward takes
# psnode_dae_bwd_tf_args_f32; x_sub: a forward call that saves for K5 keeps sub-state rows; workspace: the query that sizes its dae_backward -- "plain",
# its "own", or the "rk" family's (the same policy, so the same fit, checks and layout for any sub-steps).  par: the segments struct is
# psnode_segment_groups_f32, and both backward stems size their workspace with the family's own psnode_<stem>_<family>_workspace_size.
# stencil: behind the structs comes the device pointer of the int8 [T-1, B] stencil table (`lagrange_stencils`), or NULL.
# rkc: behind the acts comes the psnode_rkc_f32 alone (the recurrence with the stage rows, `Recurrence.abi`); its dae_backward query is _workspace_size.
# interp: behind the stencil table comes the int32 that picks the interpolant (1 linear, 2 Lagrange); dae_only: the family has no ODE entry points.
Family = collections.namedtuple("Family", "acts tab sub seg pt tf_args x_sub workspace par stencil rkc interp dae_only", defaults=(True, False, False, False, False, True, False, "own", False, False, False, False, False))
# The Python counterpart of kFamilies (csrc/psnode_generic_family.h): `GenericOpts`, `call_generic` and the prototypes of _lib.load read it.
# "plain": the entry points without a family in their name; "none": no entry point at all; "tf": the "plain" dae_backward with dataset rows.
FAMILIES = {
    "plain": Family(acts=False, tf_args=False, workspace="plain"),
    "none": Family(acts=False, tf_args=False, workspace="plain"),
    "tf": Family(acts=False),
    "act": Family(tf_args=False, workspace="plain"),
    "rk": Family(tab=True),
    "sub": Family(tab=True, sub=True, x_sub=True),
    "lin": Family(tab=True, sub=True, x_sub=True),
    "lag": Family(tab=True, sub=True, x_sub=True, stencil=True),
    "pev": Family(tab=True, sub=True, x_sub=True, workspace="rk"),
    "ab": Family(pt=True, x_sub=True, workspace="rk"),
    "ab3": Family(pt=True, x_sub=True, workspace="rk"),
    "ms": Family(tab=True, sub=True, seg=True, x_sub=True, workspace="rk"),
    "msp": Family(tab=True, sub=True, seg=True, x_sub=True, workspace="own", par=True),
    "rkc": Family(x_sub=True, rkc=True),
    "sth": Family(tab=True, sub=True, x_sub=True, stencil=True, interp=True, dae_only=True),
}
EXT_LINEAR, EXT_LAGRANGE = 1, 2      # == PSNODE_EXT_LINEAR / PSNODE_EXT_LAGRANGE

MAX_CHUNKS = 65535      # the launch grid's second dimension (csrc/psnode_generic_family.h: kMaxChunks)


def check_segment_parallel(segment_parallel, segment):
    """The value rules of `segment_parallel`: None, "auto" or an int g >= 1 (no bool); anything but None needs `segment`.  ValueError."""
    if segment_parallel is None:
        return
    if segment_parallel != "auto" and (isinstance(segment_parallel, bool) or not isinstance(segment_parallel, int) or segment_parallel < 1):
        raise ValueError(f"segment_parallel must be None, 'auto' or an int >= 1, got {segment_parallel!r}")
    if segment is None:
        raise ValueError(f"segment_parallel={segment_parallel!r} spreads the segments of segment= over workgroups: it needs segment (got None)")


def segment_chunks(T: int, segment: int, groups: int):
    """(per_group, [(k_lo, k_hi), ...]): the time chunks of a record of T grid points with a restart every `segment` steps when `groups`
    chunks are wanted -- n_seg = ceil((T - 1) / segment) segments, per_group = ceil(n_seg / min(groups, n_seg)) consecutive ones per chunk,
    chunk c the steps c per_group segment .. min((c + 1) per_group segment, T - 1) - 1.  A record without a step: (1, [])."""
    n_seg = -(-(T - 1) // segment) if T > 1 else 0
    if n_seg == 0:
        return 1, []
    per_group = -(-n_seg // min(groups, n_seg))
    span = per_group * segment
    return per_group, [(c * span, min((c + 1) * span, T - 1)) for c in range(-(-n_seg // per_group))]


def auto_segment_groups(B: int, cus: int) -> int:
    """The chunks segment_parallel="auto" asks for: as many as leave every CU at most one workgroup, max(1, CUs // tiles) with
    tiles = ceil(B / 16).  ("Segments in parallel on K0 / K5": what the measurements say of it.)"""
    return max(1, cus // max(1, -(-B // 16)))


def resolve_segment_parallel(segment_parallel, segment, T: int, B: int, dev=None, cus: Optional[int] = None) -> Optional[int]:
    """What a call with `segment_parallel` hands GenericOpts: the segments per chunk (`per_group`) where the record splits into more than
    one chunk, else None -- one chunk is the family "ms" unchanged.  "auto": `auto_segment_groups` from the device's multiprocessor count
    (`cus`, or read from `dev`).  An int the call got back from `GenericOpts.chunks` resolves to the same per_group again."""
    check_segment_parallel(segment_parallel, segment)
    if segment_parallel is None:
        return None
    if segment_parallel == "auto":
        if cus is None:
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
        segment_parallel = auto_segment_groups(B, cus)
    per_group, chunks = segment_chunks(T, segment, min(segment_parallel, MAX_CHUNKS))
    return per_group if len(chunks) > 1 else None


@dataclasses.dataclass(frozen=True)
class GenericOpts:
    """What a call asks of the generic kernels K0 / K5 beyond the three built-in formulas with ELU(1), one step per grid interval and held
    externals -- the Python counterpart of the library's K0Call: every public function builds one from its `method`, `act`, `substeps`
    and `externals` (`of`), and the value says which entry-point family the call takes (`family`, `call_generic`) and which calls are
    refused (`require_generic`, `require_plain`).  acts: one Act | None per MLP (ODE 1, DAE 2); tab: the Tableau of `method`, if it is one;
    method_id / stages: what the args struct and the saved rows need of `method` (`method_info`); per_trajectory: the call's event table
    is [T-1, B], every trajectory jumps at its own steps (only a call that HAS events carries it: `has_events`); ab: the method is two-step
    Adams-Bashforth ("ab2") -- the last option in the naming order; never together with a Tableau, sub-steps or interpolated
    externals (the solver's constructor refuses them; here a ValueError), with per_trajectory it stays the family "ab"; the value 3 is
    three-step Adams-Bashforth ("ab3", `ab_order`): the family "ab3", the same rules and refusals in its own words; segment: None, or
    an int w >= 1 -- multiple shooting, grid point k > 0 with k % w == 0 restarts from the dataset row (the family "ms", the sixth option in
    the naming order, in front of AB2, which refuses it; next to interpolated externals or per-trajectory events "none": no kernel);
    segment_parallel: None, or the segments per time chunk (an int >= 1, `resolve_segment_parallel`) of a call whose segments run side by
    side on a tiles x chunks launch grid -- the family "msp" in "ms"'s place; where the computation runs, never what is computed."""
    acts: tuple
    tab: Optional[Tableau]
    substeps: int = 1
    externals: str = "hold"
    method_id: int = _lib.EULER
    stages: int = 1
    per_trajectory: bool = False
    segment: Optional[int] = None
    # (init-only, like segment_parallel below and in front of `ab` for the reason given there: "stage" -- stage-wise algebraic heads, a DAE
    #  call with interpolated externals, more than one stage and its own i -- is the family "sth" in "lin" / "lag"'s place, so the compared
    #  value tells the two apart; an attribute of the value like every option)
    algebraic: dataclasses.InitVar[str] = "step"
    ab: bool = False      # (or 3: Adams-Bashforth 3, `ab_order`)
    # (init-only: behind `ab` in the constructor and an attribute of the value like every option, but no entry of dataclasses.fields() --
    #  the recorded field lists end with ab, family; the family, which is compared, tells "ms" from "msp")
    segment_parallel: dataclasses.InitVar[Optional[int]] = None
    family: str = dataclasses.field(init=False)

    @property
    def ab_order(self) -> int:
        """2, or 3 where `ab` is 3: three-step Adams-Bashforth ("ab3"), the family "ab3" in "ab"'s place.  (`ab` itself carries it -- False,
        True for "ab2", 3 for "ab3" -- because the recorded lists of fields and of constructor arguments end with ab / ab, segment_parallel.)"""
        return 3 if self.ab == 3 else 2

    def __post_init__(self, algebraic="step", segment_parallel=None):
        """Validates substeps and externals, and names the entry-point family: "ab" (two-step Adams-Bashforth, with or without
        per-trajectory events; a ValueError together with a Tableau, sub-steps or interpolated externals), else "pev" (per-trajectory events, every substeps >= 1; together
        with interpolated externals "none": no kernel carries both, `require_generic` refuses the call), else "lin" (linearly interpolated
        externals, every substeps >= 1) or "lag" (externals="lagrange": the same rules and refusals, its own entry points, which take the
        stencil table), else "sub" (substeps > 1), else "rk" (a Tableau), else "act" (an activation other than ELU(1)),
        else "plain"."""
        if isinstance(self.substeps, bool) or not isinstance(self.substeps, int) or not 1 <= self.substeps <= _lib.MAX_SUBSTEPS:
            raise ValueError(f"substeps must be an int in 1..{_lib.MAX_SUBSTEPS}, got {self.substeps!r}")
        if not isinstance(self.per_trajectory, bool):
            raise ValueError(f"per_trajectory must be a bool, got {self.per_trajectory!r}")
        if self.segment is not None and (isinstance(self.segment, bool) or not isinstance(self.segment, int) or self.segment < 1):
            raise ValueError(f"segment must be None or an int >= 1, got {self.segment!r}")
        if self.ab not in (False, True, 3):
            raise ValueError(f"ab must be False, True (Adams-Bashforth 2) or 3 (Adams-Bashforth 3), got {self.ab!r}")
        ab_order = self.ab_order
        if not isinstance(algebraic, str) or algebraic not in ALGEBRAIC:
            raise ValueError(f"algebraic must be one of {ALGEBRAIC}, got {algebraic!r}")
        object.__setattr__(self, "algebraic", algebraic)
        if algebraic == "stage":
            if self.ab:
                raise ValueError(f"Adams-Bashforth {ab_order} reads the right-hand side at grid points only: algebraic='stage' has no stages to act on")
            if isinstance(self.tab, Recurrence):
                raise ValueError(f"{self.tab.name} already evaluates the algebraic head in front of every stage: algebraic='stage' has nothing to add")
            if not is_linear(self.externals):
                raise ValueError("algebraic='stage' needs interpolated externals (externals='linear' / 'lagrange'): held rows cap every "
                                 "Runge-Kutta option at first order, and no build carries the pair")
        # (an ODE has no head, a one-stage method no stage s >= 1: the option is inert there and the call is the "step" call)
        sth = algebraic == "stage" and len(self.acts) == 2 and self.stages > 1
        if self.ab and ab_order == 3 and self.segment is not None:
            raise ValueError("Adams-Bashforth 3 carries the previous slopes from step to step: a multiple-shooting restart (segment=) has no "
                             f"form here (got segment={self.segment!r})")
        if self.ab and self.segment is not None:
            raise ValueError("Adams-Bashforth 2 carries the previous slope from step to step: a multiple-shooting restart (segment=) has no "
                             f"form here (got segment={self.segment!r})")
        sp = segment_parallel
        object.__setattr__(self, "segment_parallel", sp)
        if sp is not None and (isinstance(sp, bool) or not isinstance(sp, int) or sp < 1 or self.segment is None):
            raise ValueError(f"segment_parallel must be None or the segments per chunk (an int >= 1) of a call with segment, got {sp!r} "
                             f"(segment={self.segment!r})")
        if isinstance(self.tab, Recurrence):
            # a Runge-Kutta-Chebyshev recurrence rides in the tableau's field, told apart by type; `substeps` then holds its stage count (`of`
            # puts it there: the stage rows are sized and checked as the sub-state rows are), never sub-steps of the caller's
            if self.substeps != self.tab.stages or is_linear(self.externals) or self.segment is not None or self.ab:
                raise ValueError(f"{self.tab.name} takes one step per grid interval with held externals: no sub-steps (raise the stage count "
                                 f"instead), no interpolated externals, no segments (got substeps={self.substeps}, externals={self.externals!r}, "
                                 f"segment={self.segment!r})")
            fam = "none" if self.per_trajectory else "rkc"
        elif self.segment is not None:
            fam = "none" if (is_linear(self.externals) or self.per_trajectory) else ("ms" if sp is None else "msp")
        elif self.ab and ab_order == 3:
            if self.substeps != 1 or is_linear(self.externals) or self.tab is not None:
                raise ValueError(f"Adams-Bashforth 3 reads the right-hand side at grid points only: substeps != 1 and externals='{'lagrange' if self.externals == 'lagrange' else 'linear'}' would "
                                 f"need inputs between the dataset rows (got substeps={self.substeps}, externals={self.externals!r})")
            fam = "ab3"
        elif self.ab:
            if self.substeps != 1 or is_linear(self.externals) or self.tab is not None:
                raise ValueError(f"Adams-Bashforth 2 reads the right-hand side at grid points only: substeps != 1 and externals='{'lagrange' if self.externals == 'lagrange' else 'linear'}' would "
                                 f"need inputs between the dataset rows (got substeps={self.substeps}, externals={self.externals!r})")
            fam = "ab"
        elif self.per_trajectory:
            fam = "none" if is_linear(self.externals) else "pev"
        elif is_linear(self.externals):
            fam = "sth" if sth else ("lag" if is_lagrange(self.externals) else "lin")
        elif self.substeps > 1:
            fam = "sub"
        elif self.tab is not None:
            fam = "rk"
        else:
            fam = "act" if any(a is not None for a in self.acts) else "plain"
        object.__setattr__(self, "family", fam)
        object.__setattr__(self, "takes", FAMILIES[fam])      # (the family's row; an attribute, not a field of the dataclass)

    @staticmethod
    @functools.lru_cache(maxsize=256, typed=True)      # (a loop asks for the same immutable value call after call; typed: 2.0 and True are not 2 and 1)
    def of(method, acts: tuple, substeps: int = 1, externals: str = "hold", per_trajectory: bool = False, segment=None,
           segment_parallel=None, algebraic: str = "step") -> "GenericOpts":
        method_id, stages, tab = method_info(method)
        if isinstance(tab, Recurrence):      # (substeps: 1, the caller's, or the stage count a GenericOpts of this method hands on)
            if substeps not in (1, tab.stages):
                raise ValueError(f"{tab.name} takes one step per grid interval: substeps != 1 has no form here, raise the stage count instead "
                                 f"(got substeps={substeps!r})")
            substeps = tab.stages
        return GenericOpts(acts, tab, substeps, externals, method_id, stages, per_trajectory, segment, algebraic=algebraic,
                           ab=3 if ab_order(method) == 3 else is_ab(method), segment_parallel=segment_parallel)

    def chunks(self, T: int) -> Optional[int]:
        """The time chunks of a record of T grid points under these options (None without segment_parallel): as `segment_parallel=` of a
        further call on the same record it names the same grouping."""
        if self.segment_parallel is None:
            return None
        return max(1, -(-(-(-(T - 1) // self.segment)) // self.segment_parallel)) if T > 1 else 1

    def c_args(self, x_sub=None, x_true=None, family: Optional[str] = None, stencil=None) -> list:
        """The C arguments behind the args struct that the family's row of FAMILIES lists: the acts, the tableau or NULL (= the args' method),
        the sub-steps struct with `x_sub` or NULL, the segments struct with a backward call's `x_true` or NULL, the stencil table (`stencil`, an int8 [T-1, B] tensor) or NULL,
        per_trajectory.  The list
        owns the structs: keep it until the call has returned.  family: the entry point's, where it is not the options' own."""
        f = self.takes if family is None else FAMILIES[family]
        out = _act_ptrs(self.acts) if f.acts else []
        if f.rkc:
            out.append(ctypes.byref(self.tab.abi(x_sub.data_ptr() if x_sub is not None and x_sub.numel() else None)))
        if f.tab:
            out.append(ctypes.byref(self.tab.abi()) if self.tab is not None else None)
        if f.sub:
            out.append(ctypes.byref(_lib.SubstepsF32(self.substeps, x_sub.data_ptr() if x_sub is not None and x_sub.numel() else None)))
        if f.seg:
            rows = x_true.data_ptr() if x_true is not None and x_true.numel() else None
            every = min(self.segment, 0x7fffffff)      # (a segment longer than any record: no restart)
            if f.par:
                out.append(ctypes.byref(_lib.SegmentGroupsF32(every, rows, min(self.segment_parallel or 1, 0x7fffffff))))
            else:
                out.append(ctypes.byref(_lib.SegmentsF32(every, rows)))
        if f.stencil:
            out.append(ctypes.c_void_p(stencil.data_ptr() if stencil is not None and stencil.numel() else None))
        if f.interp:
            out.append(ctypes.c_int32(EXT_LAGRANGE if is_lagrange(self.externals) else EXT_LINEAR))
        if f.pt:      # (handed to the query too, which does not declare it and never reads it)
            out.append(ctypes.c_int32(1 if self.per_trajectory else 0))
        return out

    def dae_backward_args(self, rows: bool):
        """The args struct of a dae_backward call: psnode_dae_bwd_tf_args_f32 (flags 0 = no dataset rows) where the family's row of FAMILIES
        says so and for a call with dataset rows x_true / i_true (which is "tf" where it would be "plain"), else psnode_dae_bwd_args_f32."""
        assert not (rows and self.family == "act"), "dae_backward: dataset rows with an activation other than ELU(1) have no entry point"
        return _lib.DaeBwdTfArgsF32() if rows or self.takes.tf_args else _lib.DaeBwdArgsF32()

    def _first_option(self) -> str:
        """The first option the call carries, in the fixed order act, tableau, sub-steps, externals, as the subject of a refusal."""
        if any(a is not None for a in self.acts):
            return "an activation other than ELU(alpha=1) runs"
        if isinstance(self.tab, Recurrence):
            return f"a Runge-Kutta-Chebyshev recurrence ({self.tab.name}) runs"
        if self.tab is not None:
            return f"a Runge-Kutta tableau ({self.tab.name}) runs"
        if self.substeps != 1:
            return f"sub-steps per grid interval (substeps={self.substeps}) run"
        if self.externals != "hold":
            return _externals_text(self.externals) + " run"
        if self.per_trajectory:
            return "per-trajectory events (per_trajectory=True) run"
        if self.segment is not None:
            return f"multiple-shooting segments (segment={self.segment}) run"
        return "three-step Adams-Bashforth (AB3) runs" if self.ab_order == 3 else "two-step Adams-Bashforth (AB2) runs"

    def require_generic(self, what: str, kernel: str, saved: bool, teacher_forced: bool = False):
        """The options run on the generic kernels only: UnsupportedShapeError, naming the first option in the order act, tableau, sub-steps,
        externals, unless the kernel is "auto" / "generic" and no saved rows are asked for or given.  teacher_forced (an ode_backward with
        dataset rows): K5 has no such form for an activation other than ELU(1).  The fifth option in that order is per-trajectory events;
        together with interpolated externals they have no kernel at all."""
        if self.family == "plain":
            return
        self.no_teacher_forcing(what, teacher_forced)
        if self.family == "none" and isinstance(self.tab, Recurrence):
            raise _lib.UnsupportedShapeError(f"{what}: per-trajectory events (per_trajectory=True) together with a Runge-Kutta-Chebyshev "
                                             f"recurrence ({self.tab.name}) have no fused form: the recurrence build of K0 / K5 takes the shared event table")
        if self.family == "none" and self.segment is not None:
            raise _lib.UnsupportedShapeError(f"{what}: multiple-shooting segments (segment={self.segment}) together with "
                                             + (_externals_text(self.externals) if is_linear(self.externals)
                                                else "per-trajectory events (per_trajectory=True)")
                                             + " have no fused form: the multiple-shooting build of K0 / K5 holds the externals and takes the shared event table")
        if self.family == "none":
            raise _lib.UnsupportedShapeError(f"{what}: per-trajectory events (per_trajectory=True) together with {_externals_text(self.externals)} "
                                             "have no fused form: K0 / K5 carry either, not both")
        if kernel not in ("auto", "generic") or saved:
            raise _lib.UnsupportedShapeError(f"{what}: {self._first_option()} on the generic kernels K0 / K5 only (kernel 'auto' / 'generic', no saved rows); "
                                             f"got kernel={kernel!r}, saved rows={saved}")
        if teacher_forced and any(a is not None for a in self.acts):
            raise _lib.UnsupportedShapeError(f"{what}: an activation other than ELU(alpha=1) runs on the generic backward K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows, no teacher forcing)")

    def no_teacher_forcing(self, what: str, teacher_forced: bool):
        """Adams-Bashforth 2, or segments, with input_true_x / input_true_i: ValueError, on every path."""
        if self.segment is not None and teacher_forced:
            raise ValueError(f"{what}: segment={self.segment} and input_true_x / input_true_i exclude each other (every teacher-forced step "
                             "restarts from the dataset already)")
        if self.ab and self.ab_order == 3 and teacher_forced:
            raise ValueError(f"{what}: Adams-Bashforth 3 has no teacher-forced form -- every teacher-forced step starts from a dataset row, "
                             "so the previous slopes a multistep method carries are undefined")
        if self.ab and teacher_forced:
            raise ValueError(f"{what}: Adams-Bashforth 2 has no teacher-forced form -- every teacher-forced step starts from a dataset row, "
                             "so the previous slope a multistep method carries is undefined")

    def require_plain(self, what: str):
        """(method id, stages) for the specialised, latent, encoded and saved-row entries, which carry the three built-in formulas with one
        step per grid interval and held externals: UnsupportedShapeError for sub-steps, interpolated externals or a Tableau."""
        if isinstance(self.tab, Recurrence):
            builtin_method(self.tab, what)
        if self.substeps != 1:
            raise _lib.UnsupportedShapeError(f"{what}: sub-steps per grid interval (substeps={self.substeps}) run on the generic kernels K0 / K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows); this entry point takes one step per interval")
        if self.externals != "hold":
            raise _lib.UnsupportedShapeError(f"{what}: {_externals_text(self.externals)} run on the generic kernels "
                                             "K0 / K5 only (kernel 'auto' / 'generic', no saved rows); this entry point holds them over a step")
        if self.tab is not None:
            builtin_method(self.tab, what)
        if self.per_trajectory:
            raise _lib.UnsupportedShapeError(f"{what}: per-trajectory events (per_trajectory=True) run on the generic kernels K0 / K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows); this entry point jumps the whole batch at the steps "
                                             "of one int32[T-1] table")
        if self.segment is not None:
            raise _lib.UnsupportedShapeError(f"{what}: multiple-shooting segments (segment={self.segment}) run on the generic kernels K0 / K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows); this entry point runs free from the first row to the last")
        if self.ab and self.ab_order == 3:
            raise _lib.UnsupportedShapeError(f"{what}: three-step Adams-Bashforth (AB3) runs on the generic kernels K0 / K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows); this entry point carries euler / midpoint / rk4")
        if self.ab:
            raise _lib.UnsupportedShapeError(f"{what}: two-step Adams-Bashforth (AB2) runs on the generic kernels K0 / K5 only "
                                             "(kernel 'auto' / 'generic', no saved rows); this entry point carries euler / midpoint / rk4")
        return self.method_id, self.stages


def call_generic(lib, stem: str, kind: str, args, opts: GenericOpts, *tail, x_sub=None, x_true=None, stencil=None):
    """The one place that picks an entry point of the generic-kernel families and calls it: psnode_<stem>[_<family>]_<kind>(args, the
    family's `c_args`, *tail).  stem: "ode_integrate", "dae_integrate", "ode_backward", "dae_backward"; kind: "f32" (tail: workspace
    pointer, its size, stream), "supported" or, for the backward stems, "workspace_bytes".  A dae_backward whose `args` is a
    psnode_dae_bwd_tf_args_f32 (`dae_backward_args`) and whose family would be "plain" takes the "tf" entry points.  The workspace of
    ode_backward is the plain query's, that of dae_backward the one its family's row of FAMILIES names.  The family "none" has no entry
    point: its "supported" is 0, any other kind is the caller's mistake (`require_generic` refuses such a call first).
    Returns (status or value, the symbol)."""
    fam = opts.family
    if fam == "none":
        assert kind == "supported", f"{stem}: per-trajectory events with interpolated externals (or segments next to either) have no entry point"
        return 0, f"psnode_{stem}_{kind}"
    if isinstance(args, _lib.DaeBwdTfArgsF32):
        assert stem == "dae_backward" and fam != "act", f"{stem}: no entry point takes dataset rows and the acts {opts.acts} alone"
        fam = "tf" if fam == "plain" else fam
    if kind == "workspace_bytes" and (FAMILIES[fam].stencil or FAMILIES[fam].rkc) and stem == "dae_backward":      # (the family's own query, under this name)
        name = f"psnode_{stem}_{fam}_workspace_size"
        return getattr(lib, name)(ctypes.byref(args), *opts.c_args(x_sub, x_true, fam, stencil), *tail), name
    if kind == "workspace_bytes" and FAMILIES[fam].par:      # (the segment-parallel family sizes both backward stems itself)
        name = f"psnode_{stem}_{fam}_workspace_size"
        return getattr(lib, name)(ctypes.byref(args), *opts.c_args(x_sub, x_true, fam, stencil), *tail), name
    if kind == "workspace_bytes":
        assert stem in ("ode_backward", "dae_backward"), f"{stem} has no workspace query of its own"
        query = "plain" if stem == "ode_backward" else FAMILIES[fam].workspace
        if query == "plain":
            fam = "plain"
        elif query == "rk":
            # the _rk query with the call's acts and tableau -- a built-in method's stand-in is the one-stage tableau, the size does not depend on it
            tab = opts.tab.abi() if opts.tab is not None else _lib.RkTableauF32()
            if opts.tab is None:
                tab.stages, tab.b[0] = 1, 1.0
            name = f"psnode_{stem}_rk_{kind}"
            return getattr(lib, name)(ctypes.byref(args), *_act_ptrs(opts.acts), ctypes.byref(tab), *tail), name
    if fam == "plain":
        name = f"psnode_{stem}_{kind}"
        return getattr(lib, name)(ctypes.byref(args), *tail), name
    name = f"psnode_{stem}_{fam}_{kind}"
    return getattr(lib, name)(ctypes.byref(args), *opts.c_args(x_sub, x_true, fam, stencil), *tail), name


def act_of_module(m) -> Optional[object]:
    """`False` if `m` is no activation the generic kernels apply, None for ELU(alpha=1), else its Act."""
    t = type(m)
    if t is nn.ELU:
        a = float(m.alpha)
        if a == 1.0:
            return None
        return Act(_lib.ACT_ELU, alpha=a, name=f"ELU(alpha={a})") if a > 0 and math.isfinite(a) else False
    if t is nn.Tanh:
        return Act(_lib.ACT_TANH, name="Tanh")
    if t is nn.Sigmoid:
        return Act(_lib.ACT_SIGMOID, name="Sigmoid")
    if t is nn.ReLU:
        return Act(_lib.ACT_RELU, name="ReLU")
    if t is nn.LeakyReLU:
        s = float(m.negative_slope)
        return Act(_lib.ACT_LEAKY_RELU, alpha=s, name=f"LeakyReLU({s})") if s >= 0 and math.isfinite(s) else False
    if t is nn.Softplus:
        b, th = float(m.beta), float(m.threshold)
        ok = b > 0 and math.isfinite(b) and math.isfinite(th)
        return Act(_lib.ACT_SOFTPLUS, beta=b, threshold=th, name=f"Softplus(beta={b}, threshold={th})") if ok else False
    return False


def _sequential_one_act(seq, recognise):
    """(layers, act) if `seq` is nn.Sequential(Linear, A, Linear, ..., A, Linear) with ONE activation A throughout that `recognise` maps to
    an Act (or None = ELU(1)), else None."""
    if not isinstance(seq, nn.Sequential) or len(seq) == 0 or len(seq) % 2 == 0:
        return None
    out, acts = [], []
    for k, m in enumerate(seq):
        if k % 2 == 0:
            if type(m) is not nn.Linear or m.bias is None:
                return None
            out.append((m.weight, m.bias))
        else:
            a = recognise(m)
            if a is False:
                return None
            acts.append(a)
    if any(a != acts[0] for a in acts[1:]):
        return None
    if len(out) > _lib.MAX_LAYERS:
        return None
    for (w, _), (w2, _) in zip(out[:-1], out[1:]):
        if w2.shape[1] != w.shape[0]:
            return None
    return out, (acts[0] if acts else None)


def sequential_mlp(seq):
    """(layers, act) if `seq` is nn.Sequential(Linear, A, Linear, ..., A, Linear) with ONE activation A throughout that the generic kernels
    apply (ELU(alpha > 0), Tanh, Sigmoid, ReLU, LeakyReLU(slope >= 0), Softplus(beta > 0)); act None = ELU(1).  Else None (mixed activations
    included)."""
    return _sequential_one_act(seq, act_of_module)


def sequential_layers(seq) -> Optional[List[Tuple[torch.Tensor, torch.Tensor]]]:
    """[(W,b), ...] if `seq` is nn.Sequential(Linear, ELU(alpha=1), Linear, ..., Linear), else None
    (the only MLP shape the reference's live right-hand sides use, neural_00_ODE_01_no_encode.py:61-64)."""
    return _elu1_layers(sequential_mlp(seq))


def pre_act_of_module(m) -> Optional[object]:
    """`False` if `m` is no activation of the pre-activation family (derivative from the pre-activation u: SiLU, GELU (erf or tanh form),
    Mish), else its Act."""
    t = type(m)
    if t is nn.SiLU:
        return Act(_lib.ACT_SILU, name="SiLU")
    if t is nn.GELU:
        if m.approximate == "none":
            return Act(_lib.ACT_GELU, name="GELU")
        if m.approximate == "tanh":
            return Act(_lib.ACT_GELU_TANH, name="GELU(approximate='tanh')")
        return False
    if t is nn.Mish:
        return Act(_lib.ACT_MISH, name="Mish")
    return False


def sequential_mlp_any(seq):
    """(layers, act) as `sequential_mlp`, with ONE activation throughout from either family: those of `act_of_module` (derivative from the
    layer output) or those of `pre_act_of_module` (SiLU, GELU, Mish: derivative from the pre-activation).  Else None (mixed activations,
    within a family or across the two, included)."""
    def either(m):
        a = act_of_module(m)
        return pre_act_of_module(m) if a is False else a
    return _sequential_one_act(seq, either)


def _rhs_mlp_of(mod, attr: str, in_dim: int, out_dim: int):
    """(layers, act) of a right-hand-side module whose only parameters are those of its Sequential `attr`, an MLP of `sequential_mlp_any`
    from in_dim to out_dim; else None."""
    if not isinstance(mod, nn.Module) or _overrides_forward_hooks(mod):
        return None
    r = sequential_mlp_any(getattr(mod, attr, None))
    if r is None or r[0][0][0].shape[1] != in_dim or r[0][-1][0].shape[0] != out_dim:
        return None
    return r if _only_params_of(mod, getattr(mod, attr)) else None


def _elu1_layers(r):
    return r[0] if r is not None and r[1] is None else None


def de_mlp_of(x_func, n: int, x_dim: int):
    """(layers, act) of a DE_Func (attribute `x_dot`, input recipe cat(a0, s-a0, s)) whose MLP has any activation of
    `sequential_mlp_any` (act None = ELU(1)), else None."""
    return _rhs_mlp_of(x_func, "x_dot", 3 * n, x_dim)


def ae_mlp_of(i_func, n: int, m: int, i_dim: int):
    """(layers, act) of an AE_Func (attribute `i_calculator`, input recipe cat(a0, x, z, v)) whose MLP has any activation of
    `sequential_mlp_any` (act None = ELU(1)), else None."""
    return _rhs_mlp_of(i_func, "i_calculator", n + m, i_dim)


def de_layers_of(x_func, n: int, x_dim: int):
    """Layers of a DE_Func with ELU(1) hidden layers (`de_mlp_of` with act None), else None."""
    return _elu1_layers(de_mlp_of(x_func, n, x_dim))


def ae_layers_of(i_func, n: int, m: int, i_dim: int):
    """Layers of an AE_Func with ELU(1) hidden layers (`ae_mlp_of` with act None), else None."""
    return _elu1_layers(ae_mlp_of(i_func, n, m, i_dim))


def _mlp_eval(layers, u, act=None):
    for k, (w, b) in enumerate(layers):
        u = nn.functional.linear(u, w, b)
        if k + 1 < len(layers):
            u = nn.functional.elu(u) if act is None else act(u)
    return u


def _recipe_ok(mod: nn.Module, layers, kind: str, widths, act=None) -> bool:
    """Does `mod.forward` really compute the recipe the kernels hard-code?  The structural checks (attribute name, Sequential
    shape, no extra parameters) say nothing about forward(): a user DE_Func that scales its output, uses t0 or concatenates in
    another order would be integrated WRONGLY.  One numeric probe per (module, forward function): a few random rows through the
    module's own forward against MLP(cat(a0, s - a0, s)) (DE) / MLP(cat(a0, x, z, v)) (AE) on the module's device.  The result
    is cached on the module; this package's own classes are known and skip the probe."""
    fwd = type(mod).forward
    if getattr(fwd, "_psnode_recipe", None) == kind:
        return True
    key = (fwd, kind, tuple(widths), act)
    cached = mod.__dict__.get("_psnode_probe")
    if cached is not None and cached[0] == key:
        return cached[1]
    ok = False
    try:
        w0 = layers[0][0]
        dev, dt = w0.device, w0.dtype
        g = torch.Generator(device="cpu").manual_seed(1234)
        R = 5
        parts = [torch.randn(R, d, generator=g).to(device=dev, dtype=dt) for d in widths]
        a0 = torch.randn(R, sum(widths), generator=g).to(device=dev, dtype=dt)
        t0 = torch.rand(R, 1, generator=g).to(device=dev, dtype=dt)
        with torch.no_grad():
            if kind == "de_ode":
                got = mod(t0=t0, xt=parts[0], zt=parts[1], all_initial=a0)
                s_ = torch.cat(parts, -1)
                want = _mlp_eval(layers, torch.cat((a0, s_ - a0, s_), -1), act)
            elif kind == "de_dae":
                got = mod(t0=t0, xt=parts[0], zt=parts[1], vt=parts[2], it=parts[3], all_initial=a0)
                s_ = torch.cat(parts, -1)
                want = _mlp_eval(layers, torch.cat((a0, s_ - a0, s_), -1), act)
            else:   # "ae": all_initial spans x|z|v|i, the inputs x, z, v
                a0 = torch.randn(R, widths[3], generator=g).to(device=dev, dtype=dt)
                got = mod(xt=parts[0], zt=parts[1], vt=parts[2], all_initial=a0)
                want = _mlp_eval(layers, torch.cat((a0, parts[0], parts[1], parts[2]), -1), act)
            ok = bool(got.shape == want.shape and torch.allclose(got, want, rtol=1e-4, atol=1e-6))
    except Exception:
        ok = False
    mod.__dict__["_psnode_probe"] = (key, ok)
    return ok


def _overrides_forward_hooks(mod: nn.Module) -> bool:
    return bool(mod._forward_hooks) or bool(mod._forward_pre_hooks)


def _only_params_of(mod: nn.Module, seq: nn.Module) -> bool:
    """A module is taken to follow the DE / AE input recipe when its only parameters are those of its
    `x_dot` / `i_calculator` Sequential (true of every live DE_Func / AE_Func in the reference scripts; the
    legacy neural_base.DE_Func has many more sub-modules and neither attribute, so it never gets here)."""
    return {id(p) for p in mod.parameters()} == {id(p) for p in seq.parameters()}


# ----------------------------------------------------------------------------- marshalling
def _f32_dev(t: torch.Tensor, dev, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: fused integrator is fp32-only, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{name}: on {t.device}, expected {dev}")
    return t.detach()


def _view(t: Optional[torch.Tensor], dev, name: str, keep: list) -> _lib.ViewF32:
    """[T,B,D] tensor -> strided view struct; copies only when the last dim is not unit-stride."""
    if t is None or t.shape[-1] == 0:
        return _lib.ViewF32(None, 0, 0)
    t = _f32_dev(t, dev, name)
    if t.shape[-1] > 1 and t.stride(2) != 1:
        t = t.contiguous()
    keep.append(t)
    return _lib.ViewF32(t.data_ptr(), t.stride(0), t.stride(1))


def _aligned16(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The MFMA backward kernels of the latent shapes read rows as float4: a view whose base or strides are not 16-byte aligned
    would make the library report 'unsupported' AFTER the fused forward has run (the generic backward does not fit those shapes).
    Such a view -- rare: torch allocations are 256-byte aligned, widths there are multiples of 16 -- is copied once."""
    if t is None or t.shape[-1] < 4:
        return t
    if t.data_ptr() % 16 or t.stride(-1) != 1 or any(st % 4 for st in t.stride()[:-1]):
        return t.contiguous()
    return t


def _mlp(layers: Layers, dev, name: str, keep: list) -> _lib.MlpF32:
    m = _lib.MlpF32()
    if not 1 <= len(layers) <= _lib.MAX_LAYERS:
        raise ValueError(f"{name}: {len(layers)} Linear layers, supported 1..{_lib.MAX_LAYERS}")
    m.n_layers = len(layers)
    m.in_dim = layers[0][0].shape[1]
    for k, (w, b) in enumerate(layers):
        w = _f32_dev(w, dev, f"{name}.weight[{k}]").contiguous()
        b = _f32_dev(b, dev, f"{name}.bias[{k}]").contiguous()
        keep += [w, b]
        m.out_dim[k] = w.shape[0]
        m.weight[k] = w.data_ptr()
        m.bias[k] = b.data_ptr()
    return m


def _ms_rows(what: str, segment, x_true, T: int, B: int, xd: int, dev):
    """The dataset rows a backward call with `segment` reads where a step restarts (T - 1 > segment): contiguous fp32 [T, B, xd] on the
    call's device (a shorter tensor would be read out of bounds); None where no step restarts."""
    if segment is None or T - 1 <= segment:
        return None
    if x_true is None or x_true.dim() != 3 or x_true.shape[0] < T or tuple(x_true.shape[1:]) != (B, xd):
        raise ValueError(f"{what}: segment={segment} needs x_true, the dataset rows [T={T}, B={B}, {xd}] the forward call restarted from, got "
                         f"{None if x_true is None else tuple(x_true.shape)}")
    return _f32_dev(x_true.detach(), dev, "x_true").contiguous()


def _check_x_sub(what: str, substeps: int, x_sub, T: int, B: int, xd: int, dev):
    """A backward call with substeps > 1 reads x_sub as a raw pointer: the contiguous fp32 [T-1, substeps-1, B, xd] tensor on the call's
    device that the forward call returned (a shorter one would be read out of bounds)."""
    if substeps > 1 and T >= 2 and (x_sub is None or tuple(x_sub.shape) != (T - 1, substeps - 1, B, xd) or not x_sub.is_contiguous()
                                    or x_sub.dtype != torch.float32 or x_sub.device != dev):
        raise ValueError(f"{what}: substeps={substeps} needs x_sub, the contiguous fp32 [{T - 1},{substeps - 1},{B},{xd}] tensor the "
                         "forward call returned with save_sub=True")


def _check_tb(name: str, a: Optional[torch.Tensor], T: int, B: int, min_T: Optional[int] = None):
    """Leading dims of a time-major input against the call's (T, B): a mismatch would be an out-of-bounds device read."""
    if a is None or a.shape[-1] == 0:
        return
    need_T = T if min_T is None else min_T
    if a.dim() != 3 or a.shape[1] != B or a.shape[0] < need_T:
        raise ValueError(f"{name}: shape {tuple(a.shape)} does not cover [T={need_T}, B={B}, D]")


def _check_jump(name: str, j: Optional[torch.Tensor], B: int, width: int, event_idx):
    if event_idx is None or width == 0:
        return
    if j is None:
        raise ValueError(f"{name}: events need the jump values")
    if j.dim() != 3 or j.shape[0] != B or j.shape[2] != width or j.shape[1] < 1:
        raise ValueError(f"{name}: shape {tuple(j.shape)}, expected [B={B}, nE>=1, {width}]")


def _jump(j: Optional[torch.Tensor], dev, name: str, keep: list):
    if j is None or j.shape[-1] == 0:
        return None, 0, 0
    j = _f32_dev(j, dev, name)
    if j.shape[-1] > 1 and j.stride(2) != 1:
        j = j.contiguous()
    keep.append(j)
    return j.data_ptr(), j.stride(0), j.stride(1)


def _bind_jumps(a, event_idx, jumps, dev, keep: list):
    """Binds the event table and each jump of `jumps` = (("z_jump", tensor), ...) into the args struct `a` (fields <name>, <zj|vj>_stride_b,
    <zj|vj>_stride_e); nothing when there is no table."""
    if event_idx is None:
        return
    keep.append(event_idx)
    a.event_idx = event_idx.data_ptr()
    for name, j in jumps:
        ptr, sb, se = _jump(j, dev, name, keep)
        setattr(a, name, ptr)
        setattr(a, f"{name[0]}j_stride_b", sb)
        setattr(a, f"{name[0]}j_stride_e", se)


def has_events(t, event_t, event_idx=None) -> bool:
    """Does a call with these arguments have an event table (the caller's, or `event_table`'s: not None)?  Only such a call carries the
    event rule: a per-trajectory call without events is the event-less call."""
    return event_idx is not None or (event_t is not None and t.shape[0] >= 2 and event_t.shape[1] > 0)


def check_event_idx(event_idx, T: int, B: int, per_trajectory: bool, dev):
    """A caller's event table reaches the kernels as a raw pointer: int32[T-1], or -- per-trajectory events -- a contiguous int32[T-1, B]
    on the call's device (a shorter one would be read out of bounds)."""
    if per_trajectory:
        if event_idx.dtype != torch.int32 or tuple(event_idx.shape) != (T - 1, B) or not event_idx.is_contiguous() or event_idx.device != dev:
            raise ValueError(f"event_idx must be a contiguous int32[T-1={T - 1}, B={B}] on {dev} (per-trajectory events), got "
                             f"{event_idx.dtype}{list(event_idx.shape)} on {event_idx.device}")
    elif event_idx.numel() < T - 1 or event_idx.dtype != torch.int32:
        raise ValueError(f"event_idx must be int32[T-1={T - 1}], got {event_idx.dtype}[{event_idx.numel()}]")


def _bind_events(a, t, event_t, event_idx, check_events: bool, jumps, B: int, dev, keep: list, per_trajectory: bool = False):
    """Event prologue of the forward entry points: the caller's `event_idx` (int32[T-1], or int32[T-1, B] for per-trajectory events;
    validated) or the table of `event_t` (`event_table`), the jumps' shapes (`jumps` = ((name, tensor, width), ...)) and `_bind_jumps`.
    Returns the table, None = no events."""
    T = t.shape[0]
    if event_idx is None:
        event_idx = event_table(t, event_t, check_events, per_trajectory=per_trajectory)
    else:
        check_event_idx(event_idx, T, B, per_trajectory, dev)
    if event_idx is not None:
        for name, j, width in jumps:
            _check_jump(name, j, B, width, event_idx)
        _bind_jumps(a, event_idx, [(name, j) for name, j, _ in jumps], dev, keep)
    return event_idx


def event_table(t: torch.Tensor, event_t: Optional[torch.Tensor], check_duplicates: bool = False,
                per_trajectory: bool = False) -> Optional[torch.Tensor]:
    """int32[T-1] device table: index of the event at each step, -1 = none.

    Same decision as ODE_Event.event_fn / jump_change_fn (neural_base.py:52-62): trajectory 0's clock
    against trajectory 0's event list, exact fp32 equality -- resolved by one tiny kernel instead of one
    host sync per step.  `check_duplicates` synchronises and raises where the reference would
    (two events at one time make its `.view(z0.shape)` fail).

    per_trajectory=True: int32[T-1, B], row-major [k][b] -- trajectory b's clock t[k, b] against trajectory b's own list event_t[b, :],
    the same equality, the lowest matching column; an entry that matches no clock value (NaN: the padding of a shorter list) never
    fires; `check_duplicates` then raises for a duplicate in ANY trajectory (ODE_Event.hit_mask / jump_change_fn are the definition).
    """
    T = t.shape[0]
    if event_t is None or T < 2 or event_t.shape[1] == 0:      # an empty event list is "no events", as in the reference
        return None
    lib = _lib.load()
    dev = t.device
    t_arg, event_arg = t, event_t          # the caller's objects: what the duplicate-check memo is keyed on (detach() makes new ones)
    t = _f32_dev(t, dev, "t")
    event_t = _f32_dev(event_t, dev, "event_t")
    dup = torch.zeros(1, dtype=torch.int32, device=dev)
    n_ev = event_t.shape[1]
    st = torch.cuda.current_stream(dev).cuda_stream
    if per_trajectory:
        B = t.shape[1]
        if t.dim() != 3 or event_t.dim() not in (2, 3) or event_t.shape[0] != B:
            raise ValueError(f"per-trajectory events need t [T, B, 1] and event_t [B, nE(, 1)], got {tuple(t.shape)} and {tuple(event_t.shape)}")
        tab = _empty((T - 1, B), dtype=torch.int32, device=dev)
        rc = lib.psnode_event_table_pt_f32(T - 1, B, t.data_ptr(), t.stride(0), t.stride(1), event_t.data_ptr(), event_t.stride(0),
                                           event_t.stride(1), n_ev, tab.data_ptr(), dup.data_ptr(), st)
        _lib.check(rc, "psnode_event_table_pt_f32")
    else:
        tab = _empty(T - 1, dtype=torch.int32, device=dev)
        rc = lib.psnode_event_table_f32(T - 1, t.data_ptr(), t.stride(0), event_t.data_ptr(), event_t.stride(1), n_ev,
                                        tab.data_ptr(), dup.data_ptr(), st)
        _lib.check(rc, "psnode_event_table_f32")
    if check_duplicates and not _dup_check_known(t_arg, event_arg, per_trajectory):
        if int(dup.item()):
            raise RuntimeError("two events of one trajectory share one time stamp: jump_change_fn takes one event per trajectory and step"
                               if per_trajectory else
                               "two events share one time stamp: the reference's jump_change_fn cannot view "
                               "z_jump[:, mask] as z0.shape (neural_base.py:61)")
        _dup_check_remember(t_arg, event_arg, per_trajectory)
    return tab


# (clock, event list) pairs already found free of duplicate event times: the same tensor OBJECTS (or views of the same base objects)
# at the same in-place version need no second 4-byte read-back -- which is a device synchronisation per call, 0.9 ms of a 0.94 ms
# ODE_02 forward (profiles/scripts/host_overhead.py); a new batch is a new object and is checked.
_DUP_OK = {}      # id(event tensor's base) -> (weakref to it, key of the event view, weakref to the clock's base, key of the clock view)


def _dup_key(t):
    base = t._base if t._base is not None else t
    return base, (t.data_ptr(), tuple(t.shape), tuple(t.stride()), base._version)


def _dup_check_known(t, event_t, per_trajectory: bool = False) -> bool:
    """(per_trajectory: the rule a pair was checked under is remembered with it -- trajectory 0 free of duplicates says nothing about the
    other trajectories)"""
    eb, ek = _dup_key(event_t)
    tb, tk = _dup_key(t)
    hit = _DUP_OK.get(id(eb))
    return hit is not None and hit[0]() is eb and hit[1] == ek and hit[2]() is tb and hit[3] == tk and hit[4] == bool(per_trajectory)


def _dup_check_remember(t, event_t, per_trajectory: bool = False):
    eb, ek = _dup_key(event_t)
    tb, tk = _dup_key(t)
    ident = id(eb)
    _DUP_OK[ident] = (weakref.ref(eb, lambda _r, ident=ident: _DUP_OK.pop(ident, None)), ek, weakref.ref(tb), tk, bool(per_trajectory))


def _workspace_of(nbytes: int, dev):
    """A workspace of `nbytes` (what the call's *_workspace_bytes query answered) for one library call: the tensor that owns it (keep it
    until the call is enqueued), the 256-byte aligned address inside it and the bytes usable from there."""
    ws = _empty(nbytes + 256, dtype=torch.uint8, device=dev)
    p = (ws.data_ptr() + 255) // 256 * 256
    return ws, p, ws.numel() - (p - ws.data_ptr())


def _padded_hidden(h: int) -> int:
    """Width class the MFMA kernels run a hidden width at (csrc/psnode_pack.h: padded_hidden): rows they store have this many columns,
    the ones beyond `h` are exact zeros."""
    return 32 if h <= 32 else (64 if h <= 64 else 128)


def _pad_rows(m: torch.Tensor, rows: int) -> torch.Tensor:
    return m if m.shape[0] == rows else torch.cat((m, m.new_zeros((rows - m.shape[0],) + tuple(m.shape[1:]))), 0)


def gemm_tn(a2: torch.Tensor, b2: torch.Tensor, want_colsum: bool = False):
    """K10 (psnode_gemm_tn_f32): a2^T @ b2 for tall-skinny fp32 [R, p], [R, q] row tensors on the hand-written MFMA contraction kernel
    (rows as the contraction index, deterministic partial sums); with want_colsum also sum_r a2[r, :].  None if the shapes / alignment
    are outside the kernel's class (p, q <= 128 and multiples of 4, 16-byte aligned rows) -- the caller then decides."""
    if a2.dim() != 2 or b2.dim() != 2 or a2.shape[0] != b2.shape[0] or a2.device.type != "cuda" or a2.dtype != torch.float32 or b2.dtype != torch.float32:
        return None
    if a2.stride(1) != 1:
        a2 = a2.contiguous()
    if b2.stride(1) != 1:
        b2 = b2.contiguous()
    if a2.shape[0] == 0:      # nothing to contract (an empty tensor has no device pointer to hand over)
        if a2.shape[1] > 128 or b2.shape[1] > 128 or (a2.shape[1] & 3) or (b2.shape[1] & 3):
            return None
        c = torch.zeros((a2.shape[1], b2.shape[1]), dtype=torch.float32, device=a2.device)
        return (c, torch.zeros(a2.shape[1], dtype=torch.float32, device=a2.device)) if want_colsum else c
    lib = _lib.load()
    a = _lib.GemmTnArgsF32()
    a.rows, a.M, a.N = a2.shape[0], a2.shape[1], b2.shape[1]
    a.A, a.lda, a.B, a.ldb = a2.data_ptr(), a2.stride(0) if a2.shape[0] > 1 else a2.shape[1], b2.data_ptr(), b2.stride(0) if b2.shape[0] > 1 else b2.shape[1]
    if not lib.psnode_gemm_tn_supported(ctypes.byref(a)):
        return None
    dev = a2.device
    with torch.cuda.device(dev):
        c = _empty((a.M, a.N), dtype=torch.float32, device=dev)
        cs = _empty((a.M,), dtype=torch.float32, device=dev) if want_colsum else None
        a.C = c.data_ptr()
        a.colsum_a = cs.data_ptr() if cs is not None else None
        ws, wp, wn = _workspace_of(lib.psnode_gemm_tn_workspace_bytes(ctypes.byref(a)), dev)
        _lib.check(lib.psnode_gemm_tn_f32(ctypes.byref(a), wp, wn, torch.cuda.current_stream(dev).cuda_stream), "psnode_gemm_tn_f32")
    return (c, cs) if want_colsum else c


def _gemm_tn(a2: torch.Tensor, b2: torch.Tensor, groups: int) -> torch.Tensor:
    """a2^T @ b2 for tall-skinny [N, p], [N, q] (N in the millions).  Round 6: on K10 (gemm_tn above) whenever the shapes are in its class
    -- every call of the latent-wide backward at hidden % 4 == 0 --; otherwise (odd widths) `groups` independent library partial products
    + one sum."""
    c = gemm_tn(a2, b2)
    if c is not None:
        return c
    N = a2.shape[0]
    groups = max(1, min(groups, 256))     # the [groups, p, q] partial products are materialised: cap them (small B x long T chunks)
    while groups > 1 and N % groups:
        groups -= 1
    return torch.bmm(a2.view(groups, N // groups, -1).transpose(1, 2), b2.view(groups, N // groups, -1)).sum(0)


def _check_saved(act, xst, T, B, xd, S, L, dev):
    """The saved stage activations / stage inputs reach the kernels as raw pointers: a tuple from another call (other T, B, method or
    width) would be read out of bounds, so its shape is checked here ([T-1,S,L,B,Hp] / [T-1,S,B,xd], contiguous, on this device)."""
    ok = (act.dim() == 5 and tuple(act.shape[:4]) == (T - 1, S, L, B) and tuple(xst.shape) == (T - 1, S, B, xd)
          and act.is_contiguous() and xst.is_contiguous() and act.device == dev and xst.device == dev
          and act.dtype == torch.float32 and xst.dtype == torch.float32)
    if not ok:
        raise ValueError(f"saved activations do not belong to this call: got {tuple(act.shape)} / {tuple(xst.shape)}, "
                         f"expected [{T - 1},{S},{L},{B},Hp] / [{T - 1},{S},{B},{xd}] contiguous fp32 on {dev}")


def _split_grads(flat, layers):
    out, off = [], 0
    for w, b in layers:
        out.append(flat[off:off + w.numel()].view_as(w)); off += w.numel()
        out.append(flat[off:off + b.numel()].view_as(b)); off += b.numel()
    return out
