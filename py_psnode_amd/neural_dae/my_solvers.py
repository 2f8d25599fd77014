"""Fixed-grid solver base with the call surface of the reference's neural_dae/my_solvers.py.

`integrate_ODE` / `integrate_DAE` keep the reference's keyword names, tensor layout (time-major views in,
fresh contiguous [T,B,D] out) and error behaviour (my_solvers.py:11-29, 52-131).  When the right-hand
sides are the reference's ELU-MLPs on a HIP device the whole time loop runs in ONE fused HIP launch
(py_psnode_amd.fused -> libpsnode_hip.so); with autograd in play the call becomes a torch.autograd.Function
(fused forward kernel + one fused backward kernel, py_psnode_amd/autograd.py).  Arbitrary Python callbacks --
which no kernel can execute -- and shapes no backward kernel covers are stepped through
the user's own callables by `_walk_*` below.

`solver.fused` selects the route: "auto" (default; fused whenever the call is fusable, and it then FAILS
LOUDLY if libpsnode_hip.so is missing -- never a silent substitute; a call on a HIP device that has to walk
says so once with a RuntimeWarning), "require" (raise if the call is not fusable), "off" (always the walk).
"""
import abc
import inspect
import os
import warnings

import torch
import torch.nn as nn

from .. import fused as _fused
from .._lib import UnsupportedShapeError


class NotFusableError(RuntimeError):
    pass


def _autograd():
    from .. import autograd       # (imported on first use: autograd imports fused, which this module imports too)
    return autograd


class _LagWalk:
    """externals='lagrange' of one walk: hits[k] / jumped[k] -- is step k an event step, and its jumped rows (a tuple like `rows`) --, the
    stencil table's off / q per interval and trajectory, and ext_at(k, j, n): c -> the externals of interval k at theta = (j + c) / n,
        w = sum_{m < q} l_m(off + theta) node_{s+m} in increasing m,   l_m(u) = (prod_{r != m, r < q} (u - r)) / (prod_{r != m, r < q} (m - r)),
    both products in increasing r from 1,
    in the rows' dtype, as written (the device function lag_weights / lag_eval of the kernels has this order).  At theta = 0 and 1 the
    weights are exactly 0 / 1."""

    def __init__(self, t, event_fn, jump_change_fn, rows):
        T = t.shape[0]
        self.rows = rows
        self.hits = [event_fn is not None and bool(event_fn(t[k]) == True) for k in range(T - 1)]  # noqa: E712 (callbacks may return tensors)
        self.jumped = {}
        for k in range(T - 1):
            if self.hits[k]:
                res = jump_change_fn(t[k], *(w[k] for w in rows))
                self.jumped[k] = tuple(res) if isinstance(res, (tuple, list)) else (res,)
        ev = torch.tensor([0 if h else -1 for h in self.hits], dtype=torch.int32, device=t.device) if any(self.hits) else None
        codes = _fused.lagrange_stencils(t.detach(), ev).long()      # [T-1, B or 1]
        self.off, self.q = codes & 3, (codes >> 2) & 7
        # node 0 of a stencil reads these: the dataset rows with the jumped rows at the event steps
        self.rows_j = tuple(torch.stack([self.jumped[k][n] if k in self.jumped else w[k] for k in range(T)]) if self.jumped else w
                            for n, w in enumerate(rows))

    def ext_at(self, k, j, n):
        T, B = self.rows[0].shape[0], self.rows[0].shape[1]
        off, q = self.off[k].expand(B), self.q[k].expand(B)
        s, ar = k - off, torch.arange(B, device=off.device)
        nodes = [[(wj if m == 0 else w)[(s + m).clamp(max=T - 1), ar] for m in range(4)] for w, wj in zip(self.rows, self.rows_j)]

        def at(c):
            theta = (j + c) / n
            out = []
            for nd in nodes:
                u = off.to(nd[0].dtype).unsqueeze(-1) + theta
                one, acc = torch.ones_like(u), None
                for m in range(4):
                    num, den = one, one
                    for r in range(4):
                        if r != m:
                            num = num * torch.where((q > r).unsqueeze(-1), u - r, one)
                            den = den * torch.where((q > r).unsqueeze(-1), torch.full_like(u, m - r), one)
                    term = torch.where((q > m).unsqueeze(-1), num / den, torch.zeros_like(u)) * nd[m]
                    acc = term if acc is None else acc + term
                out.append(acc)
            return tuple(out)
        return at


class FixedGridODESolver(metaclass=abc.ABCMeta):
    order: int
    method = ""        # "euler" | "midpoint" | "rk4", a fused.Tableau (my_fixed_grid.ExplicitRK), "ab2" (my_fixed_grid.AB2), "ab3" (my_fixed_grid.AB3) or a fused.Recurrence (my_fixed_grid.RKC1 / RKC2): the formula the fused kernels run
    # A solver whose ONE step per interval re-evaluates a DAE's algebraic variable between its stages (my_fixed_grid.RKC1 / RKC2) sets this private
    # hook: _step_state(func=, t0=, dt=, t1=, x0=, z0=, v0=, i0=, all_initial=, head=) -> the new state, with head(x) -> i at the interval's held
    # z | v, or None where i is not re-evaluated (an ODE, input_true_i).  The base walks call it where they call step_integrate.
    _step_state = None

    def __init__(self, step_size=None, grid_constructor=None, interp="linear", substeps=1, externals="hold", segment=None,
                 segment_parallel=None, algebraic="step"):
        """algebraic ("step", the default and the reference's rule, or "stage"): where a DAE's algebraic variable i = g(x, z, v) is evaluated.
        "step": once per (sub-)step, frozen over its Runge-Kutta stages -- which caps every Runge-Kutta option at first order on a DAE.
        "stage": the standard treatment of an index-1 DAE -- stage s >= 1 of sub-step j, with X_s = x + h sum_{j' < s} a[s][j'] k_j' and
        (z_s, v_s) the interpolated externals at theta_s = (j + c_s) / substeps (the rows its DE evaluation reads), evaluates
        i_s = g(X_s, z_s, v_s, all_initial) and k_s = f(X_s, z_s, v_s, i_s): one more AE evaluation per stage, no output row, so that the method
        integrates x' = f(x, w(t), g(x, w(t))) and reaches its own order -- RK4Classic(externals="lagrange", algebraic="stage") is fourth order
        on a DAE, Heun2(externals="linear", algebraic="stage") second.  Stage 0 reads the i it reads under "step" (the carried head of grid point
        k, the event-time head on the jumped rows, for j >= 1 the in-interval head at theta = j / substeps); the head at grid point k + 1,
        both outputs, h, the events, theta and the interpolants are untouched.  input_true_x: sub-step 0 starts from x[k], the stage heads
        still see X_s.  input_true_i: every stage reads i[k] and no head runs inside an interval -- the "step" call, bit for bit; so is a
        one-stage method's (Euler), and every integrate_ODE call (no head).  `_walk_dae` is the definition (through the keyword `head` of
        `_step_func_lin`); fused on the generic kernels K0 / K5 (kernel 'auto' / 'generic') under the rules of interpolated externals.
        Needs externals="linear" / "lagrange" (held rows cap every Runge-Kutta option at order one, and no build carries the pair); AB2 / AB3
        (grid points only) and RKC1 / RKC2 (they evaluate the head at every stage already) refuse it: ValueError.
        segment_parallel (None, the default: the call it was; "auto" or an int g >= 1; needs segment): where a fused call with segments
        runs, never what it computes -- the segments of a record get no gradient through the dataset rows, so they are independent, and the
        generic kernels K0 / K5 then run them side by side: the n_seg = ceil((T - 1) / w) segments in up to g time chunks of
        ceil(n_seg / min(g, n_seg)) consecutive ones, on a launch grid of tiles x chunks workgroups.  "auto": g = max(1, CUs // tiles) with
        tiles = ceil(B / 16) -- a small batch on a long record fills the device, a batch that fills it already stays as it was.  The walks
        and fused="off" ignore it; every refusal of `segment` applies unchanged.
        segment (None, the default, or an int w >= 1): multiple shooting.  Grid point k is a restart point iff k > 0 and k % w == 0: the
        step that leaves it starts from the dataset row x[k] instead of the running state, and a DAE's DE reads the head at that row,
        g(x[k]; z_k, v_k) with the jumped rows if an event fires at k.  Output rows m w + 1 .. min((m + 1) w, T - 1) are then exactly what
        the free-running call returns in its rows 1 .. on the slices [m w : (m + 1) w + 1] started from x[m w]; xs[k] / is[k] of a restart
        point stay the previous segment's prediction.  Only sub-step 0 of the interval starts from x[k].  The dataset x gets no gradient
        (`_walk_ode` / `_walk_dae` are the definition; fused on the generic kernels K0 / K5, kernel 'auto' / 'generic').  Not together with
        input_true_x / input_true_i (every step restarts already), and a DAE needs its dataset x: ValueError.
        externals ("hold", the default and the reference's behaviour, "linear" or "lagrange"): what the stages of a grid interval read of the
        external inputs z | v.  "hold": the left grid point's rows (the jumped ones behind an event) for every stage and sub-step -- which
        leaves an O(interval) error that no method order and no number of sub-steps removes.  "linear": stage s (abscissa c_s) of sub-step j
        reads w_L + theta (w_R - w_L) at theta = (j + c_s) / substeps, w_L the left rows (jumped behind an event), w_R the dataset's rows of
        the next grid point (`_walk_ode` / `_walk_dae` are the definition; fused on the generic kernels K0 / K5, kernel 'auto' / 'generic').
        `interp` cannot carry this: the reference passes interp="linear" by default and holds.
        "lagrange": the same walk with the cubic through the four neighbouring dataset rows in the straight line's place (quadratic /
        linear where a piece has three / two rows) -- an O(H^4) floor in the data's interval H where "linear" has O(H^2), so RK4Classic is
        fourth order on sampled inputs.  Per trajectory and per column of z | v: a piece is a maximal run of intervals with t[k+1] > t[k]
        and no event step inside; interval k of piece [a, e] reads q = min(4, e - a + 1) nodes from s = clamp(k - 1, a, e - q + 1) on, node s
        the jumped row where step s has an event, and w = sum_m l_m(k - s + theta) node_{s+m} with the same theta (`_LagWalk`,
        fused.lagrange_stencils).  The nodes are taken as equally spaced (each trajectory its own spacing): on a clock that is not, the
        interpolant is still continuous and exact at the grid points, and promises nothing beyond what "linear" gives.  Everything else
        is "linear"'s contract.  The walk asks event_fn / jump_change_fn for every grid point in front of its loop; per-trajectory events
        next to it: ValueError.
        substeps (an int >= 1, default 1): every grid interval [t[k], t[k+1]] is integrated in that many equal sub-steps of
        h = (t[k+1] - t[k]) / substeps, with the interval's external inputs held over all of them and the outputs staying on the grid of t
        (`_walk_ode` / `_walk_dae` are the definition; more than 1 runs fused on the generic kernels K0 / K5, kernel 'auto' / 'generic').
        It is the supported way to integrate with a finer step than the data's sampling interval: `step_size`, `grid_constructor` and
        `interp` are kept for the reference's call surface and are read by neither integrate_ODE nor integrate_DAE, as upstream."""
        if isinstance(substeps, bool) or not isinstance(substeps, int) or substeps < 1:
            raise ValueError(f"substeps must be an int >= 1, got {substeps!r}")
        self.substeps = substeps
        if externals not in _fused.EXTERNALS:
            raise ValueError(f"externals must be one of {_fused.EXTERNALS}, got {externals!r}")
        self.externals = externals
        if not isinstance(algebraic, str) or algebraic not in _fused.ALGEBRAIC:
            raise ValueError(f"algebraic must be one of {_fused.ALGEBRAIC}, got {algebraic!r}")
        if algebraic == "stage" and externals == "hold":
            raise ValueError("algebraic='stage' needs interpolated externals (externals='linear' / 'lagrange'): held rows cap every "
                             "Runge-Kutta option at first order whatever the head does, and no kernel build carries the pair")
        self.algebraic = algebraic
        if segment is not None and (isinstance(segment, bool) or not isinstance(segment, int) or segment < 1):
            raise ValueError(f"segment must be None or an int >= 1, got {segment!r}")
        self.segment = segment
        _fused.check_segment_parallel(segment_parallel, segment)
        self.segment_parallel = segment_parallel
        # public attributes of the reference (my_solvers.py:13-18)
        self.step_size = step_size
        self.interp = interp
        self.enable_cal_time = False
        self.assert_time = 0
        self.cal_time = 0
        self.total_time = 0
        self.fused = os.environ.get("PSNODE_FUSED", "auto")
        self.kernel = os.environ.get("PSNODE_KERNEL", "auto")
        # Two events at one time stamp make the reference's jump_change_fn raise (neural_base.py:61); the fused event table would
        # take the first.  True: read the table kernel's duplicate flag back (one 4-byte D2H per call, skipped when the event list
        # has fewer than two entries or the stream is being captured into a HIP graph) and raise like the reference.
        self.check_events = os.environ.get("PSNODE_CHECK_EVENTS", "1") != "0"
        if step_size is not None and grid_constructor is not None:
            raise ValueError("step_size and grid_constructor are mutually exclusive arguments.")
        if grid_constructor is not None:
            self.grid_constructor = grid_constructor
        elif step_size is None:
            self.grid_constructor = lambda func, x0, t: t
        else:
            self.grid_constructor = self._grid_constructor_from_step_size(step_size)

    @staticmethod
    def _grid_constructor_from_step_size(step_size):
        # unused by either integrate_* in the reference as well (my_solvers.py:31-42, :54 commented out)
        def _grid_constructor(t):
            n = torch.ceil((t[-1] - t[0]) / step_size + 1).item()
            grid = torch.arange(0, n, dtype=t.dtype, device=t.device) * step_size + t[0]
            grid[-1] = t[-1]
            return grid
        return _grid_constructor

    def _note_walk(self, what, tensor):
        """The walk is the reference's own route, but on a HIP device it is ~100x slower than the fused one: never silent."""
        if self.fused == "auto" and tensor.device.type == "cuda" and not getattr(self, "_walk_warned", False):
            self._walk_warned = True
            warnings.warn(f"{what}: this call is not fusable (needs fp32 HIP tensors, DE_Func/AE_Func-style MLPs with one activation "
                          "of ELU / Tanh / Sigmoid / ReLU / LeakyReLU / Softplus / SiLU / GELU / Mish -- other than ELU(1) on kernel 'auto' / 'generic' only --, "
                          "ODE_Event/DAE_Event callbacks -- with per_trajectory=True on kernel 'auto' / 'generic' only and not together with interpolated externals --; "
                          "an ExplicitRK tableau, substeps > 1 or externals='linear' / 'lagrange' on kernel 'auto' / 'generic' only (substeps <= 1024); segment= on kernel 'auto' / 'generic' only, with held externals and shared events, dataset x without grad; under autograd also a shape with a backward kernel; teacher-forced "
                          "training: ELU(1), dataset rows without grad) -- stepping through the Python callables instead", RuntimeWarning, stacklevel=3)

    def _generic_only_ok(self, what, acts, per_trajectory=False) -> bool:
        """An activation other than ELU(1), a Runge-Kutta tableau (ExplicitRK: `method` is a fused.Tableau), sub-steps per grid interval
        (up to 1024), interpolated externals ("linear", "lagrange") and per-trajectory events (`per_trajectory`: the call has events and its event
        object applies them per trajectory) run on the generic kernels K0 / K5 only: kernel 'wave' / 'tile' / 'mfma' / 'wide'
        with one of them walks under fused='auto' and raises under 'require', naming the first in the order act, tableau, sub-steps,
        externals, events (fused.GenericOpts.require_generic's).  Per-trajectory events together with externals='linear' have no kernel."""
        generic = self.kernel in ("auto", "generic")
        lin_pt = per_trajectory and self.externals != "hold"
        fits = generic and self.substeps <= _fused._lib.MAX_SUBSTEPS
        ms_none = self.segment is not None and (per_trajectory or self.externals != "hold")      # no kernel carries these combinations
        if fits and not lin_pt and not ms_none:
            return True
        limits = "(kernel 'auto' / 'generic', substeps <= %d)" % _fused._lib.MAX_SUBSTEPS
        if not generic and any(a is not None for a in acts):
            names = ", ".join(repr(a) for a in acts if a is not None)
            text = f"has no form for the activation {names}: activations other than ELU(alpha=1) run on the generic kernels (kernel 'auto' / 'generic')"
        elif not generic and isinstance(self.method, _fused.Recurrence):
            text = f"has no form for the Runge-Kutta-Chebyshev recurrence {self.method.name}: it runs on the generic kernels (kernel 'auto' / 'generic')"
        elif not generic and isinstance(self.method, _fused.Tableau):
            text = f"has no form for the Runge-Kutta tableau {self.method.name}: tableaus run on the generic kernels (kernel 'auto' / 'generic')"
        elif not fits and self.substeps != 1:
            text = f"with substeps={self.substeps} has no fused form: sub-steps per grid interval run on the generic kernels {limits}"
        elif not fits and self.externals != "hold":
            text = f"with externals={self.externals!r} has no fused form: interpolated external inputs run on the generic kernels {limits}"
        elif lin_pt:
            text = f"with per-trajectory events and externals={self.externals!r} has no fused form: the generic kernels carry either, not both"
        elif not generic and per_trajectory:
            text = "has no form for per-trajectory events (per_trajectory=True): they run on the generic kernels (kernel 'auto' / 'generic')"
        elif ms_none:
            text = (f"with segment={self.segment} next to " + (f"externals={self.externals!r}" if self.externals != "hold" else "per-trajectory events")
                    + " has no fused form: the multiple-shooting build of the generic kernels holds the externals and takes the shared event table")
        elif not generic and self.segment is not None:
            text = f"has no form for multiple-shooting segments (segment={self.segment}): they run on the generic kernels (kernel 'auto' / 'generic')"
        else:
            return True
        if self.fused == "require":
            raise UnsupportedShapeError(f"{what}: kernel={self.kernel!r} {text}")
        return False

    def _stage_heads(self, input_true_i=False) -> bool:
        """Does a DAE call of this solver evaluate the head in front of its stages s >= 1?  algebraic="stage", the call integrates its own
        i and the method has more than one stage; every other call is the "step" call and takes its route."""
        if self.algebraic != "stage" or input_true_i:
            return False
        try:
            return _fused.method_info(self.method)[1] > 1
        except (KeyError, TypeError):      # (a user's solver class without a `method` the kernels know: its own formula decides)
            return True

    def _generic_kwargs(self, per_trajectory=False, stage_heads=False) -> dict:
        """substeps= / externals= / per_trajectory= / algebraic= for the fused calls, left out at 1 / "hold" / False / "step" (stage_heads:
        `_stage_heads` of a DAE call): those calls are then the ones they always were."""
        kw = dict(substeps=self.substeps) if self.substeps != 1 else {}
        if stage_heads:
            kw["algebraic"] = "stage"
        if self.externals != "hold":
            kw["externals"] = self.externals
        if per_trajectory:
            kw["per_trajectory"] = True
        if self.segment is not None:
            kw["segment"] = self.segment
        if self.segment_parallel is not None:
            kw["segment_parallel"] = self.segment_parallel
        return kw

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
        """-> dx of one (sub-)step whose stage at abscissa c reads the externals ext_at(c) = (z, v | None): the class's own formula with a
        per-stage external (the private path of externals='linear'; my_fixed_grid.py implements it for every solver of the package)."""
        raise NotImplementedError(f"{type(self).__name__} has no _step_func_lin: externals='linear' needs the step formula with per-stage "
                                  "external inputs")

    @staticmethod
    def _lin_ext(j, n, left, right):
        """c -> the externals at theta = (j + c) / n between the rows `left` and `right` (tuples of z[, v]): w_L + theta (w_R - w_L) in the
        tensors' dtype, as written."""
        def ext_at(c):
            theta = (j + c) / n
            return tuple(wl + theta * (wr - wl) for wl, wr in zip(left, right))
        return ext_at

    def _lag_walk(self, what, t, event_fn, jump_change_fn, rows):
        """The set-up of externals='lagrange' in front of a walk's loop (None for every other value): the events and jumped rows of every
        grid point, the stencil table, the node rows.  rows: (z,) or (z, v)."""
        if self.externals != "lagrange":
            return None
        if event_fn is not None and _fused.per_trajectory_events(event_fn):
            raise ValueError(f"{what}: externals='lagrange' together with per-trajectory events is not defined (a piece ends at an event "
                             "step of the shared table)")
        return _LagWalk(t, event_fn, jump_change_fn, rows)

    def _check_segment(self, what, teacher_forced, x=None):
        """The refusals of `segment`: teacher forcing (every step restarts already) and, for a DAE (`x` given), no dataset x."""
        if self.segment is None:
            return
        if teacher_forced:
            raise ValueError(f"{what}: segment={self.segment} and input_true_x / input_true_i exclude each other (every teacher-forced step "
                             "restarts from the dataset already)")
        if x is not None and x.shape[-1] == 0:
            raise ValueError(f"{what}: segment={self.segment} restarts from the dataset rows x[k]; this call has none (x.shape[-1] == 0)")

    def _restart(self, k) -> bool:
        """Is grid point k a restart point of `segment`?"""
        return self.segment is not None and k > 0 and k % self.segment == 0

    def _check_events_now(self, event_t):
        return (self.check_events and event_t is not None and event_t.dim() == 3 and event_t.shape[1] > 1
                and not torch.cuda.is_current_stream_capturing())

    @abc.abstractmethod
    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        """-> (dx, f0)"""

    def step_integrate(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        dx, f0 = self._step_func(func=func, t0=t0, dt=dt, t1=t1, x0=x0, z0=z0, v0=v0, i0=i0, all_initial=all_initial)
        return x0 + dx, f0

    # ------------------------------------------------------------------ ODE
    def integrate_ODE(self, x_func, t, x, z, all_initial, event_fn=None, jump_change_fn=None, input_true_x=False, x_init=None):
        """my_solvers.py:53-79.  `x_init` (an extension, default None = upstream: the integration starts from x[0]) hands the [B,x_dim]
        initial state over on its own: a caller whose x is a big differentiable tensor (the direct_encode models' Xh) otherwise gets
        d loss / d x back as a [T,B,x_dim] tensor that is zero except for row 0 -- allocated, filled and ADDED to x's other gradient."""
        if x_init is not None and input_true_x:
            raise ValueError("integrate_ODE: x_init and input_true_x exclude each other (teacher forcing starts every step from x[k])")
        self._check_segment("integrate_ODE", input_true_x)
        # (segment: a dataset x that requires grad gets none -- such a call with a restart walks, as teacher forcing does)
        ms_walk = self.segment is not None and t.shape[0] - 1 > self.segment and torch.is_grad_enabled() and x.requires_grad
        if self.fused != "off" and not ms_walk:
            plan = _fused.plan_ode(x_func, x, z, all_initial, event_fn, jump_change_fn, t=t, x_init=x_init)
            # (per-trajectory events: only a call that has events carries the rule)
            per_traj = plan is not None and plan[1] is not None and _fused.per_trajectory_events(event_fn)
            if plan is not None and not self._generic_only_ok("integrate_ODE", plan[4:], per_traj):
                plan = None
            sub = self._generic_kwargs(per_traj)
            if plan is not None:
                layers, event_t, z_jump, needs_grad, act = plan
                if not needs_grad:
                    try:
                        x_in = x if x_init is None else x_init.unsqueeze(0)
                        if x_init is not None and self.segment is not None and t.shape[0] - 1 > self.segment:
                            x_in = torch.cat((x_in, x[1:]))      # (the restarts read rows 1 ..; row 0 is the start of the call)
                        return _fused.ode_integrate(self.method, layers, t, x_in, z, all_initial,
                                                    event_t=event_t, z_jump=z_jump,
                                                    input_true_x=input_true_x, kernel=self.kernel,
                                                    check_events=self._check_events_now(event_t), act=act, **sub)
                    except UnsupportedShapeError:      # no kernel covers the shape (too wide for LDS): user callables it is
                        if self.fused == "require":
                            raise
                # training: fused forward + fused backward when the backward kernel covers the shape
                elif not input_true_x and _autograd().ode_training_supported(self.method, layers, x.shape[-1], z.shape[-1], t.shape[0],
                                                                             t.shape[1], kernel=self.kernel, act=act, **sub):
                    from ..autograd import fused_ode_integrate
                    return fused_ode_integrate(self.method, self.kernel, layers, t, x, z, all_initial, event_t, z_jump,
                                               check_events=self._check_events_now(event_t), x_init=x_init, act=act, **sub)
                # teacher-forced training (my_solvers.py:72-74): K4f in its recompute form where the shape is its, else K5 (ELU(1) only);
                # the dataset x gets no gradient
                elif input_true_x and act is None and not x.requires_grad and _autograd().ode_training_supported(
                        self.method, layers, x.shape[-1], z.shape[-1], t.shape[0], t.shape[1], kernel=self.kernel, input_true_x=True, **sub):
                    from ..autograd import fused_ode_integrate
                    return fused_ode_integrate(self.method, self.kernel, layers, t, x, z, all_initial, event_t, z_jump,
                                               check_events=self._check_events_now(event_t), input_true_x=True, **sub)
            if self.fused == "require":
                raise NotFusableError("integrate_ODE: call is not fusable (needs fp32 HIP tensors, a DE_Func-style MLP `x_dot` with one "
                                      "activation of ELU / Tanh / Sigmoid / ReLU / LeakyReLU / Softplus / SiLU / GELU / Mish, ODE_Event callbacks; with autograd: "
                                      "a shape with a backward kernel; teacher-forced training: ELU(1), kernel 'auto' / 'mfma' / 'generic', x without grad)")
            self._note_walk("integrate_ODE", x)
        if self.fused != "off" and ms_walk:
            if self.fused == "require":
                raise NotFusableError(f"integrate_ODE: segment={self.segment} with a dataset x that requires grad is not fusable (the dataset "
                                      "rows get no gradient; pass the start through x_init)")
            self._note_walk("integrate_ODE", x)
        return self._walk_ode(x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x, x_init)

    def _walk_ode(self, x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x, x_init=None):
        n_grid = t.shape[0]
        xs = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
        cur = x[0] if x_init is None else x_init
        xs[0] = cur
        lag = self._lag_walk("integrate_ODE", t, event_fn, jump_change_fn, (z,))
        for k in range(n_grid - 1):
            t0, t1, zk = t[k], t[k + 1], z[k]
            if lag is not None:      # (asked in front of the loop: a piece's end lies in the future)
                if lag.hits[k]:
                    zk = lag.jumped[k][0]
            elif event_fn is not None and event_fn(t0) == True:  # noqa: E712 (callbacks may return tensors)
                zk = jump_change_fn(t0, zk)
            start = x[k] if input_true_x else cur
            if self.segment is not None:
                self._check_segment("integrate_ODE", input_true_x)
                if self._restart(k):      # multiple shooting: this segment starts from the dataset row, which gets no gradient
                    start = x[k].detach()
            if self.externals != "hold":      # stage s of sub-step j reads zk + theta (z[k + 1] - zk), theta = (j + c_s) / n; zk jumped behind an event
                h = (t1 - t0) / self.substeps   # ("lagrange": the polynomial through the stencil's nodes at the same theta)
                cur = start
                for j in range(self.substeps):
                    ext_at = self._lin_ext(j, self.substeps, (zk,), (z[k + 1],)) if lag is None else lag.ext_at(k, j, self.substeps)
                    cur = cur + self._step_func_lin(func=x_func, t0=t0 + j * h if j else t0, dt=h, x0=cur, ext_at=lambda c: ext_at(c) + (None,),
                                                    all_initial=all_initial)
            elif self._step_state is not None:
                cur = self._step_state(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, all_initial=all_initial)
            elif self.substeps == 1:
                cur, _ = self.step_integrate(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, all_initial=all_initial)
            else:       # n equal sub-steps of h = (t1 - t0) / n with the interval's z held; only sub-step 0 starts from the dataset row
                h = (t1 - t0) / self.substeps
                cur = start
                for j in range(self.substeps):
                    cur, _ = self.step_integrate(func=x_func, t0=t0 + j * h, dt=h, t1=t0 + (j + 1) * h, x0=cur, z0=zk, all_initial=all_initial)
            xs[k + 1] = cur
        return xs

    # ------------------------------------------------------------------ DAE
    def integrate_DAE(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn=None, jump_change_fn=None,
                      input_true_x=False, input_true_i=False):
        self._check_segment("integrate_DAE", input_true_x or input_true_i, x)
        ms_walk = self.segment is not None and t.shape[0] - 1 > self.segment and torch.is_grad_enabled() and x.requires_grad
        if self.fused != "off" and not ms_walk:
            plan = _fused.plan_dae(x_init, x_func, i_func, z, v, i, all_initial, event_fn, jump_change_fn, t=t)
            per_traj = plan is not None and plan[2] is not None and _fused.per_trajectory_events(event_fn)
            if plan is not None and not self._generic_only_ok("integrate_DAE", plan[6:], per_traj):
                plan = None
            sub = self._generic_kwargs(per_traj, self._stage_heads(input_true_i))
            if plan is not None:
                de, ae, event_t, z_jump, v_jump, needs_grad, de_act, ae_act = plan
                act = None if de_act is None and ae_act is None else (de_act, ae_act)
                if not needs_grad:
                    try:
                        return _fused.dae_integrate(self.method, de, ae, x_init, t, x, z, v, i, all_initial, event_t=event_t,
                                                    z_jump=z_jump, v_jump=v_jump, input_true_x=input_true_x,
                                                    input_true_i=input_true_i, kernel=self.kernel,
                                                    check_events=self._check_events_now(event_t), act=act, **sub)
                    except UnsupportedShapeError:
                        if self.fused == "require":
                            raise
                elif not (input_true_x or input_true_i) and _autograd().dae_training_supported(
                        self.method, de, ae, x_init.shape[-1], z.shape[-1], v.shape[-1], i.shape[-1], t.shape[0], t.shape[1], act=act, **sub):
                    from ..autograd import fused_dae_integrate
                    return fused_dae_integrate(self.method, self.kernel, de, ae, x_init, t, z, v, i, all_initial, event_t, z_jump, v_jump,
                                               check_events=self._check_events_now(event_t), act=act, **sub,
                                               **(dict(x=x) if self.segment is not None else {}))
                # teacher-forced training (my_solvers.py:111-121): K7f in its recompute form where the shape is its, else K5 (ELU(1) only);
                # the dataset rows get no gradient
                elif act is None and (input_true_x or input_true_i) and not (input_true_x and x.requires_grad) and not (input_true_i and i.requires_grad) \
                        and x.shape[-1] == x_init.shape[-1] and _autograd().dae_training_supported(
                            self.method, de, ae, x_init.shape[-1], z.shape[-1], v.shape[-1], i.shape[-1], t.shape[0], t.shape[1],
                            kernel=self.kernel, input_true_x=input_true_x, input_true_i=input_true_i, **sub):
                    from ..autograd import fused_dae_integrate
                    return fused_dae_integrate(self.method, self.kernel, de, ae, x_init, t, z, v, i, all_initial, event_t, z_jump, v_jump,
                                               check_events=self._check_events_now(event_t), x=x, input_true_x=input_true_x,
                                               input_true_i=input_true_i, **sub)
            if self.fused == "require":
                raise NotFusableError("integrate_DAE: call is not fusable (needs fp32 HIP tensors, DE_Func/AE_Func-style "
                                      "MLPs with one activation each of ELU / Tanh / Sigmoid / ReLU / LeakyReLU / Softplus / SiLU / GELU / Mish, DAE_Event callbacks; with autograd: a shape with a backward kernel; teacher-forced training: ELU(1), kernel 'auto' / 'mfma' / 'generic', T >= 2, dataset rows without grad)")
            self._note_walk("integrate_DAE", z if z.numel() else v)
        if self.fused != "off" and ms_walk:
            if self.fused == "require":
                raise NotFusableError(f"integrate_DAE: segment={self.segment} with a dataset x that requires grad is not fusable (the dataset "
                                      "rows get no gradient)")
            self._note_walk("integrate_DAE", z if z.numel() else v)
        return self._walk_dae(x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn,
                              input_true_x, input_true_i)

    def _walk_dae(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i):
        n_grid = t.shape[0]
        cur_x = x_init
        cur_i = i_func(xt=x[0] if input_true_x else cur_x, zt=z[0], vt=v[0], all_initial=all_initial)
        x_shape = (*x.shape[0:2], x_init.shape[-1]) if x.shape[-1] == 0 else x.shape
        xs = torch.zeros(x_shape, dtype=x_init.dtype if x.shape[-1] == 0 else x.dtype, device=x.device)
        is_ = torch.zeros(i.shape, dtype=i.dtype, device=i.device)
        xs[0], is_[0] = cur_x, cur_i
        lag = self._lag_walk("integrate_DAE", t, event_fn, jump_change_fn, (z, v))
        heads = {}      # algebraic="stage": the head a stage s >= 1 evaluates at its own argument and externals
        if self._stage_heads(input_true_i):
            if "head" not in inspect.signature(self._step_func_lin).parameters:
                raise NotImplementedError(f"{type(self).__name__}._step_func_lin has no keyword `head`: algebraic='stage' needs the step "
                                          "formula to call head(xx, z, v) in front of every stage s >= 1")
            heads = dict(head=lambda xx, zz, vv: i_func(xt=xx, zt=zz, vt=vv, all_initial=all_initial))
        for k in range(n_grid - 1):
            t0, t1, zk, vk = t[k], t[k + 1], z[k], v[k]
            if lag.hits[k] if lag is not None else (event_fn is not None and event_fn(t0) == True):  # noqa: E712
                zk, vk = lag.jumped[k] if lag is not None else jump_change_fn(t0, zk, vk)
                if _fused.per_trajectory_events(event_fn):      # the event-time head replaces the carried i of the hit trajectories only
                    hit = event_fn.__self__.hit_mask(t0)
                    cur_i = torch.where(hit.view(-1, 1), i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial), cur_i)
                else:
                    cur_i = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
            start = x[k] if input_true_x else cur_x
            i_in = i[k] if input_true_i else cur_i
            if self.segment is not None:
                self._check_segment("integrate_DAE", input_true_x or input_true_i, x)
                if self._restart(k):      # multiple shooting: the DE starts from the dataset row and reads the head AT that row (zk | vk: the
                    start = x[k].detach()      # jumped rows behind an event); xs[k] / is[k] stay the previous segment's prediction
                    i_in = i_func(xt=start, zt=zk, vt=vk, all_initial=all_initial)
            if self.externals != "hold":      # as the ODE, for z | v; i is frozen over a sub-step's stages and never interpolated; the head in
                h = (t1 - t0) / self.substeps   # front of sub-step j >= 1 sees the state and the z | v of theta = j / n
                cur_x = start
                for j in range(self.substeps):
                    ext_at = self._lin_ext(j, self.substeps, (zk, vk), (z[k + 1], v[k + 1])) if lag is None else lag.ext_at(k, j, self.substeps)
                    if j > 0 and not input_true_i:
                        zj_, vj_ = ext_at(0.0)
                        i_in = i_func(xt=cur_x, zt=zj_, vt=vj_, all_initial=all_initial)
                    cur_x = cur_x + self._step_func_lin(func=x_func, t0=t0 + j * h if j else t0, dt=h, x0=cur_x, ext_at=ext_at, i0=i_in,
                                                        all_initial=all_initial, **heads)
            elif self._step_state is not None:      # (the head in front of a stage sees the interval's held rows, as a sub-step's does)
                head = None if input_true_i else (lambda xx, zk=zk, vk=vk: i_func(xt=xx, zt=zk, vt=vk, all_initial=all_initial))
                cur_x = self._step_state(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, v0=vk, i0=i_in, all_initial=all_initial, head=head)
            elif self.substeps == 1:
                cur_x, _ = self.step_integrate(func=x_func, t0=t0, dt=t1 - t0, t1=t1, x0=start, z0=zk, v0=vk, i0=i_in,
                                               all_initial=all_initial)
            else:       # n equal sub-steps with the interval's z | v held; the algebraic variable follows the state inside the interval
                h = (t1 - t0) / self.substeps
                cur_x = start
                for j in range(self.substeps):
                    if j > 0 and not input_true_i:
                        i_in = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
                    cur_x, _ = self.step_integrate(func=x_func, t0=t0 + j * h, dt=h, t1=t0 + (j + 1) * h, x0=cur_x, z0=zk, v0=vk, i0=i_in,
                                                   all_initial=all_initial)
            cur_i = i_func(xt=x[k + 1] if input_true_x else cur_x, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
            xs[k + 1], is_[k + 1] = cur_x, cur_i
        return xs, is_

    # dead helpers of the reference kept for API completeness (my_solvers.py:177-192); nothing calls them:
    # the integrators hold external inputs constant over a step (zero-order hold) unless externals="linear", whose walk interpolates
    # with `_lin_ext` (theta from the sub-step and stage indices, not from the clock).
    def _cubic_hermite_interp(self, t0, x0, f0, t1, x1, f1, t):
        h = (t - t0) / (t1 - t0)
        dt = t1 - t0
        return ((1 + 2 * h) * (1 - h) ** 2) * x0 + (h * (1 - h) ** 2) * dt * f0 + (h * h * (3 - 2 * h)) * x1 + (h * h * (h - 1)) * dt * f1

    def _linear_interp(self, t0, t1, x0, x1, t):
        if t == t0:
            return x0
        if t == t1:
            return x1
        return x0 + (t - t0) / (t1 - t0) * (x1 - x0)
