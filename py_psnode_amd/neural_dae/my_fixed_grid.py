"""Euler / Midpoint / RK4 (3/8 rule) with the interface of the reference's neural_dae/my_fixed_grid.py, and ExplicitRK: any explicit
Runge-Kutta tableau of up to four stages (Heun2, Ralston2, Kutta3, SSPRK3, RK4Classic) on the same call surface.

`method` names the formula the fused HIP kernel runs for the class; `_step_func` is the same formula for
the callback walk (user callables / autograd).  Callback convention (my_fixed_grid.py:16-17): ODE branch
`func(t0=, xt=, zt=, all_initial=)` when v0 is None, else `func(t0=, xt=, zt=, vt=, it=, all_initial=)`.

`_step_func_lin` is each class's formula once more for `externals="linear"` (my_solvers.py): the stage at abscissa c reads the externals
`ext_at(c)` instead of the step's frozen ones.  `_step_func`, its signature and the "hold" path are untouched by it.  Its keyword `head` (None: every statement as it was) is the
solver option algebraic="stage": called as head(xx, z, v) in front of every stage s >= 1, it gives that stage its own algebraic variable.
"""
import torch

from .. import fused as _fused
from .my_solvers import FixedGridODESolver

_one_third = 1 / 3
_two_thirds = 2 / 3


def _rhs_at(func, ext_at, i0, all_initial, head=None):
    """f(c, t, x): the right-hand side whose externals are those of abscissa c, ext_at(c) = (z, v | None) (externals='linear').
    head (algebraic='stage'; a DAE): the first call of f -- stage 0 -- reads i0, every later one i = head(x, z, v) at its own argument and
    externals."""
    if head is not None:
        return _rhs_at_heads(func, ext_at, i0, all_initial, head)

    def f(c, tt, xx):
        z0, v0 = ext_at(c)
        if v0 is None:
            return func(t0=tt, xt=xx, zt=z0, all_initial=all_initial)
        return func(t0=tt, xt=xx, zt=z0, vt=v0, it=i0, all_initial=all_initial)
    return f


def _rhs_at_heads(func, ext_at, i0, all_initial, head):
    """`_rhs_at` with stage-wise algebraic heads: stage s >= 1 evaluates i_s = head(X_s, z_s, v_s) in front of its DE evaluation."""
    first = [True]

    def f(c, tt, xx):
        z0, v0 = ext_at(c)
        it = i0 if first[0] else head(xx, z0, v0)
        first[0] = False
        return func(t0=tt, xt=xx, zt=z0, vt=v0, it=it, all_initial=all_initial)
    return f


def _rhs(func, z0, v0, i0, all_initial):
    """f(t, x) with the step's external inputs frozen."""
    if v0 is None:
        return lambda tt, xx: func(t0=tt, xt=xx, zt=z0, all_initial=all_initial)
    return lambda tt, xx: func(t0=tt, xt=xx, zt=z0, vt=v0, it=i0, all_initial=all_initial)


class Euler(FixedGridODESolver):
    order = 1
    method = "euler"

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        f0 = _rhs(func, z0, v0, i0, all_initial)(t0, x0)
        return dt * f0, f0

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None, head=None):
        return dt * _rhs_at(func, ext_at, i0, all_initial, head)(0.0, t0, x0)


class Midpoint(FixedGridODESolver):
    order = 2
    method = "midpoint"

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        f = _rhs(func, z0, v0, i0, all_initial)
        half_dt = 0.5 * dt
        f0 = f(t0, x0)
        return dt * f(t0 + half_dt, x0 + f0 * half_dt), f0

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None, head=None):
        f = _rhs_at(func, ext_at, i0, all_initial, head)
        half_dt = 0.5 * dt
        return dt * f(0.5, t0 + half_dt, x0 + f(0.0, t0, x0) * half_dt)


class RK4(FixedGridODESolver):
    order = 4
    method = "rk4"

    def rk4_alt_step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None, f0=None, perturb=False):
        """3/8-rule increment (k1 + 3(k2+k3) + k4)*dt/8 (my_fixed_grid.py:38-51)."""
        f = _rhs(func, z0, v0, i0, all_initial)
        k1 = f(t0, x0) if f0 is None else f0
        k2 = f(t0 + dt * _one_third, x0 + dt * k1 * _one_third)
        k3 = f(t0 + dt * _two_thirds, x0 + dt * (k2 - k1 * _one_third))
        k4 = f(t1, x0 + dt * (k1 - k2 + k3))
        return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        f0 = _rhs(func, z0, v0, i0, all_initial)(t0, x0)
        return self.rk4_alt_step_func(func=func, t0=t0, dt=dt, t1=t1, x0=x0, z0=z0, v0=v0, i0=i0,
                                      all_initial=all_initial, f0=f0), f0

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None, head=None):
        """The 3/8 rule with the externals of c = 0, 1/3, 2/3, 1."""
        f = _rhs_at(func, ext_at, i0, all_initial, head)
        k1 = f(0.0, t0, x0)
        k2 = f(_one_third, t0 + dt * _one_third, x0 + dt * k1 * _one_third)
        k3 = f(_two_thirds, t0 + dt * _two_thirds, x0 + dt * (k2 - k1 * _one_third))
        k4 = f(1.0, t0 + dt, x0 + dt * (k1 - k2 + k3))
        return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


class ExplicitRK(FixedGridODESolver):
    """Any explicit Runge-Kutta method of 1..4 stages: a[s][j] (j < s) is the coefficient of slope k_j in the argument of stage s, b[s] the
    weight of k_s in the update.  `method` is the fused.Tableau the generic HIP kernels run (K0 forward, K5 backward; kernel 'auto' /
    'generic'); `_step_func` is the same formula for the callback walk:
        k_s = f(t0 + c_s dt, x0 + dt * sum_{j<s} a[s][j] k_j),  c_s = sum_j a[s][j];    dx = dt * sum_s b[s] k_s
    with the sums in increasing index and a coefficient that is exactly 0 skipped."""

    def __init__(self, a, b, order, name=None, **kw):
        super().__init__(**kw)
        self.method = _fused.Tableau(name or type(self).__name__, a, b, order)
        self.order = self.method.order

    @staticmethod
    def _combine(coefs, ks):
        acc = None
        for c, k in zip(coefs, ks):
            if c != 0.0:
                acc = c * k if acc is None else acc + c * k
        return acc

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        f = _rhs(func, z0, v0, i0, all_initial)
        tab = self.method
        ks = []
        for s in range(tab.stages):
            inc = self._combine(tab.a[s][:s], ks)
            ks.append(f(t0 + tab.c[s] * dt if s else t0, x0 if inc is None else x0 + dt * inc))
        return dt * self._combine(tab.b, ks), ks[0]

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None, head=None):
        f = _rhs_at(func, ext_at, i0, all_initial, head)
        tab = self.method
        ks = []
        for s in range(tab.stages):
            inc = self._combine(tab.a[s][:s], ks)
            ks.append(f(tab.c[s], t0 + tab.c[s] * dt if s else t0, x0 if inc is None else x0 + dt * inc))
        return dt * self._combine(tab.b, ks)


class _NamedRK(ExplicitRK):
    _a, _b = (), ()

    def __init__(self, **kw):
        super().__init__(self._a, self._b, type(self).order, **kw)


class Heun2(_NamedRK):
    """Heun's method (explicit trapezoid rule)."""
    order = 2
    _a, _b = ((), (1.0,)), (0.5, 0.5)


class Ralston2(_NamedRK):
    """Ralston's second-order method (minimum truncation error bound)."""
    order = 2
    _a, _b = ((), (2 / 3,)), (0.25, 0.75)


class Kutta3(_NamedRK):
    """Kutta's third-order method."""
    order = 3
    _a, _b = ((), (0.5,), (-1.0, 2.0)), (1 / 6, 2 / 3, 1 / 6)


class SSPRK3(_NamedRK):
    """The strong-stability-preserving third-order method of Shu and Osher."""
    order = 3
    _a, _b = ((), (1.0,), (0.25, 0.25)), (1 / 6, 1 / 6, 2 / 3)


class RK4Classic(_NamedRK):
    """The classic fourth-order Runge-Kutta method."""
    order = 4
    _a, _b = ((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)


class AB2(FixedGridODESolver):
    """Two-step Adams-Bashforth: the right-hand side is evaluated at grid points only -- where the dataset rows z | v are exact and where a
    DAE's head i_k = g(x_k, z_k, v_k) is evaluated anyway -- so it is second order for ODE and DAE alike at ONE DE evaluation per step
    (Euler's cost).  Step k from grid point k to k + 1, per trajectory, h_k = t[k+1] - t[k], f_k the DE at the inputs Euler's stage reads:
        x_{k+1} = x_k + c0 f_k + c1 f_{k-1}
        restart (k = 0, an event fires at step k -- per trajectory under per_trajectory events --, or h_{k-1} == 0):  c0 = h_k, c1 = 0
        otherwise  rho = h_k / h_{k-1},  c0 = h_k (1 + rho / 2),  c1 = -h_k (rho / 2)
    written once (`_ab2_step`), in the tensors' dtype, uncontracted; the generic kernels K0 / K5 (kernel 'auto' / 'generic') use the same
    order of operations.  The walk (`_walk_ode` / `_walk_dae`, overridden here: every other solver runs the base class's statements)
    carries the previous slope and step.  `_step_func` is the Euler step, so `step_integrate` alone is a restart step.
    No sub-steps and no interpolated externals (the method reads grid rows only; both would need inputs between the rows), no teacher
    forcing (every teacher-forced step starts from a dataset row: a multistep history is undefined) -- ValueError.  Stability: the
    real-axis interval is |h lambda| < 1, half of Euler's."""
    order = 2
    method = _fused.AB2

    def __init__(self, **kw):
        if kw.get("substeps", 1) != 1:
            raise ValueError("AB2 reads the right-hand side at grid points only: substeps != 1 would need inputs between the dataset rows "
                             f"(got substeps={kw.get('substeps')!r})")
        if kw.get("externals", "hold") != "hold":
            raise ValueError("AB2 reads the right-hand side at grid points only: externals='linear' would need inputs between the dataset rows "
                             f"(got externals={kw.get('externals')!r})")
        if kw.get("algebraic", "step") == "stage":
            raise ValueError("AB2 reads the right-hand side at grid points only, where the head is evaluated anyway: it has no stages for "
                             f"algebraic={kw.get('algebraic')!r} to act on")
        if kw.get("segment") is not None:
            raise ValueError("AB2 carries the previous slope from step to step: a multiple-shooting restart (segment=) has no form here "
                             f"(got segment={kw.get('segment')!r})")
        super().__init__(**kw)

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        """The Euler step: a single step has no history, so `step_integrate` alone is a restart step."""
        f0 = _rhs(func, z0, v0, i0, all_initial)(t0, x0)
        return dt * f0, f0

    def _generic_only_ok(self, what, acts, per_trajectory=False) -> bool:
        """AB2 runs on the generic kernels K0 / K5 only: kernel 'wave' / 'tile' / 'mfma' / 'wide' walks under fused='auto' and raises under
        'require'."""
        if self.kernel in ("auto", "generic"):
            return True
        if self.fused == "require":
            raise _fused._lib.UnsupportedShapeError(f"{what}: kernel={self.kernel!r} has no form for two-step Adams-Bashforth: AB2 runs on the "
                                                    "generic kernels (kernel 'auto' / 'generic')")
        return False

    @staticmethod
    def _no_teacher_forcing(what, forced):
        if forced:
            raise ValueError(f"{what}: AB2 has no teacher-forced form -- every teacher-forced step starts from a dataset row, so the "
                             "previous slope a multistep method carries is undefined")

    @staticmethod
    def _restart_mask(event_fn, t0):
        """The trajectories whose step restarts because an event fired: bool [B, 1] under per-trajectory events, else True (all)."""
        if _fused.per_trajectory_events(event_fn):
            return event_fn.__self__.hit_mask(t0).view(-1, 1)
        return True

    @staticmethod
    def _ab2_step(x, f, h, f_prev, h_prev, hit):
        """x_{k+1} of the class docstring.  f_prev / h_prev: None at k = 0; hit: None (no event), True (every trajectory restarts) or
        bool [B, 1].  The clock carries no gradient."""
        euler = x + h * f
        if f_prev is None or hit is True:
            return euler
        restart = h_prev == 0
        if hit is not None:
            restart = restart | hit
        half_rho = (h / torch.where(restart, torch.ones_like(h_prev), h_prev)) / 2
        c0 = h * (1 + half_rho)
        c1 = -(h * half_rho)
        return torch.where(restart, euler, x + c0 * f + c1 * f_prev)

    def integrate_ODE(self, x_func, t, x, z, all_initial, event_fn=None, jump_change_fn=None, input_true_x=False, x_init=None):
        self._no_teacher_forcing("integrate_ODE", input_true_x)
        return super().integrate_ODE(x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x, x_init)

    def integrate_DAE(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn=None, jump_change_fn=None,
                      input_true_x=False, input_true_i=False):
        self._no_teacher_forcing("integrate_DAE", input_true_x or input_true_i)
        return super().integrate_DAE(x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i)

    def _walk_ode(self, x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x, x_init=None):
        self._no_teacher_forcing("integrate_ODE", input_true_x)
        xs = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
        cur = x[0] if x_init is None else x_init
        xs[0] = cur
        f_prev = h_prev = None
        for k in range(t.shape[0] - 1):
            t0, zk, hit = t[k], z[k], None
            if event_fn is not None and event_fn(t0) == True:  # noqa: E712 (callbacks may return tensors)
                zk = jump_change_fn(t0, zk)
                hit = self._restart_mask(event_fn, t0)
            h = t[k + 1] - t0
            f = x_func(t0=t0, xt=cur, zt=zk, all_initial=all_initial)
            cur = self._ab2_step(cur, f, h, f_prev, h_prev, hit)
            f_prev, h_prev = f, h
            xs[k + 1] = cur
        return xs

    def _walk_dae(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i):
        self._no_teacher_forcing("integrate_DAE", input_true_x or input_true_i)
        cur_x = x_init
        cur_i = i_func(xt=cur_x, zt=z[0], vt=v[0], all_initial=all_initial)
        x_shape = (*x.shape[0:2], x_init.shape[-1]) if x.shape[-1] == 0 else x.shape
        xs = torch.zeros(x_shape, dtype=x_init.dtype if x.shape[-1] == 0 else x.dtype, device=x.device)
        is_ = torch.zeros(i.shape, dtype=i.dtype, device=i.device)
        xs[0], is_[0] = cur_x, cur_i
        f_prev = h_prev = None
        for k in range(t.shape[0] - 1):
            t0, zk, vk, hit = t[k], z[k], v[k], None
            if event_fn is not None and event_fn(t0) == True:  # noqa: E712
                zk, vk = jump_change_fn(t0, zk, vk)
                hit = self._restart_mask(event_fn, t0)
                head = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
                cur_i = head if hit is True else torch.where(hit, head, cur_i)      # (per trajectory: the hit ones take the event-time head)
            h = t[k + 1] - t0
            f = x_func(t0=t0, xt=cur_x, zt=zk, vt=vk, it=cur_i, all_initial=all_initial)
            cur_x = self._ab2_step(cur_x, f, h, f_prev, h_prev, hit)
            f_prev, h_prev = f, h
            cur_i = i_func(xt=cur_x, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
            xs[k + 1], is_[k + 1] = cur_x, cur_i
        return xs, is_


class AB3(AB2):
    """Three-step Adams-Bashforth with a predictor-corrector restart step: like AB2 the right-hand side is read at grid points only, so it
    is third order for ODE and DAE alike on sampled inputs, at one DE evaluation per step away from the restarts.  Step k, per trajectory,
    h_k = t[k+1] - t[k], f_k the DE at the inputs AB2's / Euler's stage reads.  Restart flag and depth (both local):
        R_k: k == 0, an event fires at step k (per trajectory under per_trajectory events), or h_{k-1} == 0
        d_k = 0 if R_k;  1 if R_{k-1} or h_{k-1} + h_{k-2} == 0;  2 otherwise
    d_k = 2, with h0, h1, h2 = h_k, h_{k-1}, h_{k-2}:  g1 = h0^2 / 2, g2 = h0^3 / 3 + h1 g1, D = g2 / (h1 + h2),
        c0 = h0 + g1 / h1 + D / h1,  c1 = -g1 / h1 - D / h1 - D / h2,  c2 = D / h2;   x_{k+1} = x_k + c0 f_k + c1 f_{k-1} + c2 f_{k-2}
        (23/12, -16/12, 5/12 times h on a uniform grid)
    d_k = 1: AB2's step.   d_k = 0, the restart step, a Heun predictor-corrector on grid rows only:
        x~ = x_k + h f_k;  f~ the DE at (x~; rows k + 1 of z | v, never jumped; in a DAE i~ = AE(x~; z[k+1], v[k+1]), an evaluation of its
        own and no output);  x_{k+1} = x_k + (h / 2)(f_k + f~).  The slope kept for the history is f_k, never f~.
    Heads at grid points, outputs and the event-time head are AB2's.  Written once (`_ab3_step`), in the tensors' dtype, uncontracted;
    the generic kernels K0 / K5 (kernel 'auto' / 'generic') use the same order of operations.  Where only some trajectories of a batch
    restart, the walk evaluates the corrector for all of them and selects.  `_step_func` is the Euler step, as in AB2.  No sub-steps, no
    interpolated externals, no segments, no teacher forcing -- ValueError.  The clock gets no gradient.  Stability: the real-axis interval
    is |h lambda| < 6/11, about half of AB2's."""
    order = 3
    method = _fused.AB3

    def __init__(self, **kw):
        if kw.get("substeps", 1) != 1:
            raise ValueError("AB3 reads the right-hand side at grid points only: substeps != 1 would need inputs between the dataset rows "
                             f"(got substeps={kw.get('substeps')!r})")
        if kw.get("externals", "hold") != "hold":
            raise ValueError("AB3 reads the right-hand side at grid points only: externals='linear' would need inputs between the dataset rows "
                             f"(got externals={kw.get('externals')!r})")
        if kw.get("algebraic", "step") == "stage":
            raise ValueError("AB3 reads the right-hand side at grid points only, where the head is evaluated anyway: it has no stages for "
                             f"algebraic={kw.get('algebraic')!r} to act on")
        if kw.get("segment") is not None:
            raise ValueError("AB3 carries the previous slopes from step to step: a multiple-shooting restart (segment=) has no form here "
                             f"(got segment={kw.get('segment')!r})")
        FixedGridODESolver.__init__(self, **kw)

    def _generic_only_ok(self, what, acts, per_trajectory=False) -> bool:
        if self.kernel in ("auto", "generic"):
            return True
        if self.fused == "require":
            raise _fused._lib.UnsupportedShapeError(f"{what}: kernel={self.kernel!r} has no form for three-step Adams-Bashforth: AB3 runs on "
                                                    "the generic kernels (kernel 'auto' / 'generic')")
        return False

    @staticmethod
    def _no_teacher_forcing(what, forced):
        if forced:
            raise ValueError(f"{what}: AB3 has no teacher-forced form -- every teacher-forced step starts from a dataset row, so the "
                             "previous slopes a multistep method carries are undefined")

    @staticmethod
    def _ab3_step(x, f, h0, f1, h1, f2, h2, restart, shallow, f_corr):
        """x_{k+1} of the class docstring.  f1, h1 / f2, h2: the slopes and steps of k - 1 / k - 2 (anything finite where the depth does not
        read them); restart: R_k, shallow: d_k <= 1, both bool [B, 1]; f_corr: f~, or None where no trajectory restarts."""
        one = torch.ones_like(h0)
        deep = ~(restart | shallow)
        s1 = torch.where(restart, one, h1)
        s2 = torch.where(deep, h2, one)
        s12 = torch.where(deep, h1 + h2, one)
        half_rho = (h0 / s1) / 2
        x_ab2 = x + (h0 * (1 + half_rho)) * f + (-(h0 * half_rho)) * f1
        g1 = h0 * h0 / 2
        g2 = h0 * h0 * h0 / 3 + s1 * g1
        D = g2 / s12
        c0 = h0 + g1 / s1 + D / s1
        c1 = -g1 / s1 - D / s1 - D / s2
        c2 = D / s2
        out = torch.where(deep, x + c0 * f + c1 * f1 + c2 * f2, x_ab2)
        if f_corr is None:
            return out
        return torch.where(restart, x + (h0 * 0.5) * (f + f_corr), out)

    def _flags(self, k, h, h1, h2, r_prev, hit):
        """(R_k, d_k <= 1) as bool [B, 1] from this step's hit (None, True or bool [B, 1]) and the carried steps and flag."""
        if k == 0 or hit is True:
            restart = torch.ones_like(h, dtype=torch.bool)
        else:
            restart = h1 == 0
            if hit is not None:
                restart = restart | hit
        shallow = restart | r_prev | ((h1 + h2) == 0)
        return restart, shallow

    def _walk_ode(self, x_func, t, x, z, all_initial, event_fn, jump_change_fn, input_true_x, x_init=None):
        self._no_teacher_forcing("integrate_ODE", input_true_x)
        xs = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
        cur = x[0] if x_init is None else x_init
        xs[0] = cur
        f1 = f2 = None
        for k in range(t.shape[0] - 1):
            t0, zk, hit = t[k], z[k], None
            if event_fn is not None and event_fn(t0) == True:  # noqa: E712 (callbacks may return tensors)
                zk = jump_change_fn(t0, zk)
                hit = self._restart_mask(event_fn, t0)
            h = t[k + 1] - t0
            f = x_func(t0=t0, xt=cur, zt=zk, all_initial=all_initial)
            if f1 is None:
                f1 = f2 = torch.zeros_like(f)
                h1 = h2 = torch.zeros_like(h)
                r_prev = torch.ones_like(h, dtype=torch.bool)
            restart, shallow = self._flags(k, h, h1, h2, r_prev, hit)
            f_corr = None
            if bool(restart.any()):
                f_corr = x_func(t0=t[k + 1], xt=cur + h * f, zt=z[k + 1], all_initial=all_initial)
            cur = self._ab3_step(cur, f, h, f1, h1, f2, h2, restart, shallow, f_corr)
            f2, h2, f1, h1, r_prev = f1, h1, f, h, restart
            xs[k + 1] = cur
        return xs

    def _walk_dae(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn, jump_change_fn, input_true_x, input_true_i):
        self._no_teacher_forcing("integrate_DAE", input_true_x or input_true_i)
        cur_x = x_init
        cur_i = i_func(xt=cur_x, zt=z[0], vt=v[0], all_initial=all_initial)
        x_shape = (*x.shape[0:2], x_init.shape[-1]) if x.shape[-1] == 0 else x.shape
        xs = torch.zeros(x_shape, dtype=x_init.dtype if x.shape[-1] == 0 else x.dtype, device=x.device)
        is_ = torch.zeros(i.shape, dtype=i.dtype, device=i.device)
        xs[0], is_[0] = cur_x, cur_i
        f1 = f2 = None
        for k in range(t.shape[0] - 1):
            t0, zk, vk, hit = t[k], z[k], v[k], None
            if event_fn is not None and event_fn(t0) == True:  # noqa: E712
                zk, vk = jump_change_fn(t0, zk, vk)
                hit = self._restart_mask(event_fn, t0)
                head = i_func(xt=cur_x, zt=zk, vt=vk, all_initial=all_initial)
                cur_i = head if hit is True else torch.where(hit, head, cur_i)      # (per trajectory: the hit ones take the event-time head)
            h = t[k + 1] - t0
            f = x_func(t0=t0, xt=cur_x, zt=zk, vt=vk, it=cur_i, all_initial=all_initial)
            if f1 is None:
                f1 = f2 = torch.zeros_like(f)
                h1 = h2 = torch.zeros_like(h)
                r_prev = torch.ones_like(h, dtype=torch.bool)
            restart, shallow = self._flags(k, h, h1, h2, r_prev, hit)
            f_corr = None
            if bool(restart.any()):
                x_pred = cur_x + h * f
                i_pred = i_func(xt=x_pred, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
                f_corr = x_func(t0=t[k + 1], xt=x_pred, zt=z[k + 1], vt=v[k + 1], it=i_pred, all_initial=all_initial)
            cur_x = self._ab3_step(cur_x, f, h, f1, h1, f2, h2, restart, shallow, f_corr)
            f2, h2, f1, h1, r_prev = f1, h1, f, h, restart
            cur_i = i_func(xt=cur_x, zt=z[k + 1], vt=v[k + 1], all_initial=all_initial)
            xs[k + 1], is_[k + 1] = cur_x, cur_i
        return xs, is_


class _RKC(FixedGridODESolver):
    """A stabilised explicit (Runge-Kutta-Chebyshev) step: every grid interval is ONE step of `stages` right-hand-side evaluations whose real
    stability interval grows with stages^2 -- about 1.94 s^2 (RKC1) / 0.65 s^2 (RKC2) where `Euler(substeps=s)` has 2 s.  `method` is the
    fused.Recurrence of `fused.rkc_table(stages, order, damping)`: its fp32-rounded coefficients are the method, for this walk and for the
    generic kernels K0 / K5 (kernel 'auto' / 'generic') alike.  With h = t[k+1] - t[k], Y_0 the step's start and F_0 = F(Y_0):
        Y_1 = Y_0 + (mu_t_1 h) F_0;   Y_j = kappa_j Y_0 + mu_j Y_{j-1} + nu_j Y_{j-2} + (mu_t_j h) F(Y_{j-1}) + (gamma_t_j h) F_0,  j = 2 .. s
    summed in the order written, a coefficient that is exactly 0 skipped, in the tensors' dtype; the new state is Y_s.  The externals are
    held (the jumped rows behind an event).  A DAE that integrates its own i evaluates i = g(Y_{j-1}; z_k, v_k) in front of every stage
    j >= 2 -- the sub-step rule, which is what lets the method stabilise the coupled system --; the first stage uses the carried i or the
    event-time head, and F_0 is that first evaluation, reused.  Under input_true_i every stage reads i[k]; under input_true_x the step
    starts from x[k].  The base walks run it through the `_step_state` hook.  No sub-steps (raise the stage count), no interpolated
    externals, no segments -- ValueError.  Per-trajectory events walk (no kernel)."""
    _order = 1

    def __init__(self, stages, damping=None, **kw):
        name = type(self).__name__
        if isinstance(stages, bool) or not isinstance(stages, int):
            raise ValueError(f"{name}: stages must be an int, got {stages!r}")
        if kw.get("substeps", 1) != 1:
            raise ValueError(f"{name} takes one step per grid interval: substeps != 1 has no form here, raise the stage count instead "
                             f"(got substeps={kw.get('substeps')!r})")
        if kw.get("externals", "hold") != "hold":
            raise ValueError(f"{name} holds the external inputs over its stages: externals={kw.get('externals')!r} has no form here")
        if kw.get("segment") is not None or kw.get("segment_parallel") is not None:
            raise ValueError(f"{name} has no multiple-shooting form (got segment={kw.get('segment')!r}, "
                             f"segment_parallel={kw.get('segment_parallel')!r})")
        if kw.get("algebraic", "step") == "stage":
            raise ValueError(f"{name} already evaluates the algebraic head in front of every stage: algebraic={kw.get('algebraic')!r} has "
                             "nothing to add")
        if damping is not None and (isinstance(damping, bool) or not isinstance(damping, (int, float)) or not damping > 0):
            raise ValueError(f"{name}: damping must be a number > 0, got {damping!r}")
        self.method = _fused.rkc_table(stages, self._order, None if damping is None else float(damping))
        self.order = self._order
        self.stages = stages
        super().__init__(**kw)

    def _step_state(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None, head=None):
        m = self.method
        f0 = _rhs(func, z0, v0, i0, all_initial)(t0, x0)
        y_prev, y = x0, x0 + (m.mu_t[0] * dt) * f0
        for j in range(1, m.stages):
            i_j = i0 if head is None else head(y)
            fj = _rhs(func, z0, v0, i_j, all_initial)(t0 + m.c[j - 1] * dt, y)
            new = m.mu[j] * y
            if m.kappa[j] != 0.0:
                new = m.kappa[j] * x0 + new
            if m.nu[j] != 0.0:
                new = new + m.nu[j] * y_prev
            new = new + (m.mu_t[j] * dt) * fj
            if m.gamma_t[j] != 0.0:
                new = new + (m.gamma_t[j] * dt) * f0
            y_prev, y = y, new
        return y

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        """(Y_s - x0, F_0) with i frozen over the stages: `step_integrate` alone knows no head; the walks go through `_step_state`."""
        f0 = _rhs(func, z0, v0, i0, all_initial)(t0, x0)
        return self._step_state(func, t0, dt, t1, x0, z0, v0, i0, all_initial) - x0, f0

    def _generic_only_ok(self, what, acts, per_trajectory=False) -> bool:
        """The recurrence runs on the generic kernels K0 / K5 only, with the shared event table: kernel 'wave' / 'tile' / 'mfma' / 'wide' and
        per-trajectory events walk under fused='auto' and raise under 'require'."""
        if self.kernel in ("auto", "generic") and not per_trajectory:
            return True
        if self.fused == "require":
            raise _fused._lib.UnsupportedShapeError(
                f"{what}: " + (f"per-trajectory events (per_trajectory=True) next to {self.method.name} have no kernel" if per_trajectory
                               else f"kernel={self.kernel!r} has no form for the Runge-Kutta-Chebyshev recurrence {self.method.name}")
                + ": it runs on the generic kernels (kernel 'auto' / 'generic') with the shared event table")
        return False


class RKC1(_RKC):
    """First-order Runge-Kutta-Chebyshev, stages 1..32 (default damping 0.05): real stability interval about 1.94 stages^2; stages=1 is Euler."""
    _order = 1


class RKC2(_RKC):
    """Second-order Runge-Kutta-Chebyshev, stages 2..32 (default damping 2/13): real stability interval about 0.65 stages^2."""
    _order = 2
