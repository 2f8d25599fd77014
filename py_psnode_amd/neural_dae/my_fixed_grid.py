"""Euler / Midpoint / RK4 (3/8 rule) with the interface of the reference's neural_dae/my_fixed_grid.py, and ExplicitRK: any explicit
Runge-Kutta tableau of up to four stages (Heun2, Ralston2, Kutta3, SSPRK3, RK4Classic) on the same call surface.

`method` names the formula the fused HIP kernel runs for the class; `_step_func` is the same formula for
the callback walk (user callables / autograd).  Callback convention (my_fixed_grid.py:16-17): ODE branch
`func(t0=, xt=, zt=, all_initial=)` when v0 is None, else `func(t0=, xt=, zt=, vt=, it=, all_initial=)`.

`_step_func_lin` is each class's formula once more for `externals="linear"` (my_solvers.py): the stage at abscissa c reads the externals
`ext_at(c)` instead of the step's frozen ones.  `_step_func`, its signature and the "hold" path are untouched by it.
"""
from .. import fused as _fused
from .my_solvers import FixedGridODESolver

_one_third = 1 / 3
_two_thirds = 2 / 3


def _rhs_at(func, ext_at, i0, all_initial):
    """f(c, t, x): the right-hand side whose externals are those of abscissa c, ext_at(c) = (z, v | None) (externals='linear')."""
    def f(c, tt, xx):
        z0, v0 = ext_at(c)
        if v0 is None:
            return func(t0=tt, xt=xx, zt=z0, all_initial=all_initial)
        return func(t0=tt, xt=xx, zt=z0, vt=v0, it=i0, all_initial=all_initial)
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

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
        return dt * _rhs_at(func, ext_at, i0, all_initial)(0.0, t0, x0)


class Midpoint(FixedGridODESolver):
    order = 2
    method = "midpoint"

    def _step_func(self, func, t0, dt, t1, x0, z0=None, v0=None, i0=None, all_initial=None):
        f = _rhs(func, z0, v0, i0, all_initial)
        half_dt = 0.5 * dt
        f0 = f(t0, x0)
        return dt * f(t0 + half_dt, x0 + f0 * half_dt), f0

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
        f = _rhs_at(func, ext_at, i0, all_initial)
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

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
        """The 3/8 rule with the externals of c = 0, 1/3, 2/3, 1."""
        f = _rhs_at(func, ext_at, i0, all_initial)
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

    def _step_func_lin(self, func, t0, dt, x0, ext_at, i0=None, all_initial=None):
        f = _rhs_at(func, ext_at, i0, all_initial)
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
