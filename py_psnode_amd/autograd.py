"""torch.autograd bridge for the fused integrator: forward = psnode_ode_integrate_f32, backward = psnode_ode_backward_f32.

This is what lets the reference's training loops (`loss.backward()` through the integrator,
neural_00_ODE_01_no_encode.py:358-360) run on the fused HIP path instead of an unrolled T-step autograd graph.
"""
import functools
import inspect
import os
import warnings

import torch

from . import fused

# Save the stage activations in the training forward instead of recomputing them in the backward?  "auto": at every hidden width the
# MFMA integrators take (measured per 4096 x 1000 RK4 batch, end of round 3: hidden 128 48.2 -> 34.5 ms per ODE_01 training step, 64
# 17.5 -> 14.3, 32 10.4 -> 9.6; DAE_01 77.0 -> 52.2, 23.0 -> 21.4, 16.9 -> 14.7) whenever the rows (6 KB per state-step at 128: 25 GB for
# that batch; 3.1 KB / 13 GB at 64) fit into half of the free HBM; "1" / "0" force it on / off.
SAVE_ACTIVATIONS = os.environ.get("PSNODE_SAVE_ACTIVATIONS", "auto")
# bytes of stage activations the most recent training forward kept for its backward (0: the backward recomputes) -- bench.py reports it
last_saved_bytes = 0
_warned_generic_override = False


def _is_tableau(method) -> bool:
    """A fused.Tableau method trains on K0 + K5 alone: nothing is saved, no specialised or latent kernel is asked."""
    return isinstance(method, (fused.Tableau, fused.Recurrence))


def _rows_fit(need: int, dev) -> bool:
    """Do `need` bytes of saved rows fit into half of the free HBM of `dev`?  PSNODE_SAVE_ACTIVATIONS=1 says yes without asking."""
    if SAVE_ACTIVATIONS == "1":
        return True
    free, _ = torch.cuda.mem_get_info(dev)
    return need <= free // 2


def latent_wide_training_fits(method, de, ae, hidden, T, B, dev) -> bool:
    """Training at the latent-wide hidden widths exists in ONE form: K3w saves its rows, K9w writes as many adjoint rows again and the
    host contracts them (fused.latent_backward_wide) -- there is no recompute form to fall back to.  True if all of that fits half of the
    free HBM and PSNODE_SAVE_ACTIVATIONS is not "0"; otherwise the solver takes the walk through the user's callables (with its warning)."""
    if SAVE_ACTIVATIONS == "0":
        return False
    if T < 2:                                        # (T = 1: no step, nothing to save)
        return True
    S = fused.method_info(method)[1]
    rows = (T - 1) * S * B * hidden * 4              # one [T-1,S,B,H] tensor
    grid = T * B * hidden * 4                        # one [T,B,H] tensor
    # saved act + xst, gk + d1; d1s, the where / contiguous copies of the external blocks, (DAE) gi, da1, s_ae
    return _rows_fit(4 * rows + (6 if ae is None else 12) * grid, dev)


def _generic_only_training(opts, kernel, teacher_forced, T=2) -> bool:
    """The gate of a training call that carries an option of the generic kernels (fused.GenericOpts.family other than "plain"): K0 + K5
    alone, so kernel "auto" / "generic"; teacher forcing with ELU(1) only and, for the DAE, on a grid of T >= 2.  K5 then answers for its fit."""
    if (opts.ab or opts.segment is not None) and teacher_forced:      # (neither Adams-Bashforth 2 / 3 nor segments have a teacher-forced form on any path: the solver raises before it asks)
        return False
    return kernel in ("auto", "generic") and not (teacher_forced and (T < 2 or any(a is not None for a in opts.acts)))


def ode_training_supported(method, layers, x_dim, z_dim, T, B, kernel="auto", act=None, input_true_x=False, substeps=1,
                           externals="hold", per_trajectory=False, segment=None, segment_parallel=None) -> bool:
    """What the solver asks before it routes a call that needs autograd to the fused forward + backward pair.  act (fused.Act; None =
    ELU(1)): an activation other than ELU(1) trains on K0 + K5 alone, so K5 answers.  input_true_x: teacher-forced training -- K4f's
    recompute form on kernel "auto" / "mfma" where the shape is its, else K5 on "auto" / "generic"; ELU(1) only.
    method a fused.Tableau: K0 + K5 on kernel "auto" / "generic" (K5's tableau build answers for its fit), the same teacher-forcing rule.
    substeps > 1: K0 + K5 in their sub-step builds on kernel "auto" / "generic" (K5's answers for its fit), the same teacher-forcing rule.
    externals="linear" / "lagrange": K0 + K5 in their linear-externals / Lagrange builds for every substeps >= 1, the same rules.
    per_trajectory=True (a call WITH events): K0 + K5 in their per-trajectory builds for every substeps >= 1, the same rules; never
    together with externals="linear".
    segment (an int >= 1): K0 + K5 in their multiple-shooting builds for every substeps >= 1; never teacher-forced, never together with
    externals="linear" or per-trajectory events.  segment_parallel (None, "auto", an int >= 1): the segment-parallel builds answer
    where this record of T grid points and B trajectories splits into more than one time chunk."""
    opts = fused.GenericOpts.of(method, (act,), substeps, externals, bool(per_trajectory), segment,
                                fused.resolve_segment_parallel(segment_parallel, segment, T, B, layers[0][0].device))
    if opts.family != "plain":
        return _generic_only_training(opts, kernel, input_true_x) and fused.ode_backward_supported(
            method, layers, x_dim, z_dim, kernel, act=act, substeps=substeps, externals=externals, per_trajectory=per_trajectory,
            segment=segment, segment_parallel=opts.chunks(T))
    if input_true_x:
        if kernel in ("auto", "mfma") and fused.ode_backward_supported(method, layers, x_dim, z_dim, "wide"):
            return True
        return kernel in ("auto", "generic") and fused.ode_backward_supported(method, layers, x_dim, z_dim, "generic")
    if kernel in ("auto", "mfma") and fused.latent_wide_shape(layers, None, x_dim, z_dim):
        return latent_wide_training_fits(method, layers, None, x_dim, T, B, layers[0][0].device)
    return fused.ode_backward_supported(method, layers, x_dim, z_dim, kernel)


def _dae_tf_on_k7f(method, kernel, de, ae, x_dim, z_dim, v_dim, i_dim) -> bool:
    return not _is_tableau(method) and kernel in ("auto", "mfma") and fused.dae_backward_wide_supported(method, de, ae, x_dim, z_dim, v_dim, i_dim)


def _dae_algebraic(algebraic, input_true_i):
    """The `algebraic` a DAE call runs with: under input_true_i every stage reads i[k] and no head runs inside an interval, so "stage"
    (validated) is the "step" call."""
    if not isinstance(algebraic, str) or algebraic not in fused.ALGEBRAIC:
        raise ValueError(f"algebraic must be one of {fused.ALGEBRAIC}, got {algebraic!r}")
    return "step" if input_true_i else algebraic


def dae_training_supported(method, de, ae, x_dim, z_dim, v_dim, i_dim, T, B, act=None, kernel="auto", input_true_x=False,
                           input_true_i=False, substeps=1, externals="hold", per_trajectory=False, segment=None, segment_parallel=None,
                           algebraic="step") -> bool:
    """algebraic="stage" (with input_true_i the "step" call): K0 + K5 in their stage-heads builds, under the interpolant's rules.
    act: None (both MLPs ELU(1)) or (de_act, ae_act); an activation other than ELU(1) trains on K0 + K5 alone, so K5 answers.
    input_true_x / input_true_i: teacher-forced training (T >= 2, ELU(1) only) -- K7f's recompute form on kernel "auto" / "mfma" where the
    shape is its, else K5 on "auto" / "generic".  method a fused.Tableau: K0 + K5 on kernel "auto" / "generic", the same rules.
    substeps > 1: K0 + K5 in their sub-step builds on kernel "auto" / "generic", the same rules.
    externals="linear" / "lagrange": K0 + K5 in their linear-externals / Lagrange builds for every substeps >= 1, the same rules.
    per_trajectory=True (a call WITH events): K0 + K5 in their per-trajectory builds for every substeps >= 1, the same rules.
    segment (an int >= 1): K0 + K5 in their multiple-shooting builds, as ode_training_supported; segment_parallel: as there."""
    algebraic = _dae_algebraic(algebraic, input_true_i)
    opts = fused.GenericOpts.of(method, fused.dae_acts(act), substeps, externals, bool(per_trajectory), segment,
                                fused.resolve_segment_parallel(segment_parallel, segment, T, B, de[0][0].device), algebraic)
    teacher_forced = input_true_x or input_true_i
    if opts.family != "plain":
        if opts.family == "act":      # (an activation alone: asked without the caller's kernel, as the ELU(1) call at the bottom is)
            kernel = "auto"
        return _generic_only_training(opts, kernel, teacher_forced, T) and fused.dae_backward_supported(
            method, de, ae, x_dim, z_dim, v_dim, i_dim, act=act, kernel=kernel, substeps=substeps, externals=externals,
            per_trajectory=per_trajectory, segment=segment, segment_parallel=opts.chunks(T), algebraic=algebraic)
    if teacher_forced:
        if T < 2:
            return False
        if _dae_tf_on_k7f(method, kernel, de, ae, x_dim, z_dim, v_dim, i_dim):
            return True
        return kernel in ("auto", "generic") and fused.dae_backward_supported(method, de, ae, x_dim, z_dim, v_dim, i_dim, kernel="generic")
    if fused.latent_wide_shape(de, ae, x_dim, z_dim, v_dim, i_dim):
        return latent_wide_training_fits(method, de, ae, x_dim, T, B, de[0][0].device)
    return fused.dae_backward_supported(method, de, ae, x_dim, z_dim, v_dim, i_dim)


def _want_saved(method, kernel, layers, x_dim, z_dim, T, B):
    if _is_tableau(method):
        return False
    if fused.latent_wide_shape(layers, None, x_dim, z_dim):      # K3w saves, K9w reads: the only fused backward at these widths (the solver
        return True                                              # asked latent_wide_training_fits before it came here)
    if SAVE_ACTIVATIONS == "0" or T < 2 or kernel not in ("auto", "mfma", "wave", "tile"):
        return False
    Hp = fused.ode_save_hidden(method, layers, x_dim, z_dim, kernel)
    latent = len(layers) == 2            # the direct_encode latent shape at hidden 64: K3c saves, K9 reads
    if Hp <= 0 or not (latent or fused.ode_backward_supported(method, layers, x_dim, z_dim, "wide")):
        return False
    S = fused.method_info(method)[1]
    return _rows_fit((T - 1) * S * B * ((len(layers) - 1) * Hp + x_dim) * 4, layers[0][0].device)


def _want_saved_dae(method, kernel, de, ae, x_dim, z_dim, v_dim, i_dim, T, B):
    """The same policy for the DAE: saved rows are read by the fused-DE backward K7f, i.e. at hidden widths other than 64 (K7, the
    one-launch kernel there, recomputes)."""
    if _is_tableau(method):
        return False
    if fused.latent_wide_shape(de, ae, x_dim, z_dim, v_dim, i_dim):
        return True
    if SAVE_ACTIVATIONS == "0" or T < 2 or kernel not in ("auto", "mfma") or len(de) not in (2, 4):
        return False
    if len(de) == 2:                     # the direct_encode latent shape at hidden 64 (K3c saves, K9 reads); hidden 16 (K3a / K8) recomputes
        if fused.dae_save_hidden(method, de, ae, x_dim, z_dim, v_dim, i_dim, kernel) != 64:
            return False
        return _rows_fit(((T - 1) * fused.method_info(method)[1] * 2 + T) * 64 * B * 4, de[0][0].device)
    # hidden 64 also has the one-launch kernel K7 (recompute).  The saved form beats it at every method since round 4 (K7f requests its
    # per-step inputs a step ahead: training step at 4096 x 1000 RK4 19.7 vs 23.0 ms, Euler 9.6 vs 10.6 -- gpurun_out/r04g.log; round 3:
    # Euler 11.0 vs 10.65, which kept K7 for Euler)
    Hp = fused.dae_save_hidden(method, de, ae, x_dim, z_dim, v_dim, i_dim, kernel)
    if Hp <= 0 or not fused.dae_backward_wide_supported(method, de, ae, x_dim, z_dim, v_dim, i_dim):
        return False
    S = fused.method_info(method)[1]
    return _rows_fit(((T - 1) * S * (3 * Hp + x_dim) + 3 * T * Hp) * B * 4, de[0][0].device)


def _layers(params, n_de=None):
    """[(W, b), ...] of the flat *params of a Function; with n_de, the DE's and the AE's."""
    pairs = [(params[k], params[k + 1]) for k in range(0, len(params), 2)]
    return pairs if n_de is None else (pairs[:n_de], pairs[n_de:])


def _pack(ctx, fixed, optional, params):
    """The tensors for ctx.save_for_backward: `fixed`, those of `optional` = {name: tensor | tuple of tensors | None} that are there (None
    entries of a tuple are not), `params`.  ctx remembers which are there; `_unpack` hands them back by name."""
    layout, there = {}, []
    for name, v in optional.items():
        if v is None:
            layout[name] = None
        elif isinstance(v, tuple):
            layout[name] = [q is not None for q in v]
            there += [q for q in v if q is not None]
        else:
            layout[name] = True
            there.append(v)
    ctx.saved_layout = layout
    return (*fixed, *there, *params)


def _unpack(ctx, n_fixed):
    """(the n_fixed leading tensors, {name: what `_pack` was given under it}, params) of ctx.saved_tensors."""
    sv = ctx.saved_tensors
    rest = iter(sv[n_fixed:])
    optional = {}
    for name, lay in ctx.saved_layout.items():
        if lay is None:
            optional[name] = None
        elif lay is True:
            optional[name] = next(rest)
        else:
            optional[name] = tuple(next(rest) if there else None for there in lay)
    return sv[:n_fixed], optional, tuple(rest)


@functools.lru_cache(maxsize=None)
def _arg_index(cls) -> dict:
    """name -> position of the arguments of cls.forward between ctx and *params: the signature is the one declaration of the order."""
    return {name: k for k, name in enumerate(list(inspect.signature(cls.forward).parameters)[1:-1])}


def _arg_names(cls) -> tuple:
    return tuple(_arg_index(cls))


def _needs(ctx, cls, name) -> bool:
    return bool(ctx.needs_input_grad[_arg_index(cls)[name]])


def _grad_tuple(ctx, cls, grads, param_grads) -> tuple:
    """What cls.backward returns: grads = {forward argument: gradient} at the arguments' positions (where the input needs one), None for
    every other argument, then the parameters' gradients."""
    index = _arg_index(cls)
    out = [None] * len(index)
    for name, g in grads.items():
        k = index[name]
        out[k] = g if ctx.needs_input_grad[k] else None
    return (*out, *param_grads)


class _FusedOde(torch.autograd.Function):
    @staticmethod
    def forward(ctx, method, kernel, act, event_idx, t, x0, z, all_initial, z_jump, *params):
        # act: the MLP's activation (fused.Act), None = ELU(1)
        layers = _layers(params)
        global last_saved_bytes
        last_saved_bytes = 0
        ctx.method, ctx.act, ctx.event_idx, ctx.bwd_kernel = method, act, event_idx, "auto"
        saved = x_true = None
        if act is not None:      # K0 forward (it saves nothing) + K5 backward; no teacher forcing (the solver walks those calls)
            if x0.dim() == 3:
                raise ValueError("teacher-forced training with an activation other than ELU(1) has no fused backward")
            xs = fused.ode_integrate(method, layers, t, x0.unsqueeze(0), z, all_initial, z_jump=z_jump, event_idx=event_idx, kernel=kernel,
                                     act=act)
        elif x0.dim() == 3:      # teacher forcing (my_solvers.py:72-74): x0 is the whole dataset x [T,B,xd]; nothing is saved, K4f / K5 recompute
            x_true = x0.detach().contiguous()
            xs = fused.ode_integrate(method, layers, t, x_true, z, all_initial, z_jump=z_jump, event_idx=event_idx, kernel=kernel,
                                     input_true_x=True)
            ctx.bwd_kernel = kernel      # "auto" / "mfma": K4f where the shape is its, "auto" else and "generic": K5
            # (the dataset rows go through save_for_backward like everything else the backward reads: autograd's version counter then
            #  catches an in-place edit of x between forward and backward)
        else:
            if kernel == "generic" and not _is_tableau(method) and fused.latent_wide_shape(layers, None, x0.shape[-1], z.shape[-1]):
                global _warned_generic_override
                if not _warned_generic_override:
                    _warned_generic_override = True
                    warnings.warn("kernel='generic' is ignored for training at the latent hidden widths other than 16 / 64: the only backward "
                                  "there reads the rows K3w saves (K0 saves nothing)", RuntimeWarning, stacklevel=3)
                kernel = "auto"      # training at these widths exists on K3w + K9w only (K0 saves nothing)
            save = _want_saved(method, kernel, layers, x0.shape[-1], z.shape[-1], t.shape[0], t.shape[1])
            res = fused.ode_integrate(method, layers, t, x0.unsqueeze(0), z, all_initial, z_jump=z_jump, event_idx=event_idx, kernel=kernel,
                                      save=save)
            xs, saved = res if save else (res, None)
            last_saved_bytes = sum(q.numel() * q.element_size() for q in saved) if saved is not None else 0
            ctx.bwd_kernel = {"wave": "wave", "tile": "tile"}.get(kernel, "auto")      # a forced forward form forces its backward counterpart (K4x / K4f)
            if ctx.bwd_kernel != "auto" and not fused.ode_backward_supported(method, layers, x0.shape[-1], z.shape[-1], ctx.bwd_kernel):
                ctx.bwd_kernel = "auto"                                                    # ... where that counterpart exists for the shape
        ctx.save_for_backward(*_pack(ctx, (t, z, all_initial, xs), dict(z_jump=z_jump, saved=saved, x_true=x_true), params))
        return xs

    @staticmethod
    def backward(ctx, grad_xs):
        (t, z, a0, xs), opt, params = _unpack(ctx, 4)
        z_jump, saved, x_true = opt["z_jump"], opt["saved"], opt["x_true"]
        need_z = _needs(ctx, _FusedOde, "z")
        if x_true is not None:   # teacher forcing: every step started from a dataset row -- K4f / K5 with the dataset as `xs`, no carried adjoint
            gx0, gz, gzj, ga0, gpar = fused.ode_backward(ctx.method, _layers(params), t, z, a0, x_true, grad_xs, event_idx=ctx.event_idx,
                                                         z_jump=z_jump, need_grad_z=need_z, kernel=ctx.bwd_kernel, input_true_x=True)
            gx0 = None           # (no gradient for the dataset x)
        else:
            gx0, gz, gzj, ga0, gpar = fused.ode_backward(ctx.method, _layers(params), t, z, a0, xs, grad_xs, event_idx=ctx.event_idx, z_jump=z_jump,
                                                         need_grad_z=need_z, saved=saved, need_grad_zj=_needs(ctx, _FusedOde, "z_jump"),
                                                         kernel=ctx.bwd_kernel if saved is not None else "auto", act=ctx.act)
        if gz is None and need_z:
            gz = torch.zeros_like(z)
        return _grad_tuple(ctx, _FusedOde, dict(x0=gx0, z=gz, all_initial=ga0, z_jump=gzj), gpar)


class _FusedOdeGeneric(torch.autograd.Function):
    """integrate_ODE on the option families of the generic kernels that save sub-state rows ("sub", "lin", "pev", "ab", "ms" of
    fused.GenericOpts.family), plain or teacher-forced: K0 forward in the family's build, which also writes the start state of every
    sub-step behind an interval's first (x_sub, saved next to xs; empty for one step per interval), K5 backward in the same build.
    opts: the call's fused.GenericOpts -- its fields travel to both calls; tx: x0 is the whole dataset x [T,B,xd] (no gradient);
    event_idx: the [T-1] table, or the [T-1, B] one of per-trajectory events (a trajectory's jump gradient goes to its own row of z_jump);
    x_data: the detached dataset rows the restarts of the family "ms" read, [T, B, xd] with row 0 the start of the call ([1, B, xd] where no
    step restarts) -- no gradient, x0 gets segment 0's; None for every other family.
    The classes autograd reports (`_FAMILY_CLASSES`) are empty subclasses: one name per family, this one body."""

    @staticmethod
    def forward(ctx, method, opts, kernel, tx, event_idx, t, x0, x_data, z, all_initial, z_jump, *params):
        global last_saved_bytes
        x_in = x_data if x_data is not None else (x0.detach().contiguous() if tx else x0.unsqueeze(0))
        xs, x_sub = fused.ode_integrate(method, _layers(params), t, x_in, z, all_initial, z_jump=z_jump, event_idx=event_idx, kernel=kernel,
                                        input_true_x=tx, act=opts.acts[0], substeps=opts.substeps, save_sub=True, externals=opts.externals,
                                        per_trajectory=opts.per_trajectory, segment=opts.segment, segment_parallel=opts.chunks(t.shape[0]))
        last_saved_bytes = x_sub.numel() * x_sub.element_size()
        ctx.method, ctx.opts, ctx.kernel, ctx.tx, ctx.event_idx = method, opts, kernel, tx, event_idx
        # (tx: the backward starts every interval from the dataset row and reads no xs)
        ctx.save_for_backward(*_pack(ctx, (t, z, all_initial, x_in if tx else xs, x_sub), dict(z_jump=z_jump, x_data=x_data), params))
        return xs

    @staticmethod
    def backward(ctx, grad_xs):
        (t, z, a0, xs, x_sub), opt, params = _unpack(ctx, 5)
        opts, cls = ctx.opts, _FusedOdeGeneric
        need_z = _needs(ctx, cls, "z")
        gx0, gz, gzj, ga0, gpar = fused.ode_backward(ctx.method, _layers(params), t, z, a0, xs, grad_xs, event_idx=ctx.event_idx, z_jump=opt["z_jump"],
                                                     need_grad_z=need_z, need_grad_zj=_needs(ctx, cls, "z_jump"), kernel=ctx.kernel,
                                                     input_true_x=ctx.tx, act=opts.acts[0], substeps=opts.substeps, x_sub=x_sub,
                                                     externals=opts.externals, per_trajectory=opts.per_trajectory, segment=opts.segment,
                                                     x_true=opt["x_data"], segment_parallel=opts.chunks(t.shape[0]))
        if gz is None and need_z:
            gz = torch.zeros_like(z)
        return _grad_tuple(ctx, cls, dict(x0=None if ctx.tx else gx0, z=gz, all_initial=ga0, z_jump=gzj), gpar)


# fused.GenericOpts.family ("ab": with per_trajectory) -> the name of its Function: `_FusedOde<name>` / `_FusedDae<name>`, an empty subclass of
# the model's one body, is what xs.grad_fn reports.  A further family of K0 / K5 that saves sub-state rows adds a row here, not a class.
_FAMILY_CLASSES = {"sub": "Sub", "lin": "Lin", "lag": "Lag", "pev": "Pev", ("ab", False): "Ab", ("ab", True): "AbPev", ("ab3", False): "Ab3", ("ab3", True): "Ab3Pev", "ms": "Ms", "msp": "Msp", "rkc": "Rkc", "sth": "Sth"}
# the families that go to _FusedOde / _FusedDae / _FusedDaeTeacherForced
_OWN_CLASS = ("plain", "act", "rk")
# ... and those whose forward (fused.ode_integrate / fused.dae_integrate) is the first to check the call
_CHECKED_BY_FORWARD = _OWN_CLASS + ("sub", "lin", "lag", "sth")


def _family_classes(body, prefix) -> dict:
    return {key: type(prefix + name, (body,), {"__doc__": f"{body.__name__} for the family {key!r} of fused.GenericOpts."})
            for key, name in _FAMILY_CLASSES.items()}


def _family_class(classes, opts):
    return classes[(opts.family, opts.per_trajectory) if opts.family in ("ab", "ab3") else opts.family]


def _refuse(what, opts, kernel, teacher_forced):
    """The refusals of a differentiable call, under the name `what`: teacher forcing next to Adams-Bashforth 2 / 3 or segments (ValueError), the
    families that have no kernel, a kernel other than "auto" / "generic" (UnsupportedShapeError)."""
    if opts.family not in _CHECKED_BY_FORWARD:
        opts.no_teacher_forcing(what, teacher_forced)
        opts.require_generic(what, kernel, False)


_ODE_CLASSES = _family_classes(_FusedOdeGeneric, "_FusedOde")
globals().update({cls.__name__: cls for cls in _ODE_CLASSES.values()})      # _FusedOdeSub, ..Lin, ..Pev, ..Ab, ..AbPev, ..Ms, ..Msp


def fused_ode_integrate(method, kernel, layers, t, x, z, all_initial, event_t=None, z_jump=None, check_events=False, input_true_x=False,
                        x_init=None, act=None, substeps=1, externals="hold", per_trajectory=False, segment=None, segment_parallel=None):
    """Differentiable fused integrate_ODE: gradients flow to x[0], z, all_initial, z_jump and the MLP.  input_true_x (teacher forcing,
    my_solvers.py:72-74): every step starts from the dataset row x[k]; gradients flow to z, all_initial, z_jump and the MLP (the dataset
    x gets none: callers whose x requires grad take the callback walk).  act: the MLP's activation (fused.Act), None = ELU(1); any other
    trains on K0 + K5 (no teacher forcing).  per_trajectory: every trajectory jumps at its own event times (fused.event_table(...,
    per_trajectory=True)); a call without events is the call it is without the flag.  segment: multiple shooting -- the dataset rows get
    no gradient (a caller whose x requires grad and restarts walks).  segment_parallel (None, "auto", an int >= 1): the segments on a
    tiles x chunks launch grid, forward and backward (fused.ode_integrate); one chunk is the call without it."""
    with torch.no_grad():
        event_idx = fused.event_table(t, event_t, check_events, per_trajectory=per_trajectory)
    if event_idx is None:
        z_jump = None
    params = [p for wb in layers for p in wb]
    tx = bool(input_true_x)
    x0 = x.detach() if tx else (x[0] if x_init is None else x_init)     # (x_init: integrate_ODE's extension -- no SelectBackward)
    opts = fused.GenericOpts.of(method, (act,), substeps, externals, bool(per_trajectory) and event_idx is not None, segment,
                                fused.resolve_segment_parallel(segment_parallel, segment, t.shape[0], t.shape[1], t.device))
    _refuse("fused_ode_integrate", opts, kernel, tx)
    if opts.family in _OWN_CLASS:
        return _FusedOde.apply(method, kernel, act, event_idx, t, x0, z, all_initial, z_jump, *params)
    x_data = None
    if opts.segment is not None and t.shape[0] - 1 > opts.segment:
        x_data = x.detach() if x_init is None else torch.cat((x_init.detach().unsqueeze(0), x.detach()[1:]))
    elif opts.segment is not None:      # no step restarts: row 0, the start of the call, is all that is read
        x_data = x0.detach().unsqueeze(0)
    return _family_class(_ODE_CLASSES, opts).apply(method, opts, kernel, tx, event_idx, t, x0, x_data, z, all_initial, z_jump, *params)


def _dae_act(acts):
    """The `act=` of a fused DAE call from a call's pair of activations (fused.dae_acts): None where both are ELU(1)."""
    return acts if any(a is not None for a in acts) else None


def _dae_grads(ctx, cls, g, z, v) -> tuple:
    """The return value of a DAE Function's backward from the dict of fused.dae_backward (the dataset rows of a teacher-forced call get none)."""
    gz = g["z"] if g["z"] is not None else (torch.zeros_like(z) if _needs(ctx, cls, "z") else None)
    gv = g["v"] if g["v"] is not None else (torch.zeros_like(v) if _needs(ctx, cls, "v") else None)
    return _grad_tuple(ctx, cls, dict(x_init=g["x_init"], z=gz, v=gv, all_initial=g["all_initial"], z_jump=g["z_jump"], v_jump=g["v_jump"]),
                       (*g["de"], *g["ae"]))


class _FusedDae(torch.autograd.Function):
    @staticmethod
    def forward(ctx, method, kernel, act, event_idx, n_de, t, x_init, z, v, i_shape_like, all_initial, z_jump, v_jump, *params):
        # act: None or (de_act, ae_act); with an activation other than ELU(1): K0 + K5, nothing saved
        de, ae = _layers(params, n_de)
        T, B = t.shape[0], t.shape[1]
        x_dummy = x_init.new_zeros((1, B, 0))
        if kernel == "generic" and not _is_tableau(method) and fused.latent_wide_shape(de, ae, x_init.shape[-1], z.shape[-1], v.shape[-1],
                                                                                        i_shape_like.shape[-1]):
            kernel = "auto"
        ctx.act = _dae_act(fused.dae_acts(act))
        save = ctx.act is None and _want_saved_dae(method, kernel, de, ae, x_init.shape[-1], z.shape[-1], v.shape[-1], i_shape_like.shape[-1], T, B)
        res = fused.dae_integrate(method, de, ae, x_init, t, x_dummy, z, v, i_shape_like, all_initial, z_jump=z_jump, v_jump=v_jump,
                                  event_idx=event_idx, kernel=kernel, save=save, act=ctx.act)
        xs, is_ = res[0], res[1]
        saved = res[2] if save else None
        global last_saved_bytes
        last_saved_bytes = sum(q.numel() * q.element_size() for q in saved if q is not None) if save else 0
        ctx.method, ctx.n_de, ctx.event_idx = method, n_de, event_idx
        ctx.save_for_backward(*_pack(ctx, (t, z, v, all_initial, xs, is_), dict(z_jump=z_jump, v_jump=v_jump, saved=saved), params))
        return xs, is_

    @staticmethod
    def backward(ctx, grad_xs, grad_is):
        (t, z, v, a0, xs, is_), opt, params = _unpack(ctx, 6)
        de, ae = _layers(params, ctx.n_de)
        g = fused.dae_backward(ctx.method, de, ae, t, z, v, a0, xs, is_, grad_xs, grad_is, event_idx=ctx.event_idx, act=ctx.act, **opt)
        return _dae_grads(ctx, _FusedDae, g, z, v)


class _FusedDaeTeacherForced(torch.autograd.Function):
    """integrate_DAE with input_true_x and / or input_true_i (my_solvers.py:111-121): forward K2 / K0 with the flags (nothing saved),
    backward with the dataset rows on K7f in its recompute form (psnode_dae_bwd_wide_args_f32::x_true / i_true) where the shape is its and
    the kernel "auto" / "mfma", else on K5 (psnode_dae_bwd_tf_args_f32).  The dataset rows get no gradient."""

    @staticmethod
    def forward(ctx, method, kernel, event_idx, n_de, tx, ti, t, x_init, x, z, v, i, all_initial, z_jump, v_jump, *params):
        de, ae = _layers(params, n_de)
        xs, is_ = fused.dae_integrate(method, de, ae, x_init, t, x, z, v, i, all_initial, z_jump=z_jump, v_jump=v_jump, event_idx=event_idx,
                                      kernel=kernel, input_true_x=tx, input_true_i=ti)[:2]
        ctx.method, ctx.n_de, ctx.event_idx, ctx.tx, ctx.ti = method, n_de, event_idx, tx, ti
        ctx.k7f = _dae_tf_on_k7f(method, kernel, de, ae, x_init.shape[-1], z.shape[-1], v.shape[-1], i.shape[-1])
        ctx.kernel = kernel
        ctx.save_for_backward(*_pack(ctx, (t, z, v, all_initial, xs, is_, x, i), dict(z_jump=z_jump, v_jump=v_jump), params))
        return xs, is_

    @staticmethod
    def backward(ctx, grad_xs, grad_is):
        (t, z, v, a0, xs, is_, x, i), opt, params = _unpack(ctx, 8)
        de, ae = _layers(params, ctx.n_de)
        rows = dict(x_true=x if ctx.tx else None, i_true=i if ctx.ti else None)
        if ctx.k7f:
            g = fused.dae_backward_wide(ctx.method, de, ae, t, z, v, a0, xs, is_, grad_xs, grad_is, event_idx=ctx.event_idx, **opt, **rows)
        else:
            g = fused.dae_backward_tf(ctx.method, de, ae, t, z, v, a0, xs, is_, grad_xs, grad_is, event_idx=ctx.event_idx, kernel=ctx.kernel,
                                      **opt, **rows)
        return _dae_grads(ctx, _FusedDaeTeacherForced, g, z, v)


class _FusedDaeGeneric(torch.autograd.Function):
    """integrate_DAE on the option families of the generic kernels that save sub-state rows ("sub", "lin", "pev", "ab", "ms"), plain or
    teacher-forced: K0 forward and K5 backward in the family's builds, x_sub saved next to xs / is -- as _FusedOdeGeneric.  x / i: the
    detached dataset rows of a teacher-forced call (tx / ti) and, x, the rows [T, B, xd] the restarts of the family "ms" read; they get
    no gradient (x_init gets segment 0's)."""

    @staticmethod
    def forward(ctx, method, opts, kernel, tx, ti, event_idx, n_de, t, x_init, x, z, v, i, all_initial, z_jump, v_jump, *params):
        de, ae = _layers(params, n_de)
        act = _dae_act(opts.acts)
        xs, is_, x_sub = fused.dae_integrate(method, de, ae, x_init, t, x, z, v, i, all_initial, z_jump=z_jump, v_jump=v_jump, event_idx=event_idx,
                                             kernel=kernel, input_true_x=tx, input_true_i=ti, act=act, substeps=opts.substeps, save_sub=True,
                                             externals=opts.externals, per_trajectory=opts.per_trajectory, segment=opts.segment,
                                             segment_parallel=opts.chunks(t.shape[0]), algebraic=opts.algebraic)
        global last_saved_bytes
        last_saved_bytes = x_sub.numel() * x_sub.element_size()
        ctx.method, ctx.opts, ctx.kernel, ctx.act, ctx.tx, ctx.ti, ctx.n_de, ctx.event_idx = method, opts, kernel, act, tx, ti, n_de, event_idx
        ctx.save_for_backward(*_pack(ctx, (t, z, v, all_initial, xs, is_, x_sub, x, i), dict(z_jump=z_jump, v_jump=v_jump), params))
        return xs, is_

    @staticmethod
    def backward(ctx, grad_xs, grad_is):
        (t, z, v, a0, xs, is_, x_sub, x, i), opt, params = _unpack(ctx, 9)
        de, ae = _layers(params, ctx.n_de)
        opts = ctx.opts
        common = dict(event_idx=ctx.event_idx, kernel=ctx.kernel, substeps=opts.substeps, x_sub=x_sub, externals=opts.externals,
                      per_trajectory=opts.per_trajectory, algebraic=opts.algebraic, **opt)
        if ctx.tx or ctx.ti:
            g = fused.dae_backward_tf(ctx.method, de, ae, t, z, v, a0, xs, is_, grad_xs, grad_is, x_true=x if ctx.tx else None,
                                      i_true=i if ctx.ti else None, **common)
        else:
            g = fused.dae_backward(ctx.method, de, ae, t, z, v, a0, xs, is_, grad_xs, grad_is, act=ctx.act, segment=opts.segment,
                                   x_true=x if opts.segment is not None else None, segment_parallel=opts.chunks(t.shape[0]), **common)
        return _dae_grads(ctx, _FusedDaeGeneric, g, z, v)


_DAE_CLASSES = _family_classes(_FusedDaeGeneric, "_FusedDae")
globals().update({cls.__name__: cls for cls in _DAE_CLASSES.values()})      # _FusedDaeSub, ..Lin, ..Pev, ..Ab, ..AbPev, ..Ms, ..Msp


def fused_dae_integrate(method, kernel, de_layers, ae_layers, x_init, t, z, v, i, all_initial, event_t=None, z_jump=None, v_jump=None,
                        check_events=False, x=None, input_true_x=False, input_true_i=False, act=None, substeps=1, externals="hold",
                        per_trajectory=False, segment=None, segment_parallel=None, algebraic="step"):
    """algebraic="stage": the stage-heads family (the "step" call under input_true_i); gradients reach everything listed below.
    Differentiable fused integrate_DAE: gradients flow to x_init, z, v, all_initial, the jump inputs and both MLPs.  Without teacher
    forcing `i` only provides the width of the algebraic variable.  input_true_x / input_true_i: `x` / `i` are the dataset rows the DE
    and the heads are fed (my_solvers.py:111-121); they get no gradient.  act: None or (de_act, ae_act) (fused.Act, None = ELU(1)); an
    activation other than ELU(1) trains on K0 + K5 (no teacher forcing).  per_trajectory: as fused_ode_integrate.  segment: multiple
    shooting -- `x` is the dataset rows the restarts read; they get no gradient.  segment_parallel: as fused_ode_integrate."""
    with torch.no_grad():
        event_idx = fused.event_table(t, event_t, check_events, per_trajectory=per_trajectory)
    if event_idx is None:
        z_jump = v_jump = None
    else:
        z_jump = z_jump if (z_jump is not None and z_jump.shape[-1] > 0) else None
        v_jump = v_jump if (v_jump is not None and v_jump.shape[-1] > 0) else None
    params = [p for wb in list(de_layers) + list(ae_layers) for p in wb]
    tx, ti = bool(input_true_x), bool(input_true_i)
    opts = fused.GenericOpts.of(method, fused.dae_acts(act), substeps, externals, bool(per_trajectory) and event_idx is not None, segment,
                                fused.resolve_segment_parallel(segment_parallel, segment, t.shape[0], t.shape[1], t.device),
                                _dae_algebraic(algebraic, ti))
    _refuse("fused_dae_integrate", opts, kernel, tx or ti)
    if opts.segment is not None and (x is None or x.shape[-1] == 0):
        raise ValueError(f"fused_dae_integrate: segment={segment} restarts from the dataset rows x[k]; this call has none")
    if opts.family in _OWN_CLASS and not (tx or ti):
        return _FusedDae.apply(method, kernel, act, event_idx, len(de_layers), t, x_init, z, v, i.detach(), all_initial, z_jump, v_jump, *params)
    rows = x.detach() if (tx or opts.segment is not None) else x_init.new_zeros((1, t.shape[1], 0))
    if opts.family in _OWN_CLASS:
        return _FusedDaeTeacherForced.apply(method, kernel, event_idx, len(de_layers), tx, ti, t, x_init, rows, z, v, i.detach(), all_initial,
                                            z_jump, v_jump, *params)
    return _family_class(_DAE_CLASSES, opts).apply(method, opts, kernel, tx, ti, event_idx, len(de_layers), t, x_init, rows, z, v, i.detach(),
                                                   all_initial, z_jump, v_jump, *params)
