"""Forward entry points on raw tensors: `ode_integrate` / `dae_integrate` (psnode_ode_integrate_f32 / psnode_dae_integrate_f32 -> K1 / K1x /
K2 / K3* / K0) and the queries that tell the autograd bridge which calls can save their activations."""
import ctypes
from typing import Optional

import torch

from .. import _lib
from ._common import (is_lagrange, KERNEL_ID, GenericOpts, resolve_segment_parallel, Layers, Tableau, Recurrence, builtin_method, _aligned16, _bind_events, _check_tb, _empty, _f32_dev, _mlp, _view, _workspace_of, call_generic, dae_acts, has_events, is_linear, lagrange_stencils)

_MFMA_CLASSES = ("MFMA integrators K1 / K2 cover `in -> H -> H -> H -> out` ELU-MLPs with H <= 128 (any x_dim <= 16 for the ODE, "
                 "x_dim <= 8 and z+v+i <= 8 for the DAE), and -- weights streamed from L2 -- the ODE up to H = 192 at any x_dim <= 16 and "
                 "up to H = 256 at x_dim <= 8, the DAE up to H = 192 with z+v+i <= 6")


_k0_warned = False


def _mfma_miss(rc: int, kernel: str, what: str, de_layers: Layers):
    """kernel='mfma' on a shape the MFMA integrators do not carry: say which shapes they do, and what the fallback costs."""
    if rc == -5 and kernel == "mfma":
        widths = [int(w.shape[0]) for w, _ in de_layers[:-1]]
        raise _lib.UnsupportedShapeError(
            f"{what}: no MFMA integrator for hidden widths {widths}.  {_MFMA_CLASSES}.  kernel='auto' runs this shape on the generic "
            "kernel K0 (any layer count and widths that fit the 160 KB LDS; MFMA layers since round 6), at 2.5-4x the time per "
            "state-step of a specialised integrator (9.5 vs 3.5 ms per 4096 x 1000 RK4 batch at hidden 64; DESIGN.md 'K0')")


def _note_k0(lib, args, dae: bool, de_layers: Layers):
    """AUTO landing on K0 with a no_encode-style MLP wider than the MFMA classes: never silently slower (2.5-4x per flop)."""
    global _k0_warned
    if _k0_warned or len(de_layers) != 4:
        return
    widths = [int(w.shape[0]) for w, _ in de_layers[:-1]]
    if len(set(widths)) != 1 or widths[0] <= 128:
        return
    k = (lib.psnode_dae_kernel_for if dae else lib.psnode_ode_kernel_for)(ctypes.byref(args))
    if k == _lib.KERNEL_GENERIC:
        _k0_warned = True
        import warnings
        warnings.warn(f"hidden width {widths[0]} runs on the generic kernel K0 (weights streamed from L2), at 2-3x the time per flop of the "
                      f"MFMA integrators.  {_MFMA_CLASSES}", RuntimeWarning, stacklevel=3)


def ode_integrate(method, de_layers: Layers, t, x, z, all_initial, event_t=None, z_jump=None,
                  input_true_x: bool = False, kernel: str = "auto", event_idx: Optional[torch.Tensor] = None,
                  check_events: bool = False, out: Optional[torch.Tensor] = None, save: bool = False, act=None, substeps: int = 1,
                  save_sub: bool = False, externals: str = "hold", per_trajectory: bool = False, segment=None, segment_parallel=None):
    """Fused integrate_ODE (replaces my_solvers.py:52-80 + my_fixed_grid.py + DE_Func.forward).

    method: "euler" | "midpoint" | "rk4" (the 3/8 rule), or a fused.Tableau -- any explicit Runge-Kutta method of up to four stages, on
    the generic kernel K0 only (kernel "auto" / "generic"; save=True is refused).
    act: the hidden layers' activation (fused.Act, from `sequential_mlp`); None = ELU(1).  Any other runs on the generic kernel K0 only
    (kernel "auto" / "generic"; save=True is refused).

    substeps (1..1024): sub-steps per grid interval, each of h = (t[k+1] - t[k]) / substeps with the interval's inputs held; xs stays on the
    grid of t.  More than 1 runs on the generic kernel K0 only (kernel "auto" / "generic"; save=True is refused).  save_sub=True (training
    forward): returns (xs, x_sub) with x_sub [T-1, substeps-1, B, xd] the start states of sub-steps 1.. of every interval, for
    `ode_backward(..., substeps=, x_sub=)` (None for substeps == 1).

    externals: "hold" (the left grid point's z feeds every stage of an interval) or "linear": stage s of sub-step j reads
    z[k] + theta (z[k+1] - z[k]) at theta = (j + c_s) / substeps, z[k] being the jumped row behind an event; the generic kernel K0 in its
    linear-externals build for every substeps >= 1 (kernel "auto" / "generic"; save=True is refused; save_sub then always returns a tensor).
    "lagrange": the polynomial through the up to four neighbouring dataset rows of the interval's piece at the same theta -- the Lagrange
    build, the same rules; the stencil table (`lagrange_stencils`) is built here from t and the shared event table.

    per_trajectory=True: trajectory b jumps where ITS clock t[k, b] equals one of ITS event times event_t[b, :] (exact equality, lowest
    matching column; NaN entries never fire) -- it is computed as the shared rule computes it in a batch of b alone.  `event_idx`, if
    given, is then the int32 [T-1, B] table of `event_table(..., per_trajectory=True)`.  The generic kernel K0 in its per-trajectory
    build for every substeps >= 1 (kernel "auto" / "generic"; save=True and externals="linear" are refused; save_sub then always returns a
    tensor).  A call without events (no event_t and no event_idx, T == 1, an empty list) is the call it is without the flag.

    segment (None, or an int w >= 1): multiple shooting -- the step that leaves grid point k > 0 with k % w == 0 starts from the dataset
    row x[k] (its first sub-step only), so rows m w + 1 .. (m + 1) w are the free run on the slices [m w : (m + 1) w + 1] from x[m w];
    row 0 of x is the start of the call, and x must hold all T rows where T - 1 > w.  The generic kernel K0 in its multiple-shooting
    build for every substeps >= 1 (kernel "auto" / "generic"; save=True, externals="linear" and per_trajectory events are refused, and
    input_true_x is a ValueError; save_sub then always returns a tensor).

    segment_parallel (None, "auto" or an int g >= 1; needs segment): where the call runs, never what it computes.  The n_seg =
    ceil((T - 1) / w) segments are grouped into up to g time chunks of ceil(n_seg / min(g, n_seg)) consecutive segments, and K0 runs on a
    tiles x chunks launch grid, workgroup (tile, c) integrating its 16 trajectories over chunk c alone; xs (and x_sub) are bit for bit
    those of the call without the option.  "auto": g = max(1, CUs // tiles).  One chunk is the call without the option.

    save=True (training forward, K1 shapes only -- `ode_save_hidden`): the kernel also writes what autograd would save, the hidden
    activations [T-1,S,3,B,Hp] and the stage inputs [T-1,S,B,xd]; returns (xs, (act, xstage)) for `ode_backward(..., saved=)`.

    t[T,B,1], x[T,B,xd], z[T,B,zd] may be arbitrary strided views with a unit-stride last dim
    (the scripts pass permute(1,0,2) views); returns a fresh contiguous xs[T,B,xd].
    Only x[0] is read unless input_true_x, so x may be a [1,B,xd] view (time-chunked launches restart from the previous
    chunk's last row); `out` (contiguous [T,B,xd]) lets the caller place the result, e.g. in a slice of a larger buffer.
    """
    lib = _lib.load()
    dev = x.device
    if dev.type != "cuda":
        raise ValueError("fused integrator needs tensors on a HIP device")
    per_trajectory = bool(per_trajectory) and has_events(t, event_t, event_idx)
    per_group = resolve_segment_parallel(segment_parallel, segment, t.shape[0], x.shape[1], dev)
    opts = GenericOpts.of(method, (act,), substeps, externals, per_trajectory, segment, per_group)
    opts.require_generic("ode_integrate", kernel, save)
    opts.no_teacher_forcing("ode_integrate", input_true_x)
    T, B, xd = t.shape[0], x.shape[1], x.shape[2]
    if x.shape[0] < (T if input_true_x or (segment is not None and T - 1 > segment) else 1):
        raise ValueError("x has fewer grid points than t")
    zd = z.shape[-1]
    _check_tb("t", t, T, B)
    _check_tb("z", z, T, B)
    keep: list = []
    a = _lib.OdeArgsF32()
    a.method = opts.method_id
    a.kernel = KERNEL_ID[kernel]
    a.flags = _lib.FLAG_INPUT_TRUE_X if input_true_x else 0
    a.x_dim, a.z_dim, a.T, a.B = xd, zd, T, B
    a.de = _mlp(de_layers, dev, "de", keep)
    if save:      # the latent-wide saving forward (K3w) reads rows as float4: a misaligned view is copied once here instead of failing in
        x, z, z_jump = _aligned16(x), _aligned16(z), _aligned16(z_jump)      # the middle of a training step (the backward does the same)
    a.t = _view(t, dev, "t", keep)
    a.x = _view(x, dev, "x", keep)
    a.z = _view(z, dev, "z", keep)
    a0 = _f32_dev(all_initial, dev, "all_initial").contiguous()
    if a0.shape != (B, xd + zd):
        raise ValueError(f"all_initial has shape {tuple(a0.shape)}, expected {(B, xd + zd)}")
    keep.append(a0)
    a.all_initial = a0.data_ptr()
    with torch.cuda.device(dev):
        event_idx = _bind_events(a, t, event_t, event_idx, check_events, (("z_jump", z_jump, zd),), B, dev, keep, per_trajectory)
        if out is None:
            out = _empty((T, B, xd), dtype=torch.float32, device=dev)
        elif out.shape != (T, B, xd) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != dev:
            raise ValueError("out must be a contiguous fp32 [T,B,xd] tensor on the inputs' device")
        a.x_out = out.data_ptr()
        saved = None
        if save:
            Hp = lib.psnode_ode_save_hidden(ctypes.byref(a))
            if Hp <= 0:
                raise _lib.UnsupportedShapeError("ode_integrate(save=True): the MFMA integrator K1 does not take this shape")
            L = len(de_layers) - 1       # hidden layers: 3 for the no_encode MLPs (K1), 1 for the latent ones at hidden 64 (K3c)
            saved = (_empty((max(T - 1, 0), opts.stages, L, B, Hp), dtype=torch.float32, device=dev),
                     _empty((max(T - 1, 0), opts.stages, B, xd), dtype=torch.float32, device=dev))
            if T >= 2:
                a.save_act, a.save_xstage = saved[0].data_ptr(), saved[1].data_ptr()
        x_sub = _empty((max(T - 1, 0), opts.substeps - 1, B, xd), dtype=torch.float32, device=dev) if save_sub and opts.takes.x_sub else None
        ws, wp, wn = _workspace_of(lib.psnode_workspace_bytes(ctypes.byref(a.de), None), dev)
        stencil = lagrange_stencils(t.detach(), event_idx) if opts.takes.stencil else None      # (externals="lagrange": int8 [T-1, B])
        rc, entry = call_generic(lib, "ode_integrate", "f32", a, opts, wp, wn, torch.cuda.current_stream(dev).cuda_stream, x_sub=x_sub, stencil=stencil)
    _mfma_miss(rc, kernel, entry, de_layers)
    _lib.check(rc, entry)
    if kernel == "auto" and opts.family == "plain":
        _note_k0(lib, a, False, de_layers)
    # the stream-ordered caching allocator keeps `keep`/`ws` storage valid until the kernel has run
    if save_sub:
        return out, x_sub
    return (out, saved) if save else out


def ode_save_hidden(method, de_layers: Layers, x_dim: int, z_dim: int, kernel: str = "auto", substeps: int = 1, externals: str = "hold") -> int:
    """Row width of the saved activations if the forward for these dims can save them (K1 proper), else 0 (always for a Tableau, for
    substeps > 1 and for externals="linear")."""
    if is_linear(externals) or substeps != 1 or isinstance(method, (Tableau, Recurrence)) or de_layers[0][0].device.type != "cuda" or len(de_layers) > _lib.MAX_LAYERS:
        return 0
    lib = _lib.load()
    a = _lib.OdeArgsF32()
    a.method, a.kernel, a.x_dim, a.z_dim, a.T, a.B = builtin_method(method, "ode_save_hidden")[0], KERNEL_ID[kernel], x_dim, z_dim, 2, 1
    a.de = _mlp(de_layers, de_layers[0][0].device, "de", [])
    return int(lib.psnode_ode_save_hidden(ctypes.byref(a)))


def dae_integrate(method, de_layers: Layers, ae_layers: Layers, x_init, t, x, z, v, i, all_initial,
                  event_t=None, z_jump=None, v_jump=None, input_true_x: bool = False, input_true_i: bool = False,
                  kernel: str = "auto", event_idx: Optional[torch.Tensor] = None, check_events: bool = False, out=None,
                  save: bool = False, act=None, substeps: int = 1, save_sub: bool = False, externals: str = "hold",
                  per_trajectory: bool = False, segment=None, segment_parallel=None, algebraic: str = "step"):
    """Fused integrate_DAE (replaces my_solvers.py:82-131 + step functions + DE_Func/AE_Func forwards).
    method: "euler" | "midpoint" | "rk4", or a fused.Tableau (generic kernel K0 only: kernel "auto" / "generic"; save=True is refused).
    act: None (both MLPs ELU(1)) or (de_act, ae_act), each a fused.Act or None = ELU(1); an activation other than ELU(1) runs on the
    generic kernel K0 only (kernel "auto" / "generic"; save=True is refused).
    substeps (1..1024): sub-steps per grid interval with z | v held; without input_true_i the algebraic variable is re-evaluated from the
    state at the start of every sub-step behind the first.  More than 1: the generic kernel K0 only (kernel "auto" / "generic", no save).
    save_sub=True (training forward): returns (xs, is, x_sub), x_sub [T-1, substeps-1, B, xd] for the backward (None for substeps == 1).
    externals: "hold", or "linear" -- every stage reads z | v interpolated between grid points k (the jumped rows behind an event) and k + 1
    at theta = (j + c_s) / substeps, as does the head in front of sub-step j >= 1 (theta = j / substeps); i is never interpolated.  K0's
    linear-externals build for every substeps >= 1 (kernel "auto" / "generic", no save); "lagrange": the four-point polynomial of the
    interval's piece in the straight line's place (the Lagrange build, the same rules; `lagrange_stencils`).
    algebraic: "step" (i frozen over the stages of a (sub-)step) or "stage" -- in front of every stage s >= 1 the head is evaluated at that
    stage's argument and interpolated externals, i_s = g(X_s; z | v at theta_s), and feeds the stage's DE evaluation (no output row).  Needs
    interpolated externals (ValueError with "hold"); K0's stage-heads builds (the family "sth": kernel "auto" / "generic", no save) under the
    rules of the interpolant.  With input_true_i (every stage reads i[k]) or a one-stage method it is the "step" call, bit for bit.
    per_trajectory=True: as `ode_integrate`, for z | v together; the event-time head i0 = g(x_k; z_jump, v_jump) replaces the carried
    algebraic variable of the trajectories with a hit at step k only, the others keep theirs.  K0's per-trajectory build for every
    substeps >= 1 (kernel "auto" / "generic", no save, not with externals="linear").
    segment (None, or an int w >= 1): multiple shooting, as `ode_integrate`; the DE of a restart step reads the head at the dataset row,
    g(x[k]; z_k, v_k) with the jumped rows behind an event, while xs[k] / is[k] stay the previous segment's prediction.  Needs the dataset
    x [T, B, x_dim] (ValueError without); teacher forcing is a ValueError.  K0's multiple-shooting build (kernel "auto" / "generic", no save).
    segment_parallel (None, "auto" or an int g >= 1; needs segment): as `ode_integrate` -- the segments in up to g time chunks on a
    tiles x chunks launch grid; xs, is and x_sub bit for bit those of the call without it.
    `out` = (xs, is) contiguous [T,B,xd] / [T,B,id] tensors to write into (time-chunked launches).
    save=True (training forward, K2 shapes without teacher forcing -- `dae_save_hidden`): the kernel also writes what autograd would
    save (psnode_dae_args_f32::save_*); returns (xs, is, saved) with saved = (act [T-1,S,3,B,Hp], xstage [T-1,S,B,xd],
    ae_act [3,T,B,Hp], ev_act [nE,3,B,Hp] | None, ev_i [nE,B,16] | None) for `dae_backward(..., saved=)`."""
    lib = _lib.load()
    dev = x_init.device
    if dev.type != "cuda":
        raise ValueError("fused integrator needs tensors on a HIP device")
    per_trajectory = bool(per_trajectory) and has_events(t, event_t, event_idx)
    per_group = resolve_segment_parallel(segment_parallel, segment, t.shape[0], t.shape[1], dev)
    opts = GenericOpts.of(method, dae_acts(act), substeps, externals, per_trajectory, segment, per_group, algebraic)
    if input_true_i and algebraic == "stage":      # (validated above; no head runs inside an interval: the "step" call)
        opts = GenericOpts.of(method, dae_acts(act), substeps, externals, per_trajectory, segment, per_group)
    opts.require_generic("dae_integrate", kernel, save)
    opts.no_teacher_forcing("dae_integrate", input_true_x or input_true_i)
    if segment is not None and x.shape[-1] == 0:
        raise ValueError(f"dae_integrate: segment={segment} restarts from the dataset rows x[k]; this call has none (x.shape[-1] == 0)")
    T, B = t.shape[0], t.shape[1]
    xd, zd, vd, idim = x_init.shape[-1], z.shape[-1], v.shape[-1], i.shape[-1]
    if x_init.dim() != 2 or x_init.shape[0] != B:
        raise ValueError(f"x_init: shape {tuple(x_init.shape)}, expected [B={B}, x_dim]")
    _check_tb("t", t, T, B)
    _check_tb("z", z, T, B)
    _check_tb("v", v, T, B)
    if input_true_x or segment is not None:
        _check_tb("x", x, T, B)
    if input_true_i:
        _check_tb("i", i, T, B)
    keep: list = []
    a = _lib.DaeArgsF32()
    a.method = opts.method_id
    a.kernel = KERNEL_ID[kernel]
    a.flags = (_lib.FLAG_INPUT_TRUE_X if input_true_x else 0) | (_lib.FLAG_INPUT_TRUE_I if input_true_i else 0)
    a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = xd, zd, vd, idim, T, B
    a.de = _mlp(de_layers, dev, "de", keep)
    a.ae = _mlp(ae_layers, dev, "ae", keep)
    if save:      # (as ode_integrate)
        x_init, z, v, z_jump, v_jump = _aligned16(x_init), _aligned16(z), _aligned16(v), _aligned16(z_jump), _aligned16(v_jump)
    a.t = _view(t, dev, "t", keep)
    a.x = _view(x if input_true_x or segment is not None else None, dev, "x", keep)
    a.z = _view(z, dev, "z", keep)
    a.v = _view(v, dev, "v", keep)
    a.i = _view(i if input_true_i else None, dev, "i", keep)
    if (input_true_x or segment is not None) and x.shape[-1] != xd:
        raise ValueError("input_true_x / segment need dataset x of width x_init.shape[-1]")
    xi = _f32_dev(x_init, dev, "x_init").contiguous()
    a0 = _f32_dev(all_initial, dev, "all_initial").contiguous()
    if a0.shape != (B, xd + zd + vd + idim):
        raise ValueError(f"all_initial has shape {tuple(a0.shape)}, expected {(B, xd + zd + vd + idim)}")
    keep += [xi, a0]
    a.x_init, a.all_initial = xi.data_ptr(), a0.data_ptr()
    with torch.cuda.device(dev):
        event_idx = _bind_events(a, t, event_t, event_idx, check_events, (("z_jump", z_jump, zd), ("v_jump", v_jump, vd)), B, dev, keep,
                                 per_trajectory)
        if out is None:
            xs = _empty((T, B, xd), dtype=torch.float32, device=dev)
            is_ = _empty((T, B, idim), dtype=torch.float32, device=dev)
        else:
            xs, is_ = out
            if xs.shape != (T, B, xd) or is_.shape != (T, B, idim) or not (xs.is_contiguous() and is_.is_contiguous()):
                raise ValueError("out must be contiguous fp32 ([T,B,xd], [T,B,id])")
        a.x_out, a.i_out = xs.data_ptr(), is_.data_ptr()
        saved = None
        if save:
            Hp = lib.psnode_dae_save_hidden(ctypes.byref(a))
            if Hp <= 0:
                raise _lib.UnsupportedShapeError("dae_integrate(save=True): the MFMA integrator K2 does not take this shape")
            f32 = dict(dtype=torch.float32, device=dev)
            n_ev = (z_jump if z_jump is not None else v_jump).shape[1] if event_idx is not None else 0
            L = len(de_layers) - 1       # hidden layers: 3 (K2), 1 for the latent shapes at hidden 64 (K3c; i0 rows are then i_dim wide)
            saved = (_empty((max(T - 1, 0), opts.stages, L, B, Hp), **f32), _empty((max(T - 1, 0), opts.stages, B, xd), **f32),
                     _empty((L, T, B, Hp), **f32),
                     torch.zeros((n_ev, L, B, Hp), **f32) if n_ev else None,
                     torch.zeros((n_ev, B, 16 if L == 3 else idim), **f32) if n_ev else None)
            a.save_act, a.save_xstage, a.save_ae_act = saved[0].data_ptr(), saved[1].data_ptr(), saved[2].data_ptr()
            if T < 2:       # no step: nothing but the head at grid point 0 is written; the struct wants all three or none
                dummy = _empty(16, **f32)
                keep.append(dummy)
                a.save_act = a.save_xstage = dummy.data_ptr()
            if n_ev:
                a.save_ev_act, a.save_ev_i = saved[3].data_ptr(), saved[4].data_ptr()
        x_sub = _empty((max(T - 1, 0), opts.substeps - 1, B, xd), dtype=torch.float32, device=dev) if save_sub and opts.takes.x_sub else None
        ws, wp, wn = _workspace_of(lib.psnode_workspace_bytes(ctypes.byref(a.de), ctypes.byref(a.ae)), dev)
        stencil = lagrange_stencils(t.detach(), event_idx) if opts.takes.stencil and is_lagrange(opts.externals) else None      # (externals="lagrange": int8 [T-1, B])
        rc, entry = call_generic(lib, "dae_integrate", "f32", a, opts, wp, wn, torch.cuda.current_stream(dev).cuda_stream, x_sub=x_sub, stencil=stencil)
    _mfma_miss(rc, kernel, entry, de_layers)
    _lib.check(rc, entry)
    if kernel == "auto" and opts.family == "plain":
        _note_k0(lib, a, True, de_layers)
    if save_sub:
        return xs, is_, x_sub
    return (xs, is_, saved) if save else (xs, is_)


def dae_save_hidden(method, de_layers: Layers, ae_layers: Layers, x_dim: int, z_dim: int, v_dim: int, i_dim: int,
                    kernel: str = "auto", substeps: int = 1, externals: str = "hold") -> int:
    """Row width of the saved activations if the forward for these dims can save them (K2 proper), else 0 (always for a Tableau, for
    substeps > 1 and for externals="linear")."""
    if is_linear(externals) or substeps != 1 or isinstance(method, (Tableau, Recurrence)) or de_layers[0][0].device.type != "cuda" or max(len(de_layers), len(ae_layers)) > _lib.MAX_LAYERS:
        return 0
    lib = _lib.load()
    a = _lib.DaeArgsF32()
    a.method, a.kernel, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = builtin_method(method, "dae_save_hidden")[0], KERNEL_ID[kernel], x_dim, z_dim, v_dim, i_dim, 2, 1
    dev = de_layers[0][0].device
    a.de, a.ae = _mlp(de_layers, dev, "de", []), _mlp(ae_layers, dev, "ae", [])
    return int(lib.psnode_dae_save_hidden(ctypes.byref(a)))
