"""Backward of `ode_integrate` (psnode_ode_backward_f32): K4f in one launch at hidden <= 128, K8f / K9 / K9w for the latent shapes of the
direct_encode models, the generic K5 otherwise."""
import ctypes

import torch

from .. import _lib
from ._common import (KERNEL_ID, GenericOpts, Layers, _aligned16, _bind_jumps, _check_saved, _check_x_sub, _empty, _f32_dev, _mlp, _split_grads, _view, _workspace_of, call_generic, check_event_idx, lagrange_stencils, _ms_rows, check_segment_parallel, resolve_segment_parallel)
from .latent import latent_backward_wide, latent_wide_shape

def _bwd_args(opts, de_layers, x_dim, z_dim, T, B, dev, keep, kernel="auto"):
    a = _lib.OdeBwdArgsF32()
    a.method = opts.method_id
    a.kernel = KERNEL_ID[kernel]
    a.x_dim, a.z_dim, a.T, a.B = x_dim, z_dim, T, B
    a.de = _mlp(de_layers, dev, "de", keep)
    return a


def ode_backward_supported(method, de_layers: Layers, x_dim: int, z_dim: int, kernel: str = "auto", act=None, substeps: int = 1,
                           externals: str = "hold", per_trajectory: bool = False, segment=None, segment_parallel=None) -> bool:
    """True if a fused backward kernel covers this shape: the MFMA class (3n->64->64->64->x, x<=8, z<=4) or any MLP whose
    activations and parameter gradients fit the LDS (generic backward).  act (fused.Act) other than None = ELU(1): K5 only.
    method a fused.Tableau: K5's tableau build only (kernel "auto" / "generic"; it answers for its own LDS fit).  substeps > 1: K5's
    sub-step build only, under the same rules.  externals="linear": K5's linear-externals build only (every substeps >= 1; its own LDS fit).
    per_trajectory=True (a call WITH events): K5's per-trajectory build only (every substeps >= 1; never together with externals="linear").
    segment (an int >= 1): K5's multiple-shooting build only (every substeps >= 1; never together with either of the two before).
    segment_parallel (not None; needs segment): K5's segment-parallel build answers -- its fit is the multiple-shooting build's."""
    check_segment_parallel(segment_parallel, segment)
    if de_layers[0][0].device.type != "cuda" or len(de_layers) > _lib.MAX_LAYERS:
        return False
    opts = GenericOpts.of(method, (act,), substeps, externals, bool(per_trajectory), segment, None if segment_parallel is None else 1)
    if opts.family == "plain" and kernel in ("auto", "mfma") and latent_wide_shape(de_layers, None, x_dim, z_dim):
        return True                          # K3w (saving) + K9w + library GEMMs
    a = _bwd_args(opts, de_layers, x_dim, z_dim, 2, 1, de_layers[0][0].device, [], kernel)
    return bool(call_generic(_lib.load(), "ode_backward", "supported", a, opts)[0])


def ode_backward(method, de_layers: Layers, t, z, all_initial, xs, grad_xs, event_idx=None, z_jump=None, need_grad_z: bool = True,
                 kernel: str = "auto", saved=None, input_true_x: bool = False, need_grad_zj: bool = True, act=None, substeps: int = 1,
                 x_sub=None, externals: str = "hold", per_trajectory: bool = False, segment=None, x_true=None, segment_parallel=None):
    """Backward pass of `ode_integrate` in one launch.  `saved` = what `ode_integrate(save=True)` returned next to
    xs: K4f then skips the recompute of the stage evaluations.  input_true_x: backward of a teacher-forced call (my_solvers.py:72-74) --
    `xs` must then be the DATASET x the forward call started every step from; K4f where the shape is its (hidden <= 128, x_dim <= 8) and
    kernel is not "generic", else the generic K5 (kernel "auto" / "generic").
    need_grad_z / need_grad_zj = False: dL/dz / dL/dz_jump are not formed (the scripts' z and z_jump are dataset tensors: K4x then runs
    without its per-step dL/dz layer, and the [B,nE,zd] zero fill is not made).
    kernel: "wave" = K4x (one wave per 4 trajectories; hidden 33..64, saved rows), "wide" / "tile" = K4f; "auto" picks between them.
    act: the hidden layers' activation (fused.Act); None = ELU(1).  Any other runs on the generic backward K5 only (kernel "auto" /
    "generic", no saved rows, no teacher forcing).
    method: "euler" | "midpoint" | "rk4", or a fused.Tableau -- K5 only (kernel "auto" / "generic", no saved rows).
    substeps > 1: backward of `ode_integrate(..., substeps=, save_sub=True)`, with the x_sub [T-1, substeps-1, B, xd] it returned -- K5 only
    (kernel "auto" / "generic", no saved rows; teacher forcing with ELU(1) only).
    externals="lagrange": backward of `ode_integrate(..., externals="lagrange")` -- K5's Lagrange build, the same rules; node m's share of a
    stage's external adjoint is added to row s + m of grad_z (a jumped node's to grad_z_jump); the kernel zeroes every row itself.
    externals="linear": backward of `ode_integrate(..., externals="linear")` -- K5's linear-externals build, the same rules; grad_z row k + 1
    also receives the right-hand share theta g of interval k's stages.
    per_trajectory=True: backward of `ode_integrate(..., per_trajectory=True)`; `event_idx` is the int32 [T-1, B] table -- K5's
    per-trajectory build, the rules of substeps (x_sub where substeps > 1).  grad_z_jump[b, e] receives the adjoint of trajectory b's
    interval that event e opens (exactly 0 where it never fires), grad_z[k, b] is exactly 0 where b jumps at k.  Without an event table
    the flag means nothing.
    segment (an int w >= 1): backward of `ode_integrate(..., segment=w)` -- K5's multiple-shooting build, the rules of substeps; x_true
    [T, B, xd] is the dataset x of the forward call (needed where T - 1 > w; it gets no gradient).  The start adjoint of a restart step
    is dropped: grad_x0 is segment 0's, grad_xs[k] of a restart point still travels back into the segment before it.
    segment_parallel (None, "auto" or an int g >= 1; needs segment): K5 on a tiles x chunks launch grid, workgroup (tile, c) sweeping time
    chunk c alone (the grouping of `ode_integrate`).  grad_x0, grad_z and grad_z_jump are bit for bit those of the call without it; the
    parameter gradients and grad_all_initial are the same sums in another order (one partial per workgroup / per chunk).
    Returns (grad_x0 [B,xd], grad_z [T,B,zd] | None, grad_z_jump | None, grad_all_initial [B,n], [grad W1, b1, ..., W4, b4])."""
    lib = _lib.load()
    dev = xs.device
    T, B, xd = xs.shape
    zd = z.shape[-1]
    # kernel: "auto" / "mfma" = the one-launch K4f at every hidden width <= 128 (z_dim <= 8), K8f / K9 / K9w for the latent shapes, else the
    # generic K5 ("auto" only); "wide" forces K4f
    per_trajectory = bool(per_trajectory) and event_idx is not None
    opts = GenericOpts.of(method, (act,), substeps, externals, per_trajectory, segment, resolve_segment_parallel(segment_parallel, segment, T, B, dev))
    opts.require_generic("ode_backward", kernel, saved is not None, teacher_forced=input_true_x)
    x_true = _ms_rows("ode_backward", segment, x_true, T, B, xd, dev)
    if per_trajectory:
        check_event_idx(event_idx, T, B, True, dev)
    _check_x_sub("ode_backward", opts.substeps, x_sub, T, B, xd, dev)
    if saved is not None and not input_true_x and latent_wide_shape(de_layers, None, xd, zd):
        g = latent_backward_wide(method, de_layers, None, t, z, None, all_initial, xs, None, grad_xs, None, event_idx=event_idx,
                                 z_jump=z_jump, saved=saved, need_grad_z=need_grad_z)
        return g["x_init"], g["z"], g["z_jump"], g["all_initial"], g["de"]
    keep: list = [x_sub, x_true]
    a = _bwd_args(opts, de_layers, xd, zd, T, B, dev, keep, kernel)
    if input_true_x:
        if saved is not None:
            raise ValueError("a teacher-forced forward saves no activations")
        a.flags = _lib.FLAG_INPUT_TRUE_X
    z, z_jump = _aligned16(z), _aligned16(z_jump)
    a.t = _view(t, dev, "t", keep)
    a.z = _view(z, dev, "z", keep)
    a0 = _f32_dev(all_initial, dev, "all_initial").contiguous()
    xs_c = _f32_dev(xs, dev, "xs").contiguous()
    g_c = _f32_dev(grad_xs, dev, "grad_xs").contiguous()
    keep += [a0, xs_c, g_c]
    a.all_initial, a.xs, a.grad_xs = a0.data_ptr(), xs_c.data_ptr(), g_c.data_ptr()
    gzj = None
    _bind_jumps(a, event_idx, (("z_jump", z_jump),), dev, keep)
    if event_idx is not None:
        if z_jump is not None and zd > 0:
            a.n_events = z_jump.shape[1]
        if z_jump is not None and zd > 0 and need_grad_zj:
            gzj = torch.zeros((B, z_jump.shape[1], zd), dtype=torch.float32, device=dev)
            a.grad_z_jump = gzj.data_ptr()
    with torch.cuda.device(dev):
        gx0 = _empty((B, xd), dtype=torch.float32, device=dev)
        ga0 = _empty((B, xd + zd), dtype=torch.float32, device=dev)
        gz = _empty((T, B, zd), dtype=torch.float32, device=dev) if (need_grad_z and zd > 0) else None
        npar = lib.psnode_ode_backward_param_count(ctypes.byref(a))
        gpar = _empty(npar, dtype=torch.float32, device=dev)
        a.grad_x0, a.grad_all_initial, a.grad_params = gx0.data_ptr(), ga0.data_ptr(), gpar.data_ptr()
        a.grad_z = gz.data_ptr() if gz is not None else None
        if saved is not None and T >= 2:
            _check_saved(saved[0], saved[1], T, B, xd, opts.stages, len(de_layers) - 1, dev)
            keep += [saved[0], saved[1]]
            a.saved_act, a.saved_xstage = saved[0].data_ptr(), saved[1].data_ptr()
        nbytes = call_generic(lib, "ode_backward", "workspace_bytes", a, opts, x_sub=x_sub)[0]
        ws, wp, wn = _workspace_of(nbytes, dev)
        stencil = lagrange_stencils(t.detach(), event_idx) if opts.takes.stencil else None      # (externals="lagrange": the forward's table again)
        rc, entry = call_generic(lib, "ode_backward", "f32", a, opts, wp, wn, torch.cuda.current_stream(dev).cuda_stream, x_sub=x_sub, x_true=x_true,
                                 stencil=stencil)
    _lib.check(rc, entry)
    return gx0, gz, gzj, ga0, _split_grads(gpar, de_layers)
