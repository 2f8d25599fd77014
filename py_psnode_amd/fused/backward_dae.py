"""Backward of `dae_integrate`: K7f in one launch for the DAE_01 shape class at hidden <= 128 (psnode_dae_backward_wide_f32, + K7h for
the AE head's rows where the kernel does not form the head's gradients itself), K9 / K8 / K9w for the latent shapes, the generic K5
otherwise (psnode_dae_backward_f32); teacher-forced calls outside K7f's class go to K5 through psnode_dae_backward_tf_f32."""
import ctypes
import types

import torch

from .. import _lib
from ._common import (is_lagrange, KERNEL_ID, GenericOpts, Layers, _aligned16, _bind_jumps, _check_saved, _check_x_sub, _empty, _f32_dev, _mlp, _pad_rows, _padded_hidden, _split_grads, _view, _workspace_of, call_generic, check_event_idx, dae_acts, lagrange_stencils, _ms_rows, check_segment_parallel, resolve_segment_parallel)
from .latent import latent_backward_wide, latent_wide_shape

def dae_backward_supported(method, de_layers: Layers, ae_layers: Layers, x_dim, z_dim, v_dim, i_dim, act=None, kernel: str = "auto",
                           substeps: int = 1, externals: str = "hold", per_trajectory: bool = False, segment=None, segment_parallel=None,
                           algebraic: str = "step") -> bool:
    """algebraic="stage": K5's stage-heads builds only (the family "sth"; their fit is the interpolant's build's).
    act: None (both MLPs ELU(1)) or (de_act, ae_act); an activation other than ELU(1) is K5's alone.  kernel="generic": does K5 take
    the shape (the question a teacher-forced call outside K7f's class asks).  method a fused.Tableau: K5's tableau build only (kernel
    "auto" / "generic"; it answers for its own LDS fit).  substeps > 1: K5's sub-step build only, under the same rules.
    externals="linear": K5's linear-externals build only (every substeps >= 1; it answers for its own LDS fit).
    per_trajectory=True (a call WITH events): K5's per-trajectory build only (every substeps >= 1; never together with externals="linear").
    segment_parallel (not None; needs segment): K5's segment-parallel build answers -- its fit is the multiple-shooting build's."""
    check_segment_parallel(segment_parallel, segment)
    if de_layers[0][0].device.type != "cuda" or max(len(de_layers), len(ae_layers)) > _lib.MAX_LAYERS:
        return False
    opts = GenericOpts.of(method, dae_acts(act), substeps, externals, bool(per_trajectory), segment,      # (segment: K5's multiple-shooting build only)
                          None if segment_parallel is None else 1, algebraic)
    if opts.family == "plain" and kernel != "generic" and latent_wide_shape(de_layers, ae_layers, x_dim, z_dim, v_dim, i_dim):
        return True                          # K3w (saving) + K9w + library GEMMs
    args = opts.dae_backward_args(rows=False)
    a = args.base if isinstance(args, _lib.DaeBwdTfArgsF32) else args
    a.method, a.kernel = opts.method_id, KERNEL_ID[kernel]
    a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = x_dim, z_dim, v_dim, i_dim, 2, 1
    dev = de_layers[0][0].device
    a.de, a.ae = _mlp(de_layers, dev, "de", []), _mlp(ae_layers, dev, "ae", [])
    if call_generic(_lib.load(), "dae_backward", "supported", args, opts)[0]:      # K9 / K8 (latent shapes) or K5
        return True
    if opts.family != "plain" or kernel == "generic":
        return False
    return dae_backward_wide_supported(method, de_layers, ae_layers, x_dim, z_dim, v_dim, i_dim)      # K7f: the DAE_01 class at hidden <= 128


def dae_backward_wide_supported(method: str, de_layers: Layers, ae_layers: Layers, x_dim, z_dim, v_dim, i_dim, substeps: int = 1,
                                externals: str = "hold") -> bool:
    """Shapes of K7f (psnode_dae_backward_wide_f32): DE 3n -> h -> h -> h -> x and AE n+x+z+v -> h -> h -> h -> i with h <= 128,
    x <= 8, z+v+i <= 8."""
    method_id = GenericOpts.of(method, (None, None), substeps, externals).require_plain("dae_backward_wide_supported")[0]
    if de_layers[0][0].device.type != "cuda" or len(de_layers) != 4 or len(ae_layers) != 4:
        return False
    lib = _lib.load()
    a = _lib.DaeBwdWideArgsF32()
    a.method, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = method_id, x_dim, z_dim, v_dim, i_dim, 2, 1
    dev = de_layers[0][0].device
    a.de, a.ae = _mlp(de_layers, dev, "de", []), _mlp(ae_layers, dev, "ae", [])
    return bool(lib.psnode_dae_backward_wide_supported(ctypes.byref(a)))


def _bind_dae_inputs(a, all_initial, xs, is_, grad_xs, grad_is, dev, keep):
    """The inputs every DAE backward struct carries under these names, as contiguous fp32 device tensors: all_initial, xs, is, grad_xs (None:
    zeros) and grad_is (None goes to the kernels as NULL).  Returns them; `keep` holds them until the call has returned."""
    a0 = _f32_dev(all_initial, dev, "all_initial").contiguous()
    xs_c, is_c = _f32_dev(xs, dev, "xs").contiguous(), _f32_dev(is_, dev, "is").contiguous()
    gx_c = _f32_dev(grad_xs, dev, "grad_xs").contiguous() if grad_xs is not None else torch.zeros_like(xs_c)
    gi_c = _f32_dev(grad_is, dev, "grad_is").contiguous() if grad_is is not None else None
    keep += [a0, xs_c, is_c, gx_c, gi_c]
    a.all_initial, a.xs, a.is_, a.grad_xs = a0.data_ptr(), xs_c.data_ptr(), is_c.data_ptr(), gx_c.data_ptr()
    a.grad_is = gi_c.data_ptr() if gi_c is not None else None
    return a0, xs_c, is_c, gx_c, gi_c


def _bind_true_rows(a, x_true, i_true, dev, keep):
    """The dataset rows of a teacher-forced call (either may be None) as contiguous fp32 device tensors, with the struct's flags and pointers."""
    xt_c = _f32_dev(x_true, dev, "x_true").contiguous() if x_true is not None else None
    it_c = _f32_dev(i_true, dev, "i_true").contiguous() if i_true is not None else None
    keep += [xt_c, it_c]
    a.flags = (_lib.FLAG_INPUT_TRUE_X if xt_c is not None else 0) | (_lib.FLAG_INPUT_TRUE_I if it_c is not None else 0)
    a.x_true = xt_c.data_ptr() if xt_c is not None else None
    a.i_true = it_c.data_ptr() if it_c is not None else None
    return xt_c, it_c


def dae_backward_wide(method: str, de_layers: Layers, ae_layers: Layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx=None,
                      z_jump=None, v_jump=None, saved=None, x_true=None, i_true=None, substeps: int = 1, externals: str = "hold"):
    """Backward of `dae_integrate` at hidden <= 128 (the DAE_01 shape class): K7f (psnode_dae_backward_wide_f32) -- ONE launch over the
    whole grid that sweeps the adjoint through the DE stages, the AE head per grid point and the event-time recomputes and forms the DE's
    parameter gradients and the DE's share of the input gradients in the kernel.  With saved activations at hidden <= 64 the head's
    gradients are formed in the kernel too; otherwise its rows (one set per grid point) are contracted by K7h (`_wide_head_k7h`).
    saved = what `dae_integrate(save=True)` returned for the same call: the kernel evaluates nothing forwards.  x_true / i_true [T,B,.]:
    backward of a teacher-forced call (input_true_x / input_true_i, my_solvers.py:111-121) -- the dataset rows the forward call fed the
    DE / the heads; recompute form only.  A call whose head rows (6 x [T,B,H] + [T,B,40]) would not fit half of the free HBM is run over
    BATCH slices (trajectories are independent: parameter gradients add, per-trajectory gradients concatenate).
    Same return value as `dae_backward`."""
    method_id, S = GenericOpts.of(method, (None, None), substeps, externals).require_plain("dae_backward_wide")
    lib = _lib.load()
    dev = xs.device
    T, B, _ = xs.shape
    H = _padded_hidden(de_layers[0][0].shape[0])        # the width the kernel runs the MLPs at (zero-padded rows)
    if saved is None and B > 16:
        # the recompute form stores the AE head's rows of EVERY grid point (6 x [T,B,H] + [T,B,16] + the u rows of K7h): a very long grid on
        # a full card goes through in batch slices (a saved-activation call is not sliced: its forward already held ~S times as much)
        free, _ = torch.cuda.mem_get_info(dev)
        need = (6 * H + 40) * 4 * T * B
        if need > free // 2:
            nsl = min((B + 15) // 16, int(-(-need // max(free // 2, 1))))
            step = -(-((B + nsl - 1) // nsl) // 16) * 16
            return _dae_backward_wide_sliced(step, method, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is,
                                             event_idx, z_jump, v_jump, x_true, i_true)
    c = _wide_marshal(lib, method_id, S, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump,
                      saved, x_true, i_true)
    with torch.cuda.device(dev):
        nbytes = lib.psnode_dae_backward_wide_workspace_bytes(ctypes.byref(c.a))
        ws, wp, wn = _workspace_of(nbytes, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.psnode_dae_backward_wide_f32(ctypes.byref(c.a), wp, wn, st), "psnode_dae_backward_wide_f32")
        if c.gae_raw is not None:      # one launch did everything (the kernel added the AE's share to grad all_initial, too)
            g_ae, ga0 = _wide_head_in_kernel(c), c.ga0_de
        else:
            g_ae, Sa1 = _wide_head_k7h(lib, c, z, v, event_idx)
            ga0 = c.ga0_de + Sa1 @ _pad_rows(c.A[0][:, 0:c.n], H)
    zd, vd, n_ev = c.zd, c.vd, c.n_ev
    g = {"z_jump": None, "v_jump": None}
    g["x_init"] = c.carry_x + c.gx_c[0]
    g["all_initial"] = ga0
    g["z"] = c.gzv[..., :zd].contiguous() if zd > 0 else None
    g["v"] = c.gzv[..., zd:].contiguous() if vd > 0 else None
    if n_ev:
        g["z_jump"] = c.gjump[..., :zd].contiguous() if zd > 0 else None
        g["v_jump"] = c.gjump[..., zd:].contiguous() if vd > 0 else None
    g["de"] = _split_grads(c.gp_de, de_layers)
    g["ae"] = g_ae
    return g


def _wide_marshal(lib, method_id, S, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump, saved,
                  x_true, i_true):
    """The args struct of one K7f launch (`a`) and every tensor it points to or that the routes behind the launch read, as one namespace."""
    dev = xs.device
    T, B, xd = xs.shape
    zd, vd, idim = z.shape[-1], v.shape[-1], is_.shape[-1]
    nzv, ne = zd + vd, zd + vd + idim
    n = xd + ne
    Hr = de_layers[0][0].shape[0]                       # the MLPs' width; H = the width the kernel runs them at (zero-padded rows)
    H = _padded_hidden(Hr)
    f32 = dict(dtype=torch.float32, device=dev)
    keep: list = []
    a = _lib.DaeBwdWideArgsF32()
    a.method, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = method_id, xd, zd, vd, idim, T, B
    a.de, a.ae = _mlp(de_layers, dev, "de", keep), _mlp(ae_layers, dev, "ae", keep)
    a.t, a.z, a.v = _view(t, dev, "t", keep), _view(z, dev, "z", keep), _view(v, dev, "v", keep)
    a0, xs_c, _, gx_c, _ = _bind_dae_inputs(a, all_initial, xs, is_, grad_xs, grad_is, dev, keep)
    # (grad_is = None goes to the kernels as NULL: they read the rows of `is` instead and mask them out, branch-free.  Round 3 passed an
    #  explicit zero tensor here because NULL gave wrong AE gradients on one register class; round 4 found the cause -- a uniform
    #  `if (grad_is)` branch scheduled between an MFMA and the consumer of its result, psnode_dae_backward_wide.hip:add_gis -- and removed
    #  the branch, so the C ABI's documented NULL is safe for every caller)
    n_ev = 0
    ev_rows = ev_gi = None
    _bind_jumps(a, event_idx, (("z_jump", z_jump), ("v_jump", v_jump)), dev, keep)
    if event_idx is not None:
        n_ev = (z_jump if z_jump is not None else v_jump).shape[1]
        a.n_events = n_ev
        # rows of the event-time heads: zero-initialised, so that events no step takes contribute nothing
        ev_rows = [torch.zeros((n_ev, B, H), **f32) for _ in range(6)]
        ev_gi, ev_i = torch.zeros((n_ev, B, 16), **f32), torch.zeros((n_ev, B, 16), **f32)
        for q in range(3):
            a.ev_act[q], a.ev_delta[q] = ev_rows[q].data_ptr(), ev_rows[3 + q].data_ptr()
        a.ev_gi, a.ev_i = ev_gi.data_ptr(), ev_i.data_ptr()
        keep.append(ev_i)
    # The host-side accumulators of the AE head's K7h route are made on demand (`_wide_head_k7h`).  The one-launch route at hidden <= 64
    # (every gradient formed in the kernel) needs none of them -- 18 fills, a [T,B,z+v] copy and 2 small GEMM operands per call that the
    # step's profile showed as glue (profiles/r04o_glue_dae01.txt).
    gzv = torch.zeros((T, B, nzv), **f32)                       # dL/d(z|v) of the un-jumped inputs
    gjump = torch.zeros((B, n_ev, nzv), **f32) if n_ev else None
    carry_x = torch.zeros((B, xd), **f32)
    a.carry_x = carry_x.data_ptr()
    xt_c = None
    if x_true is not None or i_true is not None:
        if saved is not None:
            raise ValueError("teacher forcing: the recompute form only (a teacher-forced forward saves nothing)")
        xt_c, it_c = _bind_true_rows(a, x_true, i_true, dev, keep)
        if (xt_c is not None and tuple(xt_c.shape) != (T, B, xd)) or (it_c is not None and tuple(it_c.shape) != (T, B, idim)):
            raise ValueError("x_true / i_true must be [T,B,x_dim] / [T,B,i_dim]")
    gp_de = _empty(sum(w.numel() + w.shape[0] for w, _ in de_layers), **f32)
    ga0_de = _empty((B, n), **f32)
    a.grad_params_de, a.grad_all_initial_de = gp_de.data_ptr(), ga0_de.data_ptr()
    a.grad_zv = gzv.data_ptr()
    a.grad_jump = gjump.data_ptr() if gjump is not None else None
    jump_all = None
    if n_ev:
        parts = ([z_jump.detach()] if zd > 0 else []) + ([v_jump.detach()] if vd > 0 else [])
        jump_all = torch.cat(parts, -1)                         # [B, n_ev, nzv]
    if saved is not None:
        s_act, s_xst, s_ae, s_ev, s_evi = saved
        if s_ae.shape != (3, T, B, H) or s_act.shape != (T - 1, S, 3, B, H) or (n_ev and (s_ev is None or s_ev.shape != (n_ev, 3, B, H))):
            raise ValueError("saved activations do not belong to this call (shape)")
        keep += [s_act, s_xst, s_ae, s_ev, s_evi]
        a.saved_act, a.saved_xstage, a.saved_ae_act = s_act.data_ptr(), s_xst.data_ptr(), s_ae.data_ptr()
        if n_ev:
            a.saved_ev_act, a.saved_ev_i = s_ev.data_ptr(), s_evi.data_ptr()
            for q in range(3):
                ev_rows[q] = s_ev[:, q]
    # > 0 (hidden <= 64, saved activations): the AE head's gradients are formed in the kernel too -- no head rows, no K7h
    n_ae_raw = int(lib.psnode_dae_backward_wide_ae_floats(ctypes.byref(a)))
    arows = gae_raw = agi = None
    if n_ae_raw:
        gae_raw = _empty(n_ae_raw, **f32)
        a.grad_params_ae_raw = gae_raw.data_ptr()
    else:
        arows = ([s_ae[0], s_ae[1], s_ae[2]] if saved is not None else [_empty((T, B, H), **f32) for _ in range(3)])
        arows += [_empty((T, B, H), **f32) for _ in range(3)]
        agi = _empty((T, B, 16), **f32)
        for q in range(3):
            a.ae_act[q], a.ae_delta[q] = arows[q].data_ptr(), arows[3 + q].data_ptr()
        a.ae_gi = agi.data_ptr()
    return types.SimpleNamespace(a=a, keep=keep, dev=dev, f32=f32, T=T, B=B, xd=xd, zd=zd, vd=vd, nzv=nzv, ne=ne, n=n, Hr=Hr, H=H, n_ev=n_ev,
                                 A=[w.detach() for w, _ in ae_layers], a0=a0, xs_c=xs_c, gx_c=gx_c, xt_c=xt_c, ev_rows=ev_rows, ev_gi=ev_gi,
                                 gzv=gzv, gjump=gjump, carry_x=carry_x, gp_de=gp_de, ga0_de=ga0_de, jump_all=jump_all, arows=arows, agi=agi,
                                 gae_raw=gae_raw)


def _wide_head_in_kernel(c) -> list:
    """The AE's parameter gradients of a launch that formed them itself, from its raw block
    [dAW1 | db1 | dAW2 | db2 | dAW3 | db3 | P3 (16 slots x h) | sg (16 slots)]."""
    Hr, nzv, ne, raw = c.Hr, c.nzv, c.ne, c.gae_raw
    out, o = [], 0
    for cols in (c.n + c.xd + nzv, Hr, Hr):
        out.append(raw[o:o + Hr * cols].view(Hr, cols)); o += Hr * cols
        out.append(raw[o:o + Hr]); o += Hr
    P3 = raw[o:o + 16 * Hr].view(16, Hr); o += 16 * Hr
    sg = raw[o:o + 16]
    return out + [P3[nzv:ne] + P3[ne + nzv:2 * ne], sg[nzv:ne] + sg[ne + nzv:2 * ne]]


def _wide_head_k7h(lib, c, z, v, event_idx):
    """The AE head's rows of a K7f launch -> its parameter gradients and its share of the input gradients, contracted by K7h
    (psnode_dae_head_grads_f32) once over the grid points and once over the events taken.  Adds the share of z | v to c.gzv / c.gjump;
    returns ([dAW1, db1, ..., dAW4, db4], the sum over the heads of the AE's delta_1 [B, H])."""
    B, H, T, f32, dev = c.B, c.H, c.T, c.f32, c.dev
    xd, nzv, ne, n, Hr, a0 = c.xd, c.nzv, c.ne, c.n, c.Hr, c.a0
    A1 = c.A[0]
    gA = [torch.zeros_like(w) for w in c.A]
    gab = [torch.zeros(w.shape[0], **f32) for w in c.A]
    Sa1 = torch.zeros((B, H), **f32)
    zv_all = torch.cat((z.detach(), v.detach()), -1)    # [T, B, nzv] (one copy of the two input views)

    def head_grads(act, act_row_stride, delta, gi_slots, x_rows, zv_rows):
        """act = 3 device pointers' tensors whose row r lies r*act_row_stride floats behind the first; delta / gi_slots / x_rows / zv_rows
        [R, B, .] contiguous"""
        nonlocal Sa1
        R = delta[0].shape[0]
        u = torch.zeros((R, B, 16), **f32)
        u[..., :xd] = x_rows
        if nzv > 0:
            u[..., xd:xd + nzv] = zv_rows
        h = _lib.DaeHeadGradsArgsF32()
        h.R, h.B, h.hidden, h.n_zv = R, B, Hr, nzv
        for q in range(3):
            h.act[q], h.delta[q] = act[q].data_ptr(), delta[q].data_ptr()
        h.act_row_stride = act_row_stride
        h.gi, h.u = gi_slots.data_ptr(), u.data_ptr()
        A1c = A1.contiguous()
        h.aw1, h.aw1_cols, h.zv_col0 = A1c.data_ptr(), A1c.shape[1], n + xd
        gza = _empty((R, B, 8), **f32) if nzv > 0 else None
        sa1 = _empty((B, H), **f32)
        out = _empty(lib.psnode_dae_head_grads_out_floats(Hr), **f32)
        h.grad_zv = gza.data_ptr() if gza is not None else None
        h.sa1, h.out = sa1.data_ptr(), out.data_ptr()
        nb = lib.psnode_dae_head_grads_workspace_bytes(ctypes.byref(h))
        hws, hp_, hn_ = _workspace_of(nb, dev)
        _lib.check(lib.psnode_dae_head_grads_f32(ctypes.byref(h), hp_, hn_, torch.cuda.current_stream(dev).cuda_stream),
                   "psnode_dae_head_grads_f32")
        o = 0
        gA[1].add_(out[o:o + Hr * Hr].view(Hr, Hr)); o += Hr * Hr
        gA[2].add_(out[o:o + Hr * Hr].view(Hr, Hr)); o += Hr * Hr
        P3 = out[o:o + 16 * Hr].view(16, Hr); o += 16 * Hr
        gA[3].add_(P3[nzv:ne] + P3[ne + nzv:2 * ne])
        P0 = out[o:o + Hr * 16].view(Hr, 16); o += Hr * 16
        gA[0][:, n:n + xd + nzv].add_(P0[:, :xd + nzv])
        gA[0][:, :n].add_(sa1[:, :Hr].t() @ a0)
        for q in range(3):
            gab[q].add_(out[o:o + Hr]); o += Hr
        sg = out[o:o + 16]
        gab[3].add_(sg[nzv:ne] + sg[ne + nzv:2 * ne])
        Sa1 += sa1
        return gza[..., :nzv] if gza is not None else None

    # (the heads at the grid points read the dataset rows under input_true_x; the event heads below always the running state)
    gza = head_grads(c.arows[:3], B * H, c.arows[3:], c.agi, c.xt_c if c.xt_c is not None else c.xs_c, zv_all)
    if nzv > 0:
        c.gzv += gza
    c.arows = c.agi = None
    if c.n_ev:
        evl = event_idx.long()
        step_of = torch.zeros(c.n_ev, dtype=torch.long, device=dev).scatter_reduce_(
            0, evl.clamp_min(0), torch.arange(T - 1, device=dev) * (evl >= 0), "amax")
        ev_stride = c.ev_rows[0].stride(0)         # B*H (own buffers) or 3*B*H (layer q of the forward call's [nE,3,B,H])
        gza = head_grads(c.ev_rows[:3], ev_stride, c.ev_rows[3:], c.ev_gi, c.xs_c[step_of], c.jump_all.permute(1, 0, 2))
        if nzv > 0:
            c.gjump += gza.permute(1, 0, 2)
    return [q for pair in zip(gA, gab) for q in pair], Sa1


def _dae_backward_wide_sliced(step, method, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump,
                              x_true, i_true):
    """`dae_backward_wide` over batch slices of `step` trajectories: parameter gradients add, per-trajectory gradients concatenate."""
    B = xs.shape[1]
    tb = lambda q, b0, b1: None if q is None else q[:, b0:b1]          # [T, B, .] views
    bb = lambda q, b0, b1: None if q is None else q[b0:b1]             # [B, ...] tensors
    out = None
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        g = dae_backward_wide(method, de_layers, ae_layers, tb(t, b0, b1), tb(z, b0, b1), tb(v, b0, b1), bb(all_initial, b0, b1),
                              tb(xs, b0, b1), tb(is_, b0, b1), tb(grad_xs, b0, b1), tb(grad_is, b0, b1), event_idx=event_idx,
                              z_jump=bb(z_jump, b0, b1), v_jump=bb(v_jump, b0, b1), x_true=tb(x_true, b0, b1), i_true=tb(i_true, b0, b1))
        if out is None:
            out = {k: ([q.clone() for q in val] if k in ("de", "ae") else ([val] if val is not None else None)) for k, val in g.items()}
        else:
            for k, val in g.items():
                if k in ("de", "ae"):
                    for acc, q in zip(out[k], val):
                        acc.add_(q)
                elif val is not None:
                    out[k].append(val)
    cat_dim = {"x_init": 0, "all_initial": 0, "z": 1, "v": 1, "z_jump": 0, "v_jump": 0}
    return {k: (val if k in ("de", "ae") else (torch.cat(val, cat_dim[k]) if val is not None else None)) for k, val in out.items()}


def dae_backward(method, de_layers: Layers, ae_layers: Layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx=None,
                 z_jump=None, v_jump=None, kernel: str = "auto", saved=None, act=None, substeps: int = 1, x_sub=None, externals: str = "hold",
                 per_trajectory: bool = False, segment=None, x_true=None, segment_parallel=None, algebraic: str = "step"):
    """algebraic="stage": backward of `dae_integrate(..., algebraic="stage")` -- K5's stage-heads builds only, under the interpolant's rules:
    the i part of the DE's VJP of a stage s >= 1 goes through the head's VJP at that stage's argument and externals.
    Backward pass of `dae_integrate` (no teacher forcing): the one-launch K7f (`dae_backward_wide`) for the DAE_01 shape class at
    hidden <= 128, K9 / K8 / K9w for the latent shapes of the direct_encode models, else the generic backward kernel (K5);
    `kernel` = "auto" | "mfma" | "generic" | "wide" (K7f or an error).
    saved = what `dae_integrate(save=True)` returned (read by K7f, K9 and K9w; K8 / K5 recompute and refuse them).
    act: None (both MLPs ELU(1)) or (de_act, ae_act); an activation other than ELU(1) runs on K5 only (kernel "auto" / "generic").
    method: "euler" | "midpoint" | "rk4", or a fused.Tableau -- K5 only (kernel "auto" / "generic", no saved rows).
    substeps > 1: backward of `dae_integrate(..., substeps=, save_sub=True)` with the x_sub it returned -- K5 only, the same rules.
    externals="linear": backward of `dae_integrate(..., externals="linear")` -- K5's linear-externals build only, the same rules.
    externals="lagrange": backward of `dae_integrate(..., externals="lagrange")` -- K5's Lagrange build only, the same rules.
    per_trajectory=True: backward of `dae_integrate(..., per_trajectory=True)`; `event_idx` is the int32 [T-1, B] table -- K5's
    per-trajectory build only, the same rules (x_sub where substeps > 1).  Without an event table the flag means nothing.
    segment (an int w >= 1): backward of `dae_integrate(..., segment=w)` -- K5's multiple-shooting build only, the same rules; x_true
    [T, B, xd] is the dataset x of the forward call (needed where T - 1 > w; no gradient).  A restart step's start adjoint and the x part of
    its head's VJP are dropped; that head's z | v part goes to row k of grad z / v, or to the event's jump row.
    segment_parallel (None, "auto" or an int g >= 1; needs segment): as `ode_backward` -- x_init, z, v and the jump gradients bit for bit
    those of the call without it, both MLPs' gradients and all_initial the same sums in another order.
    Returns dict(x_init, z, v, z_jump, v_jump, all_initial, de=[...], ae=[...]) of gradients."""
    T, B, xd = xs.shape
    zd, vd, idim = z.shape[-1], v.shape[-1], is_.shape[-1]
    opts = GenericOpts.of(method, dae_acts(act), substeps, externals, bool(per_trajectory) and event_idx is not None, segment,
                          resolve_segment_parallel(segment_parallel, segment, T, B, xs.device), algebraic)
    opts.require_generic("dae_backward", kernel, saved is not None)
    if opts.family != "plain":      # K5 alone (an activation other than ELU(1) asks for it by name, as it always did)
        return _dae_backward_entry(opts, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump,
                                   "generic" if any(q is not None for q in opts.acts) else kernel, None, x_sub=x_sub,
                                   ms_x_true=_ms_rows("dae_backward", segment, x_true, T, B, xd, xs.device))
    if kernel in ("wide", "mfma") and T < 2 and len(de_layers) == 4:
        kernel = "generic"       # no step to sweep: K7f has no head-only form, K5 handles the single grid point
    if saved is not None and latent_wide_shape(de_layers, ae_layers, xd, zd, vd, idim):
        return latent_backward_wide(method, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx=event_idx,
                                    z_jump=z_jump, v_jump=v_jump, saved=saved)
    if kernel == "wide" or (kernel in ("auto", "mfma") and len(de_layers) == 4 and T >= 2
                            and dae_backward_wide_supported(method, de_layers, ae_layers, xd, zd, vd, idim)):
        return dae_backward_wide(method, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx=event_idx,
                                 z_jump=z_jump, v_jump=v_jump, saved=saved)
    return _dae_backward_entry(opts, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump,
                               kernel, saved)


def dae_backward_tf(method, de_layers: Layers, ae_layers: Layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx=None,
                    z_jump=None, v_jump=None, kernel: str = "auto", x_true=None, i_true=None, substeps: int = 1, x_sub=None,
                    externals: str = "hold", per_trajectory: bool = False, algebraic: str = "step"):
    """algebraic="stage": with x_true alone (with i_true every stage read i_true[k]: the "step" call).
    Backward of a teacher-forced `dae_integrate` (input_true_x / input_true_i, my_solvers.py:111-121) on the generic backward K5
    (psnode_dae_backward_tf_f32): every shape K5 takes untied.  x_true [T,B,x_dim] / i_true [T,B,i_dim]: the dataset rows the forward call
    fed the DE / the heads (None = that flag was not set; both None = `dae_backward` on K5's entry point); they get no gradient.  xs / is_:
    the forward results (an event step's recomputed head reads the running state xs[k]).  kernel: "auto" | "generic".  substeps > 1: with the
    x_sub of the forward call (`dae_integrate(..., substeps=, save_sub=True)`).  per_trajectory=True: `event_idx` is the int32 [T-1, B]
    table of the forward call (K5's per-trajectory build).
    Same return value as `dae_backward`."""
    if kernel not in ("auto", "generic"):
        raise _lib.UnsupportedShapeError("dae_backward_tf: the teacher-forced backward behind this entry point is K5's (kernel 'auto' / 'generic'); "
                                         "K7f's is dae_backward_wide")
    T, B, xd = xs.shape
    for name, q, w in (("x_true", x_true, xd), ("i_true", i_true, is_.shape[-1])):
        if q is not None and tuple(q.shape) != (T, B, w):
            raise ValueError(f"{name} must be [T,B,{w}], got {tuple(q.shape)}")
    opts = GenericOpts.of(method, (None, None), substeps, externals, bool(per_trajectory) and event_idx is not None, None, None, algebraic)
    if i_true is not None and algebraic == "stage":      # (validated above)
        opts = GenericOpts.of(method, (None, None), substeps, externals, bool(per_trajectory) and event_idx is not None)
    opts.require_generic("dae_backward_tf", kernel, False)
    opts.no_teacher_forcing("dae_backward_tf", x_true is not None or i_true is not None)
    return _dae_backward_entry(opts, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs,
                               grad_is, event_idx, z_jump, v_jump, kernel, None, x_true=x_true, i_true=i_true, x_sub=x_sub)


def _dae_backward_entry(opts, de_layers, ae_layers, t, z, v, all_initial, xs, is_, grad_xs, grad_is, event_idx, z_jump, v_jump, kernel, saved,
                        x_true=None, i_true=None, x_sub=None, ms_x_true=None):
    """The DAE backward on whichever entry point `opts` and the dataset rows select (`call_generic`): one marshalling for all of them."""
    lib = _lib.load()
    dev = xs.device
    T, B, xd = xs.shape
    zd, vd, idim = z.shape[-1], v.shape[-1], is_.shape[-1]
    _check_x_sub("dae_backward", opts.substeps, x_sub, T, B, xd, dev)
    if opts.per_trajectory:
        check_event_idx(event_idx, T, B, True, dev)
    keep: list = [x_sub, ms_x_true]
    args = opts.dae_backward_args(x_true is not None or i_true is not None)
    tf = args if isinstance(args, _lib.DaeBwdTfArgsF32) else None
    if tf is not None:
        _bind_true_rows(tf, x_true, i_true, dev, keep)
    a = tf.base if tf is not None else args      # (tf.base: a view of the struct's own memory)
    a.method = opts.method_id
    a.kernel = KERNEL_ID[kernel]
    a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = xd, zd, vd, idim, T, B
    a.de, a.ae = _mlp(de_layers, dev, "de", keep), _mlp(ae_layers, dev, "ae", keep)
    z, v, z_jump, v_jump = _aligned16(z), _aligned16(v), _aligned16(z_jump), _aligned16(v_jump)
    a.t, a.z, a.v = _view(t, dev, "t", keep), _view(z, dev, "z", keep), _view(v, dev, "v", keep)
    _bind_dae_inputs(a, all_initial, xs, is_, grad_xs, grad_is, dev, keep)
    g = {"z_jump": None, "v_jump": None}
    _bind_jumps(a, event_idx, (("z_jump", z_jump), ("v_jump", v_jump)), dev, keep)
    if event_idx is not None:
        n_ev = (z_jump if z_jump is not None else v_jump).shape[1]
        a.n_events = n_ev
        if zd > 0:
            g["z_jump"] = torch.zeros((B, n_ev, zd), dtype=torch.float32, device=dev)
            a.grad_z_jump = g["z_jump"].data_ptr()
        if vd > 0:
            g["v_jump"] = torch.zeros((B, n_ev, vd), dtype=torch.float32, device=dev)
            a.grad_v_jump = g["v_jump"].data_ptr()
    with torch.cuda.device(dev):
        g["x_init"] = _empty((B, xd), dtype=torch.float32, device=dev)
        g["all_initial"] = _empty((B, xd + zd + vd + idim), dtype=torch.float32, device=dev)
        g["z"] = _empty((T, B, zd), dtype=torch.float32, device=dev) if zd > 0 else None
        g["v"] = _empty((T, B, vd), dtype=torch.float32, device=dev) if vd > 0 else None
        npd = sum(w.numel() + b.numel() for w, b in de_layers)
        npa = sum(w.numel() + b.numel() for w, b in ae_layers)
        gde = _empty(npd, dtype=torch.float32, device=dev)
        gae = _empty(npa, dtype=torch.float32, device=dev)
        a.grad_x_init, a.grad_all_initial = g["x_init"].data_ptr(), g["all_initial"].data_ptr()
        a.grad_z = g["z"].data_ptr() if g["z"] is not None else None
        a.grad_v = g["v"].data_ptr() if g["v"] is not None else None
        a.grad_params_de, a.grad_params_ae = gde.data_ptr(), gae.data_ptr()
        if saved is not None and T >= 2:        # (K9 reads them; the C side refuses them for the kernels that recompute)
            s_act, s_xst, s_ae, s_ev, s_evi = saved
            L = len(de_layers) - 1
            _check_saved(s_act, s_xst, T, B, xd, opts.stages, L, dev)
            if tuple(s_ae.shape[:3]) != (L, T, B) or s_ae.shape[-1] != s_act.shape[-1] or not s_ae.is_contiguous() or s_ae.device != dev:
                raise ValueError("saved AE activations do not belong to this call (shape / device)")
            keep += [s_act, s_xst, s_ae, s_ev, s_evi]
            a.saved_act, a.saved_xstage, a.saved_ae_act = s_act.data_ptr(), s_xst.data_ptr(), s_ae.data_ptr()
            if event_idx is not None:
                n_ev_ = (z_jump if z_jump is not None else v_jump).shape[1]
                if s_ev is None or s_evi is None or s_ev.shape[0] != n_ev_ or s_ev.shape[2] != B or s_evi.shape[:2] != (n_ev_, B):
                    raise ValueError("saved event activations do not belong to this call (shape)")
                a.saved_ev_act, a.saved_ev_i = s_ev.data_ptr(), s_evi.data_ptr()
        nbytes = call_generic(lib, "dae_backward", "workspace_bytes", args, opts, x_sub=x_sub, x_true=ms_x_true)[0]
        ws, wp, wn = _workspace_of(nbytes, dev)
        stencil = lagrange_stencils(t.detach(), event_idx) if opts.takes.stencil and is_lagrange(opts.externals) else None      # (externals="lagrange": the forward's table again)
        rc, entry = call_generic(lib, "dae_backward", "f32", args, opts, wp, wn, torch.cuda.current_stream(dev).cuda_stream, x_sub=x_sub, x_true=ms_x_true,
                                 stencil=stencil)
    _lib.check(rc, entry)
    g["de"], g["ae"] = _split_grads(gde, de_layers), _split_grads(gae, ae_layers)
    return g
