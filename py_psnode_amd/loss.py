"""Fused masked loss (kernel K6, psnode_masked_mse_f32 / psnode_masked_loss_f32): the step right after the integrator in the
scripts' training loops, as one pass over (prediction, target, mask) that returns the loss AND d loss / d prediction.

Reference expressions (Loss_func = nn.functional.mse_loss, neural_00_ODE_01_no_encode.py:49) -- the four scripts differ:
  ODE_01  x_loss = sum(sum(Loss_func(x_pred, x, reduction='none') * mask, dim=1), dim=0) / sum(mask);  loss = sum(x_loss)
          (neural_00_ODE_01_no_encode.py:353-355; the x0_loss of :353 is computed but NOT added)              -> ode01_loss
  ODE_02  loss = Loss_func(x[:,0,:], x_pred[:,0,:]) + sum(x_loss) + Loss_func(x_re, x)
          (neural_00_ODE_02_direct_encode.py:267-270)                                                         -> ode02_loss
  DAE_01  x_loss = (sum(se*mask) + 9*sum(se[:,:,1:2]*mask)) / sum(mask);  i_loss = sum(se_i*mask)/sum(mask)
          loss = x_loss + i_loss + Loss_func(x[:,0,:], x_pred[:,0,:]) + Loss_func(i[:,0,:], i_pred[:,0,:])
          (neural_01_DAE_01_no_encode.py:414-419)                                                             -> dae01_loss
  DAE_02  as DAE_01 WITHOUT the 9x extra weight on x column 1 (commented out upstream), plus the reconstruction terms
          Loss_func(x_re, x) + Loss_func(i_re, i)   (neural_01_DAE_02_direct_encode.py:359-365)                -> dae02_loss
Tensors are in the scripts' [B,T,D] shape with any strides: the integrator's `xs.permute(1,0,2)` and the DataLoader's
B-major batches go in as they are.  There is no non-HIP implementation here.

`Loss_func` is a knob of the scripts (line 49 of each: "mse is not recommended ..."): every objective below takes `loss_func=` --
F.mse_loss (the default), F.l1_loss, F.smooth_l1_loss, F.huber_loss, a functools.partial of one carrying beta= / delta=, the
matching nn module, or a name -- see loss_kind_of.  The evaluation loop's per-sample table
`torch.sum(Loss_func(x_pred * mask, x * mask, reduction='none'), dim=1)` (neural_00_ODE_01_no_encode.py:123) is per_sample_loss."""
import ctypes
import functools
import math
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .fused import _empty, _workspace_of


def _view_bt(t: torch.Tensor, dev, name: str, keep: list) -> _lib.ViewF32:
    """[B,T,D] tensor -> time-major view struct (stride_t, stride_b); copies only if the last dim is strided."""
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: fp32 only, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{name}: on {t.device}, expected {dev}")
    t = t.detach()
    if t.shape[-1] > 1 and t.stride(2) != 1:
        t = t.contiguous()
    keep.append(t)
    return _lib.ViewF32(t.data_ptr(), t.stride(1), t.stride(0))


_COL_WEIGHTS = {}


def _loss_args(pred, target, mask, col_weight, inv_norm, scale, t0_coef, what):
    """The checks of a raw kernel call and its psnode_loss_args_f32 (out / grad_pred left to the caller); `keep` holds what it points to."""
    if pred.dim() != 3 or pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must be equal [B,T,D] shapes")
    dev = pred.device
    if dev.type != "cuda":
        raise ValueError(f"{what}: tensors must be on a HIP device (no CPU path)")
    B, T, D = pred.shape
    keep = []
    a = _lib.LossArgsF32()
    a.T, a.B, a.D = T, B, D
    a.pred, a.target = _view_bt(pred, dev, "pred", keep), _view_bt(target, dev, "target", keep)
    if mask is not None:
        if mask.dim() != 3 or mask.shape[:2] != pred.shape[:2] or mask.shape[2] not in (1, D):
            raise ValueError(f"mask {tuple(mask.shape)} must be [B,T,1] or [B,T,D]")
        a.mask_width = mask.shape[2]
        a.mask = _view_bt(mask, dev, "mask", keep)
    if col_weight is not None:
        if isinstance(col_weight, torch.Tensor):
            cw = col_weight.to(device=dev, dtype=torch.float32).contiguous()
        else:       # a python sequence (the DAE scripts' [1, 10, 1, ...]): uploaded once per (values, device) -- a pageable H2D copy
            key = (tuple(float(c) for c in col_weight), str(dev))   # per call is a device synchronisation in the middle of the step
            cw = _COL_WEIGHTS.get(key)
            if cw is None:
                cw = _COL_WEIGHTS[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
        if cw.numel() != D:
            raise ValueError(f"col_weight has {cw.numel()} entries, expected {D}")
        keep.append(cw)
        a.col_weight = cw.data_ptr()
    if inv_norm is not None:
        if inv_norm.numel() != 1 or inv_norm.dtype != torch.float32 or inv_norm.device != dev:
            raise ValueError("inv_norm must be a one-element fp32 tensor on the same device")
        keep.append(inv_norm)
        a.inv_norm = inv_norm.data_ptr()
    a.scale, a.t0_coef = float(scale), float(t0_coef)
    return a, keep, dev


def _terms_call(kind, pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad):
    """The training form: kind None = psnode_masked_mse_f32, a LossKind = psnode_masked_loss_f32 (same args, same workspace)."""
    lib = _lib.load()
    a, keep, dev = _loss_args(pred, target, mask, col_weight, inv_norm, scale, t0_coef, "masked_mse" if kind is None else "masked_loss")
    B, T, D = pred.shape
    out = _empty(D + 2, dtype=torch.float32, device=dev)
    grad = _empty((T, B, D), dtype=torch.float32, device=dev) if want_grad else None
    a.out = out.data_ptr()
    a.grad_pred = grad.data_ptr() if want_grad else None
    nbytes = lib.psnode_masked_mse_workspace_bytes(ctypes.byref(a))
    ws, p, _ = _workspace_of(nbytes, dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if kind is None:
            _lib.check(lib.psnode_masked_mse_f32(ctypes.byref(a), ctypes.c_void_p(p), ctypes.c_size_t(nbytes), ctypes.c_void_p(st)),
                       "psnode_masked_mse_f32")
        else:
            fn = _lib.LossFnF32(kind.kind, kind.param)
            _lib.check(lib.psnode_masked_loss_f32(ctypes.byref(a), ctypes.byref(fn), ctypes.c_void_p(p), ctypes.c_size_t(nbytes),
                                                  ctypes.c_void_p(st)), "psnode_masked_loss_f32")
    return out, grad


def masked_mse_terms(pred, target, mask=None, col_weight=None, inv_norm: Optional[torch.Tensor] = None, scale: float = 1.0,
                     t0_coef: float = 0.0, want_grad: bool = False):
    """Raw kernel call.  pred/target [B,T,D]; mask None | [B,T,1] | [B,T,D]; col_weight None | [D] tensor;
    inv_norm None | 0-dim/1-element DEVICE tensor.  Returns (out[D+2], grad_tm) with out = per-column masked terms,
    the t=0 term, the total; grad_tm = d total / d pred as a contiguous TIME-MAJOR [T,B,D] tensor (or None)."""
    return _terms_call(None, pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad)


class _MaskedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, col_weight, inv_norm, scale, t0_coef):
        out, grad = masked_mse_terms(pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad=pred.requires_grad)
        ctx.grad_tm = grad
        ctx.mark_non_differentiable(out)
        return out[pred.shape[2] + 1].clone(), out

    @staticmethod
    def backward(ctx, go, _go_terms):
        g = ctx.grad_tm.permute(1, 0, 2) * go      # [B,T,D] view of the time-major buffer: what PermuteBackward wants
        return g, None, None, None, None, None, None


def masked_mse(pred, target, mask=None, col_weight: Optional[Sequence[float]] = None, inv_norm: Optional[torch.Tensor] = None,
               scale: float = 1.0, t0_coef: float = 0.0):
    """Differentiable (w.r.t. pred) fused loss.  Returns (total, terms) where terms = [per-column..., t0 term, total]."""
    return _MaskedMSE.apply(pred, target, mask, col_weight, inv_norm, scale, t0_coef)


class LossKind(NamedTuple):
    """A pointwise loss of K6: kind = _lib.LOSS_*, param = beta (smooth_l1) / delta (huber), 0 where the kind has none."""
    kind: int
    param: float

    @property
    def name(self):
        return _KIND_NAMES[self.kind]


_KIND_NAMES = ("mse", "l1", "smooth_l1", "huber")
_KIND_OF_NAME = {n: k for k, n in enumerate(_KIND_NAMES)}
_KIND_OF_FUNC = {torch.nn.functional.mse_loss: 0, torch.nn.functional.l1_loss: 1, torch.nn.functional.smooth_l1_loss: 2,
                 torch.nn.functional.huber_loss: 3}
_KIND_OF_MODULE = ((torch.nn.MSELoss, 0), (torch.nn.L1Loss, 1), (torch.nn.SmoothL1Loss, 2), (torch.nn.HuberLoss, 3))
_PARAM_NAME = {2: "beta", 3: "delta"}
_ACCEPTED = ("None (= mse); 'mse' | 'l1' | 'smooth_l1' | 'huber' or a (name, beta / delta) pair; torch.nn.functional.mse_loss / l1_loss / "
             "smooth_l1_loss / huber_loss or a functools.partial of one that binds only beta= / delta=; an nn.MSELoss / L1Loss / "
             "SmoothL1Loss / HuberLoss instance; a LossKind")


def _kind(kind: int, param=None) -> LossKind:
    """torch's rules: beta, delta default to 1; smooth_l1 with beta == 0 IS l1; beta < 0 and delta <= 0 are errors."""
    if kind not in _PARAM_NAME:
        if param is not None:
            raise ValueError(f"{_KIND_NAMES[kind]} takes no parameter, got {param!r}")
        return LossKind(kind, 0.0)
    p = 1.0 if param is None else float(param)
    if not math.isfinite(p) or p < 0.0 or (p == 0.0 and kind == _lib.LOSS_HUBER):
        raise ValueError(f"{_KIND_NAMES[kind]}: {_PARAM_NAME[kind]} must be finite and {'>= 0' if kind == _lib.LOSS_SMOOTH_L1 else '> 0'}, got {p}")
    return LossKind(_lib.LOSS_L1, 0.0) if p == 0.0 else LossKind(kind, p)


def loss_kind_of(loss_func) -> LossKind:
    """What the scripts' `Loss_func` line says, as the (kind, param) K6 runs.  Anything it cannot name is a TypeError: there is no
    torch fallback."""
    if loss_func is None:
        return LossKind(_lib.LOSS_MSE, 0.0)
    if isinstance(loss_func, LossKind):
        return _kind(loss_func.kind, loss_func.param if loss_func.kind in _PARAM_NAME else None)
    if isinstance(loss_func, str):
        if loss_func not in _KIND_OF_NAME:
            raise ValueError(f"unknown loss {loss_func!r}; accepted: {_ACCEPTED}")
        return _kind(_KIND_OF_NAME[loss_func])
    if isinstance(loss_func, (tuple, list)):
        if len(loss_func) != 2 or not isinstance(loss_func[0], str):
            raise TypeError(f"a loss pair is (name, parameter), got {loss_func!r}; accepted: {_ACCEPTED}")
        if loss_func[0] not in _KIND_OF_NAME:
            raise ValueError(f"unknown loss {loss_func[0]!r}; accepted: {_ACCEPTED}")
        return _kind(_KIND_OF_NAME[loss_func[0]], loss_func[1])
    if isinstance(loss_func, functools.partial):
        kind = _KIND_OF_FUNC.get(loss_func.func)
        if kind is None:
            raise TypeError(f"partial of {loss_func.func!r} is not a loss K6 runs; accepted: {_ACCEPTED}")
        extra = sorted(set(loss_func.keywords) - {_PARAM_NAME.get(kind)})
        if loss_func.args or extra:     # reduction=, weight-like positionals: the scripts' expressions fix the reduction themselves
            raise ValueError(f"a partial of {_KIND_NAMES[kind]}_loss may bind only {_PARAM_NAME.get(kind, 'nothing')}=, got "
                             f"{len(loss_func.args)} positional and {extra}")
        return _kind(kind, loss_func.keywords.get(_PARAM_NAME.get(kind)))
    if isinstance(loss_func, torch.nn.Module):
        for cls, kind in _KIND_OF_MODULE:
            if type(loss_func) is cls:
                return _kind(kind, getattr(loss_func, _PARAM_NAME[kind]) if kind in _PARAM_NAME else None)
        raise TypeError(f"{type(loss_func).__name__} is not a loss K6 runs; accepted: {_ACCEPTED}")
    try:
        kind = _KIND_OF_FUNC.get(loss_func)
    except TypeError:       # unhashable
        kind = None
    if kind is None:
        raise TypeError(f"{loss_func!r} is not a loss K6 runs; accepted: {_ACCEPTED}")
    return _kind(kind)


def masked_loss_terms(pred, target, mask=None, loss_func=None, col_weight=None, inv_norm: Optional[torch.Tensor] = None,
                      scale: float = 1.0, t0_coef: float = 0.0, want_grad: bool = False):
    """masked_mse_terms with the pointwise loss `loss_func` (loss_kind_of) in place of the square."""
    kind = loss_kind_of(loss_func)
    if kind.kind == _lib.LOSS_MSE:
        return masked_mse_terms(pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad)
    return _terms_call(kind, pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad)


class _MaskedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, kind, col_weight, inv_norm, scale, t0_coef):
        out, grad = _terms_call(kind, pred, target, mask, col_weight, inv_norm, scale, t0_coef, want_grad=pred.requires_grad)
        ctx.grad_tm = grad
        ctx.mark_non_differentiable(out)
        return out[pred.shape[2] + 1].clone(), out

    @staticmethod
    def backward(ctx, go, _go_terms):
        g = ctx.grad_tm.permute(1, 0, 2) * go
        return g, None, None, None, None, None, None, None


def masked_loss(pred, target, mask=None, loss_func=None, col_weight: Optional[Sequence[float]] = None,
                inv_norm: Optional[torch.Tensor] = None, scale: float = 1.0, t0_coef: float = 0.0):
    """masked_mse's contract with the pointwise loss `loss_func`; None / MSE IS masked_mse."""
    kind = loss_kind_of(loss_func)
    if kind.kind == _lib.LOSS_MSE:
        return masked_mse(pred, target, mask, col_weight=col_weight, inv_norm=inv_norm, scale=scale, t0_coef=t0_coef)
    return _MaskedLoss.apply(pred, target, mask, kind, col_weight, inv_norm, scale, t0_coef)


def per_sample_loss(pred, target, mask=None, loss_func=None) -> torch.Tensor:
    """The evaluation loop's table `torch.sum(Loss_func(x_pred * mask, x * mask, reduction='none'), dim=1)` -> [B, D]
    (evalute_model, neural_00_ODE_01_no_encode.py:123; neural_01_DAE_01_no_encode.py:158-160), all four kinds, one kernel, one writer and
    one summation order per entry.  The mask multiplies both operands as the scripts write it.  Not differentiable."""
    kind = loss_kind_of(loss_func)
    lib = _lib.load()
    a, keep, dev = _loss_args(pred, target, mask, None, None, 1.0, 0.0, "per_sample_loss")
    B, _, D = pred.shape
    out = _empty((B, D), dtype=torch.float32, device=dev)
    a.out = out.data_ptr()
    fn = _lib.LossFnF32(kind.kind, kind.param)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.psnode_loss_per_sample_f32(ctypes.byref(a), ctypes.byref(fn), ctypes.c_void_p(st)), "psnode_loss_per_sample_f32")
    return out


def inv_mask_sum(mask: torch.Tensor) -> torch.Tensor:
    """1 / sum(mask) as a device scalar (no host sync)."""
    return torch.sum(mask).reciprocal().reshape(1)


def ode01_loss(x_pred, x, mask, loss_func=None):
    """ODE_01 training loss: neural_00_ODE_01_no_encode.py:353-355 (masked term only)."""
    return masked_loss(x_pred, x, mask, loss_func, inv_norm=inv_mask_sum(mask))


ode_loss = ode01_loss     # round-1 name


def recon_loss(x_re, x, loss_func=None):
    """Unmasked mean reconstruction error `Loss_func(x_re, x)`: neural_00_ODE_02_direct_encode.py:269."""
    return masked_loss(x_re, x, None, loss_func, scale=1.0 / x.numel())


def ode02_loss(x_pred, x_re, x, mask, loss_func=None):
    """ODE_02 training loss: x0 term + masked term + reconstruction (neural_00_ODE_02_direct_encode.py:267-270).
    Returns (loss, (terms of the prediction call, terms of the reconstruction call))."""
    B, _, xd = x.shape
    lp, tp = masked_loss(x_pred, x, mask, loss_func, inv_norm=inv_mask_sum(mask), t0_coef=1.0 / (B * xd))
    lr, tr = recon_loss(x_re, x, loss_func)
    return lp + lr, (tp, tr)


def dae01_loss(x_pred, x, i_pred, i, mask, x_col_weight: Optional[Sequence[float]] = None, loss_func=None):
    """DAE_01 training loss: neural_01_DAE_01_no_encode.py:414-419 (column 1 of x counted 1 + 9 times unless `x_col_weight`
    says otherwise)."""
    B, _, xd = x.shape
    idim = i.shape[2]
    if x_col_weight is None:
        x_col_weight = [10.0 if d == 1 else 1.0 for d in range(xd)]
    inv = inv_mask_sum(mask)
    lx, tx = masked_loss(x_pred, x, mask, loss_func, col_weight=x_col_weight, inv_norm=inv, t0_coef=1.0 / (B * xd))
    li, ti = masked_loss(i_pred, i, mask, loss_func, inv_norm=inv, t0_coef=1.0 / (B * idim))
    return lx + li, (tx, ti)


dae_loss = dae01_loss     # round-1 name


def dae02_loss(x_pred, i_pred, x_re, i_re, x, i, mask, loss_func=None):
    """DAE_02 training loss: unweighted columns + the two reconstruction terms (neural_01_DAE_02_direct_encode.py:359-365)."""
    base, terms = dae01_loss(x_pred, x, i_pred, i, mask, x_col_weight=[1.0] * x.shape[2], loss_func=loss_func)
    lxr, txr = recon_loss(x_re, x, loss_func)
    lir, tir = recon_loss(i_re, i, loss_func)
    return base + lxr + lir, (*terms, txr, tir)
