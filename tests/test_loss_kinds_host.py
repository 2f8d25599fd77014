"""Host half of the loss kinds (L1 / SmoothL1 / Huber on K6, the per-sample evaluation form): what `Loss_func` spellings name which
kernel kind, the statuses and the order of the checks of the three entry points (the library loads without a GPU and every check
returns before a launch), and the `loss_func=` keyword of the sharded loss on a one-rank gloo group.  No GPU."""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from py_psnode_amd import _lib  # noqa: E402
from py_psnode_amd import loss as L  # noqa: E402

MSE, L1, SMOOTH_L1, HUBER = 0, 1, 2, 3
ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4, -5


# ---------------------------------------------------------------------------------------------------------------- loss_kind_of
@pytest.mark.parametrize("spelling,want", [
    (None, (MSE, 0.0)), ("mse", (MSE, 0.0)), ("l1", (L1, 0.0)), ("smooth_l1", (SMOOTH_L1, 1.0)), ("huber", (HUBER, 1.0)),
    (("huber", 0.05), (HUBER, 0.05)), (("smooth_l1", 0.25), (SMOOTH_L1, 0.25)), (["huber", 2], (HUBER, 2.0)),
    (F.mse_loss, (MSE, 0.0)), (F.l1_loss, (L1, 0.0)), (F.smooth_l1_loss, (SMOOTH_L1, 1.0)), (F.huber_loss, (HUBER, 1.0)),
    (functools.partial(F.smooth_l1_loss, beta=0.5), (SMOOTH_L1, 0.5)), (functools.partial(F.huber_loss, delta=0.05), (HUBER, 0.05)),
    (functools.partial(F.huber_loss), (HUBER, 1.0)), (functools.partial(F.mse_loss), (MSE, 0.0)), (functools.partial(F.l1_loss), (L1, 0.0)),
    (nn.MSELoss(), (MSE, 0.0)), (nn.L1Loss(reduction="sum"), (L1, 0.0)), (nn.SmoothL1Loss(beta=0.125), (SMOOTH_L1, 0.125)),
    (nn.HuberLoss(delta=3.0, reduction="none"), (HUBER, 3.0)), (nn.SmoothL1Loss(), (SMOOTH_L1, 1.0)), (nn.HuberLoss(), (HUBER, 1.0)),
    # torch's rule: smooth_l1 with beta == 0 is l1
    (("smooth_l1", 0.0), (L1, 0.0)), (functools.partial(F.smooth_l1_loss, beta=0.0), (L1, 0.0)), (nn.SmoothL1Loss(beta=0.0), (L1, 0.0)),
])
def test_loss_kind_of_accepts(spelling, want):
    k = L.loss_kind_of(spelling)
    assert tuple(k) == want and isinstance(k.param, float)
    assert L.loss_kind_of(k) == k                       # its own result goes back in
    assert k.name == ("mse", "l1", "smooth_l1", "huber")[want[0]]
    with pytest.raises(AttributeError):                 # frozen
        k.kind = 3


@pytest.mark.parametrize("spelling,exc", [
    (torch.sum, TypeError), (lambda a, b: (a - b).abs(), TypeError), (F.cross_entropy, TypeError), (nn.BCELoss(), TypeError), (3, TypeError),
    (functools.partial(torch.sum), TypeError), (("huber",), TypeError), ((F.huber_loss, 0.1), TypeError),
    (functools.partial(F.huber_loss, reduction="sum"), ValueError), (functools.partial(F.mse_loss, reduction="none"), ValueError),
    (functools.partial(F.smooth_l1_loss, delta=0.1), ValueError), (functools.partial(F.l1_loss, beta=0.1), ValueError),
    (functools.partial(F.huber_loss, torch.zeros(1)), ValueError),
    (("huber", -1.0), ValueError), (("huber", 0.0), ValueError), (functools.partial(F.huber_loss, delta=-0.5), ValueError),
    (("smooth_l1", -0.1), ValueError), (("huber", float("nan")), ValueError), (("smooth_l1", float("inf")), ValueError),
    (("l1", 0.5), ValueError), ("l2", ValueError), ("Huber", ValueError), (("rmse", 1.0), ValueError),
])
def test_loss_kind_of_refuses(spelling, exc):
    with pytest.raises(exc) as e:
        L.loss_kind_of(spelling)
    if exc is TypeError:
        assert "huber_loss" in str(e.value) and "smooth_l1" in str(e.value)     # the message lists what is accepted


# ---------------------------------------------------------------------------------------------------------------- C entry points
def _args(T=5, B=4, D=8, mw=1, **kw):
    """A call that passes every check (the pointers are never followed: each test stops the call before its launch)."""
    a = _lib.LossArgsF32()
    a.T, a.B, a.D, a.mask_width = T, B, D, mw
    a.pred = _lib.ViewF32(0x10000, B * D, D)
    a.target = _lib.ViewF32(0x20000, D, T * D)
    a.mask = _lib.ViewF32(0x30000 if mw else None, max(mw, 1), T * max(mw, 1))
    a.scale, a.t0_coef = 1.0, 0.0
    a.out = 0x40000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fn(kind, param=0.0):
    return _lib.LossFnF32(kind, param)


def _no_pred(a):
    a.pred = _lib.ViewF32(None, 1, 1)
    return a


# the K6 defects, each as (args, workspace pointer, workspace bytes relative to the need)
_K6_DEFECTS = {
    "D=65": lambda: (_args(D=65, mw=0), None, 0),
    "mask width 3": lambda: (_args(mw=3), None, 0),
    "T=0": lambda: (_args(T=0), None, 0),
    "NULL pred": lambda: (_no_pred(_args()), None, 0),
    "NULL out": lambda: (_args(out=None), None, 0),
    "NULL workspace": lambda: (_args(), None, 0),
    "short workspace": lambda: (_args(), 0x50000, -1),
    "misaligned workspace": lambda: (_args(), 0x50008, 0),
}
_GOOD_FNS = [None, (MSE, 0.0), (L1, 0.0), (SMOOTH_L1, 0.05), (HUBER, 0.05), (MSE, float("nan")), (L1, -1.0)]
_BAD_FNS = [(4, 1.0), (-1, 1.0), (SMOOTH_L1, 0.0), (HUBER, -1.0), (HUBER, float("nan")), (SMOOTH_L1, float("inf")), (HUBER, 0.0)]


def _call(lib, a, fn, ws, rel):
    need = lib.psnode_masked_mse_workspace_bytes(ctypes.byref(a))
    f = ctypes.byref(_fn(*fn)) if fn is not None else None
    return lib.psnode_masked_loss_f32(ctypes.byref(a), f, ctypes.c_void_p(ws), ctypes.c_size_t(max(need + rel, 0)), None)


def test_null_args_come_first():
    lib = _lib.load()
    for fn in (None, (HUBER, 0.05), (4, 1.0), (HUBER, -1.0)):
        f = ctypes.byref(_fn(*fn)) if fn is not None else None
        assert lib.psnode_masked_loss_f32(None, f, None, 0, None) == ERR_NULL
        assert lib.psnode_loss_per_sample_f32(None, f, None) == ERR_NULL
        assert lib.psnode_masked_loss_supported(None, f) == 0


@pytest.mark.parametrize("fn", _BAD_FNS)
def test_bad_kind_or_parameter_is_unsupported_before_k6s_checks(fn):
    lib = _lib.load()
    for name, make in _K6_DEFECTS.items():
        a, ws, rel = make()
        assert _call(lib, a, fn, ws, rel) == ERR_UNSUPPORTED, name
        assert lib.psnode_loss_per_sample_f32(ctypes.byref(a), ctypes.byref(_fn(*fn)), None) == ERR_UNSUPPORTED, name
        assert lib.psnode_masked_loss_supported(ctypes.byref(a), ctypes.byref(_fn(*fn))) == 0, name


@pytest.mark.parametrize("fn", _GOOD_FNS)
@pytest.mark.parametrize("defect", sorted(_K6_DEFECTS))
def test_k6_defects_give_k6s_status(defect, fn):
    """... for every valid fn (the parameter of MSE and L1 is ignored, whatever it is), and `supported` agrees with the call."""
    lib = _lib.load()
    a, ws, rel = _K6_DEFECTS[defect]()
    need = lib.psnode_masked_mse_workspace_bytes(ctypes.byref(a))
    want = lib.psnode_masked_mse_f32(ctypes.byref(a), ctypes.c_void_p(ws), ctypes.c_size_t(max(need + rel, 0)), None)
    assert want in (ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_UNSUPPORTED)
    expected = {"D=65": ERR_UNSUPPORTED, "mask width 3": ERR_DIMS, "T=0": ERR_DIMS, "NULL pred": ERR_NULL, "NULL out": ERR_NULL}
    assert want == expected.get(defect, ERR_WORKSPACE)
    assert _call(lib, a, fn, ws, rel) == want
    f = ctypes.byref(_fn(*fn)) if fn is not None else None
    # `supported` has no workspace to look at: 1 exactly where the call got as far as its workspace check
    assert lib.psnode_masked_loss_supported(ctypes.byref(a), f) == (1 if want == ERR_WORKSPACE else 0)
    if want != ERR_WORKSPACE:       # the per-sample form takes no workspace: the same status for everything before it
        assert lib.psnode_loss_per_sample_f32(ctypes.byref(a), f, None) == want


@pytest.mark.parametrize("kw", [{"col_weight": 0x60000}, {"t0_coef": 0.5}, {"grad_pred": 0x70000}, {"inv_norm": 0x80000}, {"scale": 2.0}])
@pytest.mark.parametrize("fn", [None, (MSE, 0.0), (HUBER, 0.05)])
def test_per_sample_refuses_the_training_forms_extras(kw, fn):
    lib = _lib.load()
    f = ctypes.byref(_fn(*fn)) if fn is not None else None
    assert lib.psnode_loss_per_sample_f32(ctypes.byref(_args(**kw)), f, None) == ERR_UNSUPPORTED
    assert lib.psnode_loss_per_sample_f32(ctypes.byref(_args(mw=3, **kw)), f, None) == ERR_UNSUPPORTED      # before K6's dims check
    assert lib.psnode_masked_loss_supported(ctypes.byref(_args(**kw)), f) == 1                                # the training form takes them


def test_binding_struct_matches_the_header():
    assert ctypes.sizeof(_lib.LossFnF32) == 8 and [f[0] for f in _lib.LossFnF32._fields_] == ["kind", "param"]
    assert (_lib.LOSS_MSE, _lib.LOSS_L1, _lib.LOSS_SMOOTH_L1, _lib.LOSS_HUBER) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "psnode_hip.h")).read()
    assert "PSNODE_LOSS_MSE = 0, PSNODE_LOSS_L1 = 1, PSNODE_LOSS_SMOOTH_L1 = 2, PSNODE_LOSS_HUBER = 3" in hdr
    assert _lib.load().psnode_abi_version() == 10


# ---------------------------------------------------------------------------------------------------------------- Python layer
def test_python_layer_has_no_cpu_path():
    x = torch.zeros(2, 3, 4)
    m = torch.ones(2, 3, 1)
    for lf in (None, F.l1_loss, functools.partial(F.huber_loss, delta=0.05)):
        with pytest.raises(ValueError):
            L.masked_loss(x, x, m, lf)
        with pytest.raises(ValueError):
            L.masked_loss_terms(x, x, m, lf)
        with pytest.raises(ValueError):
            L.per_sample_loss(x, x, m, lf)
        with pytest.raises(ValueError):
            L.ode01_loss(x, x, m, loss_func=lf)
        with pytest.raises(ValueError):
            L.ode02_loss(x, x, x, m, loss_func=lf)
        with pytest.raises(ValueError):
            L.dae01_loss(x, x, x[:, :, :2], x[:, :, :2], m, loss_func=lf)
        with pytest.raises(ValueError):
            L.dae02_loss(x, x[:, :, :2], x, x[:, :, :2], x, x[:, :, :2], m, loss_func=lf)
    with pytest.raises(TypeError):      # an unknown Loss_func is refused before anything else
        L.ode01_loss(x, x, m, loss_func=torch.sum)


@pytest.fixture
def one_rank_gloo(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def test_sharded_loss_passes_loss_func_to_the_local_call(one_rank_gloo, monkeypatch):
    from py_psnode_amd import sharded
    g = torch.Generator().manual_seed(0)
    B, T, D = 6, 7, 3
    x = torch.randn(B, T, D, generator=g)
    pred = x + 0.1 * torch.randn(B, T, D, generator=g)
    mask = (torch.rand(B, T, 1, generator=g) > 0.3).float()
    cw = [1.0, 10.0, 1.0]
    seen = []

    def stand_in(pred, target, mask, loss_func=None, col_weight=None, inv_norm=None, scale=1.0, t0_coef=0.0):
        seen.append(loss_func)
        fn = F.mse_loss if loss_func is None else loss_func
        w = torch.tensor(col_weight if col_weight is not None else [1.0] * pred.shape[2])
        cols = (fn(pred, target, reduction="none") * mask * w).sum((0, 1)) * inv_norm * scale
        t0 = t0_coef * fn(pred[:, 0], target[:, 0], reduction="sum")
        return cols.sum() + t0, torch.cat((cols, t0.reshape(1), (cols.sum() + t0).reshape(1)))

    monkeypatch.setattr(L, "masked_loss", stand_in)
    lf = functools.partial(F.huber_loss, delta=0.05)
    share, terms = sharded.masked_mse_sharded(pred, x, mask, col_weight=cw, t0_weight=1.0, loss_func=lf)
    assert seen == [lf]
    w = torch.tensor(cw)
    want_cols = (F.huber_loss(pred, x, reduction="none", delta=0.05) * mask * w).sum((0, 1)) / mask.sum()
    want_t0 = F.huber_loss(x[:, 0], pred[:, 0], delta=0.05)
    torch.testing.assert_close(share, want_cols.sum() + want_t0, rtol=1e-6, atol=0)
    torch.testing.assert_close(terms[:D], want_cols, rtol=1e-6, atol=0)
    torch.testing.assert_close(terms[D], want_t0, rtol=1e-6, atol=0)
    torch.testing.assert_close(terms[D + 1], share, rtol=1e-6, atol=0)
    # default: no loss_func reaches the default local call as None (= MSE, the call of today)
    sharded.masked_mse_sharded(pred, x, mask)
    assert seen == [lf, None]
    # an explicit local_fn is called exactly as before: no loss_func keyword
    calls = []

    def local(pred, target, mask, col_weight=None, inv_norm=None, t0_coef=0.0):
        calls.append((col_weight, float(inv_norm), t0_coef))
        return stand_in(pred, target, mask, None, col_weight, inv_norm, 1.0, t0_coef)

    share2, _ = sharded.masked_mse_sharded(pred, x, mask, col_weight=cw, t0_weight=1.0, local_fn=local)
    assert calls == [(cw, float(1.0 / mask.sum()), 1.0 / (B * D))] and len(seen) == 3
    want = ((pred - x) ** 2 * mask * w).sum() / mask.sum() + F.mse_loss(x[:, 0], pred[:, 0])
    torch.testing.assert_close(share2, want, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        sharded.masked_mse_sharded(pred, x, mask, local_fn=local, loss_func=lf)
