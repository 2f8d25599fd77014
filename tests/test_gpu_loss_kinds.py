"""GPU parity of K6's other pointwise losses -- L1, SmoothL1(beta), Huber(delta) -- and of the per-sample evaluation form of all four
kinds, against torch's own functionals evaluated on the CPU in fp64 on the fp32 inputs, arranged in the scripts' expressions.

Tolerances are tests/test_gpu_loss.py's: values rel 2e-6, gradients and per-sample tables 1e-6 of the reference tensor's max.  The fp32
torch expression itself differs from the fp64 one by at most 1.5e-7 on these inputs (value, gradient and per-sample, all kinds), so the
bound leaves an order of magnitude for the kernel's summation order.  beta = delta = 0.05 with errors 0.05 * randn: both branches of the
piecewise kinds hold a large share of the elements (asserted on the reference)."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
RTOL_VAL, RTOL_GRAD = 2e-6, 1e-6
KNEE = 0.05
KINDS = {
    "mse": F.mse_loss,
    "l1": F.l1_loss,
    "smooth_l1": functools.partial(F.smooth_l1_loss, beta=KNEE),
    "huber": functools.partial(F.huber_loss, delta=KNEE),
}
NEW_KINDS = ["l1", "smooth_l1", "huber"]
#          fast path, float4 staging, both widths | one row | ragged both ways | scalar path            | D < 4 butterflies
SHAPES = [(32, 101, 8, 8), (32, 101, 8, 1), (1, 1, 8, 1), (33, 17, 8, 8), (5, 40, 3, 1), (41, 16, 5, 5), (70, 9, 2, 2), (7, 19, 1, 1),
          (64, 33, 2, 1), (9, 33, 16, 16), (6, 9, 32, 32), (3, 21, 64, 1), (260, 5, 8, 1), (12, 7, 4, 4), (300, 40, 8, 0)]
#          ... | wide rows                                  | more trajectory tiles than time tiles | D = 4 | no mask


def L():
    from py_psnode_amd import loss
    return loss


@functools.lru_cache(maxsize=None)
def _case(B, T, D, mw, seed=0, layout="tm"):
    """tests/test_gpu_loss.py's inputs: target 0.3 randn, pred = target + 0.05 randn, mask rand > 0.3.  Shared, never written to."""
    g = torch.Generator().manual_seed(seed)
    x = 0.3 * torch.randn(B, T, D, generator=g)
    if layout == "tm":      # what the integrator returns: time-major memory viewed as [B,T,D]
        pred = (x.permute(1, 0, 2) + 0.05 * torch.randn(T, B, D, generator=g)).contiguous().permute(1, 0, 2)
    else:
        pred = x + 0.05 * torch.randn(B, T, D, generator=g)
    mask = None
    if mw:
        mask = (torch.rand(B, T, mw, generator=g) > 0.3).float()
        mask[0, 0] = 1.0
    return pred, x, mask


def _dev(pred, layout):
    """pred on the device in the memory layout it has on the host"""
    return pred.cuda() if layout == "bm" else pred.permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)


def _close(a, b, rtol):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()) <= rtol * max(float(b.abs().max()), 1e-30)


def _col_weight(D):
    return [10.0 if d == 1 else 1.0 for d in range(D)]


def _training_reference(fn, pred, x, mask, cw):
    """DAE_01's shape of the expression in fp64: weighted masked columns over sum(mask), plus Loss_func(x[:,0,:], x_pred[:,0,:])."""
    p = pred.double().clone().requires_grad_(True)
    m = mask.double() if mask is not None else torch.ones_like(p)
    el = fn(p, x.double(), reduction="none")
    cols = torch.sum(torch.sum(el * m, dim=1), dim=0) * torch.tensor(cw, dtype=torch.float64) / torch.sum(m)
    t0 = fn(x.double()[:, 0, :], p[:, 0, :])
    total = torch.sum(cols) + t0
    total.backward()
    return total.detach(), cols.detach(), t0.detach(), p.grad, (pred.double() - x.double()).abs()


@pytest.mark.parametrize("layout", ["tm", "bm"])
@pytest.mark.parametrize("B,T,D,mw", SHAPES)
@pytest.mark.parametrize("kind", NEW_KINDS)
def test_training_form_value_terms_and_grad(kind, B, T, D, mw, layout):
    pred, x, mask = _case(B, T, D, mw, seed=B + T, layout=layout)
    cw = _col_weight(D)
    total, cols, t0, grad, ae = _training_reference(KINDS[kind], pred, x, mask, cw)
    if ae.numel() >= 256:           # both branches of the piecewise kinds are exercised
        beyond = float((ae >= KNEE).double().mean())
        assert 0.1 <= beyond <= 0.9, beyond
    pg = _dev(pred, layout).requires_grad_(True)
    mg = mask.cuda() if mask is not None else None
    inv = L().inv_mask_sum(mg) if mg is not None else torch.full((1,), 1.0 / (B * T * D), device="cuda")
    tot, terms = L().masked_loss(pg, x.cuda(), mg, KINDS[kind], col_weight=cw, inv_norm=inv, t0_coef=1.0 / (B * D))
    tot.backward()
    print(f"{kind} {B, T, D, mw} {layout}: total rel {abs(float(tot.detach()) - float(total)) / float(total):.2e}  "
          f"grad rel-to-max {float((pg.grad.double().cpu() - grad).abs().max() / grad.abs().max()):.2e}")
    assert terms.shape == (D + 2,) and not terms.requires_grad
    assert _close(tot, total, RTOL_VAL) and _close(terms[D + 1], total, RTOL_VAL)
    assert _close(terms[:D], cols, RTOL_VAL) and _close(terms[D], t0, RTOL_VAL)
    assert pg.grad.shape == grad.shape and _close(pg.grad, grad, RTOL_GRAD)
    terms2, _ = L().masked_loss_terms(pg.detach(), x.cuda(), mg, KINDS[kind], col_weight=cw, inv_norm=inv, t0_coef=1.0 / (B * D))
    assert torch.equal(terms, terms2)       # run-to-run bitwise, with and without the gradient store


@pytest.mark.parametrize("B,T,D,mw", [(33, 17, 8, 8), (41, 16, 5, 5), (70, 9, 2, 1)])
def test_l1_gradient_is_zero_at_zero_and_a_pure_sign_elsewhere(B, T, D, mw):
    """torch's rule sign(0) = 0, and no rounding anywhere else: grad = +-(norm * w * m), bit for bit."""
    pred, x, mask = _case(B, T, D, mw, seed=77)
    g = torch.Generator().manual_seed(78)
    same = torch.rand(B, T, D, generator=g) < 0.1
    pred = torch.where(same, x, pred)                   # e == 0 exactly on a tenth of the entries
    mask = mask.clone()
    mask[B // 2:, T // 3:2 * T // 3] = 0.0              # a masked-out region
    cw = _col_weight(D)
    pg = _dev(pred, "tm").requires_grad_(True)
    inv = L().inv_mask_sum(mask.cuda())
    tot, _ = L().masked_loss(pg, x.cuda(), mask.cuda(), "l1", col_weight=cw, inv_norm=inv)
    tot.backward()
    e = pred - x
    assert int((e == 0).sum()) >= same.sum() > 0
    mag = inv.cpu() * (torch.tensor(cw) * mask.expand(B, T, D))          # fp32, the kernel's own product order
    want = torch.sign(e) * mag
    got = pg.grad.cpu()
    assert torch.equal(got[e == 0], torch.zeros_like(got[e == 0]))
    assert torch.equal(got[mask.expand(B, T, D) == 0], torch.zeros_like(got[mask.expand(B, T, D) == 0]))
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,T,D,mw", [(32, 101, 8, 8), (5, 40, 3, 1)])
def test_mse_through_the_new_entry_points_is_k6_bit_for_bit(B, T, D, mw):
    pred, x, mask = _case(B, T, D, mw, seed=5)
    cw = _col_weight(D)
    xg, mg = x.cuda(), mask.cuda()
    inv = L().inv_mask_sum(mg)
    out = []
    for call in (lambda p: L().masked_mse(p, xg, mg, col_weight=cw, inv_norm=inv, t0_coef=0.25),
                 lambda p: L().masked_loss(p, xg, mg, None, col_weight=cw, inv_norm=inv, t0_coef=0.25),
                 lambda p: L().masked_loss(p, xg, mg, F.mse_loss, col_weight=cw, inv_norm=inv, t0_coef=0.25)):
        pg = _dev(pred, "tm").requires_grad_(True)
        tot, terms = call(pg)
        tot.backward()
        out.append((tot.detach(), terms, pg.grad))
    for tot, terms, grad in out[1:]:
        assert torch.equal(tot, out[0][0]) and torch.equal(terms, out[0][1]) and torch.equal(grad, out[0][2])
    # the C entry point itself with kind MSE forwards to K6
    terms_c, grad_c = L()._terms_call(L().LossKind(0, 0.0), _dev(pred, "tm"), xg, mg, cw, inv, 1.0, 0.25, True)
    assert torch.equal(terms_c, out[0][1]) and torch.equal(grad_c.permute(1, 0, 2), out[0][2])


def _per_sample_reference(fn, pred, x, mask):
    p, t = pred.double(), x.double()
    if mask is not None:
        p, t = p * mask.double(), t * mask.double()
    return torch.sum(fn(p, t, reduction="none"), dim=1)


@pytest.mark.parametrize("layout", ["tm", "bm"])
@pytest.mark.parametrize("B,T,D,mw", SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_per_sample_table(kind, B, T, D, mw, layout):
    pred, x, mask = _case(B, T, D, mw, seed=B + T, layout=layout)
    ref = _per_sample_reference(KINDS[kind], pred, x, mask)
    pg, xg, mg = _dev(pred, layout), x.cuda(), (mask.cuda() if mask is not None else None)
    out = L().per_sample_loss(pg, xg, mg, KINDS[kind])
    print(f"per-sample {kind} {B, T, D, mw} {layout}: rel-to-max {float((out.double().cpu() - ref).abs().max() / ref.abs().max()):.2e}")
    assert out.shape == (B, D) and out.is_contiguous() and out.dtype == torch.float32
    assert _close(out, ref, RTOL_GRAD)
    assert torch.equal(out, L().per_sample_loss(pg, xg, mg, KINDS[kind]))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B,T,D,mw", [(32, 101, 8, 8), (32, 101, 8, 1), (41, 16, 5, 5)])
def test_per_sample_multiplies_both_operands_by_a_non_binary_mask(kind, B, T, D, mw):
    """rho(m * e) is not m * rho(e): the table follows the scripts' expression."""
    pred, x, _ = _case(B, T, D, mw, seed=31)
    mask = torch.rand(B, T, mw, generator=torch.Generator().manual_seed(32))
    ref = _per_sample_reference(KINDS[kind], pred, x, mask)
    out = L().per_sample_loss(_dev(pred, "tm"), x.cuda(), mask.cuda(), KINDS[kind])
    assert _close(out, ref, RTOL_GRAD)
    if kind != "l1":            # (|m e| = m |e| for m >= 0: L1 alone cannot tell the two apart)
        other = torch.sum(KINDS[kind](pred.double(), x.double(), reduction="none") * mask.double(), dim=1)
        assert not _close(out, other, 1e-3)


def test_per_sample_zero_mask_gives_exact_zeros_and_mse_columns_match_k6():
    B, T, D = 33, 50, 8
    pred, x, mask = _case(B, T, D, D, seed=41)
    mask = mask.clone()
    mask[:, :, 2] = 0.0             # a column nobody observes
    mask[5] = 0.0                   # a trajectory nobody observes
    pg, xg, mg = _dev(pred, "tm"), x.cuda(), mask.cuda()
    for kind in KINDS:
        out = L().per_sample_loss(pg, xg, mg, KINDS[kind])
        assert float(out[:, 2].abs().max()) == 0.0 and float(out[5].abs().max()) == 0.0 and float(out.abs().max()) > 0.0
    m1 = mask[:, :, :1].contiguous()
    m1[7] = 0.0
    out = L().per_sample_loss(pg, xg, m1.cuda(), "huber")
    assert float(out[7].abs().max()) == 0.0 and float(out[5].abs().max()) == 0.0
    # kind MSE with a 0/1 mask: the table's column sums are K6's unnormalised per-column terms
    table = L().per_sample_loss(pg, xg, mg, "mse")
    terms, _ = L().masked_mse_terms(pg, xg, mg)
    assert _close(table.double().sum(0), terms[:D], RTOL_VAL)


# ---------------------------------------------------------------------------------------------------------------- script objectives
def _masked_cols(fn, pred, x, mask):
    return torch.sum(torch.sum(fn(pred, x, reduction="none") * mask, dim=1), dim=0) / torch.sum(mask)


@pytest.mark.parametrize("kind", ["huber", "l1"])
def test_ode02_loss_with_loss_func(kind):
    """neural_00_ODE_02_direct_encode.py:267-270 with line 49 changed."""
    fn = KINDS[kind]
    B, T, xd = 7, 3, 5
    xp, x, mask = _case(B, T, xd, xd, seed=12)
    xre, _, _ = _case(B, T, xd, 0, seed=13, layout="bm")
    pr, rr = xp.double().clone().requires_grad_(True), xre.double().clone().requires_grad_(True)
    xd64, m64 = x.double(), mask.double()
    ref = fn(xd64[:, 0, :], pr[:, 0, :]) + torch.sum(_masked_cols(fn, pr, xd64, m64)) + fn(rr, xd64)
    ref.backward()
    pg, rg = _dev(xp, "tm").requires_grad_(True), xre.cuda().requires_grad_(True)
    tot, _ = L().ode02_loss(pg, rg, x.cuda(), mask.cuda(), loss_func=fn)
    tot.backward()
    assert _close(tot, ref, RTOL_VAL) and _close(pg.grad, pr.grad, RTOL_GRAD) and _close(rg.grad, rr.grad, RTOL_GRAD)


@pytest.mark.parametrize("kind", ["huber", "l1"])
@pytest.mark.parametrize("script", ["dae01", "dae02"])
def test_dae_losses_with_loss_func(script, kind):
    """neural_01_DAE_01_no_encode.py:414-419 / neural_01_DAE_02_direct_encode.py:359-365 with line 49 changed."""
    fn = KINDS[kind]
    B, T, xd, idim = 32, 101, 8, 2
    xp, x, mask = _case(B, T, xd, 1, seed=21)
    ip, i, _ = _case(B, T, idim, 0, seed=22)
    xre, _, _ = _case(B, T, xd, 0, seed=23, layout="bm")
    ire, _, _ = _case(B, T, idim, 0, seed=24, layout="bm")
    leaves = [a.double().clone().requires_grad_(True) for a in (xp, ip, xre, ire)]
    x64, i64, m64 = x.double(), i.double(), mask.double()
    se, se_i = fn(leaves[0], x64, reduction="none"), fn(leaves[1], i64, reduction="none")
    x_loss = torch.sum(se * m64)
    if script == "dae01":
        x_loss = x_loss + 9 * torch.sum(se[:, :, 1:2] * m64)
    ref = x_loss / torch.sum(m64) + torch.sum(se_i * m64) / torch.sum(m64) + fn(x64[:, 0, :], leaves[0][:, 0, :]) + fn(i64[:, 0, :], leaves[1][:, 0, :])
    if script == "dae02":
        ref = ref + fn(leaves[2], x64) + fn(leaves[3], i64)
    ref.backward()
    dev = [_dev(xp, "tm").requires_grad_(True), _dev(ip, "tm").requires_grad_(True), xre.cuda().requires_grad_(True), ire.cuda().requires_grad_(True)]
    if script == "dae01":
        tot, _ = L().dae01_loss(dev[0], x.cuda(), dev[1], i.cuda(), mask.cuda(), loss_func=fn)
    else:
        tot, _ = L().dae02_loss(*dev, x.cuda(), i.cuda(), mask.cuda(), loss_func=fn)
    tot.backward()
    assert _close(tot, ref, RTOL_VAL)
    for a, b in zip(dev[:2 if script == "dae01" else 4], leaves):
        assert _close(a.grad, b.grad, RTOL_GRAD)


def test_train_step_fused_integrator_plus_smooth_l1_matches_cpu_autograd():
    """The ODE_01 step of tests/test_gpu_loss.py (fused forward -> fused loss -> fused backward) with Loss_func = smooth_l1(beta 0.05),
    vs CPU autograd through the unfused model and the script's expression; that test's tolerances."""
    from py_psnode_amd import models, neural_dae as nd
    lf = functools.partial(F.smooth_l1_loss, beta=KNEE)
    torch.manual_seed(0)
    B, T = 24, 21
    m_ref = models.ODE_Model(8, 2, 64, solver=nd.RK4())
    m_ref.solver.fused = "off"
    m_gpu = models.ODE_Model(8, 2, 64, solver=nd.RK4()).cuda()
    m_gpu.load_state_dict(m_ref.state_dict())
    m_gpu.solver.fused = "require"
    g = torch.Generator().manual_seed(5)
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(1, T, 1).repeat(B, 1, 1)
    x, z = 0.1 * torch.randn(B, T, 8, generator=g), 0.1 * torch.randn(B, T, 2, generator=g)
    mask = (torch.rand(B, T, 8, generator=g) > 0.2).float()
    ev, zj = -torch.ones(B, 1, 1), torch.zeros(B, 1, 2)
    ref = torch.sum(_masked_cols(lf, m_ref(t, x, z, ev, zj), x, mask))
    ref.backward()
    c = lambda a: a.cuda()
    tot, _ = L().ode01_loss(m_gpu(c(t), c(x), c(z), c(ev), c(zj)), c(x), c(mask), loss_func=lf)
    tot.backward()
    assert _close(tot, ref, 1e-5)
    for (n, pr), (_, pg) in zip(m_ref.named_parameters(), m_gpu.named_parameters()):
        assert _close(pg.grad, pr.grad, 2e-4), n


def test_full_size_huber_value_deterministic_and_linear():
    """BASELINE batch (B=4096, T=1001, xd=8), Huber: fp64 value at full size, run-to-run bit-identical, and
    loss(mask1 + mask2) == loss(mask1) + loss(mask2) for disjoint masks under one norm."""
    B, T, D = 4096, 1001, 8
    lf = KINDS["huber"]
    pred, x, mask = _case(B, T, D, 1, seed=1)
    ref = torch.sum(_masked_cols(lf, pred.double(), x.double(), mask.double()))
    pg, xg, mg = _dev(pred, "tm"), x.cuda(), mask.cuda()
    a, ta = L().ode01_loss(pg, xg, mg, loss_func=lf)
    b, tb = L().ode01_loss(pg, xg, mg, loss_func=lf)
    assert torch.equal(ta, tb)
    assert _close(a, ref, 1e-5)
    inv = L().inv_mask_sum(mg)
    half = (torch.arange(B, device="cuda") % 2 == 0).float().view(B, 1, 1)
    l1, _ = L().masked_loss(pg, xg, mg * half, lf, inv_norm=inv)
    l2, _ = L().masked_loss(pg, xg, mg * (1 - half), lf, inv_norm=inv)
    assert _close(l1 + l2, a, 1e-6)
    _case.cache_clear()             # 3 x 131 MB


def test_error_paths_through_python():
    pred, x, mask = _case(4, 5, 8, 1)
    lf = KINDS["huber"]
    big = torch.zeros(2, 3, 65, device="cuda")
    for call in (lambda *a: L().masked_loss(*a, lf), lambda *a: L().per_sample_loss(*a, lf), lambda *a: L().masked_loss_terms(*a, "l1")):
        with pytest.raises(ValueError):         # PSNODE_ERR_UNSUPPORTED: rows wider than 64
            call(big, big, None)
        with pytest.raises(TypeError):
            call(pred.cuda().double(), x.cuda().double(), None)
        with pytest.raises(ValueError):
            call(pred.cuda(), x.cuda(), mask.cuda().expand(4, 5, 3))
        with pytest.raises(ValueError):
            call(pred.cuda(), x.cuda()[:, :4], mask.cuda())
    p = pred.cuda().requires_grad_(True)
    out = L().per_sample_loss(p, x.cuda(), mask.cuda(), lf)
    assert out.grad_fn is None and not out.requires_grad and out.shape == (4, 8)
