"""The wave integrators K1x / K2x with the alternating in-quad transposes and the two-slot RK4 loop: forced
(`kernel="wave"`) against the fp64 oracle and against the 4-wave tile kernels, at the project's gate (helpers.TOL_GPU, per trajectory).

Shapes are the smallest at which these paths can go wrong: B 4 / 5 / 9 (a full wave, a ragged one, a second wave), T 2 / 3 / 4 / 70 (the peeled
last step, both parities of the loop unrolled by two and its remainder, a second 64-step block of the event table), x_dim 8 / 5 (the FAST and the
general loop), z_dim 0 / 2 / 8 (0, 1 and 4 groups of external MFMAs), hidden 64 / 20 (zero padding).  One CPU test emulates the two butterfly
orders of the transpose on the lane / register packing the asm relies on."""
import itertools

import numpy as np
import pytest
import torch

from helpers import TOL_GPU, traj_rel_err as rel_err
from oracle import psnode_oracle as O

METHODS = ("rk4", "midpoint", "euler")
BS, TS = (4, 5, 9), (2, 3, 4, 70)
SHAPES = tuple(itertools.product((8, 5), (0, 2, 8), (64, 20)))       # (x_dim, z_dim, hidden)


def _fused():
    from py_psnode_amd import fused as f
    return f


def _ode(B, Tn, xd, zd, H, seed):
    g = torch.Generator().manual_seed(seed)
    dims = [3 * (xd + zd)] + [H] * 3 + [xd]
    ls = []
    for k in range(4):
        bound = dims[k] ** -0.5
        ls.append(((2 * torch.rand(dims[k + 1], dims[k], generator=g) - 1) * bound, (2 * torch.rand(dims[k + 1], generator=g) - 1) * bound))
    t = (torch.arange(Tn, dtype=torch.float32) * 0.01).view(Tn, 1, 1).repeat(1, B, 1)
    x = 0.1 * torch.randn(Tn, B, xd, generator=g)
    z = 0.1 * torch.randn(Tn, B, zd, generator=g)
    return ls, t, x, z, torch.cat((x[0], z[0]), -1)


def _oracle64(method, ls, t, x, z, a0, **kw):
    d = lambda a: None if a is None else a.double()
    return O.integrate_ode(method, [(w.double(), b.double()) for w, b in ls], d(t), d(x), d(z), d(a0),
                           **{k: (d(v) if torch.is_tensor(v) else v) for k, v in kw.items()})


def _run(method, ls, t, x, z, a0, kernel, **kw):
    c = lambda a: a.cuda() if torch.is_tensor(a) else a
    return _fused().ode_integrate(method, [(w.cuda(), b.cuda()) for w, b in ls], c(t), c(x), c(z), c(a0), kernel=kernel,
                                  **{k: c(v) for k, v in kw.items()}).cpu()


# every (x_dim, z_dim, hidden) with every T; B cycles with the case number so that each (B, T) pair occurs
CASES = [(shape, Tn, BS[(n + n // len(TS)) % len(BS)]) for n, (shape, Tn) in enumerate(itertools.product(SHAPES, TS))]


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape,Tn,B", CASES, ids=lambda v: "x%dz%dh%d" % v if isinstance(v, tuple) else str(v))
def test_k1x_forced_vs_fp64_oracle_and_tile(shape, Tn, B, method):
    xd, zd, H = shape
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=100 + 7 * Tn + B + xd + zd + H)
    ref = _oracle64(method, ls, t, x, z, a0)
    wave, tile = _run(method, ls, t, x, z, a0, "wave"), _run(method, ls, t, x, z, a0, "tile")
    assert torch.isfinite(wave).all()
    assert rel_err(wave, ref) <= TOL_GPU
    assert rel_err(wave, tile) <= TOL_GPU


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("Tn", [3, 4, 5, 70])
def test_k1x_fast_loop_on_a_non_uniform_clock(Tn, method):
    """The FAST loop (even x_dim, no event table, no teacher forcing) on per-trajectory clocks whose steps vary by a factor of up to 8: a step
    that forms h from the wrong clock slot (RK4's loop keeps t[k] and t[k + 1] in two registers that swap roles every step) is then wrong by
    far more than the gate, which a uniform grid would not show."""
    B = 5
    ls, t, x, z, a0 = _ode(B, Tn, 8, 2, 64, seed=300 + Tn)
    g = torch.Generator().manual_seed(301 + Tn)
    t = torch.cumsum(0.004 + 0.028 * torch.rand(Tn, B, 1, generator=g), dim=0)
    ref = _oracle64(method, ls, t, x, z, a0)
    wave, tile = _run(method, ls, t, x, z, a0, "wave"), _run(method, ls, t, x, z, a0, "tile")
    assert rel_err(wave, ref) <= TOL_GPU
    assert rel_err(wave, tile) <= TOL_GPU


@pytest.mark.gpu
@pytest.mark.parametrize("B,Tn", [(5, 70), (9, 4)])
def test_k1x_forced_with_an_event_and_with_teacher_forcing(B, Tn):
    """An event table that holds events (one of them past the first 64-step block at T = 70) and teacher forcing: the general loop."""
    ls, t, x, z, a0 = _ode(B, Tn, 8, 2, 64, seed=7)
    g = torch.Generator().manual_seed(8)
    ev = torch.stack([t[1], t[min(Tn - 2, 66)]], dim=1).contiguous()
    zj = 0.1 * torch.randn(B, 2, 2, generator=g)
    for kw in (dict(event_t=ev, z_jump=zj), dict(input_true_x=True), dict(event_t=ev, z_jump=zj, input_true_x=True)):
        ref = _oracle64("rk4", ls, t, x, z, a0, **kw)
        wave, tile = _run("rk4", ls, t, x, z, a0, "wave", **kw), _run("rk4", ls, t, x, z, a0, "tile", **kw)
        assert rel_err(wave, ref) <= TOL_GPU, sorted(kw)
        assert rel_err(wave, tile) <= TOL_GPU, sorted(kw)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("Tn", [4, 70])
def test_k2x_forced_vs_fp64_oracle(Tn, method):
    """K2x on one DAE shape (x8 z2 v2 i2, hidden 64, B = 5), with events where the grid has room for them."""
    B, xd, zd, vd, idim, H = 5, 8, 2, 2, 2, 64
    g = torch.Generator().manual_seed(31 + Tn)
    n = xd + zd + vd + idim

    def mlp(dims):
        return [((2 * torch.rand(dims[k + 1], dims[k], generator=g) - 1) * dims[k] ** -0.5,
                 (2 * torch.rand(dims[k + 1], generator=g) - 1) * dims[k] ** -0.5) for k in range(len(dims) - 1)]
    de, ae = mlp([3 * n, H, H, H, xd]), mlp([n + xd + zd + vd, H, H, H, idim])
    t = (torch.arange(Tn, dtype=torch.float32) * 0.01).view(Tn, 1, 1).repeat(1, B, 1)
    r = lambda *s: 0.1 * torch.randn(*s, generator=g)
    x, z, v, i, xi = r(Tn, B, xd), r(Tn, B, zd), r(Tn, B, vd), r(Tn, B, idim), r(B, xd)
    a0 = torch.cat((xi, z[0], v[0], i[0]), -1)
    ev = torch.stack([t[3], t[Tn - 2]], dim=1).contiguous() if Tn > 5 else None
    zj, vj = r(B, 2, zd), r(B, 2, vd)
    d = lambda a: None if a is None else a.double()
    dd = lambda ls: [(w.double(), b.double()) for w, b in ls]
    ref_x, ref_i = O.integrate_dae(method, dd(de), dd(ae), d(xi), d(t), d(x), d(z), d(v), d(i), d(a0), d(ev), d(zj), d(vj))
    c = lambda a: None if a is None else a.cuda()
    dl = lambda ls: [(w.cuda(), b.cuda()) for w, b in ls]
    xs, is_ = _fused().dae_integrate(method, dl(de), dl(ae), c(xi), c(t), c(x), c(z), c(v), c(i), c(a0), event_t=c(ev), z_jump=c(zj),
                                     v_jump=c(vj), kernel="wave")
    assert rel_err(xs.cpu(), ref_x) <= TOL_GPU
    assert rel_err(is_.cpu(), ref_i) <= TOL_GPU


def _close(a, b, what, tol=1e-4):
    """The backward tests' measure (test_gpu_backward.py, test_gpu_backward_x.py): max abs error against the other side's max abs value."""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H", [64, 20])
def test_saving_forward_rows_and_gradients_wave_vs_tile(H, method):
    """The training forward (the SAVE instances of K1x: plain ELU domain, the transposes' mask carried across the divergent store branches)
    through `fused_ode_integrate` at B = 5, T = 4: the rows it returns, the rows it saves and every gradient against the tile route."""
    from py_psnode_amd import fused
    from py_psnode_amd.autograd import fused_ode_integrate
    B, Tn, xd, zd = 5, 4, 8, 2
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=500 + H)
    G = torch.randn(Tn, B, xd, generator=torch.Generator().manual_seed(9)).cuda()
    out = {}
    for kern in ("tile", "wave"):
        layers = [(w.cuda().requires_grad_(), b.cuda().requires_grad_()) for w, b in ls]
        tt, xx, zz, aa = t.cuda(), x.cuda().requires_grad_(), z.cuda().requires_grad_(), a0.cuda().requires_grad_()
        xs = fused_ode_integrate(method, kern, layers, tt, xx, zz, aa)
        (xs * G).sum().backward()
        _, saved = fused.ode_integrate(method, [(w.detach(), b.detach()) for w, b in layers], tt, xx.detach(), zz.detach(), aa.detach(),
                                       save=True, kernel=kern)
        out[kern] = (xs.detach(), saved, [xx.grad, zz.grad, aa.grad] + [p.grad for wb in layers for p in wb])
    (xs_t, sv_t, g_t), (xs_w, sv_w, g_w) = out["tile"], out["wave"]
    _close(xs_w, xs_t, "rows")
    _close(sv_w[1], sv_t[1], "saved stage inputs")
    _close(sv_w[0], sv_t[0], "saved activations")
    if H < sv_w[0].shape[-1]:
        assert float(sv_w[0][..., H:].abs().max()) == 0.0, "padding units are stored as zeros"
    for k, (p, q) in enumerate(zip(g_w, g_t)):
        assert p is not None and q is not None, k
        _close(p, q, f"gradient {k}")


# ---- the transpose's packing convention, on the CPU
# v[r][l]: register r of lane l.  D = mask ? src1 : dpp(src0), the DPP lane pattern quad_perm:[1,0,3,2] = lane ^ 1, [2,3,0,1] = lane ^ 2.
def _cnd(mask, src0, src1, xor):
    lanes = np.arange(64)
    return np.where(mask, src1, src0[lanes ^ xor])


def _stage(v, bit):
    """The butterfly stage that swaps lane bit `bit` with register bit `bit` (bit 0: masks EVEN / ODD; bit 1: masks LO / HI)."""
    lanes = np.arange(64)
    clear = (lanes >> bit) & 1 == 0
    x, o = 1 << bit, [None] * 4
    for lo_r in ((0, 2) if bit == 0 else (0, 1)):
        hi_r = lo_r + x
        o[lo_r] = _cnd(clear, v[hi_r], v[lo_r], x)        # lanes with the bit clear keep register lo_r, the others fetch hi_r across
        o[hi_r] = _cnd(~clear, v[lo_r], v[hi_r], x)
    return o


def test_both_butterfly_orders_give_the_in_quad_transpose():
    v = [np.array([100 * l + r for l in range(64)]) for r in range(4)]
    want = [np.array([100 * (4 * (l // 4) + r) + (l % 4) for l in range(64)]) for r in range(4)]      # out[r][4q + c] = in[c][4q + r]
    for order in ((0, 1), (1, 0)):
        got = v
        for bit in order:
            got = _stage(got, bit)
        for r in range(4):
            assert np.array_equal(got[r], want[r]), (order, r)
    # the masks a sequence hands on: order 0 ends on the complement of LO (bit 1 set), order 1 ends on the complement of ODD = EVEN
    EVEN, ODD, LO = 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x3333333333333333
    full = (1 << 64) - 1
    assert (~ODD) & full == EVEN and (~LO) & full == 0xCCCCCCCCCCCCCCCC
