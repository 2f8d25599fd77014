"""K1x's first layer in the operand-swapped form (A = weights, B = the state on the B operand's row broadcast, BLGP 4 + row): its accumulator
is already the next layer's A layout, so no in-quad transpose follows it, and the external slots ride the same broadcast (slot q in row q & 3
of register q >> 2).  Forced (`kernel="wave"`) against the fp64 oracle and against the 4-wave tile kernel (`kernel="tile"`), both at the
project's gate (helpers.TOL_GPU, per trajectory).

Shapes, the smallest at which the layout can go wrong: x_dim 1..8 (odd widths leave X23 empty in a row, x_dim <= 2 uses one row only, 8 uses
all four BLGP values) x z_dim {0, 1, 2, 3, 5, 8} (0..4 external registers: slots across more than one register, and slot q >= z_dim in another
row than its twin); B 1 / 3 / 4 / 5 / 9 leave invalid lanes in the last wave; T 2 / 3 / 6 are the peeled last step and both clock slots;
hidden 20 / 64.  (B, T) cycle with the case number, hidden alternates so that every x_dim and every z_dim meets both widths.  Every case
runs plain, with teacher forcing and -- where there is a z to jump -- with one event inside the grid (the general loop).
Saving forward (B = 5): its trajectory against the plain call's and the oracle, its saved rows against the tile kernel's by the measure of
test_gpu_backward.py (the two kernels sum in different orders: equal to rounding, not bit for bit)."""
import itertools

import pytest
import torch

from helpers import TOL_GPU, traj_rel_err as rel_err
from oracle import psnode_oracle as O

METHODS = ("rk4", "midpoint", "euler")
HS, XDS, ZDS, BS, TS = (20, 64), (1, 2, 3, 4, 5, 6, 7, 8), (0, 1, 2, 3, 5, 8), (1, 3, 4, 5, 9), (2, 3, 6)
BT = list(itertools.product(BS, TS))
CASES = [(HS[(ix + iz) % 2], xd, zd) + BT[(ix * len(ZDS) + iz) % len(BT)] for ix, xd in enumerate(XDS) for iz, zd in enumerate(ZDS)]
# the saving forward at B = 5: every x_dim, every z_dim, both widths, every T
SAVE_CASES = [(HS[(n // 2) % 2], XDS[n % 8], ZDS[n % 6], 5, TS[(n // 4) % 3]) for n in range(12)]


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
                                  **{k: c(v) for k, v in kw.items()})


def _variants(t, B, Tn, zd, seed):
    """Plain, teacher forcing, and (z_dim > 0) one event at the start of the last step: inside the grid, so the call takes the general loop."""
    vs = [dict(), dict(input_true_x=True)]
    if zd:
        g = torch.Generator().manual_seed(seed)
        ev = torch.full((B, 2, 1), -1.0)
        ev[:, 0] = t[Tn - 2]
        vs.append(dict(event_t=ev, z_jump=0.1 * torch.randn(B, 2, zd, generator=g)))
    return vs


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H,xd,zd,B,Tn", CASES, ids=lambda v: str(v))
def test_swapped_first_layer_vs_fp64_oracle_and_tile(H, xd, zd, B, Tn, method):
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=3000 + 97 * H + 11 * xd + 5 * zd + 3 * B + Tn)
    for kw in _variants(t, B, Tn, zd, seed=H + xd + zd):
        ref = _oracle64(method, ls, t, x, z, a0, **kw)
        wave = _run(method, ls, t, x, z, a0, "wave", **kw).cpu()
        tile = _run(method, ls, t, x, z, a0, "tile", **kw).cpu()
        assert torch.isfinite(wave).all(), sorted(kw)
        e_ref, e_tile = rel_err(wave, ref), rel_err(wave, tile)
        print(f"{sorted(kw)}: wave vs oracle {e_ref:.3e}, wave vs tile {e_tile:.3e}")
        assert e_ref <= TOL_GPU, sorted(kw)
        assert e_tile <= TOL_GPU, sorted(kw)


def _close(a, b, what, tol=1e-4):
    """test_gpu_backward.py's measure: max abs error against the other side's max abs value."""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H,xd,zd,B,Tn", SAVE_CASES, ids=lambda v: str(v))
def test_saving_forward_vs_plain_and_saved_rows_vs_tile(H, xd, zd, B, Tn, method):
    """The saved first-layer row is the post-ELU accumulator as it stands (the A layout): lane (b, t) stores units 4b .. 4b + 3."""
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=4000 + 97 * H + 11 * xd + 5 * zd + Tn)
    ref = _oracle64(method, ls, t, x, z, a0)
    plain = _run(method, ls, t, x, z, a0, "wave").cpu()
    xs_w, sv_w = _run(method, ls, t, x, z, a0, "wave", save=True)
    xs_t, sv_t = _run(method, ls, t, x, z, a0, "tile", save=True)
    assert rel_err(xs_w.cpu(), ref) <= TOL_GPU
    assert rel_err(xs_w.cpu(), plain) <= TOL_GPU
    assert rel_err(xs_w.cpu(), xs_t.cpu()) <= TOL_GPU
    assert sv_w[0].shape == sv_t[0].shape and sv_w[1].shape == sv_t[1].shape
    assert torch.equal(sv_w[1][0, 0].cpu(), x[0]), "the first stage input is the start row, bit for bit"
    _close(sv_w[1], sv_t[1], "saved stage inputs")
    _close(sv_w[0], sv_t[0], "saved activations")
    if H < sv_w[0].shape[-1]:
        assert float(sv_w[0][..., H:].abs().max()) == 0.0, "padding units are stored as zeros"
