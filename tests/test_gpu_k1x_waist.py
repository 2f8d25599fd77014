"""The waist of K1x's stage (64 -> x_dim -> 64): the output layer on the B operand's lane-group broadcast (8 blocks per dim to fold instead
of 16) and the RK arithmetic on one register pair, forced (`kernel="wave"`) against the fp64 oracle at the project's gate (helpers.TOL_GPU,
per trajectory).

Routing: W4 zero except ONE weight, for every (dim, k) on an edge of the register image (first / last k of a block, of a half, of the matrix;
first / last dim of a dim-tile) -- a wrong lane of the image is a missing or doubled contribution, far outside the gate.
Shapes: hidden <= 32 leaves the upper half of k empty, x_dim <= 4 the second dim-tile, odd x_dim takes the general loop, B 1 / 5 leave
invalid lanes in a quad, T 2 / 3 / 6 are the peeled last step and both parities of the loop unrolled by two; every case also runs with one
event and with teacher forcing (the general loop).  Saving forward: the rows it returns and saves against the 4-wave tile kernel's, by the
measure of test_gpu_backward.py (the two kernels sum in different orders: equal to rounding, not bit for bit), and against the oracle."""
import itertools

import pytest
import torch

from helpers import TOL_GPU, traj_rel_err as rel_err
from oracle import psnode_oracle as O

METHODS = ("rk4", "midpoint", "euler")


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


# ---- L4 routing, one weight at a time
EDGE_K, EDGE_D = (0, 3, 4, 28, 31, 32, 35, 60, 63), (0, 3, 4, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("zd", [0, 2])
@pytest.mark.parametrize("d,k", list(itertools.product(EDGE_D, EDGE_K)) + [(-1, -1)], ids=lambda v: str(v))
def test_l4_routes_one_weight_to_its_dim(d, k, zd):
    """(d, k) = (-1, -1): one dense random W4."""
    ls, t, x, z, a0 = _ode(4, 2, 8, zd, 64, seed=900 + zd)
    if d >= 0:
        w4 = torch.zeros_like(ls[3][0])
        w4[d, k] = 1.0
        ls[3] = (w4, ls[3][1])
    ref = _oracle64("euler", ls, t, x, z, a0)
    out = _run("euler", ls, t, x, z, a0, "wave").cpu()
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) <= TOL_GPU


# ---- shapes where a half of k or a dim-tile is empty or ragged
HS, XDS, BS, TS = (1, 20, 32, 33, 64), (1, 2, 4, 5, 7, 8), (1, 5, 8), (2, 3, 6)
BT = list(itertools.product(BS, TS))
# every (hidden, x_dim) pair; (B, T) cycles with the case number so that every pair of them occurs with every method
SHAPES = [(H, xd) + BT[n % len(BT)] for n, (H, xd) in enumerate(itertools.product(HS, XDS))]


def _variants(t, B, Tn, zd, seed):
    """Plain, one event (at the start of the last step), teacher forcing."""
    g = torch.Generator().manual_seed(seed)
    ev = torch.full((B, 2, 1), -1.0)
    ev[:, 0] = t[Tn - 2]
    zj = 0.1 * torch.randn(B, 2, zd, generator=g)
    return (dict(), dict(event_t=ev, z_jump=zj), dict(input_true_x=True))


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H,xd,B,Tn", SHAPES, ids=lambda v: str(v))
def test_ragged_halves_and_tiles_vs_fp64_oracle(H, xd, B, Tn, method):
    zd = 2
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=1000 + 97 * H + 11 * xd + 3 * B + Tn)
    for kw in _variants(t, B, Tn, zd, seed=H + xd):
        ref = _oracle64(method, ls, t, x, z, a0, **kw)
        out = _run(method, ls, t, x, z, a0, "wave", **kw).cpu()
        assert torch.isfinite(out).all(), sorted(kw)
        assert rel_err(out, ref) <= TOL_GPU, sorted(kw)


# ---- the saving forward (the SAVE instances share rhs and the pack)
def _close(a, b, what, tol=1e-4):
    """test_gpu_backward.py's measure: max abs error against the other side's max abs value."""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("H,xd,B,Tn", SHAPES, ids=lambda v: str(v))
def test_saving_forward_rows_vs_tile_and_oracle(H, xd, B, Tn, method):
    zd = 2
    ls, t, x, z, a0 = _ode(B, Tn, xd, zd, H, seed=2000 + 97 * H + 11 * xd + 3 * B + Tn)
    ref = _oracle64(method, ls, t, x, z, a0)
    xs_w, sv_w = _run(method, ls, t, x, z, a0, "wave", save=True)
    xs_t, sv_t = _run(method, ls, t, x, z, a0, "tile", save=True)
    assert rel_err(xs_w.cpu(), ref) <= TOL_GPU
    assert sv_w[0].shape == sv_t[0].shape and sv_w[1].shape == sv_t[1].shape
    assert torch.equal(sv_w[1][0, 0].cpu(), x[0]), "the first stage input is the start row, bit for bit"
    _close(sv_w[1], sv_t[1], "saved stage inputs")
    _close(sv_w[0], sv_t[0], "saved activations")
    if H < sv_w[0].shape[-1]:
        assert float(sv_w[0][..., H:].abs().max()) == 0.0, "padding units are stored as zeros"
