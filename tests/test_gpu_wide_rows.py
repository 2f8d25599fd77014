"""K11 (csrc/psnode_linear_rows.hip) and the row MLPs built on it (round 6): the encoders / decoders of the direct_encode models at the
hidden widths K3b does not carry -- the scripts' argparse default --hidden 128 (neural_00_ODE_02_direct_encode.py:64-69, 160-162) --
forward and backward without a library GEMM, against torch in fp64."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _err(a, b):
    b = b.double().cpu()
    return float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-6)


@pytest.mark.parametrize("rows", [1, 33, 1000])
@pytest.mark.parametrize("K,N", [(128, 128), (8, 128), (2, 128), (128, 8), (128, 2), (16, 16), (100, 36), (20, 100), (5, 7)])
@pytest.mark.parametrize("transposed", [False, True])
def test_linear_rows_matches_fp64(rows, K, N, transposed):
    from py_psnode_amd import fused
    g = torch.Generator().manual_seed(rows + 17 * K + N)
    X = torch.randn(rows, K, generator=g).cuda()
    W = (torch.randn(K, N, generator=g) if transposed else torch.randn(N, K, generator=g)).cuda() * 0.3
    b = torch.randn(N, generator=g).cuda()
    H = (torch.randn(rows, N, generator=g).cuda() * 0.7)
    Hh = torch.nn.functional.elu(H)
    Wm = W.t() if transposed else W
    pre = X.double() @ Wm.double().t() + b.double()
    assert _err(fused.linear_rows(X, W, b, transposed=transposed), pre) <= 2e-6
    assert _err(fused.linear_rows(X, W, b, epi=1, transposed=transposed), torch.nn.functional.elu(pre)) <= 2e-6
    dgrad = torch.where(H.double() > 0, torch.ones_like(H.double()), H.double().exp())
    nob = X.double() @ Wm.double().t()
    assert _err(fused.linear_rows(X, W, None, epi=2, hh=Hh, transposed=transposed), nob * dgrad) <= 5e-6


@pytest.mark.parametrize("din,H,dout,need_gin", [(8, 128, 128, False), (2, 128, 128, False), (128, 128, 8, True), (128, 128, 2, True), (8, 100, 100, False),
                                                 (100, 100, 8, True), (3, 36, 36, True)])
def test_wide_row_mlp_autograd_matches_torch_fp64(din, H, dout, need_gin):
    """fused.mlp_rows_autograd at the widths K3b does not carry: forward and every gradient against the same nn.Sequential in fp64, on a
    time-major VIEW of a [B,T,D] batch (what the models pass) and with a non-trivial upstream gradient."""
    from py_psnode_amd import fused
    torch.manual_seed(din * 7 + H + dout)
    seq = nn.Sequential(nn.Linear(din, H), nn.ELU(), nn.Linear(H, dout)).cuda()
    ref = nn.Sequential(nn.Linear(din, H), nn.ELU(), nn.Linear(H, dout)).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in seq.state_dict().items()})
    B, T = 37, 23
    x_bt = (0.5 * torch.randn(B, T, din)).cuda()
    x = x_bt.permute(1, 0, 2).detach().requires_grad_(need_gin)
    xr = x_bt.permute(1, 0, 2).double().cpu().detach().requires_grad_(need_gin)
    G = torch.randn(T, B, dout).cuda()
    assert fused.rows_layers_of(seq, x, allow_grad=True) is not None
    y = fused.mlp_rows_autograd(seq, x)
    yr = ref(xr)
    assert y.shape == (T, B, dout) and _err(y, yr) <= 5e-6
    (y * G).sum().backward()
    (yr * G.double().cpu()).sum().backward()
    for (n1, p), (_, q) in zip(seq.named_parameters(), ref.named_parameters()):
        assert _err(p.grad, q.grad) <= 2e-5, n1
    if need_gin:
        assert _err(x.grad, xr.grad) <= 2e-5
    with torch.no_grad():       # the no-grad route: K11 twice, no autograd node
        y2 = fused.mlp_rows(fused.sequential_layers(seq), x.detach())
    assert torch.equal(y2, y.detach())


def _offset4(*shape):
    """A contiguous tensor of `shape` whose storage starts 4 bytes past a 16-byte boundary (what a slice of a larger tensor gives)."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.empty(n + 4, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat[1:1 + n].view(*shape)


@pytest.mark.parametrize("din,H,dout", [(8, 16, 16), (2, 64, 64), (64, 64, 8),                                # K3b (+ its fused backward)
                                        (3, 36, 36), (100, 100, 8), (8, 128, 128), (128, 128, 2)])        # K11 / K10
@pytest.mark.parametrize("case", ["expand_11d", "expand_1bd", "grad_bcast", "grad_sum", "col_slice", "offset4"])
def test_row_mlp_autograd_on_broadcast_strided_and_misaligned_operands_matches_fp64(din, H, dout, case):
    """fused.mlp_rows_autograd on both row routes with the operands a caller can hand it besides a dense batch: a broadcast input
    (`expand` of [1, 1, din] / [1, B, din]: stride-0 rows, its gradient summed over them), a broadcast upstream gradient
    ((y.sum((0, 1)) * w).sum(): strides (0, 0, 1); y.sum(): all strides 0), a row-strided input (a column slice of a wider tensor) and
    an input 4 bytes off a 16-byte boundary.  Forward and every gradient against the same nn.Sequential in fp64."""
    from py_psnode_amd import fused
    from py_psnode_amd.fused import rows
    torch.manual_seed(din * 7 + H + dout)
    seq = nn.Sequential(nn.Linear(din, H), nn.ELU(), nn.Linear(H, dout)).cuda()
    ref = nn.Sequential(nn.Linear(din, H), nn.ELU(), nn.Linear(H, dout)).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in seq.state_dict().items()})
    T, B = 23, 37
    lead = {"expand_11d": (1, 1), "expand_1bd": (1, B)}.get(case, (T, B))
    base = 0.5 * torch.randn(*lead, din + (4 if case == "col_slice" else 0))
    if case == "offset4":
        leaf = _offset4(*base.shape)
        with torch.no_grad():
            leaf.copy_(base)
        leaf.requires_grad_(True)
    else:
        leaf = base.cuda().requires_grad_(True)
    leaf_r = base.double().requires_grad_(True)

    def operand(a):
        a = a[..., :din] if case == "col_slice" else a
        return a.expand(T, B, din) if case.startswith("expand") else a

    x, xr = operand(leaf), operand(leaf_r)
    assert fused.rows_layers_of(seq, x, allow_grad=True) is not None
    assert rows._k3b_class(fused.sequential_layers(seq)) == (H in (16, 64))
    y, yr = fused.mlp_rows_autograd(seq, x), ref(xr)
    assert y.shape == (T, B, dout) and _err(y, yr) <= 5e-6
    w = torch.randn(dout)
    G = torch.randn(T, B, dout)
    loss = {"grad_bcast": lambda a, w_, G_: (a.sum(dim=(0, 1)) * w_).sum(), "grad_sum": lambda a, w_, G_: a.sum()}.get(
        case, lambda a, w_, G_: (a * G_).sum())
    loss(y, w.cuda(), G.cuda()).backward()
    loss(yr, w.double(), G.double()).backward()
    for (n1, p), (_, q) in zip(seq.named_parameters(), ref.named_parameters()):
        assert _err(p.grad, q.grad) <= 2e-5, n1
    assert _err(leaf.grad, leaf_r.grad) <= 2e-5


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("K,N", [(128, 128), (36, 36), (5, 8), (16, 100)])
@pytest.mark.parametrize("rows", [1, 33, 1000])
def test_linear_rows_into_misaligned_rows_matches_fp64(epi, K, N, rows):
    """linear_rows with X, Hh and Y all 4 bytes off a 16-byte boundary and row strides that are multiples of 4 (the float4 paths of
    K11 must not take them), Y written into a wider buffer: the result against fp64 and every element outside Y's view untouched."""
    from py_psnode_amd import fused
    g = torch.Generator().manual_seed(rows + 13 * K + N + epi)
    ld = N + 4
    X = _offset4(rows, K)
    X.copy_(torch.randn(rows, K, generator=g))
    W = (0.3 * torch.randn(N, K, generator=g)).cuda()
    b = torch.randn(N, generator=g).cuda()
    Hpre = 0.7 * torch.randn(rows, N, generator=g)
    Hh = _offset4(rows, ld)[:, :N]
    Hh.copy_(torch.nn.functional.elu(Hpre))
    ybuf = _offset4(rows, ld)
    ybuf.fill_(float("nan"))
    Y = ybuf[:, :N]
    assert Y.data_ptr() % 16 == 4 and Hh.data_ptr() % 16 == 4 and X.data_ptr() % 16 == 4 and Y.stride(0) % 4 == 0
    pre = X.double().cpu() @ W.double().cpu().t()
    if epi != 2:
        pre = pre + b.double().cpu()
    want = {0: pre, 1: torch.nn.functional.elu(pre), 2: pre * torch.where(Hpre.double() > 0, 1.0, Hpre.double().exp())}[epi]
    r = fused.linear_rows(X, W, b if epi != 2 else None, epi=epi, hh=Hh if epi == 2 else None, out=Y)
    assert r.data_ptr() == Y.data_ptr()
    assert _err(Y, want) <= (5e-6 if epi == 2 else 2e-6)
    assert bool(ybuf[:, N:].isnan().all())


def test_linear_rows_and_row_mlps_refuse_foreign_operands_before_any_launch():
    """Wrong dtype, device or width: linear_rows raises before it launches; through a module the plain nn.Sequential runs and torch
    reports what it always did."""
    from py_psnode_amd import fused, models
    x = torch.randn(33, 36, device="cuda")
    W, b = torch.randn(20, 36, device="cuda"), torch.randn(20, device="cuda")
    with pytest.raises(TypeError):
        fused.linear_rows(x, W.double(), b)
    with pytest.raises(TypeError):
        fused.linear_rows(x, W, b.double())
    with pytest.raises(ValueError):
        fused.linear_rows(x, W.cpu(), b)
    with pytest.raises(ValueError):
        fused.linear_rows(x, W, b.cpu())
    with pytest.raises(ValueError):
        fused.linear_rows(torch.randn(33, 40, device="cuda"), W, b)          # wider rows than W takes: no read past W
    with pytest.raises(ValueError):
        fused.linear_rows(x, W, b[:19])
    with pytest.raises(ValueError):
        fused.linear_rows(x, W, None, epi=2, hh=torch.randn(33, 20, device="cuda").cpu())
    torch.cuda.synchronize()
    for H in (16, 36, 128):          # K3b and K11 widths
        seq = nn.Sequential(nn.Linear(36 if H != 16 else 8, H), nn.ELU(), nn.Linear(H, 8)).cuda()
        din = seq[0].in_features
        xin = torch.randn(5, 7, din, device="cuda")
        for bad, a in (("fp64 params", xin), ("cpu params", xin), ("width", torch.randn(5, 7, din + 4, device="cuda"))):
            s2 = models.RowsSequential(*copy.deepcopy(seq))
            s2 = s2.double() if bad == "fp64 params" else (s2.cpu() if bad == "cpu params" else s2)
            assert fused.rows_layers_of(s2, a, allow_grad=True) is None, (H, bad)
            with pytest.raises(RuntimeError) as got:
                s2(a)
            with pytest.raises(RuntimeError) as want:
                nn.Sequential.forward(s2, a)
            assert type(got.value) is type(want.value) and str(got.value) == str(want.value), (H, bad)


@pytest.mark.parametrize("din,H,dout", [(3, 36, 36), (8, 128, 128)])
def test_wide_row_mlp_backward_takes_library_products_when_k10_declines(din, H, dout, monkeypatch):
    """_WideRowsMlp.backward when gemm_tn answers None (outside K10's class): the weight gradients come from the library products
    instead of an unpack of None -- the same gradients as fp64."""
    from py_psnode_amd import fused
    from py_psnode_amd.fused import _common
    monkeypatch.setattr(_common, "gemm_tn", lambda *a, **k: None)
    torch.manual_seed(H)
    seq = nn.Sequential(nn.Linear(din, H), nn.ELU(), nn.Linear(H, dout)).cuda()
    ref = copy.deepcopy(seq).double().cpu()
    x = torch.randn(9, 11, din)
    G = torch.randn(9, 11, dout)
    (fused.mlp_rows_autograd(seq, x.cuda()) * G.cuda()).sum().backward()
    (ref(x.double()) * G.double()).sum().backward()
    for (n1, p), (_, q) in zip(seq.named_parameters(), ref.named_parameters()):
        assert _err(p.grad, q.grad) <= 2e-5, n1


def test_hidden128_model_training_step_has_no_library_gemm_in_its_row_mlps(monkeypatch):
    """models.ODE_Model(direct_encode, hidden 128): the encoders / decoders take the K11 / K10 route -- counted at _WideRowsMlp and at
    gemm_tn (never None) -- and both it and the plain nn.Sequential route match an fp64 CPU copy of the model (outputs per trajectory,
    gradients per tensor: 1e-5, the gate of test_grad_goldens.TOL_GPU), and each other to rounding."""
    from helpers import traj_rel_err
    from py_psnode_amd import fused, models
    from py_psnode_amd import neural_dae as nd
    from py_psnode_amd.fused import _common, rows
    torch.manual_seed(0)
    B, T = 24, 12
    m = models.ODE_Model(8, 2, 128, direct_encode=True, solver=nd.Euler())
    m64 = copy.deepcopy(m).double()
    m64.solver.fused = "off"
    m = m.cuda()
    m.solver.fused = "require"
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(1, T, 1).repeat(B, 1, 1)
    x, z = 0.1 * torch.randn(B, T, 8), 0.1 * torch.randn(B, T, 2)
    ev, zj = -torch.ones(B, 2, 1), torch.zeros(B, 2, 2)
    out64 = m64(t=t.double(), x=x.double(), z=z.double(), event_t=ev.double(), z_jump=zj.double())
    (out64[0].sum() + out64[1].sum()).backward()
    g64 = {n: p.grad for n, p in m64.named_parameters()}
    t, x, z, ev, zj = (a.cuda() for a in (t, x, z, ev, zj))
    n = {"rows": 0, "rows_bwd": 0, "k10": 0, "k10_none": 0, "in_bwd": False}
    fwd, bwd, gemm = rows._WideRowsMlp.forward, rows._WideRowsMlp.backward, _common.gemm_tn

    def counted_fwd(*a, **k):
        n["rows"] += 1
        return fwd(*a, **k)

    def counted_bwd(*a, **k):
        n["rows_bwd"] += 1
        n["in_bwd"] = True
        try:
            return bwd(*a, **k)
        finally:
            n["in_bwd"] = False

    def counted_gemm(*a, **k):
        r = gemm(*a, **k)
        if n["in_bwd"]:         # (the latent backward's contractions call it too)
            n["k10" if r is not None else "k10_none"] += 1
        return r

    with monkeypatch.context() as mp:
        mp.setattr(rows._WideRowsMlp, "forward", staticmethod(counted_fwd))
        mp.setattr(rows._WideRowsMlp, "backward", staticmethod(counted_bwd))
        mp.setattr(_common, "gemm_tn", counted_gemm)        # rows.py imports it at the call
        out = m(t=t, x=x, z=z, event_t=ev, z_jump=zj)
        (out[0].sum() + out[1].sum()).backward()
    # x / z encoders, x decoder: forward on K11, backward on K11 with both weight gradients on K10
    assert n["rows"] >= 3 and n["rows_bwd"] >= 3 and n["k10"] == 2 * n["rows_bwd"] and n["k10_none"] == 0, n
    g_fused = {k: p.grad.clone() for k, p in m.named_parameters()}
    # the same step with the row MLPs as plain modules (rows_layers_of refuses): library route
    m.zero_grad()
    with monkeypatch.context() as mp:
        mp.setattr(fused, "rows_layers_of", lambda *a, **k: None)
        mp.setattr(rows, "rows_layers_of", lambda *a, **k: None)
        mp.setattr(rows._WideRowsMlp, "forward", staticmethod(lambda *a, **k: pytest.fail("K11 on the library route")))
        out2 = m(t=t, x=x, z=z, event_t=ev, z_jump=zj)
        (out2[0].sum() + out2[1].sum()).backward()
    for route, o, g in (("fused", out, g_fused), ("library", out2, {k: p.grad for k, p in m.named_parameters()})):
        for k in range(2):
            assert traj_rel_err(o[k].detach().cpu(), out64[k].detach(), bdim=0) <= 1e-5, (route, k)
        for name, p in m64.named_parameters():
            assert _err(g[name], g64[name]) <= 1e-5, (route, name)
    assert _err(out[0], out2[0]) <= 2e-5 and _err(out[1], out2[1]) <= 2e-5
    for name, p in m.named_parameters():
        assert _err(g_fused[name], p.grad) <= 5e-4, name
