"""Multiple-shooting segments in parallel (solver.segment_parallel) on the generic kernels: K0 and K5 on a tiles x chunks launch grid.

The option changes where the work runs, never what is computed.  So every result is held against two yardsticks:
  - the references of tests/test_gpu_segments.py (Euler: the fp32 CPU oracle on the slices; every other formula: the float64 walk with
    the same segment), under helpers.TOL_GPU on traj_rel_err; gradients: torch autograd through the float64 walk, each tensor within 1e-5
    of its own max, two runs bit for bit the same;
  - the sequential run (the same solver without the option), bit for bit: xs, is, and the gradients of x_init, z, v and the jump rows --
    the arithmetic of a segment does not depend on the workgroup that runs it.  The parameter gradients and all_initial's are sums over
    tiles x chunks partials in another order: within the same 1e-5 of the sequential run's.
Cases: tests/segment_cases.py (B = 33, w in {1, 3, 7, 100}, events at steps 0, 3, 4) at T = 8 and T = 12, with g in {2, 3, 100, "auto"}:
w = 3, g = 3 puts the event of step 3 on a chunk start; w = 1, g = 3 gives chunks of 3, 3, 1 segments; g = 100 one segment per chunk;
T = 12, w = 2, g = 4 three chunks of two segments, the last chunk and the last segment short."""
import warnings

import pytest
import torch

import generic_cases as C
import segment_cases as S
import test_gpu_segments as TS
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib, fused

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-5
B0 = S.B0
GS = (2, 3, 100, "auto")
RECORDS = tuple((Tn, w) for Tn in (8, 12) for w in S.WS) + ((12, 2),)
assert fused.segment_chunks(12, 2, 4)[1] == [(0, 4), (4, 8), (8, 11)]


def _solver(name, w, n=1, g=None, mode="require", kernel="auto"):
    s = S.SOLVERS[name](substeps=n, segment=w, segment_parallel=g)
    s.fused, s.kernel = mode, kernel
    return s


def _factory(name, w, n, g):
    return lambda mode: _solver(name, w, n, g, mode)


def _chunks(Tn, w, g):
    """the chunks the call runs on: "auto" on this device resolves as the package resolves it"""
    if g == "auto":
        g = fused.auto_segment_groups(B0, torch.cuda.get_device_properties(0).multi_processor_count)
    return len(fused.segment_chunks(Tn, w, g)[1])


# ----------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(C.ODE_FWD_SHAPES))
def test_k0_ode_forward(shape, name, n):
    """every form of K0 -- register, streamed, wide register, the eight-layer instances"""
    xd, zd, hidden = C.ODE_FWD_SHAPES[shape]
    for Tn in (8, 12):
        de, t, x, z, ev, zj = S.ode_case(xd, zd, hidden, Tn=Tn, seed=3 + xd + n, t=C.dyadic_clock(Tn, B0, n))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            for T_, w in RECORDS:
                if T_ != Tn:
                    continue
                ref = TS._ode_reference(name, n, w, de, t, x, z, ev, zj)
                seq = C.ode_gpu(_solver(name, w, n), de, t, x, z, ev, zj)
                for g in GS:
                    out = C.ode_gpu(_solver(name, w, n, g), de, t, x, z, ev, zj)
                    e = traj_rel_err(out.cpu(), ref)
                    print(shape, name, n, Tn, w, g, f"chunks {_chunks(Tn, w, g)} err {e:.3e} equal {torch.equal(out, seq)}")
                    assert out.shape == x.shape and torch.isfinite(out).all() and e <= TOL_GPU
                    assert torch.equal(out, seq), (shape, name, n, Tn, w, g)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["euler", "rk4", "Kutta3"])
@pytest.mark.parametrize("shape", list(C.DAE_SHAPES))
def test_k0_dae_forward(shape, name, n):
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES[shape]
    for Tn in (8, 12):
        case = S.dae_case(xd, zd, vd, idim, dh, ah, Tn=Tn, seed=7 + n, t=C.dyadic_clock(Tn, B0, n))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            for T_, w in RECORDS:
                if T_ != Tn:
                    continue
                rx, ri = TS._dae_reference(name, n, w, case)
                sx, si = C.dae_gpu(_solver(name, w, n), case)
                for g in GS:
                    gx, gi = C.dae_gpu(_solver(name, w, n, g), case)
                    ex, ei = traj_rel_err(gx.cpu(), rx), traj_rel_err(gi.cpu(), ri)
                    print(shape, name, n, Tn, w, g, f"chunks {_chunks(Tn, w, g)} xs {ex:.3e} is {ei:.3e} equal {torch.equal(gx, sx)} {torch.equal(gi, si)}")
                    assert torch.isfinite(gx).all() and torch.isfinite(gi).all() and ex <= TOL_GPU and ei <= TOL_GPU
                    assert torch.equal(gx, sx) and torch.equal(gi, si), (shape, name, n, Tn, w, g)


@pytest.mark.parametrize("edge", ["ragged", "T1", "T2", "B16", "B1"])
def test_forward_edges(edge):
    """T = 1, T = 2 (one chunk: the sequential call), one and exactly sixteen trajectories, ragged -1-padded clocks; the inputs are views of
    allocations whose next row is NaN, so a read past the last grid point shows in the outputs"""
    Tn = {"T1": 1, "T2": 2}.get(edge, 12)
    B = {"B16": 16, "B1": 1}.get(edge, B0)
    pad = edge == "ragged"
    de, t, x, z, ev, zj = S.ode_case(8, 2, (64, 64, 64), B=B, Tn=Tn, seed=50, pad=pad)
    xd, zd, vd, idim, dh, ah = C.DAE_SHAPES["x5z4v6i6"]
    case = S.dae_case(xd, zd, vd, idim, dh, ah, B=B, Tn=Tn, seed=51, pad=pad)
    for name, n in (("rk4", 1), ("euler", 2)):
        for w in (1, 3, 100):
            ref = S.walk_ode(name, n, w, de, t, x, z, ev, zj)
            rx, ri = S.walk_dae(name, n, w, case)
            for g in (3, "auto"):
                xc, zc = TS._canary(x), TS._canary(z)
                assert torch.isnan(xc._base[Tn]).all() and xc._base.is_cuda and xc.data_ptr() == xc._base.data_ptr()
                with torch.no_grad():
                    args = (C.deepcopy(de).cuda(), t.cuda(), xc, zc, torch.cat((xc[0], zc[0]), -1), C.to_cuda(ev), C.to_cuda(zj))
                    out = C.run_ode(_solver(name, w, n, g), *args)
                    seq = C.run_ode(_solver(name, w, n), *args)
                assert out.shape == x.shape and not torch.isnan(out).any() and torch.equal(out, seq)
                C.close(out, ref, f"{edge} ode {name} n={n} w={w} g={g}", TOL_GPU)
                dz = tuple(TS._canary(q) for q in case[3:6]) + tuple(C.to_cuda(q) for q in case[6:])
                with torch.no_grad():
                    mods = (C.deepcopy(case[0]).cuda(), C.deepcopy(case[1]).cuda(), case[2].cuda())
                    gx, gi = C.run_dae(_solver(name, w, n, g), *mods, *dz)
                    sx, si = C.run_dae(_solver(name, w, n), *mods, *dz)
                assert not torch.isnan(gx).any() and not torch.isnan(gi).any() and torch.equal(gx, sx) and torch.equal(gi, si)
                C.close(gx, rx, f"{edge} dae xs {name} n={n} w={w} g={g}", TOL_GPU)
                C.close(gi, ri, f"{edge} dae is {name} n={n} w={w} g={g}", TOL_GPU)


# ----------------------------------------------------------------------------- 2. training
K5_ODE_PATHS = TS.K5_ODE_PATHS
TRAIN_GRID = [("euler", 1), ("Heun2", 2), ("RK4Classic", 1)]
# (T, w, events, the g's): every one splits into more than one chunk
TRAIN_RUNS = [(8, 3, True, (3, "auto")), (8, 1, True, (3,)), (12, 2, True, (4,)), (12, 7, True, (100,)), (8, 3, False, (2,))]
BITWISE_ODE, BITWISE_DAE = ("x_init", "z", "zj"), ("x_init", "z", "v", "zj", "vj")


def _against_the_sequential_run(got, seq, bitwise, what):
    for k, g in got.items():
        if k in bitwise:
            assert C._same_bits(g, seq[k]), f"{what}: grad {k} is not the sequential run's bit for bit"
        else:          # the parameters and all_initial: the same sums in another order
            C.close(g, None if seq[k] is None else seq[k].double().cpu(), f"{what} grad {k} vs sequential", GRAD_TOL)


def _ode_training(name, n, Tn, w, gs, case, G, what):
    ref_xs, ref = S.ode_train(_factory(name, w, n, None), case, G, "cpu")          # (the walk ignores the option)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        seq_xs, seq = S.ode_train(_factory(name, w, n, None), case, G, "cuda")
        out = {}
        for g in gs:
            assert _chunks(Tn, w, g) > 1
            xs, got = S.ode_train(_factory(name, w, n, g), case, G, "cuda")
            _, again = S.ode_train(_factory(name, w, n, g), case, G, "cuda")
            C.judge_ode_training(ref, got, again, xs, ref_xs, "_FusedOdeMsp", GRAD_TOL, f"{what} g={g}")
            assert torch.equal(xs, seq_xs)
            _against_the_sequential_run(got, seq, BITWISE_ODE, f"{what} g={g}")
            out[g] = got
    return out


def _dae_training(name, n, Tn, w, gs, case, G, Gi, what):
    rx, ri, ref = C.dae_train(_factory(name, w, n, None), case, G, Gi, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sx, si, seq = C.dae_train(_factory(name, w, n, None), case, G, Gi, "cuda")
        out = {}
        for g in gs:
            assert _chunks(Tn, w, g) > 1
            xs, is_, got = C.dae_train(_factory(name, w, n, g), case, G, Gi, "cuda")
            _, _, again = C.dae_train(_factory(name, w, n, g), case, G, Gi, "cuda")
            C.judge_dae_training(ref, got, again, (xs, is_), (rx, ri), "_FusedDaeMsp", GRAD_TOL, f"{what} g={g}")
            assert torch.equal(xs, sx) and torch.equal(is_, si)
            _against_the_sequential_run(got, seq, BITWISE_DAE, f"{what} g={g}")
            out[g] = got
    return out


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("path", list(K5_ODE_PATHS))
def test_k5_ode_training_per_path(path, name, n):
    xd, zd, h, nl = K5_ODE_PATHS[path]
    for Tn, w, events, gs in TRAIN_RUNS:
        case = S.ode_case(xd, zd, (h,) * nl, Tn=Tn, seed=23, events=events)
        G, = C.cotangents(21, case[2].shape)
        _ode_training(name, n, Tn, w, gs, case, G, f"{path} T={Tn} events={events} w={w}")


@pytest.mark.parametrize("name,n", TRAIN_GRID)
@pytest.mark.parametrize("shape", list(C.K5_DAE_SHAPES))
def test_k5_dae_training_every_shape(shape, name, n):
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES[shape]
    for Tn, w, events, gs in TRAIN_RUNS:
        case = S.dae_case(xd, zd, vd, idim, dh, ah, Tn=Tn, seed=24, events=events)
        G, Gi = C.cotangents(22, (Tn, B0, xd), case[6].shape)
        _dae_training(name, n, Tn, w, gs, case, G, Gi, f"{shape} T={Tn} events={events} w={w}")


def test_a_loss_on_the_first_chunk_alone():
    """T = 12, w = 2, g = 4: chunk 0 is the steps 0 .. 3, rows 1 .. 4.  A loss on rows 0 .. 4 leaves every input gradient beyond row 3
    exactly zero (row 4 of z | v feeds step 4, chunk 1's first), and reaches x_init; the later chunks' partials of all_initial and their
    border slots add exact zeros."""
    Tn, w, g = 12, 2, 4
    ode = S.ode_case(8, 2, (64, 64, 64), Tn=Tn, seed=27, events=False)
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = S.dae_case(xd, zd, vd, idim, dh, ah, Tn=Tn, seed=28, events=False)
    G, = C.cotangents(31, ode[2].shape)
    Gd, Gi = C.cotangents(32, (Tn, B0, xd), dae[6].shape)
    head = torch.zeros(Tn, 1, 1)
    head[:5] = 1.0
    got = _ode_training("RK4Classic", 1, Tn, w, (g,), ode, G * head, "ode chunk 0")[g]
    S.rows_beyond_are_zero(got, ("z",), 3, "ode chunk 0")
    assert got["x_init"].abs().sum() > 0 and got["z"][:4].abs().sum() > 0
    for name, n in (("RK4Classic", 1), ("euler", 2)):
        got = _dae_training(name, n, Tn, w, (g,), dae, Gd * head, Gi * head, f"dae chunk 0 {name}")[g]
        # (the head at grid point 4 reads z | v of row 4: its adjoint is chunk 0's border slot, folded onto the row chunk 1 wrote)
        S.rows_beyond_are_zero(got, ("z", "v"), 4, f"dae chunk 0 {name}")
        assert got["x_init"].abs().sum() > 0 and got["z"][4].abs().sum() > 0


# ----------------------------------------------------------------------------- 3. routing
def test_routing_on_the_device():
    de, t, x, z, ev, zj = S.ode_case(8, 2, (64, 64, 64), seed=32)
    a0 = torch.cat((x[0], z[0]), -1).cuda()
    x0 = x[0].cuda().requires_grad_(True)
    run = lambda s: s.integrate_ODE(x_func=C.deepcopy(de).cuda(), t=t.cuda(), x=x.cuda(), z=z.cuda(), all_initial=a0, x_init=x0)
    # one chunk (w = 7 at T = 8 is one segment; g = 1) is the sequential family, more than one the new one
    assert type(run(_solver("rk4", 7, g=3)).grad_fn).__name__ == "_FusedOdeMsBackward"
    assert type(run(_solver("rk4", 3, g=1)).grad_fn).__name__ == "_FusedOdeMsBackward"
    assert type(run(_solver("rk4", 100, g="auto")).grad_fn).__name__ == "_FusedOdeMsBackward"
    assert type(run(_solver("rk4", 3, g=3)).grad_fn).__name__ == "_FusedOdeMspBackward"
    assert type(run(_solver("rk4", 1, g="auto")).grad_fn).__name__ == "_FusedOdeMspBackward"
    xd, zd, vd, idim, dh, ah = C.K5_DAE_SHAPES["reg"]
    dae = S.dae_case(xd, zd, vd, idim, dh, ah, seed=33)
    xs, _, _ = C.dae_train(_factory("rk4", 7, 1, 3), dae, *C.cotangents(35, (S.T0, B0, xd), dae[6].shape), "cuda")
    assert type(xs.grad_fn).__name__ == "_FusedDaeMsBackward"
    xs, _, _ = C.dae_train(_factory("rk4", 3, 1, 3), dae, *C.cotangents(35, (S.T0, B0, xd), dae[6].shape), "cuda")
    assert type(xs.grad_fn).__name__ == "_FusedDaeMspBackward"
    # every refusal of segment applies unchanged
    ode = (de, t, x, z, ev, zj)
    ref = S.walk_ode("rk4", 1, 3, *ode)
    for kernel in ("wave", "tile", "mfma", "wide"):
        with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
            C.ode_gpu(_solver("rk4", 3, g=3, kernel=kernel), *ode)
        with pytest.warns(RuntimeWarning, match="not fusable"):
            out = C.ode_gpu(_solver("rk4", 3, g=3, mode="auto", kernel=kernel), *ode)
        assert traj_rel_err(out.cpu(), ref) <= TOL_GPU          # the walk, which ignores the option
    assert traj_rel_err(C.ode_gpu(_solver("rk4", 3, g=3, kernel="generic"), *ode).cpu(), ref) <= TOL_GPU
    lin = S.SOLVERS["rk4"](segment=3, segment_parallel=3, externals="linear")
    lin.fused = "require"
    with pytest.raises(_lib.UnsupportedShapeError, match="externals='linear'"):
        C.ode_gpu(lin, *ode)
    with pytest.raises(ValueError, match="segment"):
        C.run_ode(_solver("rk4", 3, g=3), C.deepcopy(de).cuda(), t.cuda(), x.cuda(), z.cuda(), a0, ev.cuda(), zj.cuda(), tx=True)
    xg = x.cuda().requires_grad_(True)          # a dataset x that requires grad and restarts: refused under "require"
    with pytest.raises(S.nd.NotFusableError, match="segment"):
        C.run_ode(_solver("rk4", 3, g=3), C.deepcopy(de).cuda(), t.cuda(), xg, z.cuda(), a0, ev.cuda(), zj.cuda())
