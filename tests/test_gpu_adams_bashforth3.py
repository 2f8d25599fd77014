"""Adams-Bashforth 3 on the generic kernels (nd.AB3 -> the _ab3 builds of K0 / K5), on the GPU: K0 forward in every form against the fp64
walk and next to the AB2 GPU run on the same rows, edge shapes, padded and 2 : 1 clocks, a NaN canary behind the grid, a restart on the last
step, per-trajectory hits in one workgroup alone; training against fp64 autograd through the walk (1e-5 of each tensor's max, the project's
gate; bitwise repeatable) on K5's paths, the right-row adjoint of the corrector on its own; the solver and the models under
fused = "require"; the refusals."""
import functools
import warnings
from copy import deepcopy

import pytest
import torch
import torch.nn as nn

import ab3_cases as A
import generic_cases as C
import pev_cases as P
from helpers import TOL_GPU, traj_rel_err
from py_psnode_amd import _lib, models
from py_psnode_amd import neural_dae as nd

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _ode(pattern, shape="reg", B=A.B0, Tn=A.T0, kind="ragged", act=nn.ELU):
    """(case, its fp64 walk): made once, never modified"""
    c = A.ode_case(pattern, shape, B, Tn, kind, act)
    return c, A.run_ode(A.solver("off"), c, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _dae(pattern, shape="x8z2v2i2", B=A.B0, Tn=A.T0, kind="ragged"):
    d = A.dae_case(pattern, shape, B, Tn, kind)
    return d, A.run_dae(A.solver("off"), d, dtype=torch.float64)


def _gpu(run, case, cls=None, kernel="auto"):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # (a walk on the GPU would warn: the call has to be the fused one)
        return run(A.solver("require", kernel, cls), case, "cuda")


# ----------------------------------------------------------------------------- 1. K0 forward
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("shape", list(C.ODE_FWD_SHAPES))
def test_k0_forward_ode_every_form_and_pattern(shape, pattern):
    case, ref = _ode(pattern, shape)
    got, ab2 = _gpu(A.run_ode, case), _gpu(A.run_ode, case, nd.AB2)
    e, gap = traj_rel_err(got.cpu(), ref), traj_rel_err(got.cpu(), ab2.cpu())
    print(shape, pattern, f"err {e:.3e}, distance to AB2 on the GPU {gap:.3e}")
    assert e <= TOL_GPU and gap > 100 * TOL_GPU


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("shape", list(C.DAE_SHAPES))
def test_k0_forward_dae_every_pattern(shape, pattern):
    case, (rx, ri) = _dae(pattern, shape)
    (gx, gi), (bx, _) = _gpu(A.run_dae, case), _gpu(A.run_dae, case, nd.AB2)
    e, ei, gap = traj_rel_err(gx.cpu(), rx), traj_rel_err(gi.cpu(), ri), traj_rel_err(gx.cpu(), bx.cpu())
    print(shape, pattern, f"err x {e:.3e} i {ei:.3e}, distance to AB2 on the GPU {gap:.3e}")
    assert e <= TOL_GPU and ei <= TOL_GPU and gap > 100 * TOL_GPU


@pytest.mark.parametrize("kind", ["ratio", "padded"])
def test_k0_forward_ratio_and_padded_clocks(kind):
    """the padded clock: finite everywhere, the valid prefix of every trajectory within the gate (behind the padding the walk and the
    kernel compute the same finite junk, which nothing reads)"""
    for pattern in ("s03", "mixed"):
        case, ref = _ode(pattern, kind=kind)
        got = _gpu(A.run_ode, case).cpu()
        dcase, (rx, ri) = _dae(pattern, kind=kind)
        gx, gi = (q.cpu() for q in _gpu(A.run_dae, dcase))
        assert bool(torch.isfinite(got).all() and torch.isfinite(gx).all() and torch.isfinite(gi).all())
        for b in range(A.B0):
            n = A.valid_len(A.T0, b) if kind == "padded" else A.T0
            for g, r in ((got, ref), (gx, rx), (gi, ri)):
                assert traj_rel_err(g[:n, b:b + 1], r[:n, b:b + 1]) <= TOL_GPU, (pattern, b)


@pytest.mark.parametrize("Tn,B", [(1, A.B0), (2, A.B0), (3, A.B0), (4, A.B0), (A.T0, 1), (A.T0, 16)])
def test_k0_forward_edge_shapes(Tn, B):
    """T = 2: the restart step alone; 3: then AB2's step; 4: the first three-slope step"""
    for pattern in ("s1", "mixed"):
        case, ref = _ode(pattern, B=B, Tn=Tn)
        assert traj_rel_err(_gpu(A.run_ode, case).cpu(), ref) <= TOL_GPU
        dcase, (rx, ri) = _dae(pattern, B=B, Tn=Tn)
        gx, gi = _gpu(A.run_dae, dcase)
        assert traj_rel_err(gx.cpu(), rx) <= TOL_GPU and traj_rel_err(gi.cpu(), ri) <= TOL_GPU


def test_dae_without_dataset_x_and_a_nan_canary_behind_the_grid():
    """the corrector reads row k + 1 of z | v -- on the last step row T - 1 -- and must not read row T"""
    dcase, (rx, ri) = _dae("s03", "x5z4v6i6")
    nox = C.without_x(dcase[:12]) + dcase[12:]
    gx, gi = _gpu(A.run_dae, nox)
    assert traj_rel_err(gx.cpu(), rx) <= TOL_GPU and traj_rel_err(gi.cpu(), ri) <= TOL_GPU
    canary = lambda q: torch.cat((q, torch.full_like(q[:1], float("nan"))), 0).cuda()[:-1]
    with torch.no_grad():
        d = [q.cuda() if torch.is_tensor(q) else q for q in dcase[2:12]]
        d[2], d[3] = canary(dcase[4]), canary(dcase[5])
        cx, ci = P.run_dae(A.solver("require"), deepcopy(dcase[0]).cuda(), deepcopy(dcase[1]).cuda(), *d, per_trajectory=dcase[13])
    assert torch.equal(cx, _gpu(A.run_dae, dcase)[0]) and bool(torch.isfinite(ci).all())
    for pattern in ("mixed", "last"):
        case, ref = _ode(pattern) if pattern != "last" else _last_step_restart()
        de, t, x, z, ev, zj, _, pt = case
        with torch.no_grad():
            xc, zc = x.cuda(), canary(z)
            got = P.run_ode(A.solver("require"), deepcopy(de).cuda(), t.cuda(), xc, zc, torch.cat((xc[0], zc[0]), -1), ev.cuda(), zj.cuda(), per_trajectory=pt)
        assert traj_rel_err(got.cpu(), ref) <= TOL_GPU, pattern


@functools.lru_cache(maxsize=None)
def _last_step_restart(dae=False):
    """a shared event at the last step, k = T - 2: its corrector reads the last row"""
    rows = (A.T0 - 2,)
    t = A.clock("ragged", A.T0, A.B0)
    if dae:
        case = C.dae_case(*C.DAE_SHAPES["x8z2v2i2"], A.B0, A.T0, 22, ev_rows=rows, t=t, perturb_x_init=True)
        A._scaled(case[0]), A._scaled(case[1])
        case = case + (A.shared_table(rows, A.T0, A.B0), False)
        return case, A.run_dae(A.solver("off"), case, dtype=torch.float64)
    case = C.ode_case(*C.ODE_FWD_SHAPES["reg"], A.B0, A.T0, 21, ev_rows=rows, t=t)
    A._scaled(case[0])
    case = case + (A.shared_table(rows, A.T0, A.B0), False)
    return case, A.run_ode(A.solver("off"), case, dtype=torch.float64)


def test_a_restart_on_the_last_step():
    case, ref = _last_step_restart()
    assert traj_rel_err(_gpu(A.run_ode, case).cpu(), ref) <= TOL_GPU
    dcase, (rx, ri) = _last_step_restart(True)
    gx, gi = _gpu(A.run_dae, dcase)
    assert traj_rel_err(gx.cpu(), rx) <= TOL_GPU and traj_rel_err(gi.cpu(), ri) <= TOL_GPU


def test_hits_in_one_workgroup_alone():
    """only_zero: trajectory 0 alone has an event, so workgroups 1 and 2 skip the corrector at that step while workgroup 0 runs it and
    selects it for one column"""
    case, ref = _ode("only_zero")
    assert traj_rel_err(_gpu(A.run_ode, case).cpu(), ref) <= TOL_GPU
    dcase, (rx, ri) = _dae("only_zero")
    gx, gi = _gpu(A.run_dae, dcase)
    assert traj_rel_err(gx.cpu(), rx) <= TOL_GPU and traj_rel_err(gi.cpu(), ri) <= TOL_GPU


@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_k0_forward_other_activations(act):
    case, ref = _ode("mixed", act=act)
    assert traj_rel_err(_gpu(A.run_ode, case).cpu(), ref) <= TOL_GPU


# ----------------------------------------------------------------------------- 2. training on K0 + K5
# K5's register path, the streamed path (hidden 128: global accumulators), a wide input and the staged path (132 input columns, z_dim 0)
K5_ODE = {"reg": (8, 2, (64, 64, 64)), "streamed": (8, 2, (128, 128, 128)), "wide_in": (40, 2, (64,)), "staged": (44, 0, (40, 40))}


def _train_ode(case, what, G=None):
    if G is None:
        (G,) = C.cotangents(51, case[2].shape)
    ref_xs, ref = A.ode_train(A.solver("off"), case, G, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, got = A.ode_train(A.solver("require"), case, G, "cuda")
        _, again = A.ode_train(A.solver("require"), case, G, "cuda")
    assert traj_rel_err(xs.detach().cpu(), ref_xs.detach()) <= TOL_GPU
    A.grads_close(ref, got, GRAD_TOL, what)
    for k in got:
        assert (got[k] is None and again[k] is None) or torch.equal(got[k], again[k]), (what, k)
    return ref, got


@pytest.mark.parametrize("shape,pattern", [(s, p) for s in K5_ODE for p in ("none", "s23", "mixed") if K5_ODE[s][1] > 0 or p == "none"])
def test_k5_ode_training_paths_and_event_rules(shape, pattern):
    """(z_dim 0, the staged shape, has no events)"""
    _train_ode(A.ode_case(pattern, K5_ODE[shape], kind="ratio"), f"{shape} {pattern}")


@pytest.mark.parametrize("act", [nn.Tanh, nn.SiLU])
def test_k5_ode_training_other_activations(act):
    _train_ode(A.ode_case("mixed", "reg", kind="ratio", act=act), act.__name__)


def _train_dae(case, what, G=None, Gi=None):
    if G is None:
        G, Gi = C.cotangents(52, case[3].shape, case[6].shape)
    ref_xs, ref_is, ref = A.dae_train(A.solver("off"), case, G, Gi, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xs, is_, got = A.dae_train(A.solver("require"), case, G, Gi, "cuda")
        _, _, again = A.dae_train(A.solver("require"), case, G, Gi, "cuda")
    assert traj_rel_err(xs.detach().cpu(), ref_xs.detach()) <= TOL_GPU and traj_rel_err(is_.detach().cpu(), ref_is.detach()) <= TOL_GPU
    A.grads_close(ref, got, GRAD_TOL, what)
    for k in got:
        assert (got[k] is None and again[k] is None) or torch.equal(got[k], again[k]), k
    return ref, got


@pytest.mark.parametrize("shape,pattern", [(s, p) for s in ("reg", "zvi16", "streamed", "deep") for p in ("none", "s03", "mixed", "only_zero")
                                           if p in ("none", "mixed") or s in ("reg", "zvi16")])
def test_k5_dae_training_paths_and_event_rules(shape, pattern):
    """Every shape runs without events and with per-trajectory ones; the shared rule and only_zero on two shapes.  only_zero: the
    corrector and the event-time head have hits in workgroup 0 alone -- their weight gradients must not pick up the other workgroups."""
    _train_dae(A.dae_case(pattern, shape, kind="ratio", shapes=C.K5_DAE_SHAPES), f"{shape} {pattern}")


def test_a_loss_on_the_row_behind_a_restart_gives_the_right_row_its_gradient():
    """The right-row adjoint: with a loss on xs[k + 1] alone behind a restart at k (shared events at steps 0 and 3: k = 3, and k = 0), row
    k + 1 of grad z gets its value through the corrector only -- the DE at step k reads row k or the jumped rows."""
    for k in (3, 0):
        case = A.ode_case("s03", kind="ratio")
        G = torch.zeros(case[2].shape)
        G[k + 1] = C.cotangents(53, case[2].shape)[0][k + 1]
        ref, got = _train_ode(case, f"loss on xs[{k + 1}]", G)
        want, have = ref["z"][k + 1].double(), got["z"][k + 1].double().cpu()
        assert float(want.abs().max()) > 0 and float(ref["z"][k + 2:].abs().max()) == 0 and float(got["z"][k + 2:].abs().max()) == 0
        assert float((have - want).abs().max()) <= GRAD_TOL * float(want.abs().max())
    dcase = A.dae_case("s03", "reg", kind="ratio", shapes=C.K5_DAE_SHAPES)
    G, Gi = torch.zeros(dcase[3].shape), torch.zeros(dcase[6].shape)
    G[4] = C.cotangents(54, dcase[3].shape)[0][4]
    ref, got = _train_dae(dcase, "DAE, loss on xs[4]", G, Gi)
    for name in ("z", "v"):
        want, have = ref[name][4].double(), got[name][4].double().cpu()
        assert float(want.abs().max()) > 0 and float((have - want).abs().max()) <= GRAD_TOL * float(want.abs().max())


# ----------------------------------------------------------------------------- 3. the solver, the models, the refusals
def test_solver_level_kernels_and_refusals():
    case, ref = _ode("s03")
    for kernel in ("auto", "generic"):
        assert traj_rel_err(_gpu(A.run_ode, case, kernel=kernel).cpu(), ref) <= TOL_GPU
    dcase, (rx, _) = _dae("s03")
    assert traj_rel_err(_gpu(A.run_dae, dcase, kernel="generic")[0].cpu(), rx) <= TOL_GPU
    for kernel in ("wave", "tile", "mfma", "wide"):
        with pytest.raises(_lib.UnsupportedShapeError, match="three-step Adams-Bashforth"):
            A.run_ode(A.solver("require", kernel), case, "cuda")
        with pytest.warns(RuntimeWarning, match="not fusable"):          # fused = "auto": the walk, with the warning
            got = A.run_ode(A.solver("auto", kernel), case, "cuda")
        assert traj_rel_err(got.cpu(), ref) <= TOL_GPU
    de, t, x, z = case[:4]
    xc, zc = x.cuda(), z.cuda()
    with pytest.raises(ValueError, match="teacher-forced"):
        A.solver("require").integrate_ODE(x_func=deepcopy(de).cuda(), t=t.cuda(), x=xc, z=zc, all_initial=torch.cat((xc[0], zc[0]), -1),
                                          input_true_x=True)


def test_models_route_ab3_through_rows_and_solver():
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    B, Tn = 9, A.T0
    t = P.clock(Tn, B).permute(1, 0, 2).contiguous()
    m = models.ODE_Model(8, 2, 16, direct_encode=True, solver=nd.AB3())
    x, z = 0.5 * torch.randn(B, Tn, 8, generator=g), 0.5 * torch.randn(B, Tn, 2, generator=g)
    ev, zj, vj = t[:, 1:2].clone(), 0.5 * torch.randn(B, 1, 2, generator=g), 0.5 * torch.randn(B, 1, 2, generator=g)      # an event at step 1
    m64 = deepcopy(m).double()
    m64.solver.fused = "off"
    with torch.no_grad():
        ref = m64(t.double(), x.double(), z.double(), ev.double(), zj.double())[0]
        mc = deepcopy(m).cuda()
        mc.solver.fused = "require"
        assert mc._forward_encoded(t.cuda(), x.cuda(), z.cuda(), ev.cuda(), zj.cuda()) is None
        got = mc(t.cuda(), x.cuda(), z.cuda(), ev.cuda(), zj.cuda())[0]
    assert traj_rel_err(got.cpu(), ref, bdim=0) <= TOL_GPU
    d = models.DAE_Model(8, 2, 2, 2, 64, direct_encode=True, solver=nd.AB3())
    v, i = 0.5 * torch.randn(B, Tn, 2, generator=g), 0.5 * torch.randn(B, Tn, 2, generator=g)
    d64 = deepcopy(d).double()
    d64.solver.fused = "off"
    with torch.no_grad():
        ref = d64(t.double(), x.double(), z.double(), v.double(), i.double(), ev.double(), zj.double(), vj.double())[0]
        dcu = deepcopy(d).cuda()
        dcu.solver.fused = "require"
        got = dcu(t.cuda(), x.cuda(), z.cuda(), v.cuda(), i.cuda(), ev.cuda(), zj.cuda(), vj.cuda())[0]
    assert traj_rel_err(got.cpu(), ref, bdim=0) <= TOL_GPU


def test_no_encode_models_run_ab3_fused():
    """ODE_Model / DAE_Model without encoders hand the solver their own DE_Func / AE_Func: forward under fused = "require" against the
    fp64 walk of the same model, and one training step's parameter gradients against fp64 autograd through the walk"""
    g = torch.Generator().manual_seed(5)
    B, Tn = 9, A.T0
    t = P.clock(Tn, B).permute(1, 0, 2).contiguous()
    x, z, v, i = (0.5 * torch.randn(B, Tn, w, generator=g) for w in (8, 2, 2, 2))
    ev, zj, vj = t[:, 3:4].clone(), 0.5 * torch.randn(B, 1, 2, generator=g), 0.5 * torch.randn(B, 1, 2, generator=g)      # an event at step 3
    torch.manual_seed(5)
    for m, args in ((models.ODE_Model(8, 2, 64, solver=nd.AB3()), (t, x, z, ev, zj)),
                    (models.DAE_Model(8, 2, 2, 2, 64, solver=nd.AB3()), (t, x, z, v, i, ev, zj, vj))):
        m64, mc = deepcopy(m).double(), deepcopy(m).cuda()
        m64.solver.fused, mc.solver.fused = "off", "require"
        first = lambda out: out[0] if isinstance(out, tuple) else out
        ref = first(m64(*(q.double() for q in args)))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            got = first(mc(*(q.cuda() for q in args)))
        assert traj_rel_err(got.detach().cpu(), ref.detach(), bdim=0) <= TOL_GPU
        ref.square().sum().backward()
        got.square().sum().backward()
        for (name, p64), pc in zip(m64.named_parameters(), mc.parameters()):
            if p64.grad is None:
                assert pc.grad is None or not bool(pc.grad.any()), name
                continue
            assert float((pc.grad.double().cpu() - p64.grad).abs().max()) <= GRAD_TOL * float(p64.grad.abs().max()), name
