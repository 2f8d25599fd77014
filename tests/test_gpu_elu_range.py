"""Every ELU(1) kernel over the whole activation range, against fp64.

The rest of the suite draws 0.1 randn inputs under default nn.Linear initialisation: every hidden pre-activation of those runs lies in about
[-0.4, +0.4], where ELU is almost the identity and ELU' almost 1.  Here (cases, references and gates: elu_range_cases.py; the instrument's
own tests: test_elu_range_host.py) each integrator and each backward kernel meets pre-activations from below -17 to above +5 in every
hidden layer, and probes whose result IS ELU^n(u) / prod ELU'(.) of chosen u.  The reference is always an fp64 evaluation -- the oracle on
float64 tensors, the closed form ELU^n, or fp64 autograd through the oracle's loop -- never another HIP kernel.

Which form of ELU each kernel carries (read from csrc/):
  elu_quad_scaled (log2e-scaled domain, first layer's image x log2e, last layer's / log2e)
        K1x / K2x inference (`wave`), K1 / K2 inference at every width class (`tile`, `mfma` at hidden 128 / 256): `scaled` below;
  elu_quad / elu_pair (plain domain)
        every save=True instance of those, K0 (`generic`) in its register / wide-register / LDS / streamed forms, K3a / K3c / K3w;
  the DPP form of psnode_latent_dpp.hip     K3f (hidden 16);
  elu1 (expm1f; psnode_generic_bwd_impl.h: ActCtx::act1) the recompute of K5's STAGED path only (its register and streamed paths
        recompute with elu_quad): reached at hidden (256, 256), the shape test_gpu_activations_pre.py's K5_PATHS files under "staged";
  ELU' = med3(h, -2, 0) + 1 of the stored or recomputed h       K4x, K4f, K5, K7f.
The probes below do not trust this table: an instance gets the plain-domain contract unless it is an inference instance of K1 / K1x /
K2 / K2x, and one that were filed wrongly would fail the exactness clause of that contract (u > 0 returns u bit for bit).
Out of scope: the latent backwards (K8*, K9*), the row kernels (test_inline_elu_accuracy_contract pins their ELU), and the builds with
another activation than ELU(1) (test_gpu_act_range.py runs these probes with every other kind).

Every test prints its figures (-s); profiles/elu_range_report.txt is that output of one run.
"""
import functools

import pytest
import torch

import elu_range_cases as E

pytestmark = pytest.mark.gpu
METHODS = ("euler", "midpoint", "rk4")
B_WIDE, T_WIDE = 70, 40          # ragged last wave (70 = 17 x 4 + 2) and last 16-trajectory tile

# (label, kernel=, save, xd, zd, H, n_hidden, recipe kwargs).  z_dim 0: spread from the biases alone (test_elu_range_host.py).
NOZ = dict(gain=2.0, bias_amp=8.0)
ODE_RUNS = [(f"{k}{'+save' if s else ''}", k, s, xd, zd, H, 3, kw)
            for k in ("wave", "tile") for s in (False, True) for xd, zd, H, kw in ((8, 2, 64, {}), (5, 3, 48, {}), (3, 0, 33, NOZ))]
ODE_RUNS += [("mfma h128", "mfma", False, 12, 2, 128, 3, {}), ("mfma h256 streamed", "mfma", False, 8, 2, 256, 3, {}),
             ("tile+save h128", "tile", True, 8, 2, 128, 3, {})]
ODE_RUNS += [(f"generic {what}", "generic", False, xd, zd, H, nh, kw) for what, xd, zd, H, nh, kw in (
    ("K1 class", 8, 2, 64, 3, {}), ("padded", 5, 3, 48, 3, {}), ("no z", 3, 0, 33, 3, NOZ), ("register", 20, 2, 64, 3, {}),
    ("register 1 layer", 8, 2, 48, 1, {}), ("wide register", 20, 2, 128, 3, {}), ("LDS 5 layers", 8, 2, 32, 5, {}),
    ("LDS h128 x 4", 8, 2, 128, 4, {}), ("streamed", 8, 2, 320, 3, {}))]
ODE_RUNS += [(f"latent{H}{'+save' if s else ''}", "mfma", s, H, H, H, 1, {}) for H, s in ((16, False), (64, False), (64, True), (96, False), (96, True))]
# (label, kernel, save, xd, zd, vd, idim, H, n_hidden)
DAE_RUNS = [(f"{k}{'+save' if s else ''}", k, s, *dims, 3) for k in ("wave", "tile") for s in (False, True)
            for dims in ((8, 2, 2, 2, 64), (5, 1, 1, 2, 48))]
DAE_RUNS += [("generic K2 class", "generic", False, 8, 2, 2, 2, 64, 3), ("generic padded", "generic", False, 5, 1, 1, 2, 48, 3),
             ("generic wide dims", "generic", False, 8, 4, 6, 6, 64, 3)]
DAE_RUNS += [(f"latent{H}", "mfma", False, H, H, H, H, H, 1) for H in (16, 64, 96)]

# Second trajectory gate: traj_rel_err(hip, fp64) <= FACTOR * traj_rel_err(oracle fp32, fp64) + 1e-7.  3 is the rule of
# test_accuracy_equivalent_to_reference_vs_fp64; an entry here is a kernel measured above it whose probes hold the ELU contract
# (absolute-accurate 1.2e-7 against ATen's relative accuracy): measured / oracle's, rounded up, at most 8.
FACTOR = {}


def _ids(runs):
    return [f"{r[0]} {'x'.join(str(v) for v in r[3:-1] if not isinstance(v, dict))}".replace(" ", "_") for r in runs]


def fused():
    from py_psnode_amd import fused as f
    return f


def dl(ls):
    return [(w.cuda(), b.cuda()) for w, b in ls]


def cu(a):
    return None if a is None else a.cuda()


def ode_hip(c, method, kernel, save, teacher=False):
    out = fused().ode_integrate(method, dl(c.layers), cu(c.t), cu(c.x), cu(c.z), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj),
                                input_true_x=teacher, kernel=kernel, save=save)
    return (out[0] if save else out).cpu()


def dae_hip(c, method, kernel, save, teacher=False):
    out = fused().dae_integrate(method, dl(c.de), dl(c.ae), cu(c.xi), cu(c.t), cu(c.x), cu(c.z), cu(c.v), cu(c.i), cu(c.a0), event_t=cu(c.ev),
                                z_jump=cu(c.zj), v_jump=cu(c.vj), input_true_x=teacher, input_true_i=teacher, kernel=kernel, save=save)
    return out[0].cpu(), out[1].cpu()


@functools.lru_cache(maxsize=None)
def _ode_refs(xd, zd, H, nh, kw, method):
    c = E.wide_ode_case(B_WIDE, T_WIDE, xd, zd, H, seed=11, n_hidden=nh, **dict(kw))
    return c, E.run_ode(c, method), E.run_ode(c, method, torch.float64)


@functools.lru_cache(maxsize=None)
def _dae_refs(dims, H, nh, method):
    c = E.wide_dae_case(B_WIDE, T_WIDE, *dims, H, seed=13, n_hidden=nh)
    return c, E.run_dae(c, method), E.run_dae(c, method, torch.float64)


def _gate(label, method, what, out, o32, t64):
    factor = FACTOR.get(label, 3)
    ok, e32, e64, eo = E.traj_gates(out, o32, t64, factor)
    print(f"[elu-range] traj  {label:24s} {method:8s} {what:2s} vs fp32 oracle {e32:.2e}  vs fp64 {e64:.2e}  oracle's own {eo:.2e}  "
          f"ratio {e64 / eo:.2f} (gate {factor} x + 1e-7)")
    return ok, (label, method, what, e32, e64, eo)


# ------------------------------------------------------------------------------------------------ (a) wide-range trajectories, forward
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", ODE_RUNS, ids=_ids(ODE_RUNS))
def test_wide_range_trajectories_ode(run, method):
    """70 trajectories x 40 grid points, two events, the wide recipe: <= TOL_GPU from the fp32 oracle AND no further from the fp64 truth
    than 3 x the fp32 oracle's own distance + 1e-7."""
    label, kernel, save, xd, zd, H, nh, kw = run
    c, o32, t64 = _ode_refs(xd, zd, H, nh, tuple(sorted(kw.items())), method)
    ok, figs = _gate(label + f" {xd}/{zd}/{H}", method, "x", ode_hip(c, method, kernel, save), o32, t64)
    assert ok, figs


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", DAE_RUNS, ids=_ids(DAE_RUNS))
def test_wide_range_trajectories_dae(run, method):
    """The DAE twin (DE and AE both wide), xs and is."""
    label, kernel, save, *dims, H, nh = run
    c, (x32, i32), (x64, i64) = _dae_refs(tuple(dims), H, nh, method)
    xs, is_ = dae_hip(c, method, kernel, save)
    okx, fx = _gate(label + f" {dims[0]}/{H}", method, "x", xs, x32, x64)
    oki, fi = _gate(label + f" {dims[0]}/{H}", method, "i", is_, i32, i64)
    assert okx and oki, (fx, fi)


# ------------------------------------------------------------------------------------------------ (b) one-evaluation probes, forward
def _scaled(kernel, save, nh):
    """Inference instances of the MFMA integrators K1 / K1x / K2 / K2x run the hidden layers in the log2e-scaled domain."""
    return kernel in ("wave", "tile", "mfma") and not save and nh == 3


def _identity(label, method, what, out, u, n, scaled, slack):
    gate = E.identity_gate_scaled if scaled else E.identity_gate_plain
    ok, err, bound, at = gate(out, u, n, rel_slack=slack)
    print(f"[elu-range] probe {label:24s} {method:8s} {what:2s} identity ({'scaled' if scaled else 'plain'}): worst |out - ELU^{n}(u)| {err:.2e} "
          f"(bound {bound:.2e}) at u = {at:.9g}")
    return ok, (label, method, what, err, bound, at)


PROBE_ODE = [r for r in ODE_RUNS if r[4] > 0]         # the probes feed their values through z


def _takes_tf(kernel, save, nh, dae=False):
    """Teacher forcing is refused by the saving instances, the latent kernels (K3*) and K2x; those run the T = 2 probes alone."""
    return not save and not (kernel == "mfma" and nh == 1) and not (dae and kernel == "wave")


@pytest.mark.parametrize("run", PROBE_ODE, ids=_ids(PROBE_ODE))
def test_identity_probe_ode(run):
    """Weights of zeros and ones, dt = 1, dataset x == 0: every grid point of the result is the kernel's ELU^n(u).  Teacher-forced over
    the whole magnitude set where the instance takes teacher forcing (Euler), and as one step from x0 = 0 (T = 2: K1x's peeled last step)
    under all three methods.  Plain-domain instances: the inline ELU's contract n times; scaled-domain instances: its bound (weights and
    products round once each), finite at 88 / 104 / 1e4, and plain and saving runs of one probe within the sum of their bounds.
    K1x (`wave`, plain and saving) also runs the carry probe: eight grid points without teacher forcing, z non-zero at grid row 3 only,
    so that the probed evaluation sits in the steady-state body of the time loop (the prefetching FAST loop / the ring steps of the
    saving forward) and the rows after it carry ELU^n(u) unchanged."""
    label, kernel, save, xd, zd, H, nh, _ = run
    label = f"{label} {xd}/{zd}/{H}"
    sc = _scaled(kernel, save, nh)
    fails = []
    if _takes_tf(kernel, save, nh):
        c = E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=True)
        ok, figs = _identity(label, "euler", "tf", ode_hip(c, "euler", kernel, False, teacher=True)[1:], c.u_of, nh, sc, 0.0)
        fails += [] if ok else [figs]
    c = E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=False)
    for method in METHODS:
        out = ode_hip(c, method, kernel, save)[1:]
        ok, figs = _identity(label, method, "t2", out, c.u_of, nh, sc, 0.0 if method == "euler" else E.STAGE_SLACK)
        fails += [] if ok else [figs]
        if sc and method == "euler" and (kernel, xd) != ("mfma", 12) and H <= 128:      # the saving (plain-domain) twin of this instance
            sav = ode_hip(c, method, kernel, True)[1:]
            lim = E.scaled_bound(c.u_of, nh) + nh * E.ELU_ABS
            ok = bool(((out.double() - sav.double()).abs() <= lim).all())
            fails += [] if ok else [(label, "plain vs saving", float(((out.double() - sav.double()).abs() - lim).max()))]
    if kernel == "wave":
        c = E.identity_carry_probe_ode(xd, zd, H, n_hidden=nh)
        for method in METHODS:
            out = ode_hip(c, method, kernel, save)
            if float(out[:c.row + 1].abs().max()) != 0.0:
                fails.append((label, method, "carry: rows before the probed step are not exactly 0"))
            for j in (c.row + 1, out.shape[0] - 1):       # the step that evaluates u, and the last row (carried through the peeled step)
                ok, figs = _identity(label, method, f"c{j}", out[j], c.u_of, nh, sc, 0.0 if method == "euler" else E.STAGE_SLACK)
                fails += [] if ok else [figs]
            if not torch.equal(out[c.row + 1:], out[c.row + 1:c.row + 2].expand_as(out[c.row + 1:])):
                fails.append((label, method, "carry: a later step changed the carried value (f(0) must be exactly 0)"))
    assert not fails, fails


PROBE_DAE = DAE_RUNS


@pytest.mark.parametrize("run", PROBE_DAE, ids=_ids(PROBE_DAE))
def test_identity_probe_dae(run):
    """The DAE twin: xs[j] = ELU^n of the DE's (z, v) columns, is[j] = ELU^n of the AE head's.  K2x (`wave`) and the saving instances
    refuse teacher forcing: T = 2 only.  (Plain and saving instances are each gated against the same fp64 ELU^n(u), so "they differ by no
    more than the sum of their bounds" follows by the triangle inequality and is not asserted a second time here.)"""
    label, kernel, save, xd, zd, vd, idim, H, nh = run
    label = f"{label} {xd}/{H}"
    sc = _scaled(kernel, save, nh)
    fails = []
    if _takes_tf(kernel, save, nh, dae=True):
        c = E.identity_probe_dae(xd, zd, vd, idim, H, n_hidden=nh, teacher=True)
        xs, is_ = dae_hip(c, "euler", kernel, False, teacher=True)
        for what, out, u in (("xf", xs[1:], c.u_x), ("if", is_, c.u_i)):
            ok, figs = _identity(label, "euler", what, out, u, nh, sc, 0.0)
            fails += [] if ok else [figs]
    c = E.identity_probe_dae(xd, zd, vd, idim, H, n_hidden=nh, teacher=False)
    for method in METHODS:
        xs, is_ = dae_hip(c, method, kernel, save)
        for what, out, u, slack in (("x2", xs[1:], c.u_x, 0.0 if method == "euler" else E.STAGE_SLACK), ("i2", is_, c.u_i, 0.0)):
            ok, figs = _identity(label, method, what, out, u, nh, sc, slack)
            fails += [] if ok else [figs]
    assert not fails, fails


def _random(label, what, out, ref):
    ok, ratio, b = E.random_probe_gate(out, ref)
    print(f"[elu-range] probe {label:24s} euler    {what:2s} random weights: worst |out - fp64| / max(1, |fp64|) {ratio:.2e} at trajectory {b} (gate 2e-6)")
    return ok, (label, what, ratio, b)


@pytest.mark.parametrize("run", PROBE_ODE, ids=_ids(PROBE_ODE))
def test_random_probe_ode(run):
    """One visible MLP evaluation per grid point with the wide recipe's random weights (zero padding, split-K folds, every unit): per
    trajectory within 2e-6 of max(1, |fp64|), the row kernels' one-evaluation tolerance."""
    label, kernel, save, xd, zd, H, nh, kw = run
    fails = []
    for teacher in ((True, False) if _takes_tf(kernel, save, nh) else (False,)):
        c = E.random_probe_ode(B_WIDE, 12, xd, zd, H, seed=17, n_hidden=nh, teacher=teacher, **kw)
        ok, figs = _random(f"{label} {xd}/{zd}/{H}", "tf" if teacher else "t2", ode_hip(c, "euler", kernel, save, teacher=teacher),
                           E.probe_run_ode(c, dtype=torch.float64))
        fails += [] if ok else [figs]
    assert not fails, fails


@pytest.mark.parametrize("run", PROBE_DAE, ids=_ids(PROBE_DAE))
def test_random_probe_dae(run):
    label, kernel, save, xd, zd, vd, idim, H, nh = run
    fails = []
    for teacher in ((True, False) if _takes_tf(kernel, save, nh, dae=True) else (False,)):
        c = E.random_probe_dae(B_WIDE, 12, xd, zd, vd, idim, H, seed=19, n_hidden=nh, teacher=teacher)
        xs, is_ = dae_hip(c, "euler", kernel, save, teacher=teacher)
        x64, i64 = E.probe_run_dae(c, dtype=torch.float64)
        for what, out, ref in (("x", xs, x64), ("i", is_, i64)):
            ok, figs = _random(f"{label} {xd}/{H}", what + ("f" if teacher else "2"), out, ref)
            fails += [] if ok else [figs]
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ (c) backward in the wide regime
def _close(a, b, what, tol=2e-4):
    """`_close` of test_gpu_backward_x.py: 2e-4 of each tensor's max.  -> (ok, text)"""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    return err <= tol * max(scale, 1e-6), f"{what}: err {err:.3e} vs max {scale:.3e} ({err / max(scale, 1e-6):.1e})"


# (label, forward kernel, save, backward kernel, xd, zd, H, n_hidden)
ODE_BWD = [("K4x saved", "wave", True, "wave", 8, 2, 64, 3), ("K4x saved padded", "wave", True, "wave", 5, 3, 48, 3),
           ("K4f saved", "tile", True, "wide", 8, 2, 64, 3), ("K4f recompute", "tile", False, "wide", 8, 2, 64, 3),
           ("K4f recompute h128", "tile", False, "wide", 8, 2, 128, 3), ("K5 register", "generic", False, "generic", 8, 2, 64, 3),
           # K5 prefers register, then streamed, then staged (gbwd_mode): five Linear layers of 64 only leave the register class and stream
           # with the accumulators in LDS; hidden 128 x 3 streams with them in global memory; (256, 256) no longer fits streamed (41 036
           # floats of LDS against 40 960) and is the shape the project's K5 path table (test_gpu_activations_pre.py) files under staged
           ("K5 streamed h128", "generic", False, "generic", 8, 2, 128, 3), ("K5 streamed deep 64x4", "generic", False, "generic", 8, 2, 64, 4),
           ("K5 staged 256x2", "generic", False, "generic", 8, 2, 256, 2)]


def _ode_forward_for_backward(c, method, fkern, save):
    f = fused()
    layers = dl(c.layers)
    tab = f.event_table(cu(c.t), cu(c.ev)) if c.ev is not None else None
    out = f.ode_integrate(method, layers, cu(c.t), cu(c.x), cu(c.z), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj), kernel=fkern, save=save)
    xs, saved = out if save else (out, None)
    return layers, tab, xs, saved


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", ODE_BWD, ids=[r[0].replace(" ", "_") for r in ODE_BWD])
def test_wide_range_backward_ode(run, method):
    """Every output (dL/dx0, dL/dz, dL/dz_jump, dL/dall_initial, every parameter) against fp64 autograd through the oracle's loop, in the
    wide regime (ELU' from 0 to 1 in every layer), at the suite's 2e-4 of each tensor's max.  B = 22, T = 11, two events."""
    label, fkern, save, bkern, xd, zd, H, nh = run
    c = E.wide_ode_case(22, 11, xd, zd, H, seed=23, n_hidden=nh)
    G = torch.randn(11, 22, xd, generator=torch.Generator().manual_seed(5))
    ls64 = [(w.double().requires_grad_(True), b.double().requires_grad_(True)) for w, b in c.layers]
    x0, z, a0, zj = (a.double().requires_grad_(True) for a in (c.x[0], c.z, c.a0, c.zj))
    xs64 = E.ode_walk64(method, ls64, c.t.double(), x0, z, a0, c.ev.double(), zj)
    (xs64 * G.double()).sum().backward()
    layers, tab, xs, saved = _ode_forward_for_backward(c, method, fkern, save)
    gx0, gz, gzj, ga0, gp = fused().ode_backward(method, layers, cu(c.t), cu(c.z), cu(c.a0), xs, G.cuda(), event_idx=tab, z_jump=cu(c.zj),
                                                 kernel=bkern, saved=saved)
    pairs = [("grad x0", gx0, x0.grad), ("grad z", gz, z.grad), ("grad z_jump", gzj, zj.grad), ("grad all_initial", ga0, a0.grad)]
    pairs += [(f"grad param {k}", g, p.grad) for k, (g, p) in enumerate(zip(gp, [q for wb in ls64 for q in wb]))]
    res = [_close(a, b, what) for what, a, b in pairs]
    print(f"[elu-range] bwd   {label:24s} {method:8s} worst " + max(res, key=lambda r: float(r[1].rsplit('(', 1)[1][:-1]))[1])
    assert all(ok for ok, _ in res), [txt for ok, txt in res if not ok]


DAE_BWD = [("K7f saved", "tile", True), ("K7f saved (K2x rows)", "wave", True), ("K7f+K7h recompute", "tile", False)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", DAE_BWD, ids=[r[0].replace(" ", "_") for r in DAE_BWD])
def test_wide_range_backward_dae(run, method):
    """K7f (+ K7h for the head's parameter gradients in the recompute form) on the DAE_01 class, DE and AE wide."""
    label, fkern, save = run
    xd, zd, vd, idim, H = 8, 2, 2, 2, 64
    c = E.wide_dae_case(22, 11, xd, zd, vd, idim, H, seed=29)
    g = torch.Generator().manual_seed(6)
    Gx, Gi = torch.randn(11, 22, xd, generator=g), torch.randn(11, 22, idim, generator=g)
    req = lambda a: a.double().requires_grad_(True)
    de64, ae64 = [(req(w), req(b)) for w, b in c.de], [(req(w), req(b)) for w, b in c.ae]
    xi, z, v, a0, zj, vj = (req(a) for a in (c.xi, c.z, c.v, c.a0, c.zj, c.vj))
    xs64, is64 = E.dae_walk64(method, de64, ae64, xi, c.t.double(), z, v, a0, c.ev.double(), zj, vj)
    ((xs64 * Gx.double()).sum() + (is64 * Gi.double()).sum()).backward()
    f = fused()
    de, ae = dl(c.de), dl(c.ae)
    tab = f.event_table(cu(c.t), cu(c.ev))
    xe = torch.zeros(11, 22, 0, device="cuda")
    out = f.dae_integrate(method, de, ae, cu(c.xi), cu(c.t), xe, cu(c.z), cu(c.v), cu(c.i), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj),
                          v_jump=cu(c.vj), kernel=fkern, save=save)
    xs, is_, saved = out if save else (*out, None)
    gr = f.dae_backward(method, de, ae, cu(c.t), cu(c.z), cu(c.v), cu(c.a0), xs, is_, Gx.cuda(), Gi.cuda(), event_idx=tab, z_jump=cu(c.zj),
                        v_jump=cu(c.vj), kernel="wide", saved=saved)
    pairs = [(k, gr[k], q.grad) for k, q in (("x_init", xi), ("z", z), ("v", v), ("z_jump", zj), ("v_jump", vj), ("all_initial", a0))]
    pairs += [(f"grad de {k}", a, p.grad) for k, (a, p) in enumerate(zip(gr["de"], [q for wb in de64 for q in wb]))]
    pairs += [(f"grad ae {k}", a, p.grad) for k, (a, p) in enumerate(zip(gr["ae"], [q for wb in ae64 for q in wb]))]
    res = [_close(a, b, what) for what, a, b in pairs]
    print(f"[elu-range] bwd   {label:24s} {method:8s} worst " + max(res, key=lambda r: float(r[1].rsplit('(', 1)[1][:-1]))[1])
    assert all(ok for ok, _ in res), [txt for ok, txt in res if not ok]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", ODE_BWD, ids=[r[0].replace(" ", "_") for r in ODE_BWD])
def test_elu_grad_probe_ode(run, method):
    """The identity probe (T = 2) with one-hot dL/dxs: dL/dz[0, b, d] IS prod_k ELU'(p_k) along the chain u -> ELU(u) -> ... of the unit
    that reads z[0, b, d].  Exactly 1 for u >= 0 (torch's rule: ELU'(0) = 1), exactly 0 from -88 down, within `elu_grad_bound` between."""
    label, fkern, save, bkern, xd, zd, H, nh = run
    c = E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=False)
    B = c.t.shape[1]
    nr = min(xd, zd)
    G = torch.zeros(2, B, xd)
    G[1, :, :nr] = 1.0              # output d < zd is the only output with a gradient among those that read z column d
    layers, tab, xs, saved = _ode_forward_for_backward(c, method, fkern, save)
    _, gz, _, _, _ = fused().ode_backward(method, layers, cu(c.t), cu(c.z), cu(c.a0), xs, G.cuda(), kernel=bkern, saved=saved)
    ok, err, b, at = E.elu_grad_gate(gz[0, :, :nr].cpu(), c.z[0, :, :nr], nh, rel_slack=0.0 if method == "euler" else E.STAGE_SLACK)
    print(f"[elu-range] bwd   {label:24s} {method:8s} ELU' probe: worst |g - prod ELU'| {err:.2e} (bound {b:.2e}) at u = {at:.9g}")
    assert ok, (label, method, err, b, at)
    assert float(gz[1].abs().max()) == 0.0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("run", DAE_BWD, ids=[r[0].replace(" ", "_") for r in DAE_BWD])
def test_elu_grad_probe_dae(run, method):
    """K7f: the DAE identity probe (T = 2) with a one-hot dL/dxs and dL/dis = 0: dL/dz[0] and dL/dv[0] read prod ELU' of the DE."""
    label, fkern, save = run
    xd, zd, vd, idim, H = 8, 2, 2, 2, 64
    c = E.identity_probe_dae(xd, zd, vd, idim, H, teacher=False)
    B, ne = c.t.shape[1], zd + vd
    nr = min(xd, ne)
    Gx, Gi = torch.zeros(2, B, xd), torch.zeros(2, B, idim)
    Gx[1, :, :nr] = 1.0
    f = fused()
    de, ae = dl(c.de), dl(c.ae)
    xe = torch.zeros(2, B, 0, device="cuda")
    out = f.dae_integrate(method, de, ae, cu(c.xi), cu(c.t), xe, cu(c.z), cu(c.v), cu(c.i), cu(c.a0), kernel=fkern, save=save)
    xs, is_, saved = out if save else (*out, None)
    gr = f.dae_backward(method, de, ae, cu(c.t), cu(c.z), cu(c.v), cu(c.a0), xs, is_, Gx.cuda(), Gi.cuda(), kernel="wide", saved=saved)
    got = torch.cat((gr["z"][0], gr["v"][0]), -1)[:, :nr].cpu()
    u = torch.cat((c.z[0], c.v[0]), -1)[:, :nr]
    ok, err, b, at = E.elu_grad_gate(got, u, 3, rel_slack=0.0 if method == "euler" else E.STAGE_SLACK)
    print(f"[elu-range] bwd   {label:24s} {method:8s} ELU' probe: worst |g - prod ELU'| {err:.2e} (bound {b:.2e}) at u = {at:.9g}")
    assert ok, (label, method, err, b, at)
    assert float(gr["z"][1].abs().max()) == 0.0 and float(gr["v"][1].abs().max()) == 0.0
