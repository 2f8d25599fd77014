"""The ten activation kinds of csrc/psnode_act.h on K0 and K5 over their whole range, against fp64.

test_gpu_activations*.py draw 0.5 randn inputs under default nn.Linear initialisation and compare whole trajectories at 2e-4 of each
gradient tensor's maximum: a derivative that is wrong by a percent on a few units passes there.  Here (cases, references, gates and
mutants: act_range_cases.py; the instrument's own tests: test_act_range_host.py) the identity probes of test_gpu_elu_range.py are run with
every entry of ACTS: each grid point of a probe's result IS act^n(u) of a chosen u, dL/dz[0] under a one-hot output gradient IS
prod act'(.) along the chain, and both are gated against fp64 closed forms with bounds derived from the forms themselves.  The reference
is always fp64 -- a closed form, the oracle's loop on float64 tensors with the same torch module as its activation, or fp64 autograd
through it -- never another kernel.

  1  forward identity probes on K0 (kernel="generic") in each of its modes, teacher-forced (Euler) and as one step (Euler, Midpoint,
     RK4); the DAE probe with mixed pairs (DE and AE of different families);
  2  derivative probes on each K5 path of test_gpu_activations_pre.py's K5_PATHS, and the DAE twin;
  3  random probes (wide recipe's weights: padding, split-K folds, every unit), forward and backward;
  4  wide-range trajectories and backwards (the `test_wide_range_inputs` the six-kind file lacks, rows at +-1e4 included);
  5  one case each through the tableau, sub-step and linear-externals builds, which compile the same forms;
  6  the extremes set (|u| from 1e19 to 3e38): finite, within 4 x 2^-24 relative of the fp64 limit.

What the probes found on the kernels of the commit before (profiles/act_range_report.txt, second section): K5 took Softplus' from the
layer output, beta h > thr ? 1 : 1 - e^(-beta h), where torch decides on the input.  The derivative probes fail there on every K5 path and
in the tableau, sub-step and linear-externals builds: largest |g - prod act'| 6.74e-3 for Softplus(2, 5) (at u = 2.4966), 0.368 for
Softplus(1, 1) (u = 0.5418), 1.00 for Softplus(1, 0) (u = -71.4), against bounds of about 1e-7; Softplus(1, 20) passes (1.96e-7).  And
GELU(tanh)' was NaN on the extremes set (0 x inf beyond |u| = 1.8e19).  K5 now keeps u for a Softplus below thr = 24 ln 2 (its pre
build) and GELU(tanh)' clamps u^2; all 240 cases pass.

Every test prints its figures (-s); profiles/act_range_report.txt is that output of one run.
"""
import functools
import types

import pytest
import torch
import torch.nn as nn

import act_range_cases as A
import elu_range_cases as E
from test_gpu_activations_pre import K5_PATHS

pytestmark = pytest.mark.gpu
KEYS = list(A.ACTS)
B_WIDE, T_WIDE = A.B_WIDE, A.T_WIDE
# K0's modes at the smallest shapes that reach them (test_gpu_elu_range.py): (label, xd, zd, H, hidden layers)
K0_MODES = [("register", 20, 2, 64, 3), ("one layer", 8, 2, 48, 1), ("wide register", 20, 2, 128, 3), ("LDS 5 layers", 8, 2, 32, 5),
            ("streamed", 8, 2, 320, 3)]
ELU1 = types.SimpleNamespace(key="ELU(1)", kind="elu", module=nn.ELU, act=None, alpha=1.0, beta=1.0, thr=20.0)
# (DE, AE) of different families: derivative from h / from u / Softplus below the cut / ELU(1)
PAIRS = [("Tanh", "Softplus(1,1)"), ("SiLU", "ELU(1)"), ("Sigmoid", "GELU")]


def entry(key):
    return ELU1 if key == "ELU(1)" else A.ACTS[key]


def fused():
    from py_psnode_amd import fused as f
    return f


def dl(ls):
    return [(w.cuda(), b.cuda()) for w, b in ls]


def cu(a):
    return None if a is None else a.cuda()


def slack(method):
    return 0.0 if method == "euler" else E.STAGE_SLACK


@functools.lru_cache(maxsize=None)
def _u(key):
    return A.act_probe_magnitudes(A.ACTS[key])


@functools.lru_cache(maxsize=None)
def _probe(key, xd, zd, H, nh, teacher):
    return E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=teacher, u=_u(key))


def ode_hip(c, method, a, teacher=False, **kw):
    out = fused().ode_integrate(method, dl(c.layers), cu(c.t), cu(c.x), cu(c.z), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj), input_true_x=teacher,
                                kernel="generic", act=a.act, **kw)
    return out


def ode_bwd_hip(c, method, a, G, xs=None, **kw):
    """K0 forward, then K5: -> (xs, (gx0, gz, gzj, ga0, gparams))"""
    f = fused()
    layers = dl(c.layers)
    tab = f.event_table(cu(c.t), cu(c.ev)) if c.ev is not None else None
    fkw = dict(kw)
    x_sub = None
    if kw.get("substeps", 1) > 1 or kw.get("externals") == "linear":
        fkw["save_sub"] = True
    out = f.ode_integrate(method, layers, cu(c.t), cu(c.x), cu(c.z), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj), kernel="generic", act=a.act, **fkw)
    if "save_sub" in fkw:
        out, x_sub = out
    g = f.ode_backward(method, layers, cu(c.t), cu(c.z), cu(c.a0), out, G.cuda(), event_idx=tab, z_jump=cu(c.zj), kernel="generic", act=a.act,
                       x_sub=x_sub, **kw)
    return out.cpu(), g


def _pv(tag, label, key, method, what, res, n):
    ok, err, b, at, aten = res[:5]
    print(f"[act-range] {tag:5s} {label:34s} {key:15s} {method:10s} {what:3s} worst |out - act^{n}(u)| {err:.2e} (bound {b:.2e}) at u = {at:.9g}"
          + (f"  largest {res[5][0]:.2e} at u = {res[5][1]:.9g}" if len(res) > 5 else "")
          + (f"  ATen's own relative error there {aten:.1e}" if aten is not None else ""))
    return ok, (label, key, method, what, err, b, at)


def _pg(tag, label, key, method, res, n):
    ok, err, b, at, aten, side, big = res
    print(f"[act-range] {tag:5s} {label:34s} {key:15s} {method:10s} d   worst |g - prod act'| {err:.2e} (bound {b:.2e}) at u = {at:.9g}"
          f"  largest {big[0]:.2e} at u = {big[1]:.9g}"
          + (f"  ATen's own relative error there {aten:.1e}" if aten is not None else "")
          + (f"  denormal u: the derivative of {dict(own='its own side', zero='0').get(side, side)}" if side else ""))
    return ok, (label, key, method, "d", err, b, at)


# ------------------------------------------------------------------------------------------------ 1  forward identity probes on K0
@pytest.mark.parametrize("mode", K0_MODES, ids=[m[0].replace(" ", "_") for m in K0_MODES])
@pytest.mark.parametrize("key", KEYS)
def test_forward_probe_k0(key, mode):
    """Teacher-forced over the whole probe set (B = 70, Euler), and one step from x0 = 0 (T = 2) under Euler, Midpoint and RK4."""
    label, xd, zd, H, nh = mode
    a = A.ACTS[key]
    fails = []
    c = _probe(key, xd, zd, H, nh, True)
    ok, figs = _pv("K0", label, key, "euler", "tf", A.value_gate(a, ode_hip(c, "euler", a, teacher=True).cpu()[1:], c.u_of, nh), nh)
    fails += [] if ok else [figs]
    c = _probe(key, xd, zd, H, nh, False)
    for method in ("euler", "midpoint", "rk4"):
        ok, figs = _pv("K0", label, key, method, "t2", A.value_gate(a, ode_hip(c, method, a).cpu()[1:], c.u_of, nh, rel_slack=slack(method)), nh)
        fails += [] if ok else [figs]
    assert not fails, fails


def _dae_probe(pair, teacher):
    de, ae = entry(pair[0]), entry(pair[1])
    u = torch.cat([_u(k) for k in pair if k != "ELU(1)"] + ([E.probe_magnitudes()] if "ELU(1)" in pair else []))
    return de, ae, E.identity_probe_dae(8, 2, 2, 2, 64, teacher=teacher, u=u)


def dae_hip(c, method, de, ae, teacher=False):
    out = fused().dae_integrate(method, dl(c.de), dl(c.ae), cu(c.xi), cu(c.t), cu(c.x), cu(c.z), cu(c.v), cu(c.i), cu(c.a0), event_t=cu(c.ev),
                                z_jump=cu(c.zj), v_jump=cu(c.vj), input_true_x=teacher, input_true_i=teacher, kernel="generic", act=(de.act, ae.act))
    return out[0].cpu(), out[1].cpu()


def _value_gate_any(a, out, u, n, rel_slack=0.0):
    """ELU(1) runs elu_quad, whose contract is elu_range_cases' identity_gate_plain."""
    if a.act is None:
        return (*E.identity_gate_plain(out, u, n, rel_slack=rel_slack), None)
    return A.value_gate(a, out, u, n, rel_slack=rel_slack)


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_forward_probe_dae_mixed_pair(pair):
    """xs[j] = DE_act^3 of the DE's (z, v) columns, is[j] = AE_act^3 of the head's: each MLP of a mixed pair applies its own activation."""
    fails = []
    for teacher, methods in ((True, ("euler",)), (False, ("euler", "midpoint", "rk4"))):
        de, ae, c = _dae_probe(pair, teacher)
        for method in methods:
            xs, is_ = dae_hip(c, method, de, ae, teacher)
            for what, a, out, u, sl in (("x", de, xs[1:], c.u_x, slack(method)), ("i", ae, is_, c.u_i, 0.0)):
                ok, figs = _pv("K0", "DAE 8/2/2/2/64 " + "+".join(pair), a.key, method, what + ("f" if teacher else "2"),
                               _value_gate_any(a, out, u, 3, rel_slack=0.0 if teacher else sl), 3)
                fails += [] if ok else [figs]
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 2  derivative probes on K5
def _grad_probe(a, key, label, xd, zd, H, nh, method, **kw):
    c = _probe(key, xd, zd, H, nh, False)
    B = c.t.shape[1]
    nr = min(xd, zd)
    G = torch.zeros(2, B, xd)
    G[1, :, :nr] = 1.0              # output d < zd is the only output with a gradient among those that read z column d
    xs, (_, gz, _, _, _) = ode_bwd_hip(c, method, a, G, **kw)
    sl = slack(method if isinstance(method, str) else "rk")
    okv, fv = _pv("K5", label, key, str(method), "t2", A.value_gate(a, xs[1:], c.u_of, nh, rel_slack=sl), nh)
    got = gz[0] + gz[1] if kw.get("externals") == "linear" else gz[0]       # (linear externals split dL/dz between the interval's two rows)
    okg, fg = _pg("K5", label, key, str(method), A.grad_gate(a, got[:, :nr].cpu(), c.z[0, :, :nr], nh, rel_slack=sl), nh)
    rest = float(gz[1].abs().max()) == 0.0 or kw.get("externals") == "linear"
    return ([] if okv else [fv]) + ([] if okg else [fg]) + ([] if rest else [(label, key, "dL/dz[1] is not 0")])


@pytest.mark.parametrize("path", list(K5_PATHS), ids=["register", "streamed", "streamed_deep", "streamed_160x3", "staged"])
@pytest.mark.parametrize("key", KEYS)
def test_grad_probe_k5(key, path):
    """The T = 2 identity probe with one-hot dL/dxs on each K5 path: dL/dz[0] IS prod_k act'(p_k).  Euler and RK4."""
    xd, zd, hidden = K5_PATHS[path]
    fails = []
    for method in ("euler", "rk4"):
        fails += _grad_probe(A.ACTS[key], key, path.split(" (")[0][:34], xd, zd, hidden, len(hidden), method)
    assert not fails, fails


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_grad_probe_k5_dae_mixed_pair(pair):
    """The DAE twin: a one-hot dL/dxs and dL/dis = 0; dL/dz[0] and dL/dv[0] read prod act' of the DE."""
    de, ae, c = _dae_probe(pair, False)
    xd, zd, vd, idim = 8, 2, 2, 2
    B, ne = c.t.shape[1], zd + vd
    nr = min(xd, ne)
    Gx, Gi = torch.zeros(2, B, xd), torch.zeros(2, B, idim)
    Gx[1, :, :nr] = 1.0
    f = fused()
    fails = []
    for method in ("euler", "rk4"):
        lde, lae = dl(c.de), dl(c.ae)
        xe = torch.zeros(2, B, 0, device="cuda")
        xs, is_ = f.dae_integrate(method, lde, lae, cu(c.xi), cu(c.t), xe, cu(c.z), cu(c.v), cu(c.i), cu(c.a0), kernel="generic", act=(de.act, ae.act))
        gr = f.dae_backward(method, lde, lae, cu(c.t), cu(c.z), cu(c.v), cu(c.a0), xs, is_, Gx.cuda(), Gi.cuda(), kernel="generic", act=(de.act, ae.act))
        got = torch.cat((gr["z"][0], gr["v"][0]), -1)[:, :nr].cpu()
        u = torch.cat((c.z[0], c.v[0]), -1)[:, :nr]
        ok, figs = _pg("K5", "DAE 8/2/2/2/64 " + "+".join(pair), de.key, method, A.grad_gate(de, got, u, 3, rel_slack=slack(method)), 3)
        fails += [] if ok else [figs]
        if float(gr["z"][1].abs().max()) != 0.0 or float(gr["v"][1].abs().max()) != 0.0:
            fails.append((pair, method, "dL/dz[1] or dL/dv[1] is not 0"))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 3  random probes
def _check_grads(tag, label, key, method, got, named):
    gx0, gz, gzj, ga0, gp = got
    res = [A.close_gate(g, r, what) for (what, r), g in zip(named, [gx0, gz, gzj, ga0] + list(gp)) if r is not None]
    print(f"[act-range] {tag:5s} {label:34s} {key:15s} {method:10s} bwd worst " + max(res, key=lambda r: r[2])[1])
    return [txt for ok, txt, _ in res if not ok]


@pytest.mark.parametrize("key", KEYS)
def test_random_probe(key):
    """B = 70, T = 6, the wide recipe's random weights.  Forward: one visible MLP evaluation per grid point (teacher-forced), per trajectory
    within 2e-6 of max(1, |fp64|).  Backward: the same data integrated freely, every gradient against fp64 autograd at 2e-4 of its max."""
    a = A.ACTS[key]
    c = E.random_probe_ode(B_WIDE, 6, 8, 2, 64, seed=31, teacher=True)
    with E.oracle_elu(a.module()):
        ref = E.probe_run_ode(c, dtype=torch.float64)
    ok, ratio, b = E.random_probe_gate(ode_hip(c, "euler", a, teacher=True).cpu(), ref)
    print(f"[act-range] K0    random probe 8/2/64                {key:15s} euler      tf  worst |out - fp64| / max(1, |fp64|) {ratio:.2e} at trajectory {b} (gate 2e-6)")
    G = torch.randn(6, B_WIDE, 8, generator=torch.Generator().manual_seed(7))
    _, named = A.ode_grads64(c, "euler", a, G)
    _, got = ode_bwd_hip(c, "euler", a, G)
    bad = _check_grads("K5", "random probe 8/2/64", key, "euler", got, named)
    assert ok and not bad, (ratio, b, bad)


# ------------------------------------------------------------------------------------------------ 4  wide-range trajectories and backwards
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("key", KEYS)
def test_wide_range_trajectory_and_backward(key, method):
    """70 trajectories x 40 grid points, two events, hidden pre-activations from below -17 to above +5 and five rows at +-1e4: <= TOL_GPU
    from the fp32 walk and no further from fp64 than 3 x the fp32 walk's own distance + 1e-7 (traj_gates); every gradient against fp64
    autograd at 2e-4 of its max."""
    a = A.ACTS[key]
    c = A.wide_act_case()
    G = torch.randn(T_WIDE, B_WIDE, 8, generator=torch.Generator().manual_seed(11))
    with E.oracle_elu(a.module()):
        o32 = E.run_ode(c, method)
    t64, named = A.ode_grads64(c, method, a, G)
    xs, got = ode_bwd_hip(c, method, a, G)
    ok, e32, e64, eo = E.traj_gates(xs, o32, t64)
    print(f"[act-range] K0    wide 8/2/64 70 x 40                {key:15s} {method:10s} x   vs fp32 walk {e32:.2e}  vs fp64 {e64:.2e}  the walk's own {eo:.2e} (gate 3 x + 1e-7)")
    bad = _check_grads("K5", "wide 8/2/64 70 x 40", key, method, got, named)
    assert ok and not bad, (e32, e64, eo, bad)


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_wide_range_dae_mixed_pair(pair):
    """The DAE twin (DE and AE both wide, each with its own activation), RK4: xs and is by traj_gates, every gradient at 2e-4."""
    de, ae = entry(pair[0]), entry(pair[1])
    xd, zd, vd, idim, H = 8, 2, 2, 2, 64
    c = E.wide_dae_case(B_WIDE, T_WIDE, xd, zd, vd, idim, H, seed=41)
    g = torch.Generator().manual_seed(12)
    Gx, Gi = torch.randn(T_WIDE, B_WIDE, xd, generator=g), torch.randn(T_WIDE, B_WIDE, idim, generator=g)
    mde, mae = de.module(), ae.module()
    import oracle.psnode_oracle as O

    def walk(dtype):
        req = lambda q: q.detach().to(dtype).clone().requires_grad_(True)
        de_l, ae_l = [(req(w), req(b)) for w, b in c.de], [(req(w), req(b)) for w, b in c.ae]
        xi, z, v, a0, zj, vj = (req(q) for q in (c.xi, c.z, c.v, c.a0, c.zj, c.vj))
        saved = (O.de_rhs, O.ae_rhs)       # the oracle applies F.elu in both MLPs: each right-hand side runs with its own module instead

        def de_rhs(layers, *args):
            with E.oracle_elu(mde):
                return saved[0](layers, *args)

        def ae_rhs(layers, *args):
            with E.oracle_elu(mae):
                return saved[1](layers, *args)
        O.de_rhs, O.ae_rhs = de_rhs, ae_rhs
        try:
            xs, is_ = E.dae_walk64("rk4", de_l, ae_l, xi, c.t.to(dtype), z, v, a0, c.ev.to(dtype), zj, vj)
        finally:
            O.de_rhs, O.ae_rhs = saved
        return xs, is_, (xi, z, v, zj, vj, a0), de_l, ae_l
    with torch.no_grad():
        x32, i32, *_ = walk(torch.float32)
    x64, i64, leaves, de64, ae64 = walk(torch.float64)
    ((x64 * Gx.double()).sum() + (i64 * Gi.double()).sum()).backward()
    f = fused()
    lde, lae = dl(c.de), dl(c.ae)
    tab = f.event_table(cu(c.t), cu(c.ev))
    xe = torch.zeros(T_WIDE, B_WIDE, 0, device="cuda")
    acts = (de.act, ae.act)
    xs, is_ = f.dae_integrate("rk4", lde, lae, cu(c.xi), cu(c.t), xe, cu(c.z), cu(c.v), cu(c.i), cu(c.a0), event_t=cu(c.ev), z_jump=cu(c.zj),
                              v_jump=cu(c.vj), kernel="generic", act=acts)
    gr = f.dae_backward("rk4", lde, lae, cu(c.t), cu(c.z), cu(c.v), cu(c.a0), xs, is_, Gx.cuda(), Gi.cuda(), event_idx=tab, z_jump=cu(c.zj),
                        v_jump=cu(c.vj), kernel="generic", act=acts)
    label = "DAE wide 8/2/2/2/64 " + "+".join(pair)
    oks = []
    for what, out, o32, t64 in (("x", xs, x32, x64.detach()), ("i", is_, i32, i64.detach())):
        ok, e32, e64, eo = E.traj_gates(out.cpu(), o32, t64)
        print(f"[act-range] K0    {label:34s} {'':15s} rk4        {what}   vs fp32 walk {e32:.2e}  vs fp64 {e64:.2e}  the walk's own {eo:.2e} (gate 3 x + 1e-7)")
        oks.append(ok)
    pairs = list(zip(("x_init", "z", "v", "z_jump", "v_jump", "all_initial"), leaves))
    res = [A.close_gate(gr[k], q.grad, k) for k, q in pairs]
    res += [A.close_gate(g_, p.grad, f"grad de {k}") for k, (g_, p) in enumerate(zip(gr["de"], [q for wb in de64 for q in wb]))]
    res += [A.close_gate(g_, p.grad, f"grad ae {k}") for k, (g_, p) in enumerate(zip(gr["ae"], [q for wb in ae64 for q in wb]))]
    print(f"[act-range] K5    {label:34s} {'':15s} rk4        bwd worst " + max(res, key=lambda r: r[2])[1])
    assert all(oks) and all(ok for ok, _, _ in res), [txt for ok, txt, _ in res if not ok]


# ------------------------------------------------------------------------------------------------ 5  the other builds of the same forms
def _builds():
    from py_psnode_amd import neural_dae as nd
    return {"tableau RK4Classic": (nd.RK4Classic().method, {}), "substeps=2": ("euler", dict(substeps=2)),
            "externals=linear": ("euler", dict(externals="linear"))}


@pytest.mark.parametrize("build", ["tableau RK4Classic", "substeps=2", "externals=linear"])
@pytest.mark.parametrize("key", ["Softplus(1,1)", "GELU(tanh)"])
def test_other_builds_carry_the_same_forms(key, build):
    """The tableau, sub-step and linear-externals builds keep u for every kind and compile the forms of psnode_act.h a second time: the
    T = 2 forward probe and the derivative probe, one shape each.  (Two Euler sub-steps of h = 1/2 add k / 2 twice: exact.  The probe's
    z[1] equals z[0], so interpolated externals read the same u.)"""
    method, kw = _builds()[build]
    fails = _grad_probe(A.ACTS[key], key, build, 8, 2, (64, 64, 64), 3, method, **kw)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 6  the extremes set
@pytest.mark.parametrize("shape", [(8, 2, (64, 64, 64)), (20, 3, (96, 96))], ids=["register_3_layers", "streamed_2_layers"])
@pytest.mark.parametrize("key", KEYS)
def test_extremes(key, shape):
    """u = +-1e19, +-3e19, +-1e30, +-3e38 through K0 and K5: every output and every input gradient finite, act^n(u) and prod act' within
    4 x 2^-24 relative of the fp64 limit."""
    xd, zd, hidden = shape
    nh = len(hidden)
    a = A.ACTS[key]
    c = E.identity_probe_ode(xd, zd, hidden, n_hidden=nh, teacher=False, u=A.EXTREMES)
    B, nr = c.t.shape[1], min(xd, zd)
    G = torch.zeros(2, B, xd)
    G[1, :, :nr] = 1.0
    xs, (gx0, gz, _, ga0, _) = ode_bwd_hip(c, "euler", a, G)
    ok, ev, eg = A.extremes_gate(a, xs[1], gz[0, :, :nr].cpu(), c.z[0, :, :nr], nh) if nr == xd else \
        A.extremes_gate(a, xs[1][:, :nr], gz[0, :, :nr].cpu(), c.z[0, :, :nr], nh)
    rest = A.act_n64(a, c.u_of[0], nh)
    ok_all = bool(((xs[1].double() - rest).abs() <= A.EXTREME_REL * rest.abs() + A.TINY).all())         # every output column
    finite = all(bool(torch.isfinite(q).all()) for q in (xs, gx0, gz, ga0))
    print(f"[act-range] K0+K5 {'extremes ' + str(xd) + '/' + str(zd) + '/' + str(hidden[0]) + ' x ' + str(nh):34s} {key:15s} euler      "
          f"worst |out - limit| {ev:.2e}  worst |g - limit| {eg:.2e}  all finite: {finite}")
    assert ok and ok_all and finite, (key, ev, eg, finite)
