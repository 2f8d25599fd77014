"""The instrument of the ELU range tests, tested on the CPU (elu_range_cases.py; the GPU file test_gpu_elu_range.py applies the same
cases and gates to the HIP kernels), so that a green GPU run means something:
  * the wide recipe reaches the whole activation range in EVERY hidden layer of every shape class the GPU file runs;
  * the fp32 oracle -- the reference alone -- passes every gate, on every case (no skip list);
  * every mutant of the oracle's ELU (run in fp64, so that nothing but the mutation separates it from the truth) is rejected by a probe
    gate, and the trajectory gates reject the mutants the table below names;
  * the identity probes are exact: with an activation of exact IEEE operations in ELU's place the fp32 oracle returns its n-fold
    composition bit for bit; with ELU it returns torch's own fp32 ELU^n(u) to one ulp (bit equality is not attainable against ATen: its
    vectorised and scalar expm1 paths differ in the last bit, and which one an element takes depends on its position in the tensor);
  * the ELU' gate of the backward probes accepts fp32 autograd through the oracle and rejects every mutant's derivative."""
import pytest
import torch
import torch.nn.functional as F

import elu_range_cases as E

METHODS = ("euler", "midpoint", "rk4")
# (xd, zd, H, n_hidden, kwargs): the ODE shape classes of test_gpu_elu_range.py.  z_dim == 0 has no external input to widen: there the
# spread comes from the biases alone (bias_amp 8, gain 2; measured per layer: 42 % / 28 % / 3.0 % / 18 % at the least).
ODE_CLASSES = [(8, 2, 64, 3, {}), (5, 3, 48, 3, {}), (3, 0, 33, 3, dict(gain=2.0, bias_amp=8.0)), (12, 2, 128, 3, {}), (8, 2, 256, 3, {}),
               (20, 2, 64, 3, {}), (8, 2, 48, 1, {}), (8, 2, 32, 5, {}), (20, 2, 128, 3, {}), (8, 2, 128, 4, {}), (8, 2, 320, 3, {}),
               (8, 2, 64, 4, {}), (8, 2, 256, 2, {}),
               (16, 16, 16, 1, {}), (64, 64, 64, 1, {}), (96, 96, 96, 1, {})]
# i_dim 2 at the padded class: with ONE head output a T = 2 random probe's scale is a single number, and the fp32 oracle itself then
# sits at 2.4e-6 .. 3.2e-6 of it (three of four seeds), above the 2e-6 one-evaluation gate; with two outputs it stays below 1.6e-6.
DAE_CLASSES = [(8, 2, 2, 2, 64), (5, 1, 1, 2, 48), (8, 4, 6, 6, 64)]
LATENT_DAE = [16, 64, 96]


def _assert_coverage(pre, max_x, what):
    for k, p in enumerate(pre):
        for share, (_, need, band) in zip(E.coverage_shares(p), E.COVERAGE):
            assert share >= need, f"{what}: hidden layer {k}: {share:.3f} of the pre-activations {band}, need {need}"
    assert 0.5 <= max_x <= 100.0, f"{what}: max |x| = {max_x}: the trajectory scale must be set by the dynamics"


@pytest.mark.parametrize("xd,zd,H,nh,kw", ODE_CLASSES)
def test_wide_recipe_reaches_the_whole_range_in_every_layer_ode(xd, zd, H, nh, kw):
    """Measured with the defaults (gain 3, bias_amp 1, amp_hi 30) at (8, 2, 64): at the least 45 % < -0.25, 8.8 % < -5, 1.9 % < -17,
    9.5 % > +5 over the three layers, max |x| 11.9.  (gain 2 leaves the third layer at 3.1 % < -5 and 0.1 % < -17.)"""
    c = E.wide_ode_case(70, 40, xd, zd, H, seed=11, n_hidden=nh, **kw)
    pre, max_x = E.preactivation_stats(c)
    assert len(pre) == nh
    _assert_coverage(pre, max_x, (xd, zd, H, nh))
    for m in METHODS:
        assert bool(torch.isfinite(E.run_ode(c, m, torch.float64)).all())


@pytest.mark.parametrize("dims", DAE_CLASSES)
def test_wide_recipe_reaches_the_whole_range_in_every_layer_dae(dims):
    c = E.wide_dae_case(70, 40, *dims, seed=13)
    pre, max_x = E.preactivation_stats(c)
    assert len(pre) == 6            # DE and AE
    _assert_coverage(pre, max_x, dims)
    for m in METHODS:
        xs, is_ = E.run_dae(c, m, torch.float64)
        assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(is_).all())


def test_standard_inputs_stay_in_the_identity_window():
    """What the new inputs are for: the suite's usual recipe (gain 1, no extra bias, 0.1 randn externals) never leaves (-1, 1)."""
    c = E.wide_ode_case(64, 40, 8, 2, 64, seed=0, gain=1.0, bias_amp=0.0, amp_hi=0.1, events=False)
    pre, _ = E.preactivation_stats(c)
    assert max(float(p.abs().max()) for p in pre) < 1.0


@pytest.mark.parametrize("H", LATENT_DAE)
def test_wide_recipe_and_gates_on_the_latent_dae_shapes(H):
    """x = z = v = i = H, one hidden layer: coverage, the fp32 oracle under the trajectory and probe gates."""
    c = E.wide_dae_case(70, 40, H, H, H, H, H, seed=13, n_hidden=1)
    pre, max_x = E.preactivation_stats(c)
    assert len(pre) == 2
    _assert_coverage(pre, max_x, H)
    for m in METHODS:
        (x32, i32), (x64, i64) = E.run_dae(c, m), E.run_dae(c, m, torch.float64)
        assert E.traj_gates(x32, x32, x64)[0] and E.traj_gates(i32, i32, i64)[0]
    p = E.random_probe_dae(70, 12, H, H, H, H, H, seed=19, n_hidden=1, teacher=False)
    (x32, i32), (x64, i64) = E.probe_run_dae(p), E.probe_run_dae(p, dtype=torch.float64)
    assert E.random_probe_gate(x32, x64)[0] and E.random_probe_gate(i32, i64)[0]
    q = E.identity_probe_dae(H, H, H, H, H, n_hidden=1, teacher=False)
    xs, is_ = E.probe_run_dae(q)
    assert E.identity_gate_plain(xs[1:], q.u_x, 1)[0] and E.identity_gate_plain(is_, q.u_i, 1)[0]


# ---- the reference alone passes every gate
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("xd,zd,H,nh,kw", ODE_CLASSES)
def test_fp32_oracle_passes_the_trajectory_gates_ode(xd, zd, H, nh, kw, method):
    c = E.wide_ode_case(70, 40, xd, zd, H, seed=11, n_hidden=nh, **kw)
    o32, t64 = E.run_ode(c, method), E.run_ode(c, method, torch.float64)
    ok, e32, e64, eo = E.traj_gates(o32, o32, t64)
    assert ok and e32 == 0.0 and e64 == eo
    assert eo <= 1e-6, f"the oracle's own fp32 error {eo:.2e}: the second gate would be looser than the saturation mutant needs"


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dims", DAE_CLASSES)
def test_fp32_oracle_passes_the_trajectory_gates_dae(dims, method):
    c = E.wide_dae_case(70, 40, *dims, seed=13)
    (x32, i32), (x64, i64) = E.run_dae(c, method), E.run_dae(c, method, torch.float64)
    assert E.traj_gates(x32, x32, x64)[0] and E.traj_gates(i32, i32, i64)[0]


@pytest.mark.parametrize("teacher", [True, False])
@pytest.mark.parametrize("xd,zd,H,nh", [c[:4] for c in ODE_CLASSES if c[1]])          # every class with a z to feed the probe through
def test_identity_probe_is_exact_on_the_fp32_oracle(xd, zd, H, nh, teacher):
    """The construction is exact (products with 1.0, sums with 0.0, dt = 1): with an activation made of exact IEEE operations in the
    oracle's place (u > 0 ? u : u / 2) the fp32 oracle returns that function's n-fold composition of u BIT FOR BIT; with ELU it returns
    torch's fp32 ELU^n(u) -- compared to one ulp per ELU, because ATen's vectorised and scalar expm1 paths differ in the last bit and which one an
    element takes depends on its position in the tensor (4 of 36960 values here).  Every probe value is evaluated, and the fp32 oracle
    passes both identity gates."""
    c = E.identity_probe_ode(xd, zd, H, n_hidden=nh, teacher=teacher)
    half = lambda u: torch.where(u > 0, u, 0.5 * u)
    with E.oracle_elu(half):
        got = E.probe_run_ode(c)
    want = c.u_of
    for _ in range(nh):
        want = half(want)
    assert torch.equal(got[1:], want)
    out = E.probe_run_ode(c)
    want = c.u_of
    for _ in range(nh):
        want = F.elu(want)
    assert bool(((out[1:] - want).abs() <= nh * 2.0 ** -23 * want.abs()).all())         # one ulp per ELU
    assert float((out[1:] != want).float().mean()) < 1e-3
    assert set(E.probe_magnitudes().tolist()) <= set(c.u_of.reshape(-1).tolist())
    for gate in (E.identity_gate_plain, E.identity_gate_scaled):
        ok, err, bound, at = gate(out[1:], c.u_of, nh)
        assert ok, (gate.__name__, err, bound, at)
    if not teacher:
        for m in ("midpoint", "rk4"):       # x-independent f: every stage equal, x1 = dt f up to the stage weights' rounding
            ok, err, bound, at = E.identity_gate_plain(E.probe_run_ode(c, m)[1:], c.u_of, nh, rel_slack=E.STAGE_SLACK)
            assert ok, (m, err, bound, at)


@pytest.mark.parametrize("teacher", [True, False])
@pytest.mark.parametrize("dims", DAE_CLASSES)
def test_identity_probe_is_exact_on_the_fp32_oracle_dae(dims, teacher):
    c = E.identity_probe_dae(*dims, teacher=teacher)
    xs, is_ = E.probe_run_dae(c)
    e3 = lambda u: F.elu(F.elu(F.elu(u)))
    for got, want in ((xs[1:], e3(c.u_x)), (is_, e3(c.u_i))):       # (one ulp: ATen's two expm1 paths, see the ODE test)
        assert bool(((got - want).abs() <= 2.0 ** -23 * want.abs()).all()) and float((got != want).float().mean()) < 1e-3
    half = lambda u: torch.where(u > 0, u, 0.5 * u)
    with E.oracle_elu(half):
        xs_h, is_h = E.probe_run_dae(c)
    assert torch.equal(xs_h[1:], half(half(half(c.u_x)))) and torch.equal(is_h, half(half(half(c.u_i))))
    assert E.identity_gate_plain(xs[1:], c.u_x, 3)[0] and E.identity_gate_plain(is_, c.u_i, 3)[0]
    assert E.identity_gate_scaled(xs[1:], c.u_x, 3)[0] and E.identity_gate_scaled(is_, c.u_i, 3)[0]


@pytest.mark.parametrize("xd,zd,H,nh,kw", [c for c in ODE_CLASSES if c[1]])       # the probes feed their values through z
def test_fp32_oracle_passes_the_random_probe_gate_ode(xd, zd, H, nh, kw):
    for teacher in (True, False):
        c = E.random_probe_ode(70, 12, xd, zd, H, seed=17, n_hidden=nh, teacher=teacher, **kw)
        ok, ratio, b = E.random_probe_gate(E.probe_run_ode(c), E.probe_run_ode(c, dtype=torch.float64))
        assert ok, (teacher, ratio, b)


@pytest.mark.parametrize("dims", DAE_CLASSES)
def test_fp32_oracle_passes_the_random_probe_gate_dae(dims):
    for teacher in (True, False):
        c = E.random_probe_dae(70, 12, *dims, seed=19, teacher=teacher)
        (x32, i32), (x64, i64) = E.probe_run_dae(c), E.probe_run_dae(c, dtype=torch.float64)
        assert E.random_probe_gate(x32, x64)[0] and E.random_probe_gate(i32, i64)[0]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("xd,zd,H,nh", [(8, 2, 64, 3), (5, 3, 48, 3)])
def test_carry_probe_is_exact_on_the_fp32_oracle(xd, zd, H, nh, method):
    """The multi-step probe without teacher forcing: zeros up to the probed row, then ELU^n(u) carried unchanged to the end."""
    c = E.identity_carry_probe_ode(xd, zd, H, n_hidden=nh)
    assert set(E.probe_magnitudes().tolist()) <= set(c.u_of.reshape(-1).tolist())
    half = lambda u: torch.where(u > 0, u, 0.5 * u)
    with E.oracle_elu(half):
        got = E.probe_run_ode(c, "euler")
    assert float(got[:c.row + 1].abs().max()) == 0.0
    assert torch.equal(got[c.row + 1:], half(half(half(c.u_of))).expand(got.shape[0] - c.row - 1, -1, -1))
    out = E.probe_run_ode(c, method)
    assert float(out[:c.row + 1].abs().max()) == 0.0
    slack = 0.0 if method == "euler" else E.STAGE_SLACK
    for j in range(c.row + 1, out.shape[0]):
        assert torch.equal(out[j], out[c.row + 1])
        assert E.identity_gate_plain(out[j], c.u_of, nh, rel_slack=slack)[0] and E.identity_gate_scaled(out[j], c.u_of, nh, rel_slack=slack)[0]
    with E.oracle_elu(E.ELU_MUTANTS["deep_branch_2e-5"]):
        assert not E.identity_gate_plain(E.probe_run_ode(c, dtype=torch.float64)[-1], c.u_of, nh)[0]


def _probe_grad(c, nh, dtype, elu=None):
    """dL/dz[0] of the T = 2 identity probe with a one-hot dL/dxs, by autograd through the oracle's loop."""
    nr = min(c.xd, c.zd)
    k = lambda a: a.to(dtype)
    z = k(c.z).clone().requires_grad_(True)
    ls = [(k(w), k(b)) for w, b in c.layers]
    with E.oracle_elu(elu if elu is not None else F.elu):
        xs = E.ode_walk64("euler", ls, k(c.t), k(c.x[0]), z, k(c.a0))
    xs[1, :, :nr].sum().backward()
    return z.grad[0, :, :nr], c.z[0, :, :nr]


@pytest.mark.parametrize("nh", [1, 3, 4])
def test_elu_grad_gate_accepts_the_oracle_and_rejects_every_mutant(nh):
    """The gate of the backward probes (prod ELU' through n layers; bound n (n + 1) / 2 * 1.2e-7 + (2 n - 1) 2^-24): fp32 autograd through
    the oracle passes, incl. exactly 1 at u >= 0 and exactly 0 from -88 down; the derivative of every mutant (fp64 autograd) exceeds it."""
    c = E.identity_probe_ode(8, 2, 64, n_hidden=nh, teacher=False)
    got, u = _probe_grad(c, nh, torch.float32)
    ok, err, bound, at = E.elu_grad_gate(got, u, nh, exact_zero=False)      # ATen differentiates ELU as e^u: 6e-39 at -88, not 0
    assert ok, (err, bound, at)
    assert E.elu_grad_gate(torch.where(u <= -88, torch.zeros_like(got), got), u, nh)[0]
    for name, fn in E.ELU_MUTANTS.items():
        got, u = _probe_grad(c, nh, torch.float64, fn)
        ok, err, bound, at = E.elu_grad_gate(got, u, nh, exact_zero=False)
        print(f"mutant {name:18s} ELU' gate n={nh}: worst error {err:.2e} (bound {bound:.2e}) at u = {at:.6g}")
        assert not ok and not err <= bound, (name, err, bound, at)        # (a NaN derivative, 0 * inf under torch.where, is a rejection too)


# ---- the mutants
# What the TRAJECTORY gates (wide_ode_case(70, 40, 8, 2, 64), every method) must reject.  Not in the list, with the reason:
#   deep_branch_2e-5   : its error 2e-5 e^u <= 2.7e-6 per evaluation reaches the trajectory as 5.1e-7 .. 5.5e-7 (measured), below
#                        3 x the oracle's own 2.6e-7 .. 3.1e-7 + 1e-7 -- a whole-trajectory gate tied to fp32 noise cannot see it;
#   negative_rel_2e-6  : 9.4e-7 .. 1.0e-6 against a gate of 0.9e-6 .. 1.0e-6: on the edge, rejected under Midpoint only.
# Both are the probe gates' to catch, and they do (below).
TRAJ_VISIBLE = ("saturate_at_-9", "clamp_at_32", "clamp_at_88", "zero_above_-1e-3")


@pytest.mark.parametrize("method", METHODS)
def test_trajectory_gates_reject_the_visible_mutants(method):
    c = E.wide_ode_case(70, 40, 8, 2, 64, seed=11)
    o32, t64 = E.run_ode(c, method), E.run_ode(c, method, torch.float64)
    for name, fn in E.ELU_MUTANTS.items():
        with E.oracle_elu(fn):
            mu = E.run_ode(c, method, torch.float64)
        ok, e32, e64, eo = E.traj_gates(mu, o32, t64)
        print(f"mutant {name:18s} {method:8s} vs fp32 oracle {e32:.2e}  vs fp64 {e64:.2e}  (oracle's own {eo:.2e})  {'passes' if ok else 'REJECTED'}")
        if name in TRAJ_VISIBLE:
            assert not ok, (name, e32, e64, eo)
    # the project's 1e-5 gate alone is too coarse for the saturation mutant: it is the fp64-tied gate that rejects it
    with E.oracle_elu(E.ELU_MUTANTS["saturate_at_-9"]):
        assert E.traj_rel_err(E.run_ode(c, method, torch.float64), o32) <= E.TOL_GPU


@pytest.mark.parametrize("name", sorted(E.ELU_MUTANTS))
def test_probe_gates_reject_every_mutant(name):
    """Each mutant through the identity probe on the fp64 oracle: both identity gates (plain and scaled-domain bound) reject it, with
    and without teacher forcing, for 1 and 3 hidden layers."""
    fn = E.ELU_MUTANTS[name]
    for nh, teacher in ((3, True), (3, False), (1, True)):
        c = E.identity_probe_ode(8, 2, 64, n_hidden=nh, teacher=teacher)
        with E.oracle_elu(fn):
            out = E.probe_run_ode(c, dtype=torch.float64)
        clean = E.probe_run_ode(c, dtype=torch.float64)
        for gate in (E.identity_gate_plain, E.identity_gate_scaled):
            assert gate(clean[1:], c.u_of, nh)[0], "the unmutated fp64 oracle passes"
            ok, err, bound, at = gate(out[1:], c.u_of, nh)
            print(f"mutant {name:18s} {gate.__name__:22s} n={nh} worst error {err:.2e} (bound {bound:.2e}) at u = {at:.6g}")
            assert not ok, (name, gate.__name__, nh, teacher)


def test_random_probe_gate_rejects_the_range_mutants():
    """The random probe (2e-6 per evaluation) sees the mutants whose error exceeds it: early saturation, the clamps, the flushed shallow
    side.  The two 1e-6-class mutants (deep_branch_2e-5: <= 2.7e-6 at one unit, negative_rel_2e-6) are below a 2e-6 output gate after the
    last layer's weights (|w| <= 1/8): the identity probes are the gate for those."""
    c = E.random_probe_ode(70, 12, 8, 2, 64, seed=17)
    ref = E.probe_run_ode(c, dtype=torch.float64)
    assert E.random_probe_gate(E.probe_run_ode(c), ref)[0]
    for name in ("saturate_at_-9", "clamp_at_32", "clamp_at_88", "zero_above_-1e-3"):
        with E.oracle_elu(E.ELU_MUTANTS[name]):
            ok, ratio, b = E.random_probe_gate(E.probe_run_ode(c, dtype=torch.float64), ref)
        assert not ok, (name, ratio)


def test_oracle_elu_swap_is_undone():
    from oracle import psnode_oracle as O
    with E.oracle_elu(lambda u: u):
        assert O.F.elu(torch.tensor(-1.0)) == -1.0
    assert O.F is F
