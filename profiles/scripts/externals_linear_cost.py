"""Cost of linearly interpolated externals on K0 / K5 (profiles/externals_linear_cost.txt).

    python profiles/scripts/externals_linear_cost.py [--parent DIR] > profiles/externals_linear_cost.txt

B = 4096, 1000 fine steps, hidden 64 x 3, kernel "generic".  ODE: x 20 / z 3.  DAE: x 5 / z 4 / v 6 / i 6 (the shapes of
profiles/substeps_cost.txt).  Three blocks, each a child process under its own time limit; the first that fails ends the script.
  1. RK4Classic and Euler, forward and training step (forward + backward, loss on every output row): externals "hold" against "linear", at
     T = 251 with substeps = 4 (the sub-step build against the linear build) and at T = 1001 with substeps = 1 (the tableau build against the
     linear build).  The ratio is what interpolation costs.  The alternative a user has without it -- up-sampling the data 4-fold and
     running "hold" on 1001 points -- is the hold row of T = 1001: the last column puts linear at T = 251 x 4 next to it.
  2. With --parent DIR (a checkout of the parent commit with its library built): the built-in `rk4` (ELU(1) objects) of the ODE shape,
     forward and training step, one child process per tree, alternating.  This tree's median has to lie inside the parent's [min .. max].
  3. The refold's share: K0's register form (x 8 / z 2, hidden 64 x 3: the DE's first layer keeps a folded per-step constant, which "linear"
     refolds in front of every stage whose theta changed) against its streamed form at the same step count (x 8 / z 2, hidden 160 x 3: no fold),
     forward, "hold" against "linear".
Five alternating runs; median and [min .. max] of the runs, each run the mean of ITERS launches between two stream events after one warm-up."""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, T_FINE, N, ITERS, RUNS = 4096, 1001, 4, 3, 5
print = functools.partial(print, flush=True)


def timed(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def fmt(v):
    return f"{statistics.median(v):8.2f} ms [{min(v):.2f} .. {max(v):.2f}]"


def problem(kind, Tn, dims, hidden=(64, 64, 64)):
    import torch
    from py_psnode_amd import models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xd, zd, vd, idim = dims
    t = (torch.arange(Tn, dtype=torch.float32) * (1000.0 / (Tn - 1) / 256.0)).view(Tn, 1, 1).repeat(1, B, 1)
    x, z, v, i = (0.3 * torch.randn(Tn, B, w, generator=g) for w in (xd, zd, vd, idim))
    n = xd + zd + vd + idim
    if kind == "ode":
        de, ae = models.DE_Func(n, hidden, xd).cuda(), None
    else:
        de, ae = models.DAE_DE_Func(n, hidden, xd).cuda(), models.AE_Func(n + xd + zd + vd, hidden, idim).cuda()
    c = lambda a: a.cuda().contiguous()
    return dict(de=de, ae=ae, rows=tuple(c(q) for q in (t, x, z, v, i)), a0=c(torch.cat((x[0], z[0], v[0], i[0]), -1)), x0=c(x[0]))


def legs(p, kind, method, substeps, externals):
    """(forward, training step) closures of one problem through the generic route"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    t, x, z, v, i = p["rows"]
    kw = dict(substeps=substeps) if substeps > 1 else {}
    if externals != "hold":
        kw["externals"] = externals
    de = lay(p["de"], "x_dot")
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    if kind == "ode":
        fwd = lambda: fused.ode_integrate(method, det(de), t, x[:1], z, p["a0"], kernel="generic", **kw)
        G = torch.randn_like(x)

        def train():
            for w, b in de:
                w.grad = b.grad = None
            (autograd.fused_ode_integrate(method, "generic", de, t, x, z, p["a0"], **kw) * G).sum().backward()
        return fwd, train
    ae = lay(p["ae"], "i_calculator")
    fwd = lambda: fused.dae_integrate(method, det(de), det(ae), p["x0"], t, x, z, v, i, p["a0"], kernel="generic", **kw)
    G, Gi = torch.randn(x.shape, device="cuda"), torch.randn_like(i)

    def train():
        for w, b in de + ae:
            w.grad = b.grad = None
        xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, p["x0"], t, z, v, i, p["a0"], **kw)
        ((xs * G).sum() + (is_ * Gi).sum()).backward()
    return fwd, train


def block1():
    from py_psnode_amd import neural_dae as nd
    Tc = (T_FINE - 1) // N + 1
    for kind, dims in (("ode", (20, 3, 0, 0)), ("dae", (5, 4, 6, 6))):
        P = {Tc: problem(kind, Tc, dims), T_FINE: problem(kind, T_FINE, dims)}
        for name, method in (("RK4Classic", nd.RK4Classic().method), ("Euler", nd.ExplicitRK(((),), (1.0,), 1, name="Euler-tableau").method)):
            cfg = {(Tn, n, ext): legs(P[Tn], kind, method, n, ext) for Tn, n in ((Tc, N), (T_FINE, 1)) for ext in ("hold", "linear")}
            res = {k: ([], []) for k in cfg}
            for _ in range(RUNS):
                for k, (f, tr) in cfg.items():
                    res[k][0].append(timed(f)); res[k][1].append(timed(tr))
            for (Tn, n, ext), (f, tr) in res.items():
                print(f"{kind.upper()} {name:10s} T = {Tn:4d} substeps {n} {ext:6s}: fwd {fmt(f)}   train {fmt(tr)}")
            med = lambda k, j: statistics.median(res[k][j])
            for Tn, n in ((Tc, N), (T_FINE, 1)):
                print(f"{kind.upper()} {name:10s} T = {Tn:4d} substeps {n} linear / hold: fwd {med((Tn, n, 'linear'), 0) / med((Tn, n, 'hold'), 0):.3f}, "
                      f"train {med((Tn, n, 'linear'), 1) / med((Tn, n, 'hold'), 1):.3f}")
            print(f"{kind.upper()} {name:10s} linear at T = {Tc} x {N} / hold on the {N}-fold up-sampled data (T = {T_FINE}): "
                  f"fwd {med((Tc, N, 'linear'), 0) / med((T_FINE, 1, 'hold'), 0):.3f}, train {med((Tc, N, 'linear'), 1) / med((T_FINE, 1, 'hold'), 1):.3f}")


def block3():
    from py_psnode_amd import neural_dae as nd
    method = nd.RK4Classic().method
    Tc = (T_FINE - 1) // N + 1
    for form, hidden in (("register form, hidden 64 x 3", (64, 64, 64)), ("streamed form, hidden 160 x 3", (160, 160, 160))):
        p = problem("ode", Tc, (8, 2, 0, 0), hidden)
        cfg = {ext: legs(p, "ode", method, N, ext)[0] for ext in ("hold", "linear")}
        res = {k: [] for k in cfg}
        for _ in range(RUNS):
            for k, f in cfg.items():
                res[k].append(timed(f))
        for k, v in res.items():
            print(f"ODE x 8 / z 2, {form}, RK4Classic T = {Tc} substeps {N} {k:6s}: fwd {fmt(v)}")
        print(f"ODE x 8 / z 2, {form}: linear / hold fwd {statistics.median(res['linear']) / statistics.median(res['hold']):.3f} "
              f"(+ {statistics.median(res['linear']) - statistics.median(res['hold']):.3f} ms)")


def builtin_only():
    """one run of the tree on sys.path, as a JSON line: the built-in RK4 of the ODE shape (forward, training step)"""
    fwd, train = legs(problem("ode", T_FINE, (20, 3, 0, 0)), "ode", "rk4", 1, "hold")
    print(json.dumps({"fwd": timed(fwd), "train": timed(train)}))


def child(root, *args, limit):
    """a GPU step: its own process under its own time limit; a failure or a time-out raises and ends the script"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args], cwd=root, env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, check=False)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"step {args} in {root} ended with status {r.returncode}: nothing further is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--step", default=None, choices=("block1", "block3", "builtin"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return {"block1": block1, "block3": block3, "builtin": builtin_only}[a.step]()
    print(f"# B = {B}, {T_FINE - 1} fine steps, hidden 64 x 3, kernel generic; median [min .. max] of {RUNS} alternating runs of {ITERS} launches")
    print("# 1. what interpolation costs: externals hold against linear")
    print(child(ROOT, "--step", "block1", limit=420), end="")
    if a.parent:
        print("# 2. the built-in rk4 (ELU(1) objects), ODE x 20 / z 3, 1001 points: parent against this tree, a child process per run")
        out = {"parent": ([], []), "this tree": ([], [])}
        for _ in range(RUNS):
            for k, root in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                d = json.loads(child(root, "--step", "builtin", limit=120).strip().splitlines()[-1])
                out[k][0].append(d["fwd"]); out[k][1].append(d["train"])
        for k, (f, tr) in out.items():
            print(f"built-in rk4, {k:9s}: fwd {fmt(f)}   train {fmt(tr)}")
        for j, leg in enumerate(("fwd", "train")):
            m, lo, hi = statistics.median(out["this tree"][j]), min(out["parent"][j]), max(out["parent"][j])
            print(f"built-in rk4 {leg}: this tree's median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's [{lo:.2f} .. {hi:.2f}]")
    print("# 3. the refold's share: K0's register form against its streamed form, forward")
    print(child(ROOT, "--step", "block3", limit=180), end="")


if __name__ == "__main__":
    main()
