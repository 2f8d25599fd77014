"""Cost of four-point Lagrange externals on K0 / K5 (profiles/externals_lagrange_cost.txt).

    python profiles/scripts/externals_lagrange_cost.py [--parent DIR] > profiles/externals_lagrange_cost.txt

B = 4096, 1000 fine steps, hidden 64 x 3, kernel "generic".  ODE: x 20 / z 3.  DAE: x 5 / z 4 / v 6 / i 6 (the shapes of
profiles/externals_linear_cost.txt).  Two blocks, each step a child process under its own time limit; the first that fails ends the script.
  1. RK4Classic and Euler, forward and training step (forward + backward, loss on every output row): externals "linear" against
     "lagrange" on this tree, at T = 251 with substeps = 4 and at T = 1001 with substeps = 1.  The ratio is what the two further node rows
     per stage, the per-interval refill of the node window and K5's four adjoint rows cost.
  2. With --parent DIR (a checkout of the parent commit with its library built): the built-in `rk4` (ELU(1) objects) and RK4Classic with
     externals "linear" (T = 251 x 4) of the ODE shape, forward and training step, one child process per tree and run, alternating.  This
     tree's median has to lie inside the parent's [min .. max].
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


def block1(kind):
    from py_psnode_amd import neural_dae as nd
    Tc = (T_FINE - 1) // N + 1
    dims = {"ode": (20, 3, 0, 0), "dae": (5, 4, 6, 6)}[kind]
    P = {Tc: problem(kind, Tc, dims), T_FINE: problem(kind, T_FINE, dims)}
    for name, method in (("RK4Classic", nd.RK4Classic().method), ("Euler", nd.ExplicitRK(((),), (1.0,), 1, name="Euler-tableau").method)):
        cfg = {(Tn, n, ext): legs(P[Tn], kind, method, n, ext) for Tn, n in ((Tc, N), (T_FINE, 1)) for ext in ("linear", "lagrange")}
        res = {k: ([], []) for k in cfg}
        for _ in range(RUNS):
            for k, (f, tr) in cfg.items():
                res[k][0].append(timed(f)); res[k][1].append(timed(tr))
        for (Tn, n, ext), (f, tr) in res.items():
            print(f"{kind.upper()} {name:10s} T = {Tn:4d} substeps {n} {ext:8s}: fwd {fmt(f)}   train {fmt(tr)}")
        med = lambda k, j: statistics.median(res[k][j])
        for Tn, n in ((Tc, N), (T_FINE, 1)):
            print(f"{kind.upper()} {name:10s} T = {Tn:4d} substeps {n} lagrange / linear: fwd {med((Tn, n, 'lagrange'), 0) / med((Tn, n, 'linear'), 0):.3f}, "
                  f"train {med((Tn, n, 'lagrange'), 1) / med((Tn, n, 'linear'), 1):.3f}")


def existing_only():
    """one run of the tree on sys.path, as a JSON line: the built-in RK4 (T = 1001) and RK4Classic with linear externals (T = 251 x 4) of the
    ODE shape (forward, training step)"""
    from py_psnode_amd import neural_dae as nd
    fwd, train = legs(problem("ode", T_FINE, (20, 3, 0, 0)), "ode", "rk4", 1, "hold")
    lf, lt = legs(problem("ode", (T_FINE - 1) // N + 1, (20, 3, 0, 0)), "ode", nd.RK4Classic().method, N, "linear")
    print(json.dumps({"rk4 fwd": timed(fwd), "rk4 train": timed(train), "linear fwd": timed(lf), "linear train": timed(lt)}))


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
    ap.add_argument("--step", default=None, choices=("ode", "dae", "existing"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return existing_only() if a.step == "existing" else block1(a.step)
    print(f"# B = {B}, {T_FINE - 1} fine steps, hidden 64 x 3, kernel generic; median [min .. max] of {RUNS} alternating runs of {ITERS} launches")
    print("# 1. what the cubic costs: externals linear against lagrange, this tree")
    for kind in ("ode", "dae"):
        print(child(ROOT, "--step", kind, limit=300), end="")
    if a.parent:
        print("# 2. what exists: the built-in rk4 (ELU(1) objects, 1001 points) and RK4Classic with externals linear (251 points x 4), ODE x 20 / z 3: "
              "parent against this tree, a child process per run")
        keys = ("rk4 fwd", "rk4 train", "linear fwd", "linear train")
        out = {"parent": {k: [] for k in keys}, "this tree": {k: [] for k in keys}}
        for _ in range(RUNS):
            for who, root in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                d = json.loads(child(root, "--step", "existing", limit=120).strip().splitlines()[-1])
                for k in keys:
                    out[who][k].append(d[k])
        for who, d in out.items():
            print(f"{who:9s}: " + "   ".join(f"{k} {fmt(v)}" for k, v in d.items()))
        for k in keys:
            m, lo, hi = statistics.median(out["this tree"][k]), min(out["parent"][k]), max(out["parent"][k])
            print(f"{k}: this tree's median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's [{lo:.2f} .. {hi:.2f}]")


if __name__ == "__main__":
    main()
