"""Cost of multiple-shooting segments on K0 / K5 (profiles/segments_cost.txt).

    python profiles/scripts/segments_cost.py [--parent DIR] > profiles/segments_cost.txt

B = 4096, T = 1001, hidden 64 x 3, kernel "generic", one step per grid interval, no events.  ODE: x 20 / z 3.  DAE: x 5 / z 4 / v 6 / i 6
(the shapes of profiles/substeps_cost.txt).  RK4Classic and Euler as tableaus, forward and training step (forward + backward, loss on every
output row).  Each block a child process under its own time limit; the first that fails ends the script.
  1. The free run (segment=None: the tableau build, the kernels such a call ran before this option existed -- their listings are the
     parent's, profiles/segments_listing_diff.txt) against the multiple-shooting build at w = 1000: the same arithmetic, no restart.  The
     ratio is the price of the build (the countdown and the selects).  With --parent DIR the parent tree's own free run is timed too.
  2. w = 50 and w = 10 against w = 1000: what the restarts cost -- for the ODE a dataset row instead of the running state, for the DAE one
     head evaluation per w steps forward, one head forward + VJP backward.
  3. With --parent DIR (a checkout of the parent commit with its library built): the built-in `rk4` (ELU(1) objects) of the ODE shape,
     forward and training step, one child process per tree, alternating.  This tree's median has to lie inside the parent's [min .. max].
Five alternating runs; median and [min .. max] of the runs, each run the mean of ITERS launches between two stream events after one warm-up."""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, T, ITERS, RUNS = 4096, 1001, 3, 5
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


def problem(kind, dims, hidden=(64, 64, 64)):
    import torch
    from py_psnode_amd import models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xd, zd, vd, idim = dims
    t = (torch.arange(T, dtype=torch.float32) / 256.0).view(T, 1, 1).repeat(1, B, 1)
    x, z, v, i = (0.3 * torch.randn(T, B, w, generator=g) for w in (xd, zd, vd, idim))
    n = xd + zd + vd + idim
    if kind == "ode":
        de, ae = models.DE_Func(n, hidden, xd).cuda(), None
    else:
        de, ae = models.DAE_DE_Func(n, hidden, xd).cuda(), models.AE_Func(n + xd + zd + vd, hidden, idim).cuda()
    c = lambda a: a.cuda().contiguous()
    return dict(de=de, ae=ae, rows=tuple(c(q) for q in (t, x, z, v, i)), a0=c(torch.cat((x[0], z[0], v[0], i[0]), -1)), x0=c(x[0]))


def legs(p, kind, method, segment=None):
    """(forward, training step) closures of one problem through the generic route; segment=None: the free run"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    t, x, z, v, i = p["rows"]
    kw = dict(segment=segment) if segment is not None else {}
    de = lay(p["de"], "x_dot")
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    if kind == "ode":
        fwd = lambda: fused.ode_integrate(method, det(de), t, x, z, p["a0"], kernel="generic", **kw)
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
        xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, p["x0"], t, z, v, i, p["a0"], **(dict(x=x, **kw) if kw else {}))
        ((xs * G).sum() + (is_ * Gi).sum()).backward()
    return fwd, train


def block(kind, free_only=False):
    from py_psnode_amd import neural_dae as nd
    dims = (20, 3, 0, 0) if kind == "ode" else (5, 4, 6, 6)
    p = problem(kind, dims)
    rows = (("free run (tableau build)", None),) + (() if free_only else (("w = 1000 (no restart)", 1000), ("w = 50", 50), ("w = 10", 10)))
    for name, method in (("RK4Classic", nd.RK4Classic().method), ("Euler", nd.ExplicitRK(((),), (1.0,), 1, name="Euler-tableau").method)):
        cfg = {label: legs(p, kind, method, w) for label, w in rows}
        res = {k: ([], []) for k in cfg}
        for _ in range(RUNS):
            for k, (f, tr) in cfg.items():
                res[k][0].append(timed(f)); res[k][1].append(timed(tr))
        for k, (f, tr) in res.items():
            print(f"{kind.upper()} {name:10s} {k:28s}: fwd {fmt(f)}   train {fmt(tr)}")
        med = lambda k, j: statistics.median(res[k][j])
        if not free_only:
            print(f"{kind.upper()} {name:10s} w = 1000 / free run: fwd {med(rows[1][0], 0) / med(rows[0][0], 0):.3f}, train {med(rows[1][0], 1) / med(rows[0][0], 1):.3f}")
            for label, _ in rows[2:]:
                print(f"{kind.upper()} {name:10s} {label} / w = 1000: fwd {med(label, 0) / med(rows[1][0], 0):.3f}, train {med(label, 1) / med(rows[1][0], 1):.3f}")


def builtin_only():
    """one run of the tree on sys.path, as a JSON line: the built-in RK4 of the ODE shape (forward, training step), no events"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused, models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    t = (torch.arange(T, dtype=torch.float32) / 256.0).view(T, 1, 1).repeat(1, B, 1).cuda()
    x, z = (0.3 * torch.randn(T, B, 20, generator=g)).cuda(), (0.3 * torch.randn(T, B, 3, generator=g)).cuda()
    m = models.DE_Func(23, (64, 64, 64), 20).cuda()
    de = [(q.weight, q.bias) for q in m.x_dot if isinstance(q, nn.Linear)]
    a0 = torch.cat((x[0], z[0]), -1).contiguous()
    G = torch.randn_like(x)
    fwd = lambda: fused.ode_integrate("rk4", [(w.detach(), b.detach()) for w, b in de], t, x[:1], z, a0, kernel="generic")

    def train():
        for w, b in de:
            w.grad = b.grad = None
        (autograd.fused_ode_integrate("rk4", "generic", de, t, x, z, a0) * G).sum().backward()
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
    ap.add_argument("--step", default=None, choices=("ode", "dae", "ode-free", "dae-free", "builtin"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return builtin_only() if a.step == "builtin" else block(a.step[:3], a.step.endswith("-free"))
    print(f"# B = {B}, T = {T}, hidden 64 x 3, kernel generic, one step per interval, no events; median [min .. max] of {RUNS} alternating runs of {ITERS} launches")
    print("# 1. / 2. the free run against the multiple-shooting build without a restart, then with restarts every 50 and every 10 steps")
    print(child(ROOT, "--step", "ode", limit=400), end="")
    print(child(ROOT, "--step", "dae", limit=400), end="")
    if a.parent:
        print("# 1. (parent tree) the free run of the parent commit's library")
        print(child(os.path.abspath(a.parent), "--step", "ode-free", limit=300), end="")
        print(child(os.path.abspath(a.parent), "--step", "dae-free", limit=300), end="")
        print("# 3. the built-in rk4 (ELU(1) objects), ODE x 20 / z 3, no events: parent against this tree, a child process per run")
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


if __name__ == "__main__":
    main()
