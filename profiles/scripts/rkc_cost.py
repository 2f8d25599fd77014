"""Cost of the Runge-Kutta-Chebyshev recurrence on K0 / K5 (profiles/rkc_cost.txt).

    python profiles/scripts/rkc_cost.py --parent DIR > profiles/rkc_cost.txt

B = 4096, T = 1001, hidden 64 x 3, kernel "generic".  ODE: x 20 / z 3.  DAE: x 5 / z 4 / v 6 / i 6.  Forward and training step (forward +
backward, loss on every output row).  DIR: a checkout of the parent commit with its library built.  Every run is a child process of its
own -- one tree, one method, one shape -- under its own time limit; the first that fails ends the script.  Five alternating runs; median
and [min .. max], each run the mean of ITERS launches between two stream events after one warm-up.
  1. RKC1 / RKC2 with 4 and 8 stages against Euler(substeps=4 / 8) of this tree: the same number of right-hand-side evaluations (and, for
     the DAE, of heads), so the ratio is the price of the recurrence -- two more LDS vectors per stage pass and four more multiply-adds.
  2. The built-in `rk4` (ELU(1) objects) and Euler(substeps=4) (the sub-step objects) of the parent against this tree: the listings say
     they are the same code (profiles/rkc_listing_diff.txt), so this tree's median has to lie inside the parent's [min .. max].
A single run for a profiler: `PYTHONPATH=. python profiles/scripts/rkc_cost.py --step ode|dae rkc1_4|rkc1_8|rkc2_4|rkc2_8|euler_sub4|euler_sub8|rk4`."""
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


def one_run(kind, method):
    """one run of the tree on sys.path, as a JSON line: forward and training step of `method` on the ODE or the DAE shape"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused, models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xd, zd, vd, idim = (20, 3, 0, 0) if kind == "ode" else (5, 4, 6, 6)
    kw = {}
    if method.startswith("rkc"):          # rkc<order>_<stages>: the solver classes' method value
        method = fused.rkc_table(int(method[5:]), int(method[3]))
    elif method.startswith("euler_sub"):
        method, kw = "euler", dict(substeps=int(method[9:]))
    t = (torch.arange(T, dtype=torch.float32) / 256.0).view(T, 1, 1).repeat(1, B, 1).cuda()
    x, z, v, i = ((0.3 * torch.randn(T, B, w, generator=g)).cuda() for w in (xd, zd, vd, idim))
    ev = zj = vj = None
    n = xd + zd + vd + idim
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1).contiguous()
    de = lay(models.DE_Func(n, (64, 64, 64), xd).cuda() if kind == "ode" else models.DAE_DE_Func(n, (64, 64, 64), xd).cuda(), "x_dot")
    if kind == "ode":
        G = torch.randn_like(x)
        fwd = lambda: fused.ode_integrate(method, det(de), t, x[:1], z, a0, ev, zj, kernel="generic", **kw)

        def train():
            for w, b in de:
                w.grad = b.grad = None
            (autograd.fused_ode_integrate(method, "generic", de, t, x, z, a0, ev, zj, **kw) * G).sum().backward()
    else:
        ae = lay(models.AE_Func(n + xd + zd + vd, (64, 64, 64), idim).cuda(), "i_calculator")
        x0 = x[0].contiguous()
        G, Gi = torch.randn_like(x), torch.randn_like(i)
        fwd = lambda: fused.dae_integrate(method, det(de), det(ae), x0, t, x, z, v, i, a0, ev, zj, vj, kernel="generic", **kw)

        def train():
            for w, b in de + ae:
                w.grad = b.grad = None
            xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, x0, t, z, v, i, a0, ev, zj, vj, **kw)
            ((xs * G).sum() + (is_ * Gi).sum()).backward()
    print(json.dumps({"fwd": timed(fwd), "train": timed(train)}))


def child(root, *args, limit):
    """a GPU step: its own process under its own time limit; a failure or a time-out raises and ends the script"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args], cwd=root, env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, check=False)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"step {args} in {root} ended with status {r.returncode}: nothing further is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def alternate(kind, cfg):
    """{label: ([fwd ...], [train ...])} of RUNS rounds over cfg = ((label, tree, method), ...)"""
    res = {k: ([], []) for k, _, _ in cfg}
    for _ in range(RUNS):
        for k, root, method in cfg:
            d = child(root, "--step", kind, method, limit=120)
            res[k][0].append(d["fwd"]); res[k][1].append(d["train"])
    for k, (f, tr) in res.items():
        print(f"{kind.upper()} {k:28s}: fwd {fmt(f)}   train {fmt(tr)}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=False, default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--step", nargs=2, default=None, metavar=("KIND", "METHOD"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return one_run(*a.step)
    if not a.parent:
        raise SystemExit("--parent DIR is required: the comparison is against the parent commit's rk4 and Euler(substeps=4)")
    parent = os.path.abspath(a.parent)
    print(f"# B = {B}, T = {T}, hidden 64 x 3, kernel generic; median [min .. max] of {RUNS} alternating runs of {ITERS} launches, a child process per run")
    print("# 1. RKC1 / RKC2 (this tree) against Euler with as many sub-steps (this tree);  2. rk4 and Euler(substeps=4): parent against this tree")
    for kind in ("ode", "dae"):
        res = alternate(kind, (("parent rk4", parent, "rk4"), ("this tree rk4", ROOT, "rk4"), ("parent Euler(substeps=4)", parent, "euler_sub4"),
                               ("this tree Euler(substeps=4)", ROOT, "euler_sub4"), ("this tree Euler(substeps=8)", ROOT, "euler_sub8"),
                               ("this tree RKC1(stages=4)", ROOT, "rkc1_4"), ("this tree RKC2(stages=4)", ROOT, "rkc2_4"),
                               ("this tree RKC1(stages=8)", ROOT, "rkc1_8"), ("this tree RKC2(stages=8)", ROOT, "rkc2_8")))
        med = lambda k, j: statistics.median(res[k][j])
        for n in (4, 8):
            for o in (1, 2):
                k, e = f"this tree RKC{o}(stages={n})", f"this tree Euler(substeps={n})"
                print(f"{kind.upper()} RKC{o}(stages={n}) / Euler(substeps={n}): fwd {med(k, 0) / med(e, 0):.3f}, train {med(k, 1) / med(e, 1):.3f}")
        for name in ("rk4", "Euler(substeps=4)"):
            for j, leg in enumerate(("fwd", "train")):
                m, lo, hi = med(f"this tree {name}", j), min(res[f"parent {name}"][j]), max(res[f"parent {name}"][j])
                print(f"{kind.upper()} {name} {leg}: this tree's median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's [{lo:.2f} .. {hi:.2f}]")


if __name__ == "__main__":
    main()
