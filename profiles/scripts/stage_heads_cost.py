"""Cost of stage-wise algebraic heads on K0 / K5 (profiles/stage_heads_cost.txt).

    python profiles/scripts/stage_heads_cost.py [--parent DIR] > profiles/stage_heads_cost.txt

B = 4096, T = 1001, DAE x 5 / z 4 / v 6 / i 6, hidden 64 x 3, kernel "generic", one sub-step.  Two blocks, each step a child process under its
own time limit; the first that fails ends the script.
  1. Forward and training step (forward + backward, loss on every output row) of RK4Classic(externals="lagrange") and
     Heun2(externals="linear") under algebraic "stage" against "step" on this tree, and of AB3() next to them.  Expected from the MAC counts
     at this shape (DE 12 544, AE 10 880 per evaluation): (4 DE + 4 AE) / (4 DE + 1 AE) = 1.53 for four stages, (2 DE + 2 AE) /
     (2 DE + 1 AE) = 1.30 for two -- forward; K5 recomputes a stage's i in front of its VJP, so a training step has more than that.
  2. With --parent DIR (a checkout of the parent commit with its library built): the built-in `rk4` DAE run (ELU(1) objects), forward and
     training step, one child process per tree and run, alternating.  This tree's median has to lie inside the parent's [min .. max].
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
DIMS = (5, 4, 6, 6)
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


def problem(hidden=(64, 64, 64)):
    import torch
    from py_psnode_amd import models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xd, zd, vd, idim = DIMS
    t = (torch.arange(T, dtype=torch.float32) * (1000.0 / (T - 1) / 256.0)).view(T, 1, 1).repeat(1, B, 1)
    x, z, v, i = (0.3 * torch.randn(T, B, w, generator=g) for w in (xd, zd, vd, idim))
    n = xd + zd + vd + idim
    de, ae = models.DAE_DE_Func(n, hidden, xd).cuda(), models.AE_Func(n + xd + zd + vd, hidden, idim).cuda()
    c = lambda a: a.cuda().contiguous()
    return dict(de=de, ae=ae, rows=tuple(c(q) for q in (t, x, z, v, i)), a0=c(torch.cat((x[0], z[0], v[0], i[0]), -1)), x0=c(x[0]))


def legs(p, method, **kw):
    """(forward, training step) closures of the problem through the generic route; kw: externals= / algebraic="""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    t, x, z, v, i = p["rows"]
    de, ae = lay(p["de"], "x_dot"), lay(p["ae"], "i_calculator")
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    fwd = lambda: fused.dae_integrate(method, det(de), det(ae), p["x0"], t, x, z, v, i, p["a0"], kernel="generic", **kw)
    G, Gi = torch.randn(x.shape, device="cuda"), torch.randn_like(i)

    def train():
        for w, b in de + ae:
            w.grad = b.grad = None
        xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, p["x0"], t, z, v, i, p["a0"], **kw)
        ((xs * G).sum() + (is_ * Gi).sum()).backward()
    return fwd, train


def block1():
    from py_psnode_amd import fused
    from py_psnode_amd import neural_dae as nd
    p = problem()
    cfg = {}
    for name, method, ext in (("RK4Classic lagrange", nd.RK4Classic().method, "lagrange"), ("Heun2 linear", nd.Heun2().method, "linear")):
        for alg in ("step", "stage"):
            cfg[(name, alg)] = legs(p, method, externals=ext, **(dict(algebraic="stage") if alg == "stage" else {}))
    cfg[("AB3", "-")] = legs(p, fused.AB3)
    res = {k: ([], []) for k in cfg}
    for _ in range(RUNS):
        for k, (f, tr) in cfg.items():
            res[k][0].append(timed(f)); res[k][1].append(timed(tr))
    for (name, alg), (f, tr) in res.items():
        print(f"{name:20s} {alg:5s}: fwd {fmt(f)}   train {fmt(tr)}")
    med = lambda k, j: statistics.median(res[k][j])
    for name, flop in (("RK4Classic lagrange", 1.53), ("Heun2 linear", 1.30)):
        print(f"{name:20s} stage / step: fwd {med((name, 'stage'), 0) / med((name, 'step'), 0):.3f} (MAC ratio {flop:.2f}), "
              f"train {med((name, 'stage'), 1) / med((name, 'step'), 1):.3f}")
        print(f"{name:20s} stage / AB3 : fwd {med((name, 'stage'), 0) / med(('AB3', '-'), 0):.3f}, train {med((name, 'stage'), 1) / med(('AB3', '-'), 1):.3f}")


def existing_only():
    """one run of the tree on sys.path, as a JSON line: the built-in RK4 of the DAE shape (forward, training step)"""
    fwd, train = legs(problem(), "rk4")
    print(json.dumps({"rk4 fwd": timed(fwd), "rk4 train": timed(train)}))


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
    ap.add_argument("--step", default=None, choices=("stage", "existing"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return existing_only() if a.step == "existing" else block1()
    print(f"# B = {B}, T = {T}, DAE x 5 / z 4 / v 6 / i 6, hidden 64 x 3, kernel generic; median [min .. max] of {RUNS} alternating runs of {ITERS} launches")
    print("# 1. what the stage heads cost: algebraic stage against step, and AB3, this tree")
    print(child(ROOT, "--step", "stage", limit=300), end="")
    if a.parent:
        print("# 2. what exists: the built-in rk4 DAE run (ELU(1) objects): parent against this tree, a child process per run")
        keys = ("rk4 fwd", "rk4 train")
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
