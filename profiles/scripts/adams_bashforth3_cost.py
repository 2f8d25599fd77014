"""Cost of three-step Adams-Bashforth on K0 / K5 (profiles/adams_bashforth3_cost.txt).

    python profiles/scripts/adams_bashforth3_cost.py --parent DIR > profiles/adams_bashforth3_cost.txt

B = 4096, T = 1001, hidden 64 x 3, kernel "generic".  ODE: x 20 / z 3.  DAE: x 5 / z 4 / v 6 / i 6 (the shapes of
profiles/adams_bashforth_cost.txt).  Forward and training step (forward + backward, loss on every output row).  DIR: a checkout of the
parent commit with its library built.  Every run is a child process of its own -- one tree, one method, one shape -- under its own time
limit; the first that fails ends the script.  Five alternating runs; median and [min .. max], each run the mean of ITERS launches between
two stream events after one warm-up.
  1. AB3 of this tree against AB2 of the parent on identical rows, without events: the steady-state step (one DE evaluation, one more
     slope term) plus the restart step at k = 0 alone.
  2. AB3 of this tree with 10 shared events (steps 50, 150, .., 950) against the same call without them and against the parent's AB2
     with them: the price of the restart steps (two DE evaluations, a DAE one more head; K5 the corrector's VJP in front of the DE's).
  3. AB2 and the built-in `rk4` (ELU(1) objects) of the parent against this tree: the listings say they are the same code
     (profiles/adams_bashforth3_listing_diff.txt), so this tree's median has to lie inside the parent's [min .. max].
A single run for a profiler: `PYTHONPATH=. python profiles/scripts/adams_bashforth3_cost.py --step ode|dae ab2|ab3|ab2_ev|ab3_ev|rk4`."""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, T, ITERS, RUNS = 4096, 1001, 3, 5
EVENT_STEPS = tuple(range(50, 1000, 100))
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
    events = method.endswith("_ev")
    method = method[:-3] if events else method
    t = (torch.arange(T, dtype=torch.float32) / 256.0).view(T, 1, 1).repeat(1, B, 1).cuda()
    x, z, v, i = ((0.3 * torch.randn(T, B, w, generator=g)).cuda() for w in (xd, zd, vd, idim))
    ev = zj = vj = None
    if events:
        ev = t[list(EVENT_STEPS)].permute(1, 0, 2).contiguous()
        zj, vj = ((0.3 * torch.randn(B, len(EVENT_STEPS), w, generator=g)).cuda() for w in (zd, vd))
    n = xd + zd + vd + idim
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    a0 = torch.cat((x[0], z[0], v[0], i[0]), -1).contiguous()
    de = lay(models.DE_Func(n, (64, 64, 64), xd).cuda() if kind == "ode" else models.DAE_DE_Func(n, (64, 64, 64), xd).cuda(), "x_dot")
    if kind == "ode":
        G = torch.randn_like(x)
        fwd = lambda: fused.ode_integrate(method, det(de), t, x[:1], z, a0, ev, zj, kernel="generic")

        def train():
            for w, b in de:
                w.grad = b.grad = None
            (autograd.fused_ode_integrate(method, "generic", de, t, x, z, a0, ev, zj) * G).sum().backward()
    else:
        ae = lay(models.AE_Func(n + xd + zd + vd, (64, 64, 64), idim).cuda(), "i_calculator")
        x0 = x[0].contiguous()
        G, Gi = torch.randn_like(x), torch.randn_like(i)
        fwd = lambda: fused.dae_integrate(method, det(de), det(ae), x0, t, x, z, v, i, a0, ev, zj, vj, kernel="generic")

        def train():
            for w, b in de + ae:
                w.grad = b.grad = None
            xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, x0, t, z, v, i, a0, ev, zj, vj)
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
        print(f"{kind.upper()} {k:24s}: fwd {fmt(f)}   train {fmt(tr)}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=False, default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--step", nargs=2, default=None, metavar=("KIND", "METHOD"))
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        return one_run(*a.step)
    if not a.parent:
        raise SystemExit("--parent DIR is required: the comparison is against the parent commit's AB2 and rk4")
    parent = os.path.abspath(a.parent)
    print(f"# B = {B}, T = {T}, hidden 64 x 3, kernel generic; median [min .. max] of {RUNS} alternating runs of {ITERS} launches, a child process per run")
    print(f"# 1. + 2. + 3. AB3 (this tree) against AB2 (parent, this tree), without events and with {len(EVENT_STEPS)} shared events")
    for kind in ("ode", "dae"):
        res = alternate(kind, (("parent AB2", parent, "ab2"), ("this tree AB2", ROOT, "ab2"), ("this tree AB3", ROOT, "ab3"),
                               ("parent AB2, 10 events", parent, "ab2_ev"), ("this tree AB3, 10 events", ROOT, "ab3_ev")))
        med = lambda k, j: statistics.median(res[k][j])
        print(f"{kind.upper()} AB3 / parent AB2, no events: fwd {med('this tree AB3', 0) / med('parent AB2', 0):.3f}, train {med('this tree AB3', 1) / med('parent AB2', 1):.3f}")
        print(f"{kind.upper()} AB3 with 10 events / AB3 without: fwd {med('this tree AB3, 10 events', 0) / med('this tree AB3', 0):.3f}, "
              f"train {med('this tree AB3, 10 events', 1) / med('this tree AB3', 1):.3f}")
        print(f"{kind.upper()} AB3 / parent AB2, 10 events: fwd {med('this tree AB3, 10 events', 0) / med('parent AB2, 10 events', 0):.3f}, "
              f"train {med('this tree AB3, 10 events', 1) / med('parent AB2, 10 events', 1):.3f}")
        for j, leg in enumerate(("fwd", "train")):
            m, lo, hi = med("this tree AB2", j), min(res["parent AB2"][j]), max(res["parent AB2"][j])
            print(f"{kind.upper()} AB2 {leg}: this tree's median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's [{lo:.2f} .. {hi:.2f}]")
            m, lo, hi = med("this tree AB3", j), min(res["parent AB2"][j]), max(res["parent AB2"][j])
            print(f"{kind.upper()} AB3 {leg}, no events: median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent AB2's [{lo:.2f} .. {hi:.2f}]")
    print("# 3. the built-in rk4 (ELU(1) objects), ODE x 20 / z 3: parent against this tree")
    out = alternate("ode", (("parent rk4", parent, "rk4"), ("this tree rk4", ROOT, "rk4")))
    for j, leg in enumerate(("fwd", "train")):
        m, lo, hi = statistics.median(out["this tree rk4"][j]), min(out["parent rk4"][j]), max(out["parent rk4"][j])
        print(f"built-in rk4 {leg}: this tree's median {m:.2f} ms {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's [{lo:.2f} .. {hi:.2f}]")


if __name__ == "__main__":
    main()
