"""What segment_parallel buys on K0 / K5 (profiles/segment_parallel_cost.txt).

    python profiles/scripts/segment_parallel_cost.py [--parent DIR] > profiles/segment_parallel_cost.txt

T = 1001, w = 50 (20 segments), hidden 64 x 3, kernel "generic", one step per grid interval, no events.  ODE: x 20 / z 3.  DAE: x 5 / z 4 /
v 6 / i 6 (the shapes of profiles/segments_cost.txt).  RK4Classic and Euler as tableaus, forward and training step (forward + backward, loss
on every output row), B in {16, 32, 256, 1024, 4096}.  Per shape: the sequential segment=50 run, then segment_parallel = 2, 4, 8, 20 and
"auto"; with --parent DIR (a checkout of the parent commit with its library built) the parent's sequential run too.  Five alternating runs;
median and [min .. max] of the runs, each run the mean of ITERS launches between two stream events after one warm-up.  Each block (one
model kind on one tree, all batches) is a child process under its own time limit; the first that fails ends the script.
Per row: the speed-up over this tree's sequential median, next to the ideal min(C, CUs / tiles) -- C chunks, tiles = ceil(B / 16) -- and a
mark where the measured speed-up is under half of it.  The five runs of a block share one process, whose [min .. max] is narrower than
the spread from process to process; so with --parent the sequential run is also timed the way profiles/segments_cost.txt compares trees:
B = 32 and B = 4096, one child process per run, parent and this tree alternating, this tree's median against the parent's range.
    --step trace:<kind>:<B>   one training step and one forward of the sequential and the "auto" call, three times each: the program of a
                              kernel-trace run of its own (rocprofv3 --kernel-trace --stats -- python ... --step trace:ode:32)"""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not os.environ.get("PYTHONPATH") and ROOT not in sys.path:      # (a step started by hand, e.g. under the profiler; a child names its tree)
    sys.path.insert(0, ROOT)
T, W, ITERS, RUNS = 1001, 50, 3, 5
BATCHES = (16, 32, 256, 1024, 4096)
GROUPS = (2, 4, 8, 20, "auto")
DIMS = {"ode": (20, 3, 0, 0), "dae": (5, 4, 6, 6)}
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


def problem(kind, B, hidden=(64, 64, 64)):
    import torch
    from py_psnode_amd import models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xd, zd, vd, idim = DIMS[kind]
    t = (torch.arange(T, dtype=torch.float32) / 256.0).view(T, 1, 1).repeat(1, B, 1)
    x, z, v, i = (0.3 * torch.randn(T, B, w, generator=g) for w in (xd, zd, vd, idim))
    n = xd + zd + vd + idim
    if kind == "ode":
        de, ae = models.DE_Func(n, hidden, xd).cuda(), None
    else:
        de, ae = models.DAE_DE_Func(n, hidden, xd).cuda(), models.AE_Func(n + xd + zd + vd, hidden, idim).cuda()
    c = lambda a: a.cuda().contiguous()
    return dict(de=de, ae=ae, rows=tuple(c(q) for q in (t, x, z, v, i)), a0=c(torch.cat((x[0], z[0], v[0], i[0]), -1)), x0=c(x[0]))


def legs(p, kind, method, groups=None):
    """(forward, training step) closures of one problem through the generic route with segment = W; groups: segment_parallel"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    t, x, z, v, i = p["rows"]
    kw = dict(segment=W, **(dict(segment_parallel=groups) if groups is not None else {}))
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
        xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, p["x0"], t, z, v, i, p["a0"], x=x, **kw)
        ((xs * G).sum() + (is_ * Gi).sum()).backward()
    return fwd, train


def methods():
    from py_psnode_amd import neural_dae as nd
    return (("RK4Classic", nd.RK4Classic().method), ("Euler", nd.ExplicitRK(((),), (1.0,), 1, name="Euler-tableau").method))


def block(kind, sequential_only, batches=BATCHES, runs=RUNS):
    """one JSON line per (B, method, variant): the runs of both legs"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in batches:
        p = problem(kind, B)
        for name, method in methods():
            variants = (None,) if sequential_only else (None,) + GROUPS
            cfg = {g: legs(p, kind, method, g) for g in variants}
            res = {g: ([], []) for g in cfg}
            for _ in range(runs):
                for g, (f, tr) in cfg.items():
                    res[g][0].append(timed(f)); res[g][1].append(timed(tr))
            for g, (f, tr) in res.items():
                chunks = 1
                if g is not None:
                    from py_psnode_amd import fused
                    gg = fused.auto_segment_groups(B, cus) if g == "auto" else g
                    chunks = len(fused.segment_chunks(T, W, gg)[1])
                print(json.dumps(dict(kind=kind, B=B, method=name, g=g, chunks=chunks, cus=cus, fwd=f, train=tr)))
        del p
        torch.cuda.empty_cache()


def trace(kind, B):
    import torch
    p = problem(kind, B)
    for name, method in methods():
        for g in (None, "auto"):
            f, tr = legs(p, kind, method, g)
            for _ in range(3):
                f(); tr()
    torch.cuda.synchronize()


def child(root, *args, limit):
    """a GPU step: its own process under its own time limit; a failure or a time-out raises and ends the script"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args], cwd=root, env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, check=False)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"step {args} in {root} ended with status {r.returncode}: nothing further is started")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def fmt(v):
    return f"{statistics.median(v):7.2f} ms [{min(v):.2f} .. {max(v):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:      # (a child: PYTHONPATH names its tree)
        what, *rest = a.step.split(":")
        if what == "trace":
            return trace(rest[0], int(rest[1]))
        return block(rest[0], True, (32, 4096), 1) if what == "one" else block(rest[0], what == "seq")
    print(f"# T = {T}, segment = {W} ({-(-(T - 1) // W)} segments), hidden 64 x 3, kernel generic, one step per interval, no events; median [min .. max] of {RUNS} "
          f"alternating runs of {ITERS} launches")
    print("# speed-up: this tree's sequential median / the row's median; ideal: min(C, CUs / tiles); `<half`: under half the ideal")
    slow, b32 = [], []
    for kind in ("ode", "dae"):
        rows = child(ROOT, "--step", f"all:{kind}", limit=540)
        parent = child(os.path.abspath(a.parent), "--step", f"seq:{kind}", limit=300) if a.parent else []
        for B in BATCHES:
            for name in ("RK4Classic", "Euler"):
                mine = [r for r in rows if r["B"] == B and r["method"] == name]
                seq = next(r for r in mine if r["g"] is None)
                par = next((r for r in parent if r["B"] == B and r["method"] == name), None)
                tiles = -(-B // 16)
                for leg in ("fwd", "train"):
                    head = f"{kind.upper()} {name:10s} B={B:<4d} {leg:5s}"
                    s_med = statistics.median(seq[leg])
                    if par is not None:
                        lo, hi = min(par[leg]), max(par[leg])
                        print(f"{head} sequential, parent    : {fmt(par[leg])}")
                        print(f"{head} sequential            : {fmt(seq[leg])}   {'inside' if lo <= s_med <= hi else 'OUTSIDE'} the parent's range")
                    else:
                        print(f"{head} sequential            : {fmt(seq[leg])}")
                    for r in mine:
                        if r["g"] is None:
                            continue
                        m, C = statistics.median(r[leg]), r["chunks"]
                        ideal = max(1.0, min(C, r["cus"] / tiles))
                        up = s_med / m
                        mark = "  <half" if up < ideal / 2 else ""
                        print(f"{head} g = {str(r['g']):4s} (C = {C:2d})     : {fmt(r[leg])}   x{up:5.2f} of ideal x{ideal:5.2f}{mark}")
                        if r["g"] == "auto":
                            if B == 32:
                                b32.append((head, m < min(seq[leg])))
                            if min(r[leg]) > max(seq[leg]):
                                slow.append(head)
    if a.parent:
        print("# the sequential segment = 50 run, one child process per run, parent and this tree alternating")
        for kind in ("ode", "dae"):
            out = {}
            for _ in range(RUNS):
                for tree, root in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                    for r in child(root, "--step", f"one:{kind}", limit=120):
                        for leg in ("fwd", "train"):
                            out.setdefault((r["B"], r["method"], leg), {}).setdefault(tree, []).append(r[leg][0])
            for (B, name, leg), v in out.items():
                m, lo, hi = statistics.median(v["this tree"]), min(v["parent"]), max(v["parent"])
                print(f"{kind.upper()} {name:10s} B={B:<4d} {leg:5s} parent {fmt(v['parent'])} | this tree {fmt(v['this tree'])}: median "
                      f"{'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's range ({100 * (m / statistics.median(v['parent']) - 1):+.2f} %)")
    print("# conditions")
    print("B = 32, \"auto\" faster than every sequential run: " + ("yes, all of " + str(len(b32)) if all(ok for _, ok in b32) else "NO: " + ", ".join(h for h, ok in b32 if not ok)))
    print("\"auto\" slower than the sequential run beyond the run-to-run range: " + ("nowhere" if not slow else ", ".join(slow)))


if __name__ == "__main__":
    main()
