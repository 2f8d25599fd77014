"""Cost of sub-steps per grid interval on K0 / K5 (profiles/substeps_cost.txt).

    python profiles/scripts/substeps_cost.py [--parent DIR] > profiles/substeps_cost.txt

Same number of fine steps on both sides, B = 4096, kernel "generic", RK4Classic and Euler:
  (i)  the n-times refined problem, one step per interval, through the tableau route (_rk entry points): 1001 fine grid points.  The
       tableau objects psnode_generic_rk / psnode_generic_bwd_rk of this tree are, kernel for kernel, the listings of its parent
       (profiles/scripts/listing_diff.py), so this is what the parent runs; with --parent the ODE RK4Classic leg of (i) is also timed in the
       parent checkout itself;
  (ii) T = 251 grid points with substeps = 4.
Forward, and a training step (forward + backward) with the loss on the coarse rows -- for (i) rows ::4 of the fine result.  ODE: x 20 / z 3,
hidden 64 x 3.  DAE: x 5 / z 4 / v 6 / i 6, hidden 64 x 3 both MLPs.  Five alternating runs of (i) and (ii); median and [min .. max] of
the runs, each run the mean of ITERS launches between two stream events after one warm-up.
Also: the built-in 3/8 rule (the ELU(1) objects) at 4096 x 1000 steps, next to the same method through the tableau build and the sub-step
build (ELU(1) runs as ELU(alpha) there); with --parent DIR (a checkout of the parent commit with its library built) the same built-in run
in a child process per tree, alternating, to show the existing kernels are what they were."""
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


def problems(root):
    sys.path.insert(0, root)
    import torch
    from py_psnode_amd import models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    out = {}
    for kind, (xd, zd, vd, idim) in (("ode", (20, 3, 0, 0)), ("dae", (5, 4, 6, 6))):
        Tc = (T_FINE - 1) // N + 1
        t = (torch.arange(Tc, dtype=torch.float32) * (N / 256.0)).view(Tc, 1, 1).repeat(1, B, 1)
        rows = lambda w: 0.3 * torch.randn(Tc, B, w, generator=g)
        x, z, v, i = rows(xd), rows(zd), rows(vd), rows(idim)
        fine = lambda a: torch.cat((a[:-1].unsqueeze(1).repeat(1, N, 1, 1).reshape((Tc - 1) * N, B, a.shape[-1]), a[-1:]), 0)
        h = (t[1:] - t[:-1]) / N
        tf = torch.cat((torch.stack([t[:-1] + j * h for j in range(N)], 1).reshape(-1, B, 1), t[-1:]), 0)
        n = xd + zd + vd + idim
        if kind == "ode":
            de, ae = models.DE_Func(n, (64, 64, 64), xd).cuda(), None
        else:
            de, ae = models.DAE_DE_Func(n, (64, 64, 64), xd).cuda(), models.AE_Func(n + xd + zd + vd, (64, 64, 64), idim).cuda()
        a0 = torch.cat((x[0], z[0], v[0], i[0]), -1)
        c = lambda a: a.cuda().contiguous()
        out[kind] = dict(de=de, ae=ae, coarse=tuple(c(q) for q in (t, x, z, v, i)), fine=tuple(c(q) for q in (tf, fine(x), fine(z), fine(v), fine(i))),
                         a0=c(a0), x0=c(x[0]))
    return out


def legs(p, kind, method, substeps):
    """(forward, training step) closures of one problem through the generic route"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import autograd, fused
    lay = lambda m, attr: [(q.weight, q.bias) for q in getattr(m, attr) if isinstance(q, nn.Linear)]
    t, x, z, v, i = p["coarse"] if substeps > 1 else p["fine"]
    stride = 1 if substeps > 1 else N
    kw = dict(substeps=substeps) if substeps > 1 else {}
    de = lay(p["de"], "x_dot")
    if kind == "ode":
        fwd = lambda: fused.ode_integrate(method, [(w.detach(), b.detach()) for w, b in de], t, x[:1], z, p["a0"], kernel="generic", **kw)
        G = torch.randn_like(x[::stride])

        def train():
            for w, b in de:
                w.grad = b.grad = None
            xs = autograd.fused_ode_integrate(method, "generic", de, t, x, z, p["a0"], **kw)
            (xs[::stride] * G).sum().backward()
        return fwd, train
    ae = lay(p["ae"], "i_calculator")
    det = lambda ls: [(w.detach(), b.detach()) for w, b in ls]
    fwd = lambda: fused.dae_integrate(method, det(de), det(ae), p["x0"], t, x, z, v, i, p["a0"], kernel="generic", **kw)
    G, Gi = torch.randn(x[::stride].shape, device="cuda"), torch.randn_like(i[::stride])

    def train():
        for w, b in de + ae:
            w.grad = b.grad = None
        xs, is_ = autograd.fused_dae_integrate(method, "generic", de, ae, p["x0"], t, z, v, i, p["a0"], **kw)
        ((xs[::stride] * G).sum() + (is_[::stride] * Gi).sum()).backward()
    return fwd, train


def builtin_only(root):
    """one run of the tree at `root`, as a JSON line: the built-in RK4 and leg (i) -- the refined problem through the tableau route,
    RK4Classic -- of the ODE shape (forward, training step)"""
    from py_psnode_amd import neural_dae as nd
    p = problems(root)["ode"]
    fwd, train = legs(p, "ode", "rk4", 1)
    rfwd, rtrain = legs(p, "ode", nd.RK4Classic().method, 1)
    print(json.dumps({"fwd": timed(fwd), "train": timed(train), "rk_fwd": timed(rfwd), "rk_train": timed(rtrain)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--builtin-only", default=None, metavar="ROOT")
    a = ap.parse_args()
    sys.path.insert(0, a.builtin_only or ROOT)
    if a.builtin_only:
        return builtin_only(a.builtin_only)
    import torch
    from py_psnode_amd import neural_dae as nd
    P = problems(ROOT)
    print(f"# {torch.cuda.get_device_name(0)}; B = {B}, {T_FINE - 1} fine steps; (i) refined grid of {T_FINE} points through the tableau route, "
          f"(ii) {(T_FINE - 1) // N + 1} points x substeps {N}; median [min .. max] of {RUNS} alternating runs of {ITERS} launches")
    print("# (i) runs this tree's tableau objects, whose device listings equal the parent's kernel for kernel; with --parent its ODE RK4Classic leg "
          "is also timed in the parent checkout (last rows), the DAE and Euler legs of (i) in this tree only")
    for kind in ("ode", "dae"):
        for name, method in (("RK4Classic", nd.RK4Classic().method), ("Euler", nd.ExplicitRK(((),), (1.0,), 1, name="Euler-tableau").method)):
            f1, t1 = legs(P[kind], kind, method, 1)
            f2, t2 = legs(P[kind], kind, method, N)
            res = {k: [] for k in ("fwd (i)", "fwd (ii)", "train (i)", "train (ii)")}
            for _ in range(RUNS):
                res["fwd (i)"].append(timed(f1)); res["fwd (ii)"].append(timed(f2))
                res["train (i)"].append(timed(t1)); res["train (ii)"].append(timed(t2))
            for k, v in res.items():
                print(f"{kind.upper()} {name:10s} {k:10s} {fmt(v)}")
            for leg in ("fwd", "train"):
                print(f"{kind.upper()} {name:10s} {leg} (ii) / (i) = {statistics.median(res[leg + ' (ii)']) / statistics.median(res[leg + ' (i)']):.3f}")
    # ELU(1) as ELU(alpha): the 3/8 rule on the ELU(1) objects, the tableau build and the sub-step build, the same 1000 fine steps
    p = P["ode"]
    rk38 = nd.ExplicitRK(((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125), 4, name="rk4-tableau").method
    rows = {"built-in rk4, ELU(1) objects": legs(p, "ode", "rk4", 1), "3/8 tableau, tableau build": legs(p, "ode", rk38, 1),
            "built-in rk4, substeps 4, sub-step build": legs(p, "ode", "rk4", N)}
    res = {k: ([], []) for k in rows}
    for _ in range(RUNS):
        for k, (f, tr) in rows.items():
            res[k][0].append(timed(f)); res[k][1].append(timed(tr))
    for k, (f, tr) in res.items():
        print(f"ODE {k:42s} fwd {fmt(f)}   train {fmt(tr)}")
    base = res["built-in rk4, ELU(1) objects"]
    for k in list(rows)[1:]:
        print(f"ODE {k} / ELU(1) objects: fwd {statistics.median(res[k][0]) / statistics.median(base[0]):.3f}, "
              f"train {statistics.median(res[k][1]) / statistics.median(base[1]):.3f}")
    Tc = (T_FINE - 1) // N + 1
    print(f"x_sub at this size: (T-1) (n-1) B x_dim 4 = {(Tc - 1) * (N - 1) * B * 20 * 4 / 2**20:.1f} MiB (ODE, x 20), "
          f"{(Tc - 1) * (N - 1) * B * 5 * 4 / 2**20:.1f} MiB (DAE, x 5)")
    if a.parent:
        out = {"this tree": ([], [], [], []), "parent": ([], [], [], [])}
        for _ in range(RUNS):
            for k, root in (("this tree", ROOT), ("parent", os.path.abspath(a.parent))):
                env = dict(os.environ, PYTHONPATH=root)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--builtin-only", root], cwd=root, env=env, capture_output=True, text=True,
                                   timeout=300, check=True)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                out[k][0].append(d["fwd"]); out[k][1].append(d["train"]); out[k][2].append(d["rk_fwd"]); out[k][3].append(d["rk_train"])
        for k, (f, tr, rf, rtr) in out.items():
            print(f"built-in rk4, 4096 x 1000 steps, {k:9s}: fwd {fmt(f)}   train {fmt(tr)}")
        for k, (f, tr, rf, rtr) in out.items():
            print(f"(i) ODE RK4Classic, refined, tableau route, {k:9s}: fwd {fmt(rf)}   train {fmt(rtr)}")


if __name__ == "__main__":
    main()
