"""Teacher-forced training on the generic backward K5: timings for profiles/k5_teacher_forcing.txt.

    python profiles/scripts/k5_teacher_forcing.py [--parent-lib build/parent/lib.so] [--B 4096] [--T 1000]

Training step = fused forward + loss + backward of one 4096 x 1000 batch, timed with device events after warm-up, for
  ODE x_dim 20 / z 3 / hidden 64^3 and DAE x 8 / z 4 / v 6 / i 6 / hidden 64^3, Euler and RK4:
  (a) teacher-forced fused (K0 + K5 with the flags) vs the Python walk (fused="off") on the same inputs -- the walk at 100 steps, scaled
      to T - 1 steps (it is linear in the step count);
  (b) teacher-forced vs untied fused step, alternating, five repeats each;
  (c) --parent-lib: the untied ODE step on a build of the parent commit vs this build, alternating child processes (one library each):
      the x_dim 20 shape (register path), x_dim 20 / hidden 96^2 (fully streamed, accumulators in LDS: generic_backward_kernel
      <false, false, false, 2>) and x_dim 8 / hidden 128^3 at kernel="generic" with twice the batch (fully streamed, accumulators in global
      memory: <true, false, true, 2>).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _tolerate_missing_tf_exports():
    """a library of the commit before has no psnode_dae_backward_tf_*: do not ask for them (the untied step never calls them)"""
    from py_psnode_amd import _lib
    _lib.EXPORTS = tuple(e for e in _lib.EXPORTS if not e.startswith("psnode_dae_backward_tf_"))


def _setup(kind, B, T, dev, xd_ode=20, zd_ode=3, hidden=(64, 64, 64)):
    import torch
    from py_psnode_amd import models
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    r = lambda *s: (0.3 * torch.randn(*s, generator=g)).to(dev)
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, B, 1).to(dev)
    if kind == "ode":
        xd, zd = xd_ode, zd_ode
        de = models.DE_Func(xd + zd, hidden, xd).to(dev)
        x, z = r(T, B, xd), r(T, B, zd)
        return dict(kind=kind, de=de, t=t, x=x, z=z, a0=torch.cat((x[0], z[0]), -1), G=r(T, B, xd))
    xd, zd, vd, idim = 8, 4, 6, 6
    n = xd + zd + vd + idim
    de = models.DAE_DE_Func(n, (64, 64, 64), xd).to(dev)
    ae = models.AE_Func(n + xd + zd + vd, (64, 64, 64), idim).to(dev)
    x, z, v, i = r(T, B, xd), r(T, B, zd), r(T, B, vd), r(T, B, idim)
    return dict(kind=kind, de=de, ae=ae, t=t, x=x, z=z, v=v, i=i, a0=torch.cat((x[0], z[0], v[0], i[0]), -1), G=r(T, B, xd), H=r(T, B, idim))


def _step(c, method, mode, tf, steps=None, kernel="auto"):
    """one training step; steps: use the first steps + 1 grid points only"""
    from py_psnode_amd import neural_dae as nd
    s = {"euler": nd.Euler, "rk4": nd.RK4}[method]()
    s.fused, s.kernel = mode, kernel
    n = None if steps is None else steps + 1
    cut = lambda a: a if n is None else a[:n]
    for p in list(c["de"].parameters()) + (list(c["ae"].parameters()) if "ae" in c else []):
        p.grad = None
    if c["kind"] == "ode":
        xs = s.integrate_ODE(x_func=c["de"], t=cut(c["t"]), x=cut(c["x"]), z=cut(c["z"]), all_initial=c["a0"], input_true_x=tf)
        (xs * cut(c["G"])).sum().backward()
    else:
        xs, is_ = s.integrate_DAE(x_init=c["x"][0], x_func=c["de"], i_func=c["ae"], t=cut(c["t"]), x=cut(c["x"]), z=cut(c["z"]), v=cut(c["v"]),
                                  i=cut(c["i"]), all_initial=c["a0"], input_true_x=tf, input_true_i=tf)
        ((xs * cut(c["G"])).sum() + (is_ * cut(c["H"])).sum()).backward()


def _time(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _fmt(v):
    return f"median {statistics.median(v):8.2f} ms  (min {min(v):.2f}, max {max(v):.2f})"


def child(args):
    """--child: the untied ODE step on whatever library PSNODE_LIB_PATH names; prints one JSON line"""
    if args.tolerate:
        _tolerate_missing_tf_exports()
    c = _setup("ode", args.B, args.T, "cuda")
    res = {f"x20_h64 {m}": _time(lambda m=m: _step(c, m, "require", False), 5) for m in ("euler", "rk4")}
    del c
    c = _setup("ode", args.B, args.T, "cuda", 20, 3, (96, 96))
    res.update({f"x20_h96x2 {m}": _time(lambda m=m: _step(c, m, "require", False), 5) for m in ("euler", "rk4")})
    del c
    c = _setup("ode", 2 * args.B, args.T, "cuda", 8, 2, (128, 128, 128))
    res.update({f"x8_h128_generic_2B {m}": _time(lambda m=m: _step(c, m, "require", False, kernel="generic"), 5) for m in ("euler", "rk4")})
    print("CHILD " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tolerate", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    print(f"device: {torch.cuda.get_device_name(0)};  B = {args.B}, T = {args.T}; training step, device events, 2 warm-up + 5 timed")
    for kind in ("ode", "dae"):
        c = _setup(kind, args.B, args.T, "cuda")
        name = "ODE x20 z3 h64^3" if kind == "ode" else "DAE x8 z4 v6 i6 h64^3"
        for method in ("euler", "rk4"):
            tf, un = [], []
            for f in (True, False):
                _step(c, method, "require", f)
                _step(c, method, "require", f)
            for _ in range(5):                      # alternating
                tf += _time(lambda: _step(c, method, "require", True), 1, warm=0)
                un += _time(lambda: _step(c, method, "require", False), 1, warm=0)
            walk = _time(lambda: _step(c, method, "off", True, steps=100), 2, warm=1)
            scaled = statistics.median(walk) * (args.T - 1) / 100.0
            print(f"{name} {method:6s} teacher-forced fused: {_fmt(tf)}")
            print(f"{name} {method:6s} untied fused        : {_fmt(un)}")
            print(f"{name} {method:6s} teacher-forced walk : {statistics.median(walk):.1f} ms per 100 steps -> {scaled:.0f} ms scaled to {args.T - 1} steps;"
                  f" speed-up {scaled / statistics.median(tf):.1f} x")
        del c
        torch.cuda.empty_cache()
    if args.parent_lib:
        res = {"parent": {}, "this": {}}
        for rnd in range(2):                        # alternating processes: parent, this, parent, this
            for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("this", None)):
                env = dict(os.environ)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--B", str(args.B), "--T", str(args.T)]
                if lib:
                    env["PSNODE_LIB_PATH"] = lib
                    cmd.append("--tolerate")
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
                if p.returncode != 0:
                    print(f"child ({who}) failed with {p.returncode}: {p.stderr[-400:]}")
                    return 1
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1]
                for m, v in json.loads(line[6:]).items():
                    res[who].setdefault(m, []).extend(v)
        for m in res["this"]:
            for who in ("parent", "this"):
                print(f"untied ODE {m:26s} {who:6s} build: {_fmt(res[who][m])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
