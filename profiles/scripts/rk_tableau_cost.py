"""What the tableau form of the generic kernels costs: timings for profiles/rk_tableau_cost.txt.

    python profiles/scripts/rk_tableau_cost.py [--parent-tree DIR] [--runs 5] [--B 4096] [--T 1000] [--out profiles/rk_tableau_cost.txt]

ODE_01 (x 8, z 2) and x_dim 20 (z 3), hidden 64^3, one B x T batch, kernel="generic": the fused forward (K0) and a training step (K0 + loss
+ K5), timed with device events after a warm-up, median of three per run.
  (i)  the built-in 3/8 RK4 on this tree and -- with --parent-tree, a checkout of the parent commit with its library built -- on that tree:
       alternating child processes (one tree each), `--runs` runs of each; the two must agree within the parent's own run-to-run spread;
  (ii) on this tree the 3/8 rule as a tableau, RK4Classic, Kutta3 and Heun2, in the same child processes.
--where: the breakdown of the 3/8 step by kernel (K0, K5 alone) and build, see `where`.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"ODE_01 x8 z2": (8, 2), "x20 z3": (20, 3)}
THREE_EIGHTHS = (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125), 4)


def child(tree, B, T, tableaus):
    sys.path.insert(0, tree)
    import torch
    from py_psnode_amd import models
    from py_psnode_amd import neural_dae as nd
    dev = "cuda"
    solvers = {"rk4 (built-in 3/8)": nd.RK4}
    if tableaus:
        solvers.update({"3/8 tableau": lambda: nd.ExplicitRK(*THREE_EIGHTHS, name="three-eighths"), "RK4Classic": nd.RK4Classic,
                        "Kutta3": nd.Kutta3, "Heun2": nd.Heun2})
    out = {}
    for shape, (xd, zd) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        torch.manual_seed(0)
        r = lambda *s: (0.3 * torch.randn(*s, generator=g)).to(dev)
        de = models.DE_Func(xd + zd, (64, 64, 64), xd).to(dev)
        t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, B, 1).to(dev)
        x, z, G = r(T, B, xd), r(T, B, zd), r(T, B, xd)
        a0 = torch.cat((x[0], z[0]), -1)
        for name, make in solvers.items():
            s = make()
            s.fused, s.kernel = "require", "generic"

            def fwd():
                with torch.no_grad():
                    s.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0)

            def train():
                for p in de.parameters():
                    p.grad = None
                (s.integrate_ODE(x_func=de, t=t, x=x, z=z, all_initial=a0) * G).sum().backward()

            for what, f in (("forward", fwd), ("training step", train)):
                f()
                torch.cuda.synchronize()
                ms = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                out[f"{shape} | {what} | {name}"] = statistics.median(ms)
    print("RESULT " + json.dumps(out), flush=True)


def where(B, T):
    """Where the tableau form's time goes: the same 3/8 RK4 step on K0 and on K5 ALONE (fused.ode_backward, kernel="generic": the solver
    route trains the ODE_01 shape on K4f / K4x, which no tableau runs on) in three builds -- ELU(1) (built-in), the activation build with
    ELU(alpha = 1 - 2^-20) (the same ELU code the tableau build runs ELU(1) through, built-in formulas) and the tableau build."""
    sys.path.insert(0, HERE)
    import torch
    from py_psnode_amd import _lib, fused, models
    dev = "cuda"
    tab = fused.Tableau("three-eighths", *THREE_EIGHTHS)
    elu_a = fused.Act(_lib.ACT_ELU, alpha=1.0 - 2.0 ** -20, name="ELU(1 - 2^-20)")
    lines = ["where the time goes: 3/8 RK4 on K0 and on K5 alone, ms (median of five after a warm-up)"]
    for shape, (xd, zd) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        r = lambda *s: (0.3 * torch.randn(*s, generator=g)).to(dev)
        de = models.DE_Func(xd + zd, (64, 64, 64), xd).to(dev)
        layers = [(m.weight.detach(), m.bias.detach()) for m in de.x_dot if isinstance(m, torch.nn.Linear)]
        t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, B, 1).to(dev)
        x, z, G = r(T, B, xd), r(T, B, zd), r(T, B, xd)
        a0 = torch.cat((x[0], z[0]), -1)
        for label, method, act in (("built-in, ELU(1) build", "rk4", None), ("built-in, activation build", "rk4", elu_a), ("3/8 tableau build", tab, None)):
            xs = fused.ode_integrate(method, layers, t, x, z, a0, kernel="generic", act=act)
            res = {}
            for what, f in (("K0 forward", lambda: fused.ode_integrate(method, layers, t, x, z, a0, kernel="generic", act=act)),
                            ("K5 backward", lambda: fused.ode_backward(method, layers, t, z, a0, xs, G, kernel="generic", act=act))):
                f()
                torch.cuda.synchronize()
                ms = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                res[what] = statistics.median(ms)
            lines.append(f"    {shape:<14} {label:<28} K0 forward {res['K0 forward']:8.3f}   K5 backward {res['K5 backward']:8.3f}")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rk_tableau_cost.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--tableaus", type=int, default=1)
    ap.add_argument("--where", action="store_true", help="only the K0 / K5 breakdown by build (printed; append it to the report)")
    a = ap.parse_args()
    if a.where:
        return where(a.B, a.T)
    if a.child:
        return child(a.child, a.B, a.T, bool(a.tableaus))

    def run(tree, tableaus):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--tableaus", str(int(tableaus)), "--B", str(a.B), "--T", str(a.T)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"child on {tree} ended with status {p.returncode}: nothing more is started")
        line = [q for q in p.stdout.splitlines() if q.startswith("RESULT ")][-1]
        return json.loads(line[7:])

    here, parent = [], []
    for k in range(a.runs):           # alternating: drift of the machine hits both trees alike
        if a.parent_tree:
            parent.append(run(os.path.abspath(a.parent_tree), False))
        here.append(run(HERE, True))
        print(f"run {k + 1} / {a.runs} done", flush=True)
    med = lambda rs, key: statistics.median(r[key] for r in rs)
    lines = [f"rk_tableau_cost: {a.B} x {a.T} batch, hidden 64^3, kernel=generic, ms per launch / step; median of {a.runs} runs "
             "(each the median of three timed repeats after a warm-up), [min .. max] over the runs", ""]
    for shape in SHAPES:
        for what in ("forward", "training step"):
            base_key = f"{shape} | {what} | rk4 (built-in 3/8)"
            base = med(here, base_key)
            lines.append(f"{shape}, {what}")
            if parent:
                ps = [r[base_key] for r in parent]
                lines.append(f"    built-in 3/8 RK4, parent commit     {statistics.median(ps):9.3f}   [{min(ps):.3f} .. {max(ps):.3f}]  spread {max(ps) - min(ps):.3f}")
            for name in ("rk4 (built-in 3/8)", "3/8 tableau", "RK4Classic", "Kutta3", "Heun2"):
                key = f"{shape} | {what} | {name}"
                hs = [r[key] for r in here]
                label = "built-in 3/8 RK4, this commit" if name.startswith("rk4") else name
                extra = ""
                if name.startswith("rk4") and parent:
                    extra = f"  (this - parent: {statistics.median(hs) - statistics.median(ps):+.3f} ms)"
                elif not name.startswith("rk4"):
                    extra = f"  x{statistics.median(hs) / base:.3f} of the built-in"
                lines.append(f"    {label:<35} {statistics.median(hs):9.3f}   [{min(hs):.3f} .. {max(hs):.3f}]{extra}")
            lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
