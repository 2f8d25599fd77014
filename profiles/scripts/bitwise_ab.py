"""Bit-for-bit A/B of two builds of the library on the tile backward kernels K4f, K7f and K7h.

    python profiles/scripts/bitwise_ab.py LIB_A LIB_B [--timeout SECONDS]

For each library in turn one fresh child process (PSNODE_LIB_PATH set, under its own `timeout -k 10`) runs the cases below on inputs drawn on
the CPU from fixed seeds and writes one SHA-256 per output tensor to a JSON file; the parent compares the two files and prints the names that
differ.  The second child is not started when the first one fails.  These kernels sum in a fixed order, so every digest has to be equal.
Cases (T = 4 grid points, B = 17 trajectories: one full tile of 16 and a ragged one; one event with jump values):
  K4f   fused.ode_backward(kernel="wide"): hidden 32 / 48 / 64 / 128, euler / midpoint / rk4, (x, z) = (3, 0) / (8, 2) / (8, 7),
        recompute form, saved-row form (two-role kernels at hidden <= 64), teacher-forced recompute form
  K7f + K7h   fused.dae_backward(kernel="wide") (recompute form) / fused.dae_backward_wide (saved form, teacher forcing: K7f's own entry,
        no other kernel behind it): hidden 32 / 64 / 128, the three methods,
        (x, z, v, i) = (8, 2, 2, 2) / (3, 1, 0, 1) / (2, 2, 4, 2), recompute and saved forms, teacher forcing of x, of i and of both
The library does not report which kernel a call took: kernel="wide" takes K4f / K7f or raises, which is what the child relies on.
(The ODE inputs follow tests/test_gpu_backward.py:_case with the hidden width as a parameter; the DAE ones are its _dae_raw_case.)"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
METHODS = ("euler", "midpoint", "rk4")
T, B = 4, 17


def _digest(a):
    return None if a is None else hashlib.sha256(a.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _ode_case(H, xd, zd, seed):
    import torch
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd
    dims = [3 * n, H, H, H, xd]
    layers = [(l.weight.detach().cuda(), l.bias.detach().cuda()) for l in [nn.Linear(dims[k], dims[k + 1]) for k in range(4)]]
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, B, 1)
    t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, B - 1, 1, generator=g))
    x, z = 0.1 * torch.randn(T, B, xd, generator=g), 0.1 * torch.randn(T, B, zd, generator=g)
    ev = t[2, :, :].unsqueeze(1).contiguous()
    zj = 0.1 * torch.randn(B, 1, zd, generator=g)
    G = torch.randn(T, B, xd, generator=g)
    return layers, t.cuda(), x.cuda(), z.cuda(), ev.cuda(), zj.cuda(), G.cuda()


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    from py_psnode_amd import _lib, fused
    from test_gpu_backward import _dae_raw_case
    assert os.path.samefile(_lib.LIB_PATH, os.environ["PSNODE_LIB_PATH"]), _lib.LIB_PATH
    res = {}
    for H in (32, 48, 64, 128):
        for method in METHODS:
            for xd, zd in ((3, 0), (8, 2), (8, 7)):
                layers, t, x, z, ev, zj, G = _ode_case(H, xd, zd, seed=1000 + H + 10 * xd + zd)
                a0 = torch.cat((x[0], z[0]), -1)
                xs, saved = fused.ode_integrate(method, layers, t, x, z, a0, event_t=ev, z_jump=zj, save=True)
                tab = fused.event_table(t, ev)
                runs = {"rec": dict(xs=xs), "saved": dict(xs=xs, saved=saved), "tf": dict(xs=x, input_true_x=True)}
                for form, kw in runs.items():
                    gx0, gz, gzj, ga0, gp = fused.ode_backward(method, layers, t, z, a0, kw.pop("xs"), G, event_idx=tab, z_jump=zj, kernel="wide", **kw)
                    out = dict(x0=gx0, z=gz, zj=gzj, a0=ga0, **{f"p{k}": q for k, q in enumerate(gp)})
                    for name, q in out.items():
                        res[f"K4f h{H} {method} x{xd}z{zd} {form} {name}"] = _digest(q)
    for H in (32, 64, 128):
        for method in METHODS:
            for xd, zd, vd, idim in ((8, 2, 2, 2), (3, 1, 0, 1), (2, 2, 4, 2)):
                g = torch.Generator().manual_seed(7 + H + xd)
                de, ae, t, z, v, xi, a0, ev, zj, vj, Gx, Gi = _dae_raw_case(B, T, xd, zd, vd, idim, seed=2000 + H + 10 * xd + vd, events=True, H=H)
                xe, ie = torch.zeros(T, B, 0, device="cuda"), torch.zeros(T, B, idim, device="cuda")
                xs, is_, saved = fused.dae_integrate(method, de, ae, xi, t, xe, z, v, ie, a0, event_t=ev, z_jump=zj, v_jump=vj, save=True)
                tab = fused.event_table(t, ev)
                xt, it = (0.1 * torch.randn(T, B, xd, generator=g)).cuda(), (0.1 * torch.randn(T, B, idim, generator=g)).cuda()
                common = dict(event_idx=tab, z_jump=zj, v_jump=vj)
                runs = {"rec": fused.dae_backward(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, kernel="wide", **common),
                        "saved": fused.dae_backward_wide(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, saved=saved, **common),
                        "tfx": fused.dae_backward_wide(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, x_true=xt, **common),
                        "tfi": fused.dae_backward_wide(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, i_true=it, **common),
                        "tfxi": fused.dae_backward_wide(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, x_true=xt, i_true=it, **common)}
                for form, out in runs.items():
                    for name, q in out.items():
                        for k, qq in enumerate(q if isinstance(q, (list, tuple)) else [q]):
                            res[f"K7f h{H} {method} x{xd}z{zd}v{vd}i{idim} {form} {name}{k}"] = _digest(qq)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f"child: {len(res)} digests from {_lib.LIB_PATH}")


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    limit = sys.argv[sys.argv.index("--timeout") + 1] if "--timeout" in sys.argv else "420"
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, lib in enumerate(libs):
            out = os.path.join(tmp, f"{k}.json")
            rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child", out],
                                env=dict(os.environ, PSNODE_LIB_PATH=lib)).returncode
            if rc != 0:
                print(f"child for {lib} exited with {rc}: stopping")
                return 2
            got.append(json.load(open(out)))
    a, b = got
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"A = {libs[0]}\nB = {libs[1]}\n{len(a)} / {len(b)} digests, {len(differ)} differ")
    for k in differ:
        print("    differs:", k)
    print("ALL DIGESTS EQUAL" if not differ and a else "DIFFERENCES")
    return 1 if differ or not a else 0


if __name__ == "__main__":
    sys.exit(main())
