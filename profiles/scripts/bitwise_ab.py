"""Bit-for-bit A/B of two builds of the library on every specialised kernel family (K1 .. K9w, K11): a change to their host side -- which
instance a call launches, its grid, the pointers it binds -- shows up as a different digest.

    python profiles/scripts/bitwise_ab.py LIB_A LIB_B [--timeout SECONDS]

For each library in turn one fresh child process (PSNODE_LIB_PATH set, under its own `timeout -k 10`) runs the cases below on inputs drawn on
the CPU from fixed seeds and writes one SHA-256 per output tensor to a JSON file; the parent compares the two files and prints the names that
differ.  The second child is not started when the first one fails.  These kernels sum in a fixed order, so every digest has to be equal; run
A against A first and leave out what is not (none so far).
Cases (T = 4 grid points, B = 17 trajectories: one full tile of 16 and a ragged one, and B = 5 -- a ragged wave -- for the one-wave
kernels; events with jump values wherever z or v exist; euler / midpoint / rk4 throughout).  The dispatch arm each case reaches follows
from the launchers' own formulas: NZM = (2 ne + 3) / 4 with ne = z (+ v + i), NZA = (z + v + 3) / 4:
  K1    ode_integrate(kernel="tile"): hidden 64, x 3, z 0 / 1 / 3 / 5 / 7 (NZM 0 .. 4), plain and save=True; hidden 32 / 128 / 192 / 256
        (2 / 8 / 12 / 16 waves) and x 12 (the four-register form of x_dim 9 .. 16) at z 2
  K1x   ode_integrate(kernel="wave"): the same z list at hidden 48, plain and save=True, B = 5 and 17
  K2    dae_integrate(kernel="tile"): hidden 64, x 3, (z, v, i) = (0,1,1) (1,1,1) (2,2,2) (2,3,1) (2,2,4) (4,3,1) -- the pairs NZM NZA =
        11 21 31 32 41 42 --, plain and save=True; hidden 32 / 128 / 192 at (2,2,2)
  K2x   dae_integrate(kernel="wave"): (0,1,1) (1,1,1) (2,2,2) (2,3,1), plain and save=True, B = 5 and 17
  K3a / K3f / K3c / K3w   the latent shapes x = v = i = H, z = H or 0, through ode_integrate / dae_integrate(kernel="mfma") at H = 16
        (K3f the ODE, K3a the DAE), 64 (K3c), 32 and 128 (K3w at 4 and 8 waves), plain and -- H >= 32 -- save=True
  K3f encoded / K3g   ode_encoded_integrate, dae_encoded_integrate (z 2 and z 0)
  K4f   fused.ode_backward(kernel="wide"): hidden 32 / 48 / 64 / 128, (x, z) = (3, 0) / (8, 2) / (8, 7), recompute form, saved-row form
        (two-role kernels at hidden <= 64), teacher-forced recompute form
  K4x   fused.ode_backward(kernel="wave", saved=): hidden 48, z 0 / 3 / 7, with and without grad_z, B = 5 and 17
  K7f + K7h   fused.dae_backward(kernel="wide") (recompute form) / fused.dae_backward_wide (saved form, teacher forcing: K7f's own entry,
        no other kernel behind it): hidden 32 / 64 / 128, (x, z, v, i) = (8, 2, 2, 2) / (3, 1, 0, 1) / (2, 2, 4, 2), recompute and saved
        forms, teacher forcing of x, of i and of both; hidden 64, x 3 over K2's six (z, v, i), recompute and saved forms
  K8f / K8 / K9 / K9w   ode_backward / dae_backward(kernel="mfma") on the latent shapes: H = 16 (K8f the ODE, K8 the DAE with z and without),
        64 (K9: the ODE form, the DAE recompute form and -- saved= -- the DAE roles form, each at nbe 3 (z) and 2 (no z)), 32 and 128
        (K9w at 4 and 8 waves, saved rows)
  K11   fused.linear_rows: K = 16 .. 128 in steps of 16 (the float4 instances) and K = 3 / 7 / 13 / 30 / 61 / 100 (the scalar ones), epi 0 / 1
The library does not report which kernel a call took: a forced `kernel=` takes that kernel or raises, which is what the child relies on;
a case the library refuses (UnsupportedShapeError) is recorded as such and printed, never skipped silently.
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


def _ode_case(H, xd, zd, seed, Bn=B):
    import torch
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = xd + zd
    dims = [3 * n, H, H, H, xd]
    layers = [(l.weight.detach().cuda(), l.bias.detach().cuda()) for l in [nn.Linear(dims[k], dims[k + 1]) for k in range(4)]]
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, Bn, 1)
    t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, Bn - 1, 1, generator=g))
    x, z = 0.1 * torch.randn(T, Bn, xd, generator=g), 0.1 * torch.randn(T, Bn, zd, generator=g)
    ev = t[2, :, :].unsqueeze(1).contiguous()
    zj = 0.1 * torch.randn(Bn, 1, zd, generator=g)
    G = torch.randn(T, Bn, xd, generator=g)
    return layers, t.cuda(), x.cuda(), z.cuda(), ev.cuda(), zj.cuda(), G.cuda()


def _latent_case(H, zd, dae, seed, Bn):
    """x = v = i = H, z = H or 0; one event"""
    import torch
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    mk = lambda dims: [(l.weight.detach().cuda(), l.bias.detach().cuda()) for l in [nn.Linear(dims[k], dims[k + 1]) for k in range(len(dims) - 1)]]
    nblk = (4 if zd else 3) if dae else 2
    de, ae = mk([3 * nblk * H, H, H]), mk([(2 * nblk - 1) * H, H, H]) if dae else None
    r = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
    t = (torch.arange(T, dtype=torch.float32) * 0.01).view(T, 1, 1).repeat(1, Bn, 1)
    t[:, 1:] = t[:, 1:] * (0.5 + torch.rand(1, Bn - 1, 1, generator=g))
    x, z, v, i, xi = r(T, Bn, H), r(T, Bn, zd), r(T, Bn, H), r(T, Bn, H), r(Bn, H)
    ev = t[2, :, :].unsqueeze(1).contiguous().cuda()
    zj, vj = r(Bn, 1, zd), r(Bn, 1, H)
    Gx, Gi = r(T, Bn, H), r(T, Bn, H)
    return de, ae, t.cuda(), x, z, v, i, xi, ev, zj, vj, Gx, Gi


def _flat(out):
    """(name, tensor) of a fused call's result: a tensor, a tuple / list of them (nested), or a dict"""
    if out is None or hasattr(out, "detach"):
        return [("", out)]
    items = out.items() if isinstance(out, dict) else enumerate(out)
    return [(f".{k}{n}", q) for k, o in items for n, q in _flat(o)]


def new_cases(res):
    """every family but K4f / K7f (child() below keeps those)"""
    import torch
    import torch.nn as nn
    from py_psnode_amd import _lib, fused
    from test_gpu_backward import _dae_raw_case

    def put(name, fn):
        try:
            out = fn()
        except _lib.UnsupportedShapeError as e:
            res[name] = "refused: " + str(e)[:60]
            print("refused:", name)
            return None
        for n, q in _flat(out):
            res[name + n] = _digest(q)
        return out

    ZS = (0, 1, 3, 5, 7)
    ZVI = ((0, 1, 1), (1, 1, 1), (2, 2, 2), (2, 3, 1), (2, 2, 4), (4, 3, 1))
    for method in METHODS:
        # K1 / K1x (and K4x on K1x's saved rows)
        ode = [("tile", 64, 3, zd, B) for zd in ZS] + [("tile", H, 3, 2, B) for H in (32, 128, 192, 256)] + [("tile", 64, 12, 2, B)]
        ode += [("wave", 48, 3, zd, Bn) for zd in ZS for Bn in (5, B)]
        for kern, H, xd, zd, Bn in ode:
            layers, t, x, z, ev, zj, G = _ode_case(H, xd, zd, seed=3000 + H + 10 * xd + zd, Bn=Bn)
            a0 = torch.cat((x[0], z[0]), -1)
            evs = dict(event_t=ev, z_jump=zj) if zd else {}
            tag = f"{'K1' if kern == 'tile' else 'K1x'} h{H} {method} x{xd}z{zd} B{Bn}"
            put(tag + " plain", lambda: fused.ode_integrate(method, layers, t, x, z, a0, kernel=kern, **evs))
            if H <= 128 and xd <= 8:
                got = put(tag + " save", lambda: fused.ode_integrate(method, layers, t, x, z, a0, kernel=kern, save=True, **evs))
                if kern == "wave" and got is not None and zd in (0, 3, 7):
                    tab = fused.event_table(t, ev) if zd else None
                    for gz in (True, False):
                        put(f"K4x h{H} {method} x{xd}z{zd} B{Bn} gz{int(gz)}",
                            lambda: fused.ode_backward(method, layers, t, z, a0, got[0], G, event_idx=tab, z_jump=zj if zd else None, kernel="wave",
                                                       saved=got[1], need_grad_z=gz, need_grad_zj=gz))
        # K2 / K2x
        dae = [("tile", 64, zvi, B) for zvi in ZVI] + [("tile", H, (2, 2, 2), B) for H in (32, 128, 192)]
        dae += [("wave", 48, zvi, Bn) for zvi in ZVI[:4] for Bn in (5, B)]
        for kern, H, (zd, vd, idim), Bn in dae:
            de, ae, t, z, v, xi, a0, ev, zj, vj, Gx, Gi = _dae_raw_case(Bn, T, 3, zd, vd, idim, seed=4000 + H + 100 * zd + 10 * vd + idim, events=True, H=H)
            xe, ie = torch.zeros(T, Bn, 0, device="cuda"), torch.zeros(T, Bn, idim, device="cuda")
            tag = f"{'K2' if kern == 'tile' else 'K2x'} h{H} {method} z{zd}v{vd}i{idim} B{Bn}"
            for save in (False, True) if H <= 128 else (False,):
                put(tag + (" save" if save else " plain"),
                    lambda: fused.dae_integrate(method, de, ae, xi, t, xe, z, v, ie, a0, event_t=ev, z_jump=zj, v_jump=vj, kernel=kern, save=save))
        # K7f over the same (z, v, i): every NZM / NZA pair
        for zd, vd, idim in ZVI:
            de, ae, t, z, v, xi, a0, ev, zj, vj, Gx, Gi = _dae_raw_case(B, T, 3, zd, vd, idim, seed=4500 + 100 * zd + 10 * vd + idim, events=True, H=64)
            xe, ie = torch.zeros(T, B, 0, device="cuda"), torch.zeros(T, B, idim, device="cuda")
            xs, is_, saved = fused.dae_integrate(method, de, ae, xi, t, xe, z, v, ie, a0, event_t=ev, z_jump=zj, v_jump=vj, save=True)
            common = dict(event_idx=fused.event_table(t, ev), z_jump=zj, v_jump=vj)
            tag = f"K7f h64 {method} x3z{zd}v{vd}i{idim}"
            put(tag + " rec", lambda: fused.dae_backward(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, kernel="wide", **common))
            put(tag + " saved", lambda: fused.dae_backward_wide(method, de, ae, t, z, v, a0, xs, is_, Gx, Gi, saved=saved, **common))
        # the latent shapes, forward and backward
        for H in (16, 64, 32, 128):
            for dae_, zd in ((False, H), (True, H), (True, 0)):
                de, ae, t, x, z, v, i, xi, ev, zj, vj, Gx, Gi = _latent_case(H, zd, dae_, seed=5000 + H + (7 if dae_ else 0) + (zd > 0), Bn=B)
                tag = f"latent h{H} {method} {'dae' if dae_ else 'ode'} z{zd}"
                tab = fused.event_table(t, ev)
                if not dae_:
                    a0 = torch.cat((x[0], z[0]), -1)
                    fwd = lambda save: fused.ode_integrate(method, de, t, x, z, a0, event_t=ev, z_jump=zj, kernel="mfma", save=save)
                    bwd = lambda xs, sv: fused.ode_backward(method, de, t, z, a0, xs, Gx, event_idx=tab, z_jump=zj, kernel="mfma", saved=sv)
                else:
                    a0 = torch.cat((xi, z[0], v[0], i[0]), -1)
                    jumps = dict(z_jump=zj if zd else None, v_jump=vj)
                    fwd = lambda save: fused.dae_integrate(method, de, ae, xi, t, x, z, v, i, a0, event_t=ev, kernel="mfma", save=save, **jumps)
                    bwd = lambda xs, sv: fused.dae_backward(method, de, ae, t, z, v, a0, xs[0], xs[1], Gx, Gi, event_idx=tab, kernel="mfma", saved=sv,
                                                            **jumps)
                out = put(tag + " fwd", lambda: fwd(False))
                if out is not None and H in (16, 64):
                    put(tag + " bwd rec", lambda: bwd(out, None))
                if H >= 32:
                    got = put(tag + " fwd save", lambda: fwd(True))
                    if got is not None:
                        put(tag + " bwd saved", lambda: bwd(got[:2] if dae_ else got[0], got[-1]))
        # the one-launch models
        g = torch.Generator().manual_seed(61)
        torch.manual_seed(61)
        mlp2 = lambda din, h, dout: [(l.weight.detach().cuda(), l.bias.detach().cuda()) for l in (nn.Linear(din, h), nn.Linear(h, dout))]
        r = lambda *s: (0.3 * torch.randn(*s, generator=g)).cuda()
        tb = ((torch.arange(T, dtype=torch.float32) * 0.01).view(1, T, 1).repeat(B, 1, 1)).cuda()
        evb = tb[:, [2], :].contiguous()
        put(f"K3f encoded {method}", lambda: fused.ode_encoded_integrate(method, mlp2(5, 16, 16), mlp2(3, 16, 16), mlp2(16, 16, 5), mlp2(96, 16, 16), tb,
                                                                          r(B, T, 5), r(B, T, 3), event_t=evb, z_jump=r(B, 1, 3), want_latent=True))
        for zd in (2, 0):
            nblk = 4 if zd else 3
            put(f"K3g {method} z{zd}", lambda: fused.dae_encoded_integrate(
                method, mlp2(5, 64, 64), mlp2(zd, 64, 64) if zd else None, mlp2(3, 64, 64), mlp2(2, 64, 64), mlp2(64, 64, 5), mlp2(64, 64, 2),
                mlp2(3 * nblk * 64, 64, 64), mlp2((2 * nblk - 1) * 64, 64, 64), r(B, 5), tb, r(B, T, 5), r(B, T, zd), r(B, T, 3), r(B, T, 2),
                event_t=evb, z_jump=r(B, 1, zd), v_jump=r(B, 1, 3)))
    # K11
    g = torch.Generator().manual_seed(71)
    for K in (16, 32, 48, 64, 80, 96, 112, 128, 3, 7, 13, 30, 61, 100):
        x2, W, bias = (torch.randn(37, K, generator=g).cuda(), torch.randn(24, K, generator=g).cuda(), torch.randn(24, generator=g).cuda())
        for epi in (0, 1):
            put(f"K11 K{K} epi{epi}", lambda: fused.linear_rows(x2, W, bias, epi=epi))


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    from py_psnode_amd import _lib, fused
    from test_gpu_backward import _dae_raw_case
    assert os.path.samefile(_lib.LIB_PATH, os.environ["PSNODE_LIB_PATH"]), _lib.LIB_PATH
    res = {}
    new_cases(res)
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
    limit = sys.argv[sys.argv.index("--timeout") + 1] if "--timeout" in sys.argv else "540"
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
