"""A/B of what the K0 / K5 option-family tests feed the solvers, between two checkouts; needs no GPU and launches nothing.

    python profiles/scripts/test_inputs_ab.py PARENT_CHECKOUT [HEAD_CHECKOUT] [--out FILE]

For each checkout in turn one fresh child process loads the six GPU test modules of its tests/ directory and calls every test function
once per entry of its own parametrisation lists (the pytest.mark.parametrize marks, outermost first), with
  - FixedGridODESolver.integrate_ODE / integrate_DAE replaced by a recorder: it writes down a SHA-256, dtype and shape of everything the
    call was given -- solver class, method, substeps, externals, fused, kernel; every parameter of the modules; t, x, z, v, i, x_init,
    all_initial; the event times and jump rows; the teacher-forcing flags; which tensors are leaves -- returns zeros that hang on the
    leaves, and records the cotangent that later arrives at each output (the G / Gi / Hi of the training tests);
  - `.cuda()` and `.to(device=...)` the identity on the device, so that a case reaches the recorder the way it would reach the kernels;
  - the modules of tests/ compiled without their assert statements and pytest.raises / pytest.warns swallowing, so that a test goes on to
    its next solver call where the zeros would fail a gate.
A test that still stops (it calls fused.* directly, which refuses host tensors) is compared up to there and counted under "stopped".
The parent compares the two recordings per test id, call by call, tensor by tensor; the table is: file x tests x solver calls x tensors
compared x mismatches.  Whatever a case builder, a cotangent generator or a test body does to an input between the seed and the solver
shows here; the figures of a run are kept in profiles/test_harness_ab.txt."""
import hashlib
import importlib.machinery
import importlib.util
import itertools
import json
import os
import subprocess
import sys
import tempfile

FILES = ("test_gpu_activations", "test_gpu_activations_pre", "test_gpu_rk_tableau", "test_gpu_substeps", "test_gpu_externals_linear",
         "test_gpu_teacher_forced_generic")


# ----------------------------------------------------------------------------- child: record one checkout
class _NoAsserts(importlib.machinery.SourceFileLoader):
    def get_code(self, fullname):
        with open(self.get_filename(fullname), "rb") as f:
            return compile(f.read(), self.get_filename(fullname), "exec", optimize=1)


class _TestsDirFinder:
    def __init__(self, tests):
        self.tests = tests

    def find_spec(self, name, path=None, target=None):
        p = os.path.join(self.tests, name + ".py")
        if "." not in name and os.path.exists(p):
            return importlib.util.spec_from_file_location(name, p, loader=_NoAsserts(name, p))
        return None


class _Swallow:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return True


def _record(root, out_path):
    tests = os.path.join(root, "tests")
    sys.dont_write_bytecode = True
    sys.path[:0] = [tests, root]
    sys.meta_path.insert(0, _TestsDirFinder(tests))
    import warnings
    import pytest
    import torch
    import torch.nn as nn
    from py_psnode_amd import neural_dae as nd
    warnings.simplefilter("ignore")

    log = []

    def digest(a):
        if a is None:
            return None
        d = a.detach()
        return [str(d.dtype), list(d.shape), bool(a.requires_grad), hashlib.sha256(d.contiguous().numpy().tobytes()).hexdigest()]

    def event_of(fn):
        ev = getattr(fn, "__self__", None)
        return None if ev is None else {k: digest(v) for k, v in sorted(vars(ev).items()) if torch.is_tensor(v)}

    def solver_of(s):
        m = s.method
        return [type(s).__name__, m if isinstance(m, str) else repr(m), getattr(s, "substeps", None), getattr(s, "externals", None), s.fused, s.kernel]

    def outputs(entry, shapes, like, leaves):
        anchor = sum((q.sum() for q in leaves if q.requires_grad), torch.zeros((), dtype=like.dtype)) * 0.0
        outs = []
        for k, shape in enumerate(shapes):
            o = torch.zeros(shape, dtype=like.dtype) + anchor
            if o.requires_grad:
                o.register_hook(lambda g, k=k: log.append([entry + " cotangent", k, digest(g)]))
            outs.append(o)
        return outs

    def integrate_ODE(self, x_func, t, x, z, all_initial, event_fn=None, jump_change_fn=None, input_true_x=False, x_init=None):
        params = list(x_func.parameters())
        log.append(["integrate_ODE", solver_of(self), [digest(p) for p in params], {k: digest(v) for k, v in
                   dict(t=t, x=x, z=z, all_initial=all_initial, x_init=x_init).items()}, event_of(event_fn), bool(input_true_x)])
        leaves = params + [q for q in (x, z, all_initial, x_init) if q is not None] + [v for v in vars(getattr(event_fn, "__self__", None) or nn.Identity()).values() if torch.is_tensor(v)]
        return outputs("integrate_ODE", [x.shape], all_initial, leaves)[0]

    def integrate_DAE(self, x_init, x_func, i_func, t, x, z, v, i, all_initial, event_fn=None, jump_change_fn=None, input_true_x=False,
                      input_true_i=False):
        params = list(x_func.parameters()) + list(i_func.parameters())
        log.append(["integrate_DAE", solver_of(self), [digest(p) for p in params], {k: digest(q) for k, q in
                   dict(x_init=x_init, t=t, x=x, z=z, v=v, i=i, all_initial=all_initial).items()}, event_of(event_fn),
                    [bool(input_true_x), bool(input_true_i)]])
        leaves = params + [x_init, x, z, v, i, all_initial] + [q for q in vars(getattr(event_fn, "__self__", None) or nn.Identity()).values() if torch.is_tensor(q)]
        return tuple(outputs("integrate_DAE", [t.shape[:2] + x_init.shape[-1:], i.shape], all_initial, leaves))

    nd.FixedGridODESolver.integrate_ODE, nd.FixedGridODESolver.integrate_DAE = integrate_ODE, integrate_DAE
    t_to, m_to = torch.Tensor.to, nn.Module.to
    host = lambda kw: {k: v for k, v in kw.items() if k != "device"}
    here = lambda a: [q for q in a if not isinstance(q, (str, torch.device))]

    def tensor_to(self, *a, **k):          # (a copy to the device is a new tensor that hangs on the old one)
        r = t_to(self, *here(a), **host(k))
        return r.clone() if r is self and (len(here(a)) < len(a) or "device" in k) else r

    torch.Tensor.cuda = lambda self, *a, **k: self.clone()
    torch.Tensor.to = tensor_to
    nn.Module.cuda = lambda self, *a, **k: self
    nn.Module.to = lambda self, *a, **k: m_to(self, *here(a), **host(k))
    torch.cuda.synchronize = lambda *a, **k: None

    class _Pytest:
        raises = warns = _Swallow

        def __getattr__(self, name):
            return getattr(pytest, name)

    result = {}
    for name in FILES:
        mod = importlib.import_module(name)
        mod.pytest = _Pytest()
        for fname, fn in sorted(vars(mod).items()):
            if not fname.startswith("test_") or not callable(fn):
                continue
            marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
            axes = []
            for m in reversed(marks):          # (the lowest decorator is the first mark)
                names = [q.strip() for q in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
                axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
            for combo in itertools.product(*axes):
                kw = {k: v for part in combo for k, v in part.items()}
                if "monkeypatch" in fn.__code__.co_varnames[:fn.__code__.co_argcount]:
                    kw["monkeypatch"] = pytest.MonkeyPatch()
                del log[:]
                stopped = None
                try:
                    fn(**kw)
                except BaseException as e:      # (pytest.skip raises a BaseException)
                    stopped = f"{type(e).__name__}: {str(e)[:120]}"
                tid = f"{name}::{fname}[{'-'.join(f'{k}={v!r}' for k, v in sorted(kw.items()) if k != 'monkeypatch')}]"
                result[tid] = {"calls": json.loads(json.dumps(log)), "stopped": stopped}
    with open(out_path, "w") as f:
        json.dump(result, f)


# ----------------------------------------------------------------------------- parent: run both children, compare
def _tensors(rec):
    """(label, digest) of every tensor of one recorded call; everything that is not a tensor digest goes into one 'settings' item"""
    if rec[0].endswith("cotangent"):
        return [(f"cotangent {rec[1]}", rec[2])]
    out = [("settings", [rec[1], rec[5]])]
    out += [(f"param {k}", d) for k, d in enumerate(rec[2])]
    out += [(k, d) for k, d in rec[3].items()]
    out += [(f"event {k}", d) for k, d in (rec[4] or {}).items()]
    return out


def main(argv):
    if argv[:1] == ["--record"]:
        return _record(argv[1], argv[2])
    out = None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        argv = [a for k, a in enumerate(argv) if a != "--out" and argv[k - 1] != "--out"]
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    roots = [os.path.abspath(argv[0]), os.path.abspath(argv[1]) if len(argv) > 1 else here]
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, root in enumerate(roots):
            path = os.path.join(tmp, f"{k}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--record", root, path], check=True, stdout=subprocess.DEVNULL)
            with open(path) as f:
                recs.append(json.load(f))
    a, b = recs
    lines = [f"{'file':36s} {'tests':>6s} {'stopped':>8s} {'solver calls':>13s} {'cotangents':>11s} {'tensors':>8s} {'mismatches':>11s}"]
    bad = []
    total = [0] * 6
    for name in FILES:
        ids = sorted(set(k for k in a if k.startswith(name + "::")) | set(k for k in b if k.startswith(name + "::")))
        row = [len(ids), 0, 0, 0, 0, 0]
        for tid in ids:
            ra, rb = a.get(tid), b.get(tid)
            if ra is None or rb is None:
                row[5] += 1
                bad.append(f"{tid}: only in {'head' if ra is None else 'parent'}")
                continue
            row[1] += (ra["stopped"] is not None) or (rb["stopped"] is not None)
            if len(ra["calls"]) != len(rb["calls"]) or (ra["stopped"] is None) != (rb["stopped"] is None):
                row[5] += 1
                bad.append(f"{tid}: {len(ra['calls'])} records / stopped {ra['stopped']!r} at the parent, {len(rb['calls'])} / {rb['stopped']!r} at head")
            for k, (ca, cb) in enumerate(zip(ra["calls"], rb["calls"])):
                row[3 if ca[0].endswith("cotangent") else 2] += 1
                ta, tb = _tensors(ca), _tensors(cb)
                if ca[0] != cb[0] or [l for l, _ in ta] != [l for l, _ in tb]:
                    row[5] += 1
                    bad.append(f"{tid}: record {k} is {ca[0]} with {[l for l, _ in ta]} at the parent, {cb[0]} with {[l for l, _ in tb]} at head")
                    continue
                for (label, da), (_, db) in zip(ta, tb):
                    row[4] += label != "settings" and da is not None
                    if da != db:
                        row[5] += 1
                        bad.append(f"{tid}: record {k} ({ca[0]}) {label}: {da} at the parent, {db} at head")
        total = [p + q for p, q in zip(total, row)]
        lines.append(f"{name:36s} {row[0]:6d} {row[1]:8d} {row[2]:13d} {row[3]:11d} {row[4]:8d} {row[5]:11d}")
    lines.append(f"{'total':36s} {total[0]:6d} {total[1]:8d} {total[2]:13d} {total[3]:11d} {total[4]:8d} {total[5]:11d}")
    lines += bad[:200]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 1 if total[5] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
