"""Which torch.autograd.Function, which forward call and which backward call `autograd.fused_ode_integrate` / `fused_dae_integrate` make of
a call's options -- against a recorded table (no GPU, no built library: recording stand-ins take the place of the `fused` functions).

tests/autograd_route_table.txt has one line per case, `<case> -> <outcome>`.  A case is one point of the grid
    model x method x act x substeps x externals x events x segment x teacher forcing x kernel
(written in this order, blank-separated; two values each but three methods, three kinds of events and, for the DAE, teacher forcing off / x / i --
a segment that no step reaches and teacher forcing of x and i together were dropped to keep the table below the size of
tests/workspace_bytes_table.txt) on tiny CPU tensors (T=5, B=3, x 2, z 1, v 1, i 1, hidden 4) with every differentiable input requiring a gradient.  The outcome:
    <class of xs.grad_fn> | <forward call> | <backward call> | grads <the named inputs that got one> | saved <autograd.last_saved_bytes>
or, where the call raises, `E<n>`, which a line `# E<n> = <exception type>: <its message>` at the top of the table writes out.  An MLP
[(W, b), ...] is written as its widths, `mlp:in-h-..-out`.  A call is written as the stand-in received it, bound against the REAL
function's signature with the defaults applied: only the arguments that differ from their defaults are printed, tensors as shapes, so that
handing a default over and leaving it out are the same line.  `saved -1`: the route does not touch last_saved_bytes.
The forward stand-ins run what the real functions run before anything else (`GenericOpts.of`, `require_generic` under their own name,
`no_teacher_forcing`, the DAE's segment-without-x ValueError) and return zero tensors of the documented shapes; `event_table` returns a
fixed table.
The table is recorded at the commit BEFORE a change to the routing, never from the changed code:
    git checkout <that commit> -- py_psnode_amd && python tests/test_autograd_routes_host.py --record [--commit <its id>]"""
import contextlib
import inspect
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from py_psnode_amd import _lib, autograd, fused  # noqa: E402

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "autograd_route_table.txt")
T, B, XD, ZD, VD, ID, H = 5, 3, 2, 1, 1, 1, 4
TANH = fused.Act(_lib.ACT_TANH, name="Tanh")
HEUN = fused.Tableau("Heun", ((), (1.0,)), (0.5, 0.5), 2)
METHODS = ("rk4", HEUN, "ab2")
EVENTS = ("-", "shared", "per")
SEGMENTS = (None, 2)          # 2 < T - 1: grid point 2 and 4 restart
TF = {"ode": ("-", "x"), "dae": ("-", "x", "i")}
KERNELS = ("auto", "mfma")
N_CASES = 1440          # 576 ODE cases + 864 DAE cases
STAND_INS = ("ode_integrate", "dae_integrate", "ode_backward", "dae_backward", "dae_backward_tf", "dae_backward_wide", "event_table")
REAL = {name: getattr(fused, name) for name in STAND_INS}
CLASSES = ["_FusedOde", "_FusedDae", "_FusedDaeTeacherForced"] + [f"_Fused{m}{f}" for m in ("Ode", "Dae") for f in ("Sub", "Lin", "Pev", "Ab", "AbPev", "Ms")]


def show(v) -> str:
    if isinstance(v, torch.Tensor):
        return ("" if v.dtype == torch.float32 else str(v.dtype).replace("torch.", "") + ":") + "x".join(str(n) for n in v.shape)
    if isinstance(v, list) and v and all(isinstance(q, tuple) and len(q) == 2 and isinstance(q[0], torch.Tensor) for q in v):
        return "mlp:" + "-".join([str(v[0][0].shape[1])] + [str(b.shape[0]) for _, b in v])          # [(W[out,in], b[out]), ...] as its widths
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(show(q) for q in v) + "]"
    if isinstance(v, fused.Tableau):
        return f"Tableau({v.name})"
    return repr(v) if isinstance(v, fused.Act) else str(v)


def bound(name, args, kwargs):
    b = inspect.signature(REAL[name]).bind(*args, **kwargs)
    b.apply_defaults()
    return b.arguments


def call_text(name, arguments) -> str:
    """`name(argument=value, ...)` of the arguments that are not their defaults."""
    defaults = {k: p.default for k, p in inspect.signature(REAL[name]).parameters.items()}
    given = [(k, v) for k, v in arguments.items() if isinstance(v, (torch.Tensor, list, tuple)) or v != defaults[k]]
    return f"{name}({', '.join(f'{k}={show(v)}' for k, v in given)})"


class StandIns:
    """The recording stand-ins of the `fused` functions autograd.py calls."""

    def __init__(self):
        self.calls = []

    def _note(self, name, args, kwargs):
        a = bound(name, args, kwargs)
        self.calls.append(call_text(name, a))
        return a

    def ode_integrate(self, *args, **kwargs):
        a = self._note("ode_integrate", args, kwargs)
        pt = bool(a["per_trajectory"]) and fused.has_events(a["t"], a["event_t"], a["event_idx"])
        opts = fused.GenericOpts.of(a["method"], (a["act"],), a["substeps"], a["externals"], pt, a["segment"])
        opts.require_generic("ode_integrate", a["kernel"], a["save"])
        opts.no_teacher_forcing("ode_integrate", a["input_true_x"])
        xs = torch.zeros((a["t"].shape[0], a["x"].shape[1], a["x"].shape[2]))
        if a["save_sub"]:
            return xs, self._x_sub(opts, xs)
        return (xs, None) if a["save"] else xs

    def dae_integrate(self, *args, **kwargs):
        a = self._note("dae_integrate", args, kwargs)
        pt = bool(a["per_trajectory"]) and fused.has_events(a["t"], a["event_t"], a["event_idx"])
        opts = fused.GenericOpts.of(a["method"], fused.dae_acts(a["act"]), a["substeps"], a["externals"], pt, a["segment"])
        opts.require_generic("dae_integrate", a["kernel"], a["save"])
        opts.no_teacher_forcing("dae_integrate", a["input_true_x"] or a["input_true_i"])
        if a["segment"] is not None and a["x"].shape[-1] == 0:
            raise ValueError(f"dae_integrate: segment={a['segment']} restarts from the dataset rows x[k]; this call has none (x.shape[-1] == 0)")
        n_t, n_b = a["t"].shape[0], a["t"].shape[1]
        xs, is_ = torch.zeros((n_t, n_b, a["x_init"].shape[-1])), torch.zeros((n_t, n_b, a["i"].shape[-1]))
        if a["save_sub"]:
            return xs, is_, self._x_sub(opts, xs)
        return (xs, is_, None) if a["save"] else (xs, is_)

    @staticmethod
    def _x_sub(opts, xs):
        return torch.zeros((xs.shape[0] - 1, opts.substeps - 1, xs.shape[1], xs.shape[2])) if opts.takes.x_sub else None

    def ode_backward(self, *args, **kwargs):
        a = self._note("ode_backward", args, kwargs)
        z, zj = a["z"], a["z_jump"]
        gz = torch.zeros(z.shape) if a["need_grad_z"] else None
        gzj = torch.zeros(zj.shape) if (a["event_idx"] is not None and zj is not None and a["need_grad_zj"]) else None
        return (torch.zeros(a["xs"].shape[1:]), gz, gzj, torch.zeros(a["all_initial"].shape),
                [torch.zeros(q.shape) for wb in a["de_layers"] for q in wb])

    def _dae_backward(self, name, args, kwargs):
        a = self._note(name, args, kwargs)
        like = lambda q: None if q is None else torch.zeros(q.shape)
        return dict(x_init=torch.zeros(a["xs"].shape[1:]), z=like(a["z"]), v=like(a["v"]), z_jump=like(a["z_jump"]), v_jump=like(a["v_jump"]),
                    all_initial=like(a["all_initial"]), de=[like(q) for wb in a["de_layers"] for q in wb],
                    ae=[like(q) for wb in a["ae_layers"] for q in wb])

    def dae_backward(self, *args, **kwargs):
        return self._dae_backward("dae_backward", args, kwargs)

    def dae_backward_tf(self, *args, **kwargs):
        return self._dae_backward("dae_backward_tf", args, kwargs)

    def dae_backward_wide(self, *args, **kwargs):
        return self._dae_backward("dae_backward_wide", args, kwargs)

    def event_table(self, *args, **kwargs):
        a = bound("event_table", args, kwargs)
        if a["event_t"] is None:
            return None
        table = torch.tensor([-1, 0, -1, -1], dtype=torch.int32)
        return table.view(T - 1, 1).repeat(1, B).contiguous() if a["per_trajectory"] else table


@contextlib.contextmanager
def stand_ins():
    s = StandIns()
    try:
        for name in STAND_INS:
            setattr(fused, name, getattr(s, name))
        yield s
    finally:
        for name in STAND_INS:
            setattr(fused, name, REAL[name])


def mlp(widths):
    return [(torch.zeros((o, i), requires_grad=True), torch.zeros(o, requires_grad=True)) for i, o in zip(widths[:-1], widths[1:])]


def grid():
    for model in ("ode", "dae"):
        yield from itertools.product((model,), METHODS, (None, TANH), (1, 2), ("hold", "linear"), EVENTS, SEGMENTS, TF[model], KERNELS)


def case_text(model, method, act, substeps, externals, events, segment, tf, kernel) -> str:
    return f"{model} {show(method)} {'Tanh' if act else '-'} {substeps} {externals} {events} {segment or '-'} {tf} {kernel}"


def run(model, method, act, substeps, externals, events, segment, tf, kernel) -> str:
    """The outcome of one case under the stand-ins."""
    g = lambda *shape: torch.zeros(shape, requires_grad=True)
    t = torch.arange(T, dtype=torch.float32).view(T, 1, 1).repeat(1, B, 1)
    event_t = None if events == "-" else t[2].view(B, 1, 1).clone()
    common = dict(substeps=substeps, externals=externals, per_trajectory=events == "per", segment=segment)
    autograd.last_saved_bytes = -1
    with stand_ins() as s:
        try:
            if model == "ode":
                named = dict(x0=g(T, B, XD), z=g(T, B, ZD), all_initial=g(B, XD + ZD), z_jump=g(B, 1, ZD))
                layers = mlp((3 * (XD + ZD), H, H, H, XD))
                params = [q for wb in layers for q in wb]
                xs = autograd.fused_ode_integrate(method, kernel, layers, t, named["x0"], named["z"], named["all_initial"], event_t=event_t,
                                                  z_jump=named["z_jump"], input_true_x=tf == "x", act=act, **common)
                out = xs.sum()
            else:
                n = XD + ZD + VD + ID
                named = dict(x_init=g(B, XD), z=g(T, B, ZD), v=g(T, B, VD), all_initial=g(B, n), z_jump=g(B, 1, ZD), v_jump=g(B, 1, VD))
                de, ae = mlp((3 * n, H, H, H, XD)), mlp((n + XD + ZD + VD, H, H, H, ID))
                params = [q for wb in de + ae for q in wb]
                xs, is_ = autograd.fused_dae_integrate(method, kernel, de, ae, named["x_init"], t, named["z"], named["v"], torch.zeros((T, B, ID)),
                                                       named["all_initial"], event_t=event_t, z_jump=named["z_jump"], v_jump=named["v_jump"],
                                                       x=torch.zeros((T, B, XD)), input_true_x="x" in tf, input_true_i="i" in tf,
                                                       act=(act, None) if act else None, **common)
                out = xs.sum() + is_.sum()
            n_fwd = len(s.calls)
            out.backward()
        except Exception as e:      # noqa: BLE001 (the type and the text are what the table records)
            return f"{type(e).__name__}: {e}"
    got = [k for k, q in named.items() if q.grad is not None] + (["params"] if all(q.grad is not None for q in params) else [])
    return (f"{type(xs.grad_fn).__name__} | {'; '.join(s.calls[:n_fwd])} | {'; '.join(s.calls[n_fwd:])} | grads {','.join(got)} | "
            f"saved {autograd.last_saved_bytes}")


def body(cases=None):
    """The table's lines behind its first: one `# E<n> = <exception type>: <message>` per distinct refusal, in the order met, then one line
    per case, a refused one with its E<n>."""
    cases = [(case_text(*c), run(*c)) for c in grid()] if cases is None else cases
    refusals = {}
    for _, outcome in cases:
        if " | " not in outcome:
            refusals.setdefault(outcome, f"E{len(refusals) + 1}")
    return [f"# {k} = {text}" for text, k in refusals.items()] + [f"{c} -> {refusals.get(o, o)}" for c, o in cases]


def read_recorded():
    """(the lines behind the first, [(case, outcome with the refusal written out)])"""
    with open(RECORDED) as f:
        table = [ln.rstrip("\n") for ln in f][1:]
    refusals = dict(ln[2:].split(" = ", 1) for ln in table if ln.startswith("# E"))
    cases = [ln.split(" -> ", 1) for ln in table if not ln.startswith("#")]
    return table, [(c, refusals.get(o, o)) for c, o in cases]


def test_every_route_is_the_recorded_one():
    table, cases = read_recorded()
    now = body()
    assert len(cases) == N_CASES and len(table) == len(now)
    bad = [f"table {a}\nnow   {b}" for a, b in zip(table, now) if a != b]
    assert not bad, "\n".join(bad[:20])


def test_the_grid_reaches_every_class_and_both_refusals():
    outcomes = [o for _, o in read_recorded()[1]]
    reached = {o.split(" | ")[0] for o in outcomes if " | " in o}
    assert reached == {c + "Backward" for c in CLASSES}
    assert all(hasattr(autograd, c) for c in CLASSES)
    assert {o.split(":")[0] for o in outcomes if " | " not in o} == {"UnsupportedShapeError", "ValueError"}
    assert fused.ode_integrate is REAL["ode_integrate"]          # the stand-ins are gone


def record(commit):
    out = body()
    with open(RECORDED, "w") as f:
        f.write(f"# tests/test_autograd_routes_host.py --record, from py_psnode_amd at commit {commit}\n")
        f.write("\n".join(out) + "\n")
    print(f"{len(out)} lines -> {RECORDED} ({os.path.getsize(RECORDED)} bytes)")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
