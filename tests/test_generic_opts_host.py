"""`fused.GenericOpts` -- the one value that routes activation, tableau, sub-steps and externals on the Python side -- against a recorded
table, and the gradient-tuple helper of py_psnode_amd/autograd.py (no GPU, no built library: a recording stand-in takes the library's place).

tests/generic_entry_table.txt has one line per case, `<case> -> <outcome>`:
    <stem> <kind> acts=.. tab=.. substeps=.. externals=.. rows=..    the symbol called and, per argument, its ctypes struct, NULL or int
    refuse <name> kernel=.. saved=.. act=.. tab=.. substeps=.. externals=..    "ok", or the option the refusal names
Lines that end in `# rule` are written from the rule below (`rule`), not recorded: the backward calls with dataset rows and every
workspace query sat inside functions that need device tensors.  Every other line in front of the second header was recorded by driving
the helpers `GenericOpts` replaced (`call_entry` / `entry_supported` with the structs their callers hand them; `_act_route_ok`,
`_rk_route_ok`, `sub_route_ok` in the order the forward functions called them) with the same stand-in, at commit 4b90c56.
The lines behind the second header carry per_trajectory (`pt=`), segment and the method "ab2" (`tab=ab2`), which became the families
_pev, _ms and _ab later: `<case> pt=.. segment=..` with the call as above, "0 without a call" (the family "none"), or the exception type and
the options its message names; and `refuse <require_generic | require_plain | no_teacher_forcing> ..` with "ok" or the same.  They are
recorded by driving `GenericOpts` / `call_generic` themselves with the stand-in, at the commit BEFORE a change to them, never from the
changed code:
    git checkout <that commit> -- py_psnode_amd && python tests/test_generic_opts_host.py --record [--commit <its id>]"""
import ctypes
import dataclasses
import inspect
import itertools
import os
import re
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from py_psnode_amd import _lib, autograd, fused  # noqa: E402
from py_psnode_amd.fused import _common  # noqa: E402

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "generic_entry_table.txt")
TANH = fused.Act(_lib.ACT_TANH, name="Tanh")
HEUN = fused.Tableau("Heun", ((), (1.0,)), (0.5, 0.5), 2)
STEMS = {"ode_integrate": (1, _lib.OdeArgsF32), "dae_integrate": (2, _lib.DaeArgsF32), "ode_backward": (1, _lib.OdeBwdArgsF32),
         "dae_backward": (2, None)}          # stem -> (acts, args struct; the DAE backward's depends on the family)
SUB_EXT = ((1, "hold"), (2, "hold"), (1, "linear"), (3, "linear"))
ROWS = ("-", "x", "i", "xi")          # dataset rows of a teacher-forced dae_backward
KERNELS = ("auto", "generic", "mfma", "wide", "tile", "wave")
OPTION = {"act": "activation other than ELU", "tableau": "Runge-Kutta tableau (Heun)", "substeps": "(substeps=2)", "externals": "externals='linear'"}


class Recorder:
    """Stands in for the loaded library: every attribute is a function that notes its name and what each argument is, and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(f"{name}({', '.join(describe(a) for a in args)})")
            return 0
        return fn


def describe(arg) -> str:
    if arg is None:
        return "NULL"
    if isinstance(arg, ctypes.c_int32):
        return f"int32[{arg.value}]"
    obj = getattr(arg, "_obj", None)          # ctypes.byref(obj)
    if obj is None:
        return type(arg).__name__
    if isinstance(obj, _lib.SegmentsF32):
        return f"SegmentsF32[{obj.every}]"
    return f"SubstepsF32[{obj.substeps}]" if isinstance(obj, _lib.SubstepsF32) else type(obj).__name__


def option_rows(stem):
    n = STEMS[stem][0]
    return itertools.product(itertools.product((None, TANH), repeat=n), (None, HEUN), SUB_EXT)


def entry_case(stem, kind, acts, tab, substeps, externals, rows="-") -> str:
    return (f"{stem} {kind} acts={','.join('Tanh' if a else '-' for a in acts)} tab={tab.name if tab else '-'} substeps={substeps} "
            f"externals={externals} rows={rows}")


def refuse_case(name, kernel, saved, act, tab, substeps, externals) -> str:
    return f"refuse {name} kernel={kernel} saved={int(saved)} act={int(act)} tab={int(tab)} substeps={substeps} externals={externals}"


def named_option(message: str) -> str:
    hits = [k for k, text in OPTION.items() if text in message]
    assert len(hits) == 1, message
    return hits[0]


def rule(stem, kind, acts, tab, substeps, externals, rows="-") -> str:
    """The outcome of a case as the family rule states it, written out independently of the package."""
    fam = "lin" if externals == "linear" else "sub" if substeps > 1 else "rk" if tab else "act" if any(acts) else "plain"
    if rows != "-":
        if fam == "act":
            return "AssertionError"          # dataset rows next to a non-ELU act: no entry point takes both without a tableau or sub-steps
        fam = "tf" if fam == "plain" else fam
    args = STEMS[stem][1] or (_lib.DaeBwdTfArgsF32 if fam in ("tf", "rk", "sub", "lin") else _lib.DaeBwdArgsF32)
    a = ["ActF32" if q else "NULL" for q in acts]
    more = {"plain": [], "tf": [], "act": a, "rk": a + ["RkTableauF32"]}.get(fam, a + ["RkTableauF32" if tab else "NULL", f"SubstepsF32[{substeps}]"])
    if kind == "workspace_bytes" and (stem == "ode_backward" or fam in ("plain", "act")):
        fam, more = "plain", []          # the plain query answers for these
    name = f"psnode_{stem}_{kind}" if fam == "plain" else f"psnode_{stem}_{fam}_{kind}"
    return f"{name}({', '.join([args.__name__] + more + (['int'] * 3 if kind == 'f32' else []))})"


def rule_cases():
    """The cases no CPU run of the helpers before the change reaches: dataset rows, workspace queries."""
    for stem in ("ode_backward", "dae_backward"):
        for acts, tab, (n, ext) in option_rows(stem):
            for rows in (ROWS if stem == "dae_backward" else ROWS[:1]):
                for kind in ("f32", "supported", "workspace_bytes"):
                    if rows != "-" or kind == "workspace_bytes":
                        yield (stem, kind, acts, tab, n, ext, rows)


def read_recorded():
    table, ruled = {}, set()
    with open(RECORDED) as f:
        for line in f:
            line = line.rstrip("\n")
            if line and not line.startswith("#"):
                case, outcome = line.split(" -> ")
                if outcome.endswith("  # rule"):
                    outcome = outcome[:-len("  # rule")]
                    ruled.add(case)
                table[case] = outcome
    return table, ruled


def now(stem, kind, acts, tab, substeps, externals, rows="-") -> str:
    lib = Recorder()
    opts = _common.GenericOpts.of(tab if tab else "rk4", acts, substeps, externals)
    try:
        args = STEMS[stem][1]() if STEMS[stem][1] else opts.dae_backward_args(rows != "-")
        value, name = _common.call_generic(lib, stem, kind, args, opts, *((1, 2, 3) if kind == "f32" else ()))
    except AssertionError:
        return "AssertionError"
    assert value == 0 and len(lib.calls) == 1 and lib.calls[0].startswith(name + "("), (name, lib.calls)
    return lib.calls[0]


# ---- 1. the entry table
def test_every_entry_is_the_recorded_one():
    table, ruled = read_recorded()
    cases = [(stem, kind, acts, tab, n, ext, "-") for stem in STEMS for kind in ("f32", "supported") for acts, tab, (n, ext) in option_rows(stem)]
    assert len(cases) == 2 * 96 and not ruled & {entry_case(*c) for c in cases}          # recorded, each of them
    for kind in ("f32", "supported"):          # 72 distinct symbol-and-argument-type patterns over the 96 option rows (96 with the sub-step counts)
        got = {table[entry_case(*c)] for c in cases if c[1] == kind}
        assert len(got) == 96 and len({re.sub(r"\[\d+\]", "", q) for q in got}) == 72
    extra = list(rule_cases())
    assert {entry_case(*c) for c in extra} == {c for c in ruled if not c.startswith("refuse")}
    bad = [f"{entry_case(*c)}\n    table {table[entry_case(*c)]}\n    now   {now(*c)}" for c in cases + extra if now(*c) != table[entry_case(*c)]]
    assert not bad, "\n".join(bad[:40])
    assert all(rule(*c) == table[entry_case(*c)] for c in cases + extra)          # the rule agrees with what was recorded, too


def test_the_c_arguments_stay_alive_and_carry_their_values():
    opts = _common.GenericOpts.of(HEUN, (TANH, None), 3, "linear")
    a_de, a_ae, tab, sub = opts.c_args()
    assert a_ae is None and a_de._obj.kind == _lib.ACT_TANH and tab._obj.stages == 2 and sub._obj.substeps == 3 and not sub._obj.x_sub
    assert (opts.family, opts.method_id, opts.stages) == ("lin", _lib.EULER, 2)
    assert _common.GenericOpts.of("rk4", (None,)).c_args() == [] and _common.GenericOpts.of("rk4", (None,)).family == "plain"
    with pytest.raises(AssertionError):
        _common.call_generic(Recorder(), "ode_integrate", "workspace_bytes", _lib.OdeArgsF32(), _common.GenericOpts.of("rk4", (None,)))


# ---- 2. the refusals
def refused(name, kernel, saved, act, tab, substeps, externals, tf=False):
    """None if `require_generic` lets the call through, else the exception."""
    opts = _common.GenericOpts.of(HEUN if tab else "rk4", (TANH if act else None,) * (2 if name.startswith("dae") else 1), substeps, externals)
    try:
        opts.require_generic(name, kernel, saved, teacher_forced=tf)
    except Exception as e:          # noqa: BLE001 (the type is what the test is about)
        return e
    return None


def test_require_generic_refuses_what_was_refused():
    table, ruled = read_recorded()
    n_raise = 0
    for name, kernel, saved, act, tab, substeps, externals, tf in itertools.product(
            STEMS, KERNELS, (False, True), (False, True), (False, True), (1, 2), ("hold", "linear"), (False, True)):
        if tf and name != "ode_backward":
            continue
        offending = [k for k, on in (("act", act), ("tableau", tab), ("substeps", substeps > 1), ("externals", externals == "linear")) if on]
        want = bool(offending) and (kernel not in ("auto", "generic") or saved)
        if tf and act:          # a teacher-forced ode_backward has no form for a non-ELU act, whatever else the call asks
            want, offending = True, offending if kernel not in ("auto", "generic") or saved else ["act"]
        e = refused(name, kernel, saved, act, tab, substeps, externals, tf)
        case = refuse_case(name, kernel, saved, act, tab, substeps, externals)
        assert (e is not None) == want, case
        if e is not None:
            n_raise += 1
            assert type(e) is _lib.UnsupportedShapeError and str(e).startswith(name + ": "), (case, e)
            assert named_option(str(e)) == offending[0], (case, e)          # the first in the order act, tableau, sub-steps, externals
        if name.endswith("integrate"):
            assert case not in ruled and table[case] == (named_option(str(e)) if e is not None else "ok"), (case, e)
    # 15 option sets x 10 (kernel, saved) pairs per name and once more for the teacher-forced ode_backward, + its 2 x 8 calls with an act on 'auto' / 'generic'
    assert n_raise == 5 * 15 * 10 + 2 * 8


def test_require_plain_and_the_constructor():
    of = _common.GenericOpts.of
    assert of("rk4", (None,)).require_plain("x") == (_lib.RK4_38, 4) and of("midpoint", (None, None)).require_plain("x") == (_lib.MIDPOINT, 2)
    for kw, word in ((dict(substeps=2), "substeps"), (dict(externals="linear"), "externals"), (dict(method=HEUN), "tableau")):
        with pytest.raises(_lib.UnsupportedShapeError, match=word):
            of(kw.pop("method", "rk4"), (None,), **kw).require_plain("a specialised entry")
    with pytest.raises(_lib.UnsupportedShapeError, match="substeps"):          # the order of complaint: sub-steps, externals, tableau
        of(HEUN, (None,), 2, "linear").require_plain("x")
    with pytest.raises(_lib.UnsupportedShapeError, match="externals"):
        of(HEUN, (None,), 1, "linear").require_plain("x")
    with pytest.raises(ValueError, match="externals must be one of"):
        of("rk4", (None,), 1, "cubic")
    for bad in (0, -1, 1025, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="substeps must be an int in 1..1024"):
            of("rk4", (None,), bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        of("rk4", (None,)).substeps = 2


# ---- 3. the gradient tuple
GRADS = {"_FusedOde": ("x0", "z", "all_initial", "z_jump"), "_FusedOdeSub": ("x0", "z", "all_initial", "z_jump"),
         "_FusedOdeLin": ("x0", "z", "all_initial", "z_jump"),
         "_FusedDae": ("x_init", "z", "v", "all_initial", "z_jump", "v_jump"), "_FusedDaeTeacherForced": ("x_init", "z", "v", "all_initial", "z_jump", "v_jump"),
         "_FusedDaeSub": ("x_init", "z", "v", "all_initial", "z_jump", "v_jump"), "_FusedDaeLin": ("x_init", "z", "v", "all_initial", "z_jump", "v_jump")}


@pytest.mark.parametrize("cls_name", sorted(GRADS))
def test_gradients_land_on_the_inputs_they_are_named_for(cls_name):
    cls = getattr(autograd, cls_name)
    names = autograd._arg_names(cls)
    sig = list(inspect.signature(cls.forward).parameters.values())
    assert sig[0].name == "ctx" and sig[-1].kind is inspect.Parameter.VAR_POSITIONAL and names == tuple(p.name for p in sig[1:-1])
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig[1:-1]) and set(GRADS[cls_name]) <= set(names)
    params = [object() for _ in range(6)]
    grads = {name: object() for name in GRADS[cls_name]}
    n = len(names) + len(params)
    every = types.SimpleNamespace(needs_input_grad=(True,) * n)
    out = autograd._grad_tuple(every, cls, grads, params)
    assert len(out) == n and list(out[len(names):]) == params
    for k, name in enumerate(names):
        assert out[k] is grads.get(name), (k, name)          # its sentinel, None where none was stated
        assert autograd._needs(every, cls, name)
    for one in range(len(names)):
        ctx = types.SimpleNamespace(needs_input_grad=tuple(k == one for k in range(n)))
        out = autograd._grad_tuple(ctx, cls, grads, params)
        assert len(out) == n and list(out[len(names):]) == params
        for k, name in enumerate(names):
            assert out[k] is (grads.get(name) if k == one else None), (one, k, name)
            assert autograd._needs(ctx, cls, name) == (k == one)
    with pytest.raises(KeyError):
        autograd._grad_tuple(every, cls, {"no_such_input": object()}, params)


def test_saved_tensors_unpack_by_name():
    a, b, c, p, q = (object() for _ in range(5))
    ctx = types.SimpleNamespace()
    packed = autograd._pack(ctx, (a, b), dict(z_jump=None, rows=(c, None), x_true=None), (p, q))
    assert packed == (a, b, c, p, q)
    ctx.saved_tensors = packed
    fixed, opt, params = autograd._unpack(ctx, 2)
    assert fixed == (a, b) and opt == dict(z_jump=None, rows=(c, None), x_true=None) and tuple(params) == (p, q)
    assert autograd._layers((a, b, c, p), 1) == ([(a, b)], [(c, p)]) and autograd._layers((a, b, c, p)) == [(a, b), (c, p)]


# ---- 4. per-trajectory events, segments and "ab2": the rows added to the table when those options had become three families
AB2 = "ab2"
NAMED = {"act": "activation other than ELU", "tableau": "Runge-Kutta tableau", "substeps": "substeps", "externals": "externals='linear'",
         "per_trajectory": "per_trajectory=True", "segment": "segment=", "ab2": "Adams-Bashforth"}
EXT_HEADER = "# the rows of per_trajectory, segment and the method 'ab2'"
EXT_KINDS = {"ode_integrate": ("f32", "supported"), "dae_integrate": ("f32", "supported"), "ode_backward": ("f32", "supported", "workspace_bytes"),
             "dae_backward": ("f32", "supported", "workspace_bytes")}


def named_options(e) -> str:
    """The exception's type and every option its message names in front of the values it got, in the order of NAMED."""
    return f"{type(e).__name__} {'+'.join(k for k, text in NAMED.items() if text in str(e).split('got ')[0])}"


def extended_rows(stem):
    """option_rows x the method 'ab2' x per_trajectory x segment, without the rows option_rows has."""
    n = STEMS[stem][0]
    for acts, method, (sub, ext), pt, seg in itertools.product(itertools.product((None, TANH), repeat=n), ("rk4", HEUN, AB2), SUB_EXT, (False, True),
                                                               (None, 2)):
        if method == AB2 or pt or seg is not None:
            yield acts, method, sub, ext, pt, seg


def _method_name(method) -> str:
    return "-" if method == "rk4" else str(method)


def extended_case(stem, kind, acts, method, substeps, externals, pt, seg) -> str:
    return (f"{stem} {kind} acts={','.join('Tanh' if a else '-' for a in acts)} tab={_method_name(method)} substeps={substeps} "
            f"externals={externals} rows=- pt={int(pt)} segment={seg or '-'}")


def extended_now(stem, kind, acts, method, substeps, externals, pt, seg) -> str:
    """The call the case makes, "<value> without a call" (the family "none"), or the exception: what `__post_init__` or `call_generic` raise."""
    lib = Recorder()
    try:
        opts = _common.GenericOpts.of(method, acts, substeps, externals, pt, seg)
        args = STEMS[stem][1]() if STEMS[stem][1] else opts.dae_backward_args(False)
        value, _ = _common.call_generic(lib, stem, kind, args, opts, *((1, 2, 3) if kind == "f32" else ()))
    except (ValueError, AssertionError) as e:
        return named_options(e) if isinstance(e, ValueError) else "AssertionError"
    assert value == 0 and len(lib.calls) <= 1, lib.calls
    return lib.calls[0] if lib.calls else f"{value} without a call"


def refusal_cases():
    """(case, thunk): require_generic over kernel, saved rows and teacher forcing, require_plain and no_teacher_forcing, for every valid
    set of the three options (and interpolated externals, which two of them refuse) that has at least one of them."""
    sets = [(m, pt, seg, ext) for m, pt, seg, ext in itertools.product(("rk4", AB2), (False, True), (None, 2), ("hold", "linear"))
            if (m == AB2 and seg is None and ext == "hold") or (m != AB2 and (pt or seg is not None))]
    for m, pt, seg, ext in sets:
        tag = f"method={m} pt={int(pt)} segment={seg or '-'} externals={ext}"
        for name, kernel, saved, tf in itertools.product(STEMS, ("auto", "mfma"), (False, True), (False, True)):
            yield (f"refuse require_generic {name} kernel={kernel} saved={int(saved)} tf={int(tf)} {tag}",
                   lambda o=(m, (None,) * STEMS[name][0], 1, ext, pt, seg), a=(name, kernel, saved, tf):
                   _common.GenericOpts.of(*o).require_generic(a[0], a[1], a[2], teacher_forced=a[3]))
        o = (m, (None,), 1, ext, pt, seg)
        yield f"refuse require_plain {tag}", lambda o=o: _common.GenericOpts.of(*o).require_plain("x")
        for tf in (False, True):
            yield f"refuse no_teacher_forcing tf={int(tf)} {tag}", lambda o=o, tf=tf: _common.GenericOpts.of(*o).no_teacher_forcing("x", tf)


def refusal_now(thunk) -> str:
    try:
        thunk()
    except (ValueError, _lib.UnsupportedShapeError) as e:
        return named_options(e)
    return "ok"


def test_every_extended_entry_and_refusal_is_the_recorded_one():
    table, ruled = read_recorded()
    cases = [(extended_case(stem, kind, *row), (stem, kind) + row) for stem in STEMS for kind in EXT_KINDS[stem] for row in extended_rows(stem)]
    assert len(cases) == (2 + 2 + 3 + 3) * 80 + (2 + 3) * 80 and not ruled & {c for c, _ in cases}          # 80 rows per act tuple: 2 + 2 * 2 of them
    got = {table[c] for c, _ in cases}
    for fam in ("pev", "ab", "ms"):          # each family is reached from every stem, and so are "none" and the constructor's refusals
        assert all(any(q.startswith(f"psnode_{stem}_{fam}_") for q in got) for stem in STEMS), fam
    assert {"0 without a call", "AssertionError", "ValueError segment+ab2", "ValueError substeps+externals+ab2"} <= got
    bad = [f"{c}\n    table {table[c]}\n    now   {extended_now(*a)}" for c, a in cases if extended_now(*a) != table[c]]
    refusals = list(refusal_cases())
    assert len(refusals) == 8 * (4 * 8 + 1 + 2) and {table[c] for c, _ in refusals} >= {"ok", "ValueError segment", "ValueError ab2"}
    bad += [f"{c}\n    table {table[c]}\n    now   {refusal_now(t)}" for c, t in refusals if refusal_now(t) != table[c]]
    assert not bad, "\n".join(bad[:40])
    assert len(table) == 914 - 2 + len(cases) + len(refusals)          # and the file holds nothing else


# ---- the recorder of section 4 (run at the commit before the change).  The lines in front of EXT_HEADER were recorded at commit 4b90c56 from
# helpers that `GenericOpts` has since replaced; they are kept as they are.
def record(commit):
    with open(RECORDED) as f:
        kept = f.read().split(EXT_HEADER)[0]
    lines = [f"{extended_case(stem, kind, *row)} -> {extended_now(stem, kind, *row)}" for stem in STEMS for kind in EXT_KINDS[stem]
             for row in extended_rows(stem)]
    lines += [f"{case} -> {refusal_now(thunk)}" for case, thunk in refusal_cases()]
    with open(RECORDED, "w") as f:
        f.write(kept + f"{EXT_HEADER}: tests/test_generic_opts_host.py --record, from py_psnode_amd at commit {commit}\n")
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {RECORDED} ({os.path.getsize(RECORDED)} bytes)")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
