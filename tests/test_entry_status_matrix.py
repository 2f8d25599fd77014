"""The status of every K0 / K5 entry point of the C ABI over a grid of argument defects, against a recorded file (no GPU, nothing launches).

The 62 exported functions of the _act, _tf, _rk, _sub, _lin, _pev, _ab and _ms families
(psnode_{ode,dae}_{integrate,backward}_{act,rk,sub,lin,pev,ab,ms}_{supported,f32}, psnode_dae_backward_{tf,rk,sub,lin}_workspace_bytes,
psnode_dae_backward_tf_{supported,f32}) and the four plain _f32 entry points they forward to are called with valid dims-only args spoiled
by no defect, by each single defect and by each pair of defects; with no data pointer set or with every required one set to a dummy; and,
for the families that take them, with every act x tableau x sub-steps x segments x per_trajectory x workspace combination.  The defect
"ev" (event_idx set, the jumps it makes required set with the other pointers) is recorded for the _pev, _ab and _ms families alone.  The
order in which an entry point checks its arguments is behaviour (py_psnode_amd/_lib.py maps statuses to exception types): a call that is
wrong in two ways has to go on answering with the status it answered with.

A row is one (entry point, defect set, pointers) with one character per remaining grid column:
    _f32               the digit n of status -n (1 NULL, 2 DIMS, 3 METHOD, 4 WORKSPACE, 5 UNSUPPORTED, 6 HIP); never 0 -- no case launches
    _supported         the value returned
    _workspace_bytes   0, or + for any other size
Columns run act-major (groups parted by a blank), then tableau, sub-steps, segments (_ms), per_trajectory (the _ab call), workspace; a
family has the columns of the arguments it takes.
Rows of two defects carry a thinned act x sub-steps x segments grid (PAIR_ACTS, PAIR_SUBS, PAIR_SEGS), rows of none or one the whole grid.
tests/entry_status_matrix.txt holds the 10584 rows grouped: per entry point, each distinct row once, followed by the cases (defect set and
pointers, in the short codes of CODES) that give it.  A case whose status changes moves to another group in the file's diff, and the
failing test names it in full.

The file is recorded from a build of the commit BEFORE a change to the entry points, never from the changed code:
    PSNODE_LIB_PATH=<that build's libpsnode_hip.so> python tests/test_entry_status_matrix.py --record [--commit <its id>]"""
import ctypes
import functools
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from py_psnode_amd import _lib  # noqa: E402

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "entry_status_matrix.txt")
R = ctypes.byref
DUMMY = 256          # a non-NULL, 256-byte aligned address that nothing on the host reads through
XD, ZD, VD, ID, HIDDEN, T, B = 8, 2, 2, 2, 64, 12, 5          # the dims-only args of tests/test_substeps_host.py

# ---- the grid
DEFECTS = ("method", "T0", "T1", "xdim0", "indim", "wide", "h512", "generic", "mfma", "wave", "save", "savex", "tf", "ev")
EXCLUSIVE = (("T0", "T1"), ("generic", "mfma"), ("generic", "wave"), ("mfma", "wave"))      # pairs that set one field twice
EV_FAMILIES = ("pev", "ab", "ms")          # "ev" (event_idx set) is recorded for these alone: _pev needs the table, _ab reads it as shared or [T-1, B]
SINGLE_ONLY = ("savex",)          # save_xstage / saved_xstage alone (the families differ in which pointers they look at): in no pair, for the file's size
ACTS = ("null", "elu1", "tanh", "silu", "kind17", "elu-1")
TABS = ("null", "heun", "stages5")
SUBS = ("null", "0", "1", "2", "2+x_sub")
SEGS = ("null", "0", "2", "2+x_true")          # _ms: T - 1 > 2, so a backward call restarts and needs x_true
PTS = ("0", "1")          # _ab's call: per_trajectory
WORKSPACES = ((None, 0), (DUMMY, 16))          # never a valid one: the last status a call can reach is PSNODE_ERR_WORKSPACE
PAIR_ACTS = ("null", "tanh", "kind17")
PAIR_SUBS = ("null", "1", "2", "2+x_sub")
PAIR_SEGS = ("null", "2", "2+x_true")
# stem -> (args kind, act arity, the families next to the plain entry point); "dae_backward_base": the entry points of the DAE backward that
# take psnode_dae_bwd_args_f32 (no flags: the "tf" defect does not exist for them)
STEMS = {
    "ode_integrate": ("ode_fwd", 1, ("plain", "act", "rk", "sub", "lin", "pev", "ab", "ms")),
    "dae_integrate": ("dae_fwd", 2, ("plain", "act", "rk", "sub", "lin", "pev", "ab", "ms")),
    "ode_backward": ("ode_bwd", 1, ("plain", "act", "rk", "sub", "lin", "pev", "ab", "ms")),
    "dae_backward_base": ("dae_bwd", 2, ("plain", "act")),
    "dae_backward": ("dae_bwd", 2, ("tf", "rk", "sub", "lin", "pev", "ab", "ms")),
}
FAMILY_COLUMNS = {"plain": (), "tf": (), "act": ("act",), "rk": ("act", "tab"), "sub": ("act", "tab", "sub"), "lin": ("act", "tab", "sub"),
                  "pev": ("act", "tab", "sub"), "ab": ("act", "pt"), "ms": ("act", "tab", "sub", "seg")}          # pt: an int of the _f32 call alone


def _act(name):
    if name == "null":
        return None
    a = _lib.ActF32()
    a.kind, a.alpha = {"elu1": (_lib.ACT_ELU, 1.0), "tanh": (_lib.ACT_TANH, 0.0), "silu": (_lib.ACT_SILU, 0.0), "kind17": (17, 0.0),
                       "elu-1": (_lib.ACT_ELU, -1.0)}[name]
    return a


def _tab(name):
    if name == "null":
        return None
    t = _lib.RkTableauF32()          # Heun: a[1][0] = 1, b = (1/2, 1/2)
    t.stages = 2 if name == "heun" else 5
    t.a[1][0] = 1.0
    t.b[0] = t.b[1] = 0.5
    return t


def _sub(name):
    if name == "null":
        return None
    s = _lib.SubstepsF32()
    s.substeps, s.x_sub = int(name[0]), DUMMY if name.endswith("x_sub") else None
    return s


def _seg(name):
    if name == "null":
        return None
    g = _lib.SegmentsF32()
    g.every, g.x_true = int(name[0]), DUMMY if name.endswith("x_true") else None
    return g


def _mlp(m, in_dim, out, ptrs):
    m.n_layers, m.in_dim = 4, in_dim
    for l, o in enumerate((HIDDEN, HIDDEN, HIDDEN, out)):
        m.out_dim[l] = o
        if ptrs:
            m.weight[l] = m.bias[l] = DUMMY


def _args(kind, defects, ptrs):
    """Valid args of `kind` with every required data pointer NULL or DUMMY (save_* / saved_* and event_idx stay NULL), then the defects."""
    dae = kind.startswith("dae")
    a = {"ode_fwd": _lib.OdeArgsF32, "dae_fwd": _lib.DaeArgsF32, "ode_bwd": _lib.OdeBwdArgsF32, "dae_bwd": _lib.DaeBwdTfArgsF32}[kind]()
    b = a.base if kind == "dae_bwd" else a
    b.method, b.kernel, b.x_dim, b.z_dim, b.T, b.B = _lib.RK4_38, _lib.KERNEL_AUTO, XD, ZD, T, B
    n = XD + ZD
    if dae:
        b.v_dim, b.i_dim = VD, ID
        n += VD + ID
        _mlp(b.ae, n + XD + ZD + VD, ID, ptrs)
    _mlp(b.de, 3 * n, XD, ptrs)
    if ptrs:
        need = {"ode_fwd": ("all_initial", "x_out"), "dae_fwd": ("x_init", "all_initial", "x_out", "i_out"),
                "ode_bwd": ("all_initial", "xs", "grad_xs", "grad_x0", "grad_all_initial", "grad_params"),
                "dae_bwd": ("all_initial", "xs", "is_", "grad_xs", "grad_x_init", "grad_all_initial", "grad_params_de", "grad_params_ae")}[kind]
        for f in need:
            setattr(b, f, DUMMY)
        for v in {"ode_fwd": "txz", "dae_fwd": "txzvi", "ode_bwd": "tz", "dae_bwd": "tzv"}[kind]:
            getattr(b, v).ptr = DUMMY
        if kind == "dae_bwd":
            a.x_true = a.i_true = DUMMY
    fwd = kind.endswith("fwd")
    for d in defects:
        if d == "method":
            b.method = 77
        elif d in ("T0", "T1"):
            b.T = int(d[1])
        elif d == "xdim0":
            b.x_dim = 0
        elif d == "indim":
            b.de.in_dim += 1
        elif d == "wide":
            b.de.out_dim[1] = _lib.MAX_WIDTH + 1
        elif d == "h512":
            for m in (b.de, b.ae) if dae else (b.de,):
                m.out_dim[0] = m.out_dim[1] = m.out_dim[2] = 512
        elif d in ("generic", "mfma", "wave"):
            b.kernel = {"generic": _lib.KERNEL_GENERIC, "mfma": _lib.KERNEL_MFMA, "wave": _lib.KERNEL_MFMA_WAVE}[d]
        elif d in ("save", "savex"):          # save: every side-output pointer; savex: the stage rows alone (an inconsistent pair)
            names = ("act", "xstage") + (("ae_act", "ev_act", "ev_i") if dae else ())
            for f in names if d == "save" else ("xstage",):
                setattr(b, ("save_" if fwd else "saved_") + f, DUMMY)
        elif d == "tf":
            a.flags = 3 if dae else 1
        elif d == "ev":          # the table, and with `ptrs` the jumps it makes required
            b.event_idx = DUMMY
            if ptrs:
                b.z_jump = DUMMY
                if dae:
                    b.v_jump = DUMMY
    return a


def defect_sets(stem):
    ds = [d for d in DEFECTS if not (d == "tf" and stem == "dae_backward_base")]
    pairs = [p for p in itertools.combinations([d for d in ds if d not in SINGLE_ONLY], 2) if p not in EXCLUSIVE]
    return [()] + [(d,) for d in ds] + pairs


def functions(stem):
    """(exported name, family, what it returns) of every function of the stem."""
    name = stem.replace("_base", "")
    out = []
    for fam in STEMS[stem][2]:
        if fam == "plain":
            out.append((f"psnode_{name}_f32", fam, "f32"))
            continue
        out.append((f"psnode_{name}_{fam}_supported", fam, "supported"))
        if name == "dae_backward" and fam in ("tf", "rk", "sub", "lin"):
            out.append((f"psnode_{name}_{fam}_workspace_bytes", fam, "workspace_bytes"))
        out.append((f"psnode_{name}_{fam}_f32", fam, "f32"))
    return out


def _columns(fam, thin):
    cols = FAMILY_COLUMNS[fam]
    acts = (PAIR_ACTS if thin else ACTS) if "act" in cols else ("null",)
    tabs = TABS if "tab" in cols else ("null",)
    subs = (PAIR_SUBS if thin else SUBS) if "sub" in cols else ("null",)
    segs = (PAIR_SEGS if thin else SEGS) if "seg" in cols else ("null",)
    return cols, acts, tabs, subs, segs


def _row(lib, stem, fn_name, fam, what, a, thin, extras):
    fn = getattr(lib, fn_name)
    n_act = STEMS[stem][1]
    arg0 = R(a.base) if stem == "dae_backward_base" else R(a)
    cols, acts, tabs, subs, segs = _columns(fam, thin)
    pts = PTS if "pt" in cols and what == "f32" else ("0",)
    groups = []
    for act in acts:
        chars = []
        for tab in tabs:
            for sub, seg, pt in itertools.product(subs, segs, pts):
                extra = ([extras["act", act]] * n_act if "act" in cols else []) + ([extras["tab", tab]] if "tab" in cols else []) + \
                        ([extras["sub", sub]] if "sub" in cols else []) + ([extras["seg", seg]] if "seg" in cols else []) + \
                        ([int(pt)] if "pt" in cols and what == "f32" else [])
                if what == "f32":
                    for ws, nbytes in WORKSPACES:
                        rc = fn(arg0, *extra, ws, nbytes, None)
                        chars.append(str(-rc) if -6 <= rc <= 0 else "?")
                elif what == "supported":
                    v = fn(arg0, *extra)
                    chars.append(str(v) if 0 <= v <= 9 else "?")
                else:
                    chars.append("+" if fn(arg0, *extra) else "0")
        groups.append("".join(chars))
    return " ".join(groups)


@functools.lru_cache(maxsize=None)
def matrix():
    """{row label: row} over the whole grid, computed once."""
    lib = _lib.load()
    extras = {}
    for kind, names, make in (("act", ACTS, _act), ("tab", TABS, _tab), ("sub", SUBS, _sub), ("seg", SEGS, _seg)):
        for nm in names:
            obj = make(nm)
            extras[kind, nm] = (obj, R(obj) if obj is not None else None)
    refs = {k: v[1] for k, v in extras.items()}
    rows = {}
    for stem, (kind, _, _) in STEMS.items():
        for ds in defect_sets(stem):
            for ptrs in (False, True):
                a = _args(kind, ds, ptrs)
                for fn_name, fam, what in functions(stem):
                    if "ev" in ds and fam not in EV_FAMILIES:
                        continue
                    label = f"{fn_name[len('psnode_'):]} {'+'.join(ds) or 'none'} {'ptrs' if ptrs else 'null'}"
                    rows[label] = _row(lib, stem, fn_name, fam, what, a, len(ds) == 2, refs)
    return rows


# ---- the recorded file: per entry point, one group per distinct row -- the row, then every (defect set, pointers) that gives it
CODES = {"method": "M", "T0": "T0", "T1": "T1", "xdim0": "X", "indim": "I", "wide": "W", "h512": "H", "generic": "g", "mfma": "f", "wave": "v",
         "save": "S", "savex": "Sx", "tf": "F", "ev": "E"}
NAMES = {c: d for d, c in CODES.items()}


def write_recorded(rows, commit):
    by_fn = {}
    for label, row in rows.items():
        fn, ds, ptrs = label.split()
        short = ".".join(CODES[d] for d in ds.split("+")) if ds != "none" else "ok"
        by_fn.setdefault(fn, {}).setdefault(row, []).append(short + ("+" if ptrs == "ptrs" else "-"))
    with open(RECORDED, "w") as f:
        f.write(f"# tests/test_entry_status_matrix.py --record, from the library built at commit {commit}\n")
        f.write(f"# columns: act {ACTS} x tableau {TABS} x sub-steps {SUBS} x workspace (NULL, 16 bytes)\n")
        f.write(f"# _ms: segments {SEGS} between sub-steps and workspace; the _ab call: per_trajectory {PTS} in front of the workspace\n")
        f.write(f"# rows of two defects: act {PAIR_ACTS}, sub-steps {PAIR_SUBS}, segments {PAIR_SEGS}\n")
        f.write("# cases: " + " ".join(f"{c}={d}" for d, c in CODES.items()) + " ok=none, joined by '.'; then + every required pointer set, - none\n")
        for fn, groups in by_fn.items():
            f.write(f"== {fn}\n")
            for row, cases in groups.items():
                f.write(f"{row} :\n")
                for k in range(0, len(cases), 24):
                    f.write("    " + " ".join(cases[k:k + 24]) + "\n")


def read_recorded():
    rows, fn, row = {}, None, None
    with open(RECORDED) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("== "):
                fn = line[3:]
            elif line.endswith(" :"):
                row = line[:-2]
            elif line.startswith("    "):
                for case in line.split():
                    ds = "none" if case[:-1] == "ok" else "+".join(NAMES[c] for c in case[:-1].split("."))
                    rows[f"{fn} {ds} {'ptrs' if case[-1] == '+' else 'null'}"] = row
    return rows


def test_grid_covers_every_entry_point_and_launches_nothing():
    names = {fn for stem in STEMS for fn, _, _ in functions(stem)}
    fams = [n for n in _lib.EXPORTS if any(f"_{f}_" in n for f in ("act", "tf", "rk", "sub", "lin", "pev", "ab", "ms")) and ("_integrate_" in n or "_backward_" in n)]
    assert len(fams) == 62 and set(fams) <= names and len(names) == 66
    seen = set()
    for label, row in matrix().items():
        if label.split()[0].endswith("_f32"):
            assert "0" not in row and "?" not in row, label          # PSNODE_OK would have launched
            seen |= set(row) - {" "}
    assert seen == set("12345"), seen          # every error status short of PSNODE_ERR_HIP occurs


def test_every_status_is_the_recorded_one():
    got, want = matrix(), read_recorded()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    bad = [f"{label}\n    recorded {want[label]}\n    now      {got[label]}" for label in want if got[label] != want[label]]
    print(f"{len(want)} rows, {sum(len(r.replace(' ', '')) for r in want.values())} statuses, {len(bad)} rows differ")
    assert not bad, "\n".join(bad[:40])


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    rows = matrix()
    write_recorded(rows, commit)
    print(f"{len(rows)} rows -> {RECORDED} ({os.path.getsize(RECORDED)} bytes)")
