"""Multiple-shooting segments in parallel (solver.segment_parallel), everything that needs no GPU: the value rules of the option, the walk
(which ignores it), the chunk-bound formula against a brute-force partition, what fused.GenericOpts routes and hands the library, and the
statuses of the psnode_*_msp_* entry points with nothing launched (the form of tests/test_entry_status_matrix.py: every pointer NULL or
the constant 256, no workspace, no stream).

The option never changes what is computed: with segment = w a record of T grid points has n_seg = ceil((T - 1) / w) segments; with g
chunks wanted, per_group = ceil(n_seg / min(g, n_seg)) consecutive segments form a time chunk, C = ceil(n_seg / per_group) chunks, chunk c
the steps c per_group w .. min((c + 1) per_group w, T - 1) - 1."""
import ctypes

import pytest
import torch

import capi_args as A
import generic_cases as C
import segment_cases as S
from capi_args import R
from capi_args import sub as _sub
from py_psnode_amd import _lib, autograd, fused, models
from py_psnode_amd import neural_dae as nd

STEMS = ("ode_integrate", "dae_integrate", "ode_backward", "dae_backward")
MSP_EXPORTS = tuple(f"psnode_{s}_msp_{k}" for s in STEMS for k in ("supported", "f32")) + \
    ("psnode_ode_backward_msp_workspace_size", "psnode_dae_backward_msp_workspace_size")
CLASSES = (nd.Euler, nd.Midpoint, nd.RK4, nd.Kutta3, nd.Heun2, nd.RK4Classic)


# ----------------------------------------------------------------------------- 1. the option's values
def test_constructor_value_rules():
    assert nd.RK4(segment=50).segment_parallel is None
    assert nd.RK4(segment=50, segment_parallel="auto").segment_parallel == "auto"
    for cls in CLASSES:
        for g in ("auto", 1, 2, 20, 10 ** 9):
            assert cls(segment=3, segment_parallel=g).segment_parallel == g
        for bad in (True, False, 0, -1, 2.0, "AUTO", "2", (2,)):
            with pytest.raises(ValueError, match="segment_parallel"):
                cls(segment=3, segment_parallel=bad)
        for g in ("auto", 1, 4):          # anything but None needs segment
            with pytest.raises(ValueError, match="segment_parallel"):
                cls(segment_parallel=g)
    with pytest.raises(ValueError, match="segment"):          # AB2 refuses segment already
        nd.AB2(segment=3, segment_parallel="auto")
    with pytest.raises(ValueError, match="segment_parallel"):
        nd.AB2(segment_parallel=2)
    assert nd.AB2().segment_parallel is None


@pytest.mark.parametrize("g", [2, 3, 100, "auto"])
@pytest.mark.parametrize("name,n", [("euler", 1), ("rk4", 2), ("Kutta3", 1)])
def test_the_walk_ignores_the_option(name, n, g):
    """fused='off': the walk with and without the option, bit for bit, ODE and DAE, every w of the cases and T = 8 and 12"""
    for Tn in (8, 12):
        de, t, x, z, ev, zj = S.ode_case(6, 2, (32, 32), Tn=Tn, seed=60)
        case = S.dae_case(5, 2, 3, 2, (32, 32), (24, 24), Tn=Tn, seed=61)
        a0 = torch.cat((x[0], z[0]), -1)
        for w in S.WS + (2,):
            plain = S.solver(name, w, n)
            par = S.SOLVERS[name](substeps=n, segment=w, segment_parallel=g)
            par.fused = "off"
            with torch.no_grad():
                assert torch.equal(C.run_ode(plain, de, t, x, z, a0, ev, zj), C.run_ode(par, de, t, x, z, a0, ev, zj))
                px, pi = C.run_dae(plain, *case)
                qx, qi = C.run_dae(par, *case)
            assert torch.equal(px, qx) and torch.equal(pi, qi)


# ----------------------------------------------------------------------------- 2. the chunk bounds
def test_chunk_bounds_against_a_brute_force_partition():
    """T in 1..40, w in 1..9, g in 1..12: every step lies in exactly one chunk, every chunk start is 0 or a restart point, the chunks are
    consecutive groups of whole segments, all but the last of per_group of them, and there are at most g"""
    for Tn in range(1, 41):
        for w in range(1, 10):
            segs = S.slices(Tn, w)          # [(first grid point, last grid point)] of the segments
            for g in range(1, 13):
                per_group, chunks = fused.segment_chunks(Tn, w, g)
                if Tn == 1:
                    assert (per_group, chunks) == (1, [])
                    continue
                n_seg = len(segs)
                assert n_seg == -(-(Tn - 1) // w) and per_group == -(-n_seg // min(g, n_seg)) and len(chunks) == -(-n_seg // per_group) <= g
                owner = [[c for c, (lo, hi) in enumerate(chunks) if lo <= k < hi] for k in range(Tn - 1)]
                assert all(len(o) == 1 for o in owner), (Tn, w, g)
                for c, (lo, hi) in enumerate(chunks):
                    assert lo < hi <= Tn - 1 and (lo == 0 or lo % w == 0), (Tn, w, g, c)
                    mine = segs[c * per_group:(c + 1) * per_group]          # brute force: the c-th group of per_group segments
                    assert (lo, hi) == (mine[0][0], mine[-1][1]) and (len(mine) == per_group or c == len(chunks) - 1)
                assert chunks[0][0] == 0 and chunks[-1][1] == Tn - 1
                assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    # the issue's examples: T = 12, w = 2 has 6 segments, g = 4 gives 3 chunks of 2; w = 1, g = 3 at T = 8 gives chunks of 3, 3, 1
    assert fused.segment_chunks(12, 2, 4) == (2, [(0, 4), (4, 8), (8, 11)])
    assert fused.segment_chunks(8, 1, 3) == (3, [(0, 3), (3, 6), (6, 7)])
    assert fused.segment_chunks(8, 3, 3) == (1, [(0, 3), (3, 6), (6, 7)])          # the event of step 3 on a chunk start
    assert fused.segment_chunks(8, 3, 100) == fused.segment_chunks(8, 3, 3)        # one segment per chunk


def test_resolution_and_the_auto_heuristic():
    r = fused.resolve_segment_parallel
    assert r(None, 3, 8, 33) is None and r(None, None, 8, 33) is None
    assert r(3, 3, 8, 33) == 1 and r(2, 3, 8, 33) == 2 and r(100, 1, 8, 33) == 1 and r(3, 1, 8, 33) == 3 and r(4, 2, 12, 33) == 2
    for g in (1, 2, 100):          # one chunk: the call without the option
        assert r(g, 7, 8, 33) is None and r(g, 100, 8, 33) is None and r(g, 3, 1, 33) is None and r(g, 1, 2, 33) is None
    assert r(1, 1, 12, 33) is None
    # "auto": g = max(1, CUs // tiles), tiles = ceil(B / 16)
    assert fused.auto_segment_groups(32, 256) == 128 and fused.auto_segment_groups(33, 256) == 85 and fused.auto_segment_groups(4096, 256) == 1
    assert fused.auto_segment_groups(4097, 256) == 1 and fused.auto_segment_groups(1, 256) == 256 and fused.auto_segment_groups(1024, 256) == 4
    assert r("auto", 50, 1001, 32, cus=256) == 1 and r("auto", 50, 1001, 4096, cus=256) is None and r("auto", 50, 1001, 1024, cus=256) == 5
    for bad in (True, 0, -2, 1.5, "all"):
        with pytest.raises(ValueError, match="segment_parallel"):
            r(bad, 3, 8, 33, cus=256)
    with pytest.raises(ValueError, match="segment_parallel"):
        r(2, None, 8, 33)
    # the chunk count a resolved call reports names the same grouping again
    for Tn in (2, 8, 12, 40):
        for w in (1, 2, 3, 7):
            for g in (1, 2, 3, 5, 100):
                pg = r(g, w, Tn, 33)
                o = fused.GenericOpts.of("rk4", (None,), 1, "hold", False, w, pg)
                assert (o.chunks(Tn) is None) == (pg is None)
                if pg is not None:
                    assert o.chunks(Tn) == len(fused.segment_chunks(Tn, w, g)[1]) > 1 and r(o.chunks(Tn), w, Tn, 33) == pg


# ----------------------------------------------------------------------------- 3. GenericOpts
def test_generic_opts_family_and_c_args():
    of = fused.GenericOpts.of
    seq, par = of("rk4", (None,), 2, "hold", False, 7), of("rk4", (None,), 2, "hold", False, 7, 3)
    assert seq.family == "ms" and seq.segment_parallel is None and par.family == "msp" and par.segment_parallel == 3
    assert fused.FAMILIES["msp"].seg and fused.FAMILIES["msp"].par and fused.FAMILIES["msp"].workspace == "own" and not fused.FAMILIES["ms"].par
    assert [f.name for f in fused.GenericOpts.__dataclass_fields__.values() if f.init][-2:] == ["ab", "segment_parallel"]
    rows = torch.zeros(2, 2, 2)
    c, p = seq.c_args(x_true=rows), par.c_args(x_true=rows)
    assert isinstance(c[3]._obj, _lib.SegmentsF32) and isinstance(p[3]._obj, _lib.SegmentGroupsF32)
    assert (p[3]._obj.every, p[3]._obj.per_group, p[3]._obj.x_true) == (7, 3, rows.data_ptr()) and p[2]._obj.substeps == 2 and p[0] is None
    assert not par.c_args()[3]._obj.x_true and of("rk4", (None,), 1, "hold", False, 10 ** 12, 10 ** 12).c_args()[3]._obj.per_group == 0x7fffffff
    # next to what segment has no kernel for, the option changes nothing: "none"
    assert of("rk4", (None,), 1, "linear", False, 3, 2).family == "none" and of("rk4", (None,), 1, "hold", True, 3, 2).family == "none"
    for bad in (True, 0, -1, 2.0, "auto"):
        with pytest.raises(ValueError, match="segment_parallel"):
            of("rk4", (None,), 1, "hold", False, 3, bad)
    with pytest.raises(ValueError, match="segment_parallel"):
        of("rk4", (None,), 1, "hold", False, None, 2)
    with pytest.raises(ValueError, match="segment"):
        of("ab2", (None,), 1, "hold", False, 3, 2)
    with pytest.raises(ValueError, match="segment"):
        par.require_generic("x", "generic", False, teacher_forced=True)
    for kernel, save in (("wave", False), ("mfma", False), ("tile", False), ("wide", False), ("auto", True)):
        with pytest.raises(_lib.UnsupportedShapeError, match="segment=3"):
            of("rk4", (None,), 1, "hold", False, 3, 2).require_generic("x", kernel, save)
    with pytest.raises(_lib.UnsupportedShapeError, match="segment"):
        of("rk4", (None,), 1, "hold", False, 3, 2).require_plain("a specialised entry")
    assert autograd._FusedOdeMsp.__name__ == "_FusedOdeMsp" and autograd._FusedDaeMsp.__name__ == "_FusedDaeMsp"
    assert issubclass(autograd._FusedOdeMsp, autograd._FusedOdeGeneric) and issubclass(autograd._FusedDaeMsp, autograd._FusedDaeGeneric)


def test_python_predicates_and_refusals():
    layers = A.hip_layers
    ode01 = layers(models.DE_Func(10, (64, 64, 64), 8).x_dot)
    n = 8 + 2 + 2 + 2
    de = layers(models.DAE_DE_Func(n, (64, 64, 64), 8).x_dot)
    ae = layers(models.AE_Func(n + 8 + 2 + 2, (64, 64, 64), 2).i_calculator)
    for method in ("euler", "rk4", nd.Kutta3().method):
        for g in (1, 2, 20):
            kw = dict(substeps=2, segment=3, segment_parallel=g)
            assert autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, **kw)
            assert autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, **kw)
            assert fused.ode_backward_supported(method, ode01, 8, 2, "generic", **kw)
            assert fused.dae_backward_supported(method, de, ae, 8, 2, 2, 2, kernel="generic", **kw)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, input_true_x=True, **kw)
            assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, input_true_i=True, **kw)
            assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, externals="linear", **kw)
            assert not autograd.dae_training_supported(method, de, ae, 8, 2, 2, 2, 50, 33, per_trajectory=True, **kw)
            for kernel in ("wave", "tile", "mfma", "wide"):
                assert not autograd.ode_training_supported(method, ode01, 8, 2, 50, 33, kernel=kernel, **kw)
                assert not fused.ode_backward_supported(method, ode01, 8, 2, kernel, **kw)
    for fn, args in ((fused.ode_backward_supported, ("rk4", ode01, 8, 2)), (fused.dae_backward_supported, ("rk4", de, ae, 8, 2, 2, 2))):
        with pytest.raises(ValueError, match="segment_parallel"):
            fn(*args, segment_parallel=2)
        with pytest.raises(ValueError, match="segment_parallel"):
            fn(*args, segment=3, segment_parallel=True)
    with pytest.raises(ValueError, match="segment_parallel"):
        autograd.ode_training_supported("rk4", ode01, 8, 2, 50, 33, segment_parallel=2)


def test_the_time_chunked_launches_refuse_the_option():
    from py_psnode_amd import sharded
    for kw in (dict(segment=3, segment_parallel=2), dict(segment_parallel="auto")):
        for what in ("integrate_ode_pipelined", "integrate_dae_pipelined"):
            with pytest.raises(ValueError, match="segment"):
                sharded._no_segments(what, kw)


# ----------------------------------------------------------------------------- 4. the C ABI
DIMS = dict(method=_lib.RK4_38, T=12, B=5)
_ode_args, _dae_args, _ode_bwd_args, _dae_bwd_args = A.bound(**DIMS)
ENTRIES = (("ode_integrate", _ode_args, 1), ("dae_integrate", _dae_args, 2), ("ode_backward", _ode_bwd_args, 1), ("dae_backward", _dae_bwd_args, 2))


def _grp(every, per_group, x_true=None):
    g = _lib.SegmentGroupsF32()
    g.every, g.x_true, g.per_group = every, x_true, per_group
    return g


def _tail(n_act, tab, sub, grp, act):
    return [act] * n_act + [tab, R(sub) if sub is not None else None, R(grp) if grp is not None else None]


def _supported(lib, stem, a, n_act, tab=None, sub=None, grp=None, act=None):
    return getattr(lib, f"psnode_{stem}_msp_supported")(R(a) if a is not None else None, *_tail(n_act, tab, sub, grp, act))


def _call(lib, stem, a, n_act, tab=None, sub=None, grp=None, act=None, ws=None, nbytes=0):
    return getattr(lib, f"psnode_{stem}_msp_f32")(R(a) if a is not None else None, *_tail(n_act, tab, sub, grp, act), ws, nbytes, None)


def _size(lib, stem, a, n_act, tab=None, sub=None, grp=None, act=None):
    return getattr(lib, f"psnode_{stem}_msp_workspace_size")(R(a) if a is not None else None, *_tail(n_act, tab, sub, grp, act))


def _with_x(a, stem):
    if stem == "dae_integrate":
        a.x.ptr = 256          # (a DAE forward without dataset rows is refused: the restarts read them)
    return a


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.psnode_abi_version() == 10 == _lib.ABI_VERSION
    grp_p = ctypes.POINTER(_lib.SegmentGroupsF32)
    for name in MSP_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        # the names the counting tests look for stay what they were
        assert not name.endswith("_workspace_bytes") and not any(f in name for f in ("_act_", "_tf_", "_rk_", "_sub_", "_lin_", "_pev_", "_ab_", "_ms_"))
    assert len([n for n in _lib.EXPORTS if "_msp_" in n]) == 10
    for stem, _, n_act in ENTRIES:
        ms_q, ms_f = getattr(lib, f"psnode_{stem}_ms_supported").argtypes, getattr(lib, f"psnode_{stem}_ms_f32").argtypes
        assert getattr(lib, f"psnode_{stem}_msp_supported").argtypes == ms_q[:-1] + [grp_p]
        assert getattr(lib, f"psnode_{stem}_msp_f32").argtypes == ms_f[:-4] + [grp_p] + ms_f[-3:]
        if "backward" in stem:
            fn = getattr(lib, f"psnode_{stem}_msp_workspace_size")
            assert fn.argtypes == ms_q[:-1] + [grp_p] and fn.restype is ctypes.c_size_t
    assert [f[0] for f in _lib.SegmentGroupsF32._fields_] == ["every", "x_true", "per_group"] and ctypes.sizeof(_lib.SegmentGroupsF32) == 24


@pytest.mark.parametrize("stem,make,n_act", ENTRIES)
def test_msp_argument_checks_and_status_order(stem, make, n_act):
    """the _ms family's order, with per_group < 1 next to every < 1"""
    lib = _lib.load()
    mk = lambda **kw: _with_x(make(**kw), stem)
    tab = R(nd.Kutta3().method.abi())
    ok = _grp(3, 2, 256)
    # the struct comes first: NULL, then every < 1 or per_group < 1 -- whatever else is wrong with the call
    for a in (mk(), None, mk(kernel=_lib.KERNEL_MFMA), mk(method=77)):
        assert _call(lib, stem, a, n_act, None, _sub(0), None) == -1 and _supported(lib, stem, a, n_act, None, _sub(0), None) == 0
        for every, per_group in ((0, 2), (-4, 2), (3, 0), (3, -1), (0, 0)):
            g = _grp(every, per_group)
            assert _call(lib, stem, a, n_act, None, _sub(0), g) == -2 and _supported(lib, stem, a, n_act, None, _sub(0), g) == 0
    for tb in (None, tab):
        assert _supported(lib, stem, mk(), n_act, tb, None, ok) == 1 and _call(lib, stem, mk(), n_act, tb, None, ok) == -1
        for n in (0, -3, 1025):
            assert _call(lib, stem, mk(), n_act, tb, _sub(n), ok) == -2 and _supported(lib, stem, mk(), n_act, tb, _sub(n), ok) == 0
        for n in (1, 2, 1024):
            for every in (1, 3, 11, 1000, 0x7fffffff):
                for per_group in (1, 2, 4, 11, 0x7fffffff):          # per_group >= n_seg is legal: one chunk
                    assert _supported(lib, stem, mk(), n_act, tb, _sub(n), _grp(every, per_group)) == 1
            assert _supported(lib, stem, mk(kernel=_lib.KERNEL_GENERIC), n_act, tb, _sub(n), ok) == 1
            assert _call(lib, stem, mk(), n_act, tb, _sub(n), ok) == -1
            for kernel in (_lib.KERNEL_MFMA_WAVE, _lib.KERNEL_MFMA_TILE, _lib.KERNEL_MFMA, _lib.KERNEL_MFMA_WIDE):
                assert _supported(lib, stem, mk(kernel=kernel), n_act, tb, _sub(n), ok) == 0
                assert _call(lib, stem, mk(kernel=kernel), n_act, tb, _sub(n), ok) == -5
        assert _call(lib, stem, None, n_act, tb, _sub(2), ok) == -1
    for sub in (None, _sub(1), _sub(2)):
        assert _call(lib, stem, mk(method=77), n_act, None, sub, ok) == -3 and _supported(lib, stem, mk(method=77), n_act, None, sub, ok) == 0
        assert _supported(lib, stem, mk(method=77), n_act, tab, sub, ok) == 1
    bad = nd.Kutta3().method.abi()
    bad.stages = 5
    unknown = _lib.ActF32()
    unknown.kind = 17
    assert _call(lib, stem, mk(), n_act, R(bad), _sub(2), ok) == -3
    assert _call(lib, stem, mk(), n_act, tab, _sub(2), ok, R(unknown)) == -3 and _supported(lib, stem, mk(), n_act, tab, _sub(2), ok, R(unknown)) == 0
    # order: the struct | sub-steps | act pair | NULL args | tableau | route
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(0), _grp(3, 0), R(unknown)) == -2
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2), ok, R(unknown)) == -3
    assert _call(lib, stem, None, n_act, R(bad), _sub(2), ok) == -1
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, R(bad), _sub(2), ok) == -3
    assert _call(lib, stem, mk(kernel=_lib.KERNEL_MFMA), n_act, tab, _sub(2), ok) == -5
    # more chunks than the launch grid's second dimension takes: refused with the route
    long = mk()
    (long.base if stem == "dae_backward" else long).T = 70000
    assert _supported(lib, stem, long, n_act, None, None, _grp(1, 1, 256)) == 0 and _call(lib, stem, long, n_act, None, None, _grp(1, 1, 256)) == -5
    assert _supported(lib, stem, long, n_act, None, None, _grp(1, 2, 256)) == 1


def _fill_ode_bwd(b):
    for l in range(4):
        b.de.weight[l] = b.de.bias[l] = 256
    b.t.ptr = b.z.ptr = b.all_initial = b.xs = b.grad_xs = b.grad_x0 = b.grad_all_initial = b.grad_params = 256


def _fill_dae_bwd(q):
    for m in (q.de, q.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    q.t.ptr = q.z.ptr = q.v.ptr = q.all_initial = q.xs = q.is_ = q.grad_xs = q.grad_x_init = q.grad_all_initial = 256
    q.grad_params_de = q.grad_params_ae = 256


def test_refusals_the_dataset_rows_and_the_workspace():
    lib = _lib.load()
    sub, ok = _sub(3), _grp(3, 2, 256)
    a = _ode_args()
    a.save_act = a.save_xstage = 256
    assert _supported(lib, "ode_integrate", a, 1, None, sub, ok) == 0 and _call(lib, "ode_integrate", a, 1, None, sub, ok) == -5
    d = _with_x(_dae_args(), "dae_integrate")
    d.save_act = d.save_xstage = d.save_ae_act = 256
    assert _supported(lib, "dae_integrate", d, 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", d, 2, None, sub, ok) == -5
    b = _ode_bwd_args()
    b.saved_act = b.saved_xstage = 256
    assert _supported(lib, "ode_backward", b, 1, None, sub, ok) == 0 and _call(lib, "ode_backward", b, 1, None, sub, ok) == -5
    assert _size(lib, "ode_backward", b, 1, None, sub, ok) == 0
    e = _dae_bwd_args()
    e.base.saved_act = 256
    assert _supported(lib, "dae_backward", e, 2, None, sub, ok) == 0 and _call(lib, "dae_backward", e, 2, None, sub, ok) == -5
    assert _size(lib, "dae_backward", e, 2, None, sub, ok) == 0
    # every teacher-forcing flag
    fa = _ode_args()
    fa.flags = _lib.FLAG_INPUT_TRUE_X
    assert _supported(lib, "ode_integrate", fa, 1, None, sub, ok) == 0 and _call(lib, "ode_integrate", fa, 1, None, sub, ok) == -5
    for flags in (1, 2, 3):
        fd = _with_x(_dae_args(), "dae_integrate")
        fd.flags = flags
        assert _supported(lib, "dae_integrate", fd, 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", fd, 2, None, sub, ok) == -5
        tfd = _dae_bwd_args(flags=flags)
        assert _supported(lib, "dae_backward", tfd, 2, None, sub, ok) == 0 and _call(lib, "dae_backward", tfd, 2, None, sub, ok) == -5
    tfo = _ode_bwd_args(flags=_lib.FLAG_INPUT_TRUE_X)
    assert _supported(lib, "ode_backward", tfo, 1, None, sub, ok) == 0 and _call(lib, "ode_backward", tfo, 1, None, sub, ok) == -5
    # a DAE forward whose x view is empty
    assert _supported(lib, "dae_integrate", _dae_args(), 2, None, sub, ok) == 0 and _call(lib, "dae_integrate", _dae_args(), 2, None, sub, ok) == -5
    # forward calls with every pointer in place get as far as the workspace check: missing, then one byte short
    a = _ode_args()
    for l in range(4):
        a.de.weight[l] = a.de.bias[l] = 256
    a.t.ptr = a.x.ptr = a.z.ptr = a.all_initial = a.x_out = 256
    need = lib.psnode_workspace_bytes(R(a.de), None)
    assert _call(lib, "ode_integrate", a, 1, None, None, ok) == -4 and _call(lib, "ode_integrate", a, 1, None, _sub(2), _grp(1, 1)) == -4
    assert _call(lib, "ode_integrate", a, 1, None, None, ok, ws=256, nbytes=need - 1) == -4
    d = _with_x(_dae_args(), "dae_integrate")
    for m in (d.de, d.ae):
        for l in range(4):
            m.weight[l] = m.bias[l] = 256
    d.t.ptr = d.z.ptr = d.v.ptr = d.x_init = d.all_initial = d.x_out = d.i_out = 256
    assert _call(lib, "dae_integrate", d, 2, None, None, ok) == -4
    # backward calls: x_sub where there are sub-steps, x_true where a step restarts (T - 1 = 11 > every), then the workspace
    b = _ode_bwd_args()
    _fill_ode_bwd(b)
    assert _call(lib, "ode_backward", b, 1, None, _sub(2), ok) == -1               # no x_sub
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), _grp(3, 2)) == -1  # no x_true, and 11 > 3
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), _grp(11, 1)) == -4    # no restart: x_true may be NULL
    need = _size(lib, "ode_backward", b, 1, None, _sub(2, 256), ok)
    assert need > 0 and _call(lib, "ode_backward", b, 1, None, _sub(2, 256), ok) == -4
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), ok, ws=256, nbytes=need - 1) == -4
    assert _call(lib, "ode_backward", b, 1, None, _sub(2, 256), ok, ws=260, nbytes=need) == -4          # misaligned
    e = _dae_bwd_args()
    _fill_dae_bwd(e.base)
    assert _call(lib, "dae_backward", e, 2, None, _sub(2), ok) == -1
    assert _call(lib, "dae_backward", e, 2, None, None, _grp(3, 1)) == -1 and _call(lib, "dae_backward", e, 2, None, None, _grp(100, 1)) == -4
    need = _size(lib, "dae_backward", e, 2, None, _sub(2, 256), ok)
    assert need > 0 and _call(lib, "dae_backward", e, 2, None, _sub(2, 256), ok, ws=256, nbytes=need - 1) == -4


@pytest.mark.parametrize("B", [1, 16, 33, 4096])
def test_the_workspace_query_against_the_layout(B):
    """The layout: gbwd_layout with one parameter partial and one tile-major slice per workgroup of the tiles x C grid, then the
    grad_all_initial partials [C - 1, B, n] and (DAE) the border slots [C - 1, B, zd + vd].  Against the sequential layout's size (the
    _rk query; the ODE's plain one), which is the same function at C = 1: the difference is what C - 1 further chunks add.  A workgroup
    costs np natural-order floats and tm tile-major ones; their sum is read off two sequential sizes."""
    lib = _lib.load()
    xd, zd, vd, idim, Tn = 8, 2, 2, 2, 101
    one_stage = _lib.RkTableauF32()
    one_stage.stages, one_stage.b[0] = 1, 1.0

    def ode(Bq):
        a = A.ode_bwd_args(method=_lib.RK4_38, T=Tn, B=Bq, kernel=_lib.KERNEL_GENERIC, hidden=(192, 192))
        return a, lib.psnode_ode_backward_workspace_bytes(R(a)) // 4

    def dae(Bq):
        a = A.dae_bwd_args(method=_lib.RK4_38, T=Tn, B=Bq, kernel=_lib.KERNEL_GENERIC)
        return a, lib.psnode_dae_backward_rk_workspace_bytes(R(a), None, None, R(one_stage)) // 4

    for stem, make, n_act, n, nzv in (("ode_backward", ode, 1, xd + zd, 0), ("dae_backward", dae, 2, xd + zd + vd + idim, zd + vd)):
        a, seq = make(B)
        tiles = -(-B // 16)
        per_wg = (make(16 * (tiles + 64))[1] - seq) // 64          # np + tm floats a further workgroup costs (64 of them: no rounding left)
        assert per_wg > 0
        for every, per_group in ((50, 1), (10, 3), (3, 1), (1, 100), (7, 2), (100, 1), (50, 2)):
            C_ = max(1, -(-(-(-(Tn - 1) // every)) // per_group))
            got = _size(lib, stem, a, n_act, None, None, _grp(every, per_group, 256))
            want = seq + (C_ - 1) * (tiles * per_wg + B * n + B * nzv)
            assert got == 4 * want, (stem, B, every, per_group, C_, got, 4 * want)
