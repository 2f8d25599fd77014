"""The bytes every exported *_workspace_bytes query of the C ABI returns over a grid of shapes, against a recorded file (no GPU: the
queries read the args struct and nothing behind its pointers).

Each launcher's workspace is described once, by a layout function that the size query runs on a counting arena and the launch on the
caller's pointer (py_psnode_amd/csrc/psnode_workspace.h).  This test pins what the queries answer: a layout that gains a segment, loses
one or rounds differently changes a size here, on a machine without a GPU, instead of writing out of bounds on one.  The 16 queries of
include/psnode_hip.h (psnode_dae_backward_wide_ae_floats, which sizes a caller buffer, rides along) are asked over

    B               1, 15, 16, 17, 4608, 4609            tile and wave raggedness; the K4x / K4f switch
    hidden          16 .. 320 (HIDDENS)                  the width classes
    hidden layers   1 .. 5 and the mixed [128, 64, 32]   the K5 and K0 classes
    x_dim           1, 7, 8, 9, 16, 20, 64
    externals       z 0 / 2 / 8; DAE: v and i of 1 / 4 / 6, z + v + i of 8 and 16
    method          all three                            the K4f / K7f ring depends on the stage count at 8 waves
    saved rows      absent and present                   k7f_npa
    latent shapes   hidden 16 and 64, ODE and DAE, the DAE with and without z
    rows            0, 1, 63, 64, 65, 1 000 000          the row queries
    reduce parts    1 and 4097

thinned where the product would only repeat itself: every MLP shape at B = 17, the 3-hidden-layer shapes at x_dim 8 (the ODE: and 9) and
the first four external widths at every B, every method x saved rows at B = 17 and 4609 of those, the K5 families (one layout, K5's) at x_dim 8.
A case is `<query> <label>`; tests/workspace_bytes_table.txt holds them grouped: per query, each distinct size once, followed by the labels
that give it.

The file is recorded from a build of the commit BEFORE a change to a workspace layout, never from the changed code:
    PSNODE_LIB_PATH=<that build's libpsnode_hip.so> python tests/test_workspace_bytes_host.py --record [--commit <its id>]"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from py_psnode_amd import _lib  # noqa: E402

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes_table.txt")
R = ctypes.byref
DUMMY = 256          # a non-NULL, 256-byte aligned address that nothing on the host reads through

# ---- the grid
BS = (1, 15, 16, 17, 4608, 4609)
B_ALL_VARIANTS = (17, 4609)          # the batch sizes that carry every method x saved rows
HIDDENS = (16, 30, 32, 33, 64, 65, 128, 129, 192, 256, 320)
DEPTH_HIDDENS = (16, 64, 128, 320)          # the widths of the shapes with 1, 2, 4, 5 hidden layers
XDIMS = (1, 7, 8, 9, 16, 20, 64)
DEPTH_XDIMS = (1, 8, 20)
ODE_EXT = ((0,), (2,), (8,))          # (z,)
DAE_EXT = ((0, 1, 1), (2, 4, 2), (0, 4, 4), (2, 6, 6), (8, 4, 4), (8, 1, 6), (0, 6, 1))          # (z, v, i); z + v + i of 8 and 16 among them
METHODS = (_lib.EULER, _lib.MIDPOINT, _lib.RK4_38)
ROWS = (0, 1, 63, 64, 65, 1000000)
PARTS = (1, 4097)
T = 12


def hidden_stacks():
    """(label, hidden widths, full) of every MLP body: `full` shapes run at every B, x_dim and external width."""
    out = [(f"h{h}x3", (h,) * 3, True) for h in HIDDENS]
    out += [(f"h{h}x{n}", (h,) * n, False) for n in (1, 2, 4, 5) for h in DEPTH_HIDDENS]
    out.append(("h128.64.32", (128, 64, 32), False))
    return out


def _mlp(m, in_dim, widths):
    m.n_layers, m.in_dim = len(widths), in_dim
    for l, w in enumerate(widths):
        m.out_dim[l] = w
        m.weight[l] = m.bias[l] = DUMMY


def _fill(a, fields):
    for f in fields:
        setattr(a, f, DUMMY)


def _views(a, names):
    for v in names:
        getattr(a, v).ptr = DUMMY
        getattr(a, v).stride_t, getattr(a, v).stride_b = 64, 64 * T


ODE_SAVED = ("saved_act", "saved_xstage")
DAE_SAVED = ODE_SAVED + ("saved_ae_act", "saved_ev_act", "saved_ev_i")


def ode_bwd_args(xd, zd, widths, B, method, saved, in_dim=None):
    a = _lib.OdeBwdArgsF32()
    a.method, a.kernel, a.x_dim, a.z_dim, a.T, a.B = method, _lib.KERNEL_AUTO, xd, zd, T, B
    _mlp(a.de, in_dim or 3 * (xd + zd), widths + (xd,))
    _fill(a, ("all_initial", "xs", "grad_xs", "grad_x0", "grad_all_initial", "grad_params") + (ODE_SAVED if saved else ()))
    _views(a, "tz")
    return a


def dae_bwd_args(cls, xd, zd, vd, idim, de_widths, ae_widths, B, method, saved):
    """cls: DaeBwdTfArgsF32 (its .base is the plain call's struct) or DaeBwdWideArgsF32."""
    a = cls()
    b = a.base if cls is _lib.DaeBwdTfArgsF32 else a
    b.method, b.x_dim, b.z_dim, b.v_dim, b.i_dim, b.T, b.B = method, xd, zd, vd, idim, T, B
    n = xd + zd + vd + idim
    _mlp(b.de, 3 * n, de_widths + (xd,))
    _mlp(b.ae, n + xd + zd + vd, ae_widths + (idim,))
    _fill(b, ("all_initial", "xs", "is_", "grad_xs", "grad_params_de") + (DAE_SAVED if saved else ()))
    if cls is _lib.DaeBwdTfArgsF32:
        b.kernel = _lib.KERNEL_AUTO
        _fill(b, ("grad_x_init", "grad_all_initial", "grad_params_ae"))
    _views(b, "tzv")
    return a


def _heun():
    t = _lib.RkTableauF32()
    t.stages = 2
    t.a[1][0] = 1.0
    t.b[0] = t.b[1] = 0.5
    return t


def _variants(B, bs):
    """(label suffix, method, saved rows) of a case at batch size B of a shape that runs at the batch sizes bs."""
    if B in B_ALL_VARIANTS and len(bs) > 1:
        return [(f".m{m}.s{int(s)}", m, s) for m in METHODS for s in (False, True)]
    return [("", _lib.RK4_38, False)]


def _shapes(ext_list, latent_zs, b_xdims):
    """(label, x_dim, externals, hidden widths, batch sizes): the recipe shapes -- every B at the x_dim of b_xdims and the first four external
    widths -- then the latent ones (x = v = i = hidden, z = hidden or 0)."""
    for name, widths, full in hidden_stacks():
        for xd in XDIMS if full else DEPTH_XDIMS:
            for ext in ext_list:
                every_b = full and xd in b_xdims and ext in ext_list[:4]
                yield f"{name}.x{xd}.e{'_'.join(map(str, ext))}", xd, ext, widths, (BS if every_b else (17,))
    for h in (16, 64):
        for z in latent_zs:
            ext = (h if z else 0,) + (h,) * (len(ext_list[0]) - 1)
            yield f"latent{h}.z{ext[0]}", h, ext, (h,), BS


@functools.lru_cache(maxsize=None)
def table():
    """{`<query> <label>`: bytes} over the whole grid, computed once."""
    lib = _lib.load()
    rows = {}

    def put(query, label, value):
        key = f"{query} {label}"
        assert key not in rows, key
        rows[key] = int(value)

    # the forward query (MLP shapes alone) and the ODE backward
    for label, xd, (zd,), widths, bs in _shapes(ODE_EXT, (True,), (8, 9)):
        m = _lib.MlpF32()
        _mlp(m, 3 * (xd + zd), widths + (xd,))
        put("workspace_bytes", "ode." + label, lib.psnode_workspace_bytes(R(m), None))
        for B in bs:
            for suffix, method, saved in _variants(B, bs):
                a = ode_bwd_args(xd, zd, widths, B, method, saved)
                put("ode_backward_workspace_bytes", f"{label}.B{B}{suffix}", lib.psnode_ode_backward_workspace_bytes(R(a)))
    # the DAE: forward, the plain backward and the K5 families, the wide backward (K7f) and its AE buffer
    tanh, heun, sub2 = _lib.ActF32(), _heun(), _lib.SubstepsF32()
    tanh.kind, sub2.substeps, sub2.x_sub = _lib.ACT_TANH, 2, DUMMY
    for label, xd, (zd, vd, idim), widths, bs in _shapes(DAE_EXT, (True, False), (8,)):
        latent = label.startswith("latent")
        de_w, ae_w = widths, widths
        de, ae = _lib.MlpF32(), _lib.MlpF32()
        n = xd + zd + vd + idim
        _mlp(de, 3 * n, de_w + (xd,))
        _mlp(ae, n + xd + zd + vd, ae_w + (idim,))
        put("workspace_bytes", "dae." + label, lib.psnode_workspace_bytes(R(de), R(ae)))
        for B in bs:
            for suffix, method, saved in _variants(B, bs):
                a = dae_bwd_args(_lib.DaeBwdTfArgsF32, xd, zd, vd, idim, de_w, ae_w, B, method, saved)
                case = f"{label}.B{B}{suffix}"
                put("dae_backward_workspace_bytes", case, lib.psnode_dae_backward_workspace_bytes(R(a.base)))
                if len(widths) == 3 and not latent:
                    w = dae_bwd_args(_lib.DaeBwdWideArgsF32, xd, zd, vd, idim, de_w, ae_w, B, method, saved)
                    put("dae_backward_wide_workspace_bytes", case, lib.psnode_dae_backward_wide_workspace_bytes(R(w)))
                    if B == 17:
                        put("dae_backward_wide_ae_floats", case, lib.psnode_dae_backward_wide_ae_floats(R(w)))
                if saved or method != _lib.RK4_38 or xd != 8 or B not in B_ALL_VARIANTS or len(widths) == 1:          # the K5 families: K5's one layout again
                    continue
                a.flags, a.x_true, a.i_true = 3, DUMMY, DUMMY
                put("dae_backward_tf_workspace_bytes", case, lib.psnode_dae_backward_tf_workspace_bytes(R(a)))
                a.flags = 0
                put("dae_backward_rk_workspace_bytes", case, lib.psnode_dae_backward_rk_workspace_bytes(R(a), R(tanh), R(tanh), R(heun)))
                put("dae_backward_sub_workspace_bytes", case, lib.psnode_dae_backward_sub_workspace_bytes(R(a), R(tanh), R(tanh), R(heun), R(sub2)))
                put("dae_backward_lin_workspace_bytes", case, lib.psnode_dae_backward_lin_workspace_bytes(R(a), R(tanh), R(tanh), R(heun), R(sub2)))
    # the encoded DAE forward (K3g), with and without z
    for zd in (0, 8):
        e = _lib.DaeEncodedArgsF32()
        e.method, e.x_dim, e.z_dim, e.v_dim, e.i_dim, e.T, e.B = _lib.RK4_38, 16, zd, 4, 4, T, 17
        nblk = 4 if zd else 3
        for name, in_dim, ws in (("x_encoder", 16, (64, 64)), ("z_encoder", zd, (64, 64)), ("v_encoder", 4, (64, 64)), ("i_encoder", 4, (64, 64)),
                                 ("x_decoder", 64, (64, 16)), ("i_decoder", 64, (64, 4)), ("de", 3 * nblk * 64, (64, 64)),
                                 ("ae", (2 * nblk - 1) * 64, (64, 64))):
            if in_dim:
                _mlp(getattr(e, name), in_dim, ws)
        put("dae_encoded_workspace_bytes", f"z{zd}", lib.psnode_dae_encoded_workspace_bytes(R(e)))
    # the wide latent backward (K9w), the AE head's contractions (K7h), the loss (K6), the contraction over rows (K10)
    for h in (4, 16, 20, 32, 64, 68, 128, 132):
        put("latent_backward_wide_workspace_bytes", f"h{h}", lib.psnode_latent_backward_wide_workspace_bytes(h))
    for h in (16, 30, 64, 65, 128, 129):
        for B in BS:
            for rws in (63, 64):
                g = _lib.DaeHeadGradsArgsF32()
                g.R, g.B, g.hidden, g.n_zv = rws, B, h, 4
                put("dae_head_grads_workspace_bytes", f"h{h}.B{B}.R{rws}", lib.psnode_dae_head_grads_workspace_bytes(R(g)))
    for B in BS:
        for D in (1, 8, 20):
            for mw in sorted({0, 1, D}):
                lo = _lib.LossArgsF32()
                lo.T, lo.B, lo.D, lo.mask_width, lo.scale = T, B, D, mw, 1.0
                for v, w in (("pred", D), ("target", D), ("mask", max(mw, 1))):
                    getattr(lo, v).ptr, getattr(lo, v).stride_t, getattr(lo, v).stride_b = DUMMY, B * w, w
                lo.out = DUMMY
                put("masked_mse_workspace_bytes", f"B{B}.D{D}.w{mw}", lib.psnode_masked_mse_workspace_bytes(R(lo)))
    for rws in ROWS:
        for M, N in ((4, 4), (64, 64), (128, 16), (20, 128)):
            g = _lib.GemmTnArgsF32()
            g.rows, g.M, g.N, g.lda, g.ldb = rws, M, N, M, N
            put("gemm_tn_workspace_bytes", f"r{rws}.M{M}.N{N}", lib.psnode_gemm_tn_workspace_bytes(R(g)))
    # the row MLPs (K3b) and the encoder / decoder pair (K3r): partials | mid
    for H in (16, 64):
        for in_dim, out in sorted({(1, H), (7, H), (16, H), (H, H), (H, 1), (H, 8), (H, 16)}):
            m = _lib.MlpF32()
            _mlp(m, in_dim, (H, out))
            for rws in ROWS:
                put("mlp_rows_backward_workspace_bytes", f"H{H}.i{in_dim}.o{out}.r{rws}", lib.psnode_mlp_rows_backward_workspace_bytes(R(m), rws))
            for parts in PARTS:
                put("mlp_rows_reduce_workspace_bytes", f"H{H}.i{in_dim}.o{out}.p{parts}", lib.psnode_mlp_rows_reduce_workspace_bytes(R(m), parts))
        for d in (1, 7, 8, 16):
            enc, dec = _lib.MlpF32(), _lib.MlpF32()
            _mlp(enc, d, (H, H))
            _mlp(dec, H, (H, d))
            for rws in ROWS:
                put("recon_rows_backward_workspace_bytes", f"H{H}.d{d}.r{rws}", lib.psnode_recon_rows_backward_workspace_bytes(R(enc), R(dec), rws))
    return rows


QUERIES = tuple(n[len("psnode_"):] for n in _lib.EXPORTS if n.endswith("_workspace_bytes")) + ("dae_backward_wide_ae_floats",)


# ---- the recorded file: per query, one group per distinct size -- the size, then every case that gives it
def write_recorded(rows, commit):
    by_query = {}
    for key, value in rows.items():
        query, label = key.split()
        by_query.setdefault(query, {}).setdefault(value, []).append(label)
    with open(RECORDED, "w") as f:
        f.write(f"# tests/test_workspace_bytes_host.py --record, from the library built at commit {commit}\n")
        f.write("# per query: `<bytes> :`, then the cases that return it (hidden stack . x_dim . externals z_v_i . B . method . saved rows)\n")
        for query, groups in by_query.items():
            f.write(f"== {query}\n")
            for value, cases in groups.items():
                f.write(f"{value} :\n")
                for k in range(0, len(cases), 8):
                    f.write("    " + " ".join(cases[k:k + 8]) + "\n")


def read_recorded():
    rows, query, value = {}, None, None
    with open(RECORDED) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("== "):
                query = line[3:]
            elif line.endswith(" :"):
                value = int(line[:-2])
            elif line.startswith("    "):
                for label in line.split():
                    rows[f"{query} {label}"] = value
    return rows


def test_grid_reaches_every_query_and_every_kernel_class():
    got = table()
    assert {k.split()[0] for k in got} == set(QUERIES) and len(QUERIES) == 17
    for q in QUERIES:          # every query answers some case with a size and (but for the constant-size ones) several sizes
        sizes = {v for k, v in got.items() if k.startswith(q + " ")}
        assert sizes - {0}, q
    lib = _lib.load()
    # the ODE backward's classes: K4x and K4f on both sides of B = 4608, K5 beyond their widths, K8f and K9 at the latent shapes
    for label in ("h64x3.x8.e2.B4608", "h64x3.x8.e2.B4609.m2.s1", "h128x3.x8.e2.B17.m0.s0", "h192x3.x9.e2.B17.m2.s0",
                  "latent16.z16.B17.m2.s0", "latent64.z64.B17.m2.s1", "h128.64.32.x8.e2.B17"):
        assert got[f"ode_backward_workspace_bytes {label}"] > 0, label
    # K7f's ring: the size at 8 waves grows with the stage count
    k7f = [got[f"dae_backward_wide_workspace_bytes h128x3.x8.e2_4_2.B4609.m{m}.s0"] for m in METHODS]
    assert k7f[0] < k7f[1] < k7f[2], k7f
    assert got["dae_backward_wide_ae_floats h64x3.x8.e2_4_2.B17.m2.s1"] > 0 == got["dae_backward_wide_ae_floats h64x3.x8.e2_4_2.B17.m2.s0"]
    assert lib.psnode_workspace_bytes(None, None) == 0


def test_every_size_is_the_recorded_one():
    got, want = table(), read_recorded()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    bad = [f"{key}: recorded {want[key]}, now {got[key]}" for key in want if got[key] != want[key]]
    print(f"{len(want)} rows, {len(set(want.values()))} distinct sizes, {len(bad)} rows differ")
    assert not bad, "\n".join(bad[:40])


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    rows = table()
    write_recorded(rows, commit)
    print(f"{len(rows)} rows -> {RECORDED} ({os.path.getsize(RECORDED)} bytes)")
