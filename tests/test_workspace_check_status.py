"""The status of every _f32 entry point that checks a caller workspace, over four workspaces that must all be refused, against a recorded
file (no GPU, nothing launches).

Each entry point is called with valid dims and a dummy non-NULL, 256-byte aligned address for every pointer it looks at, so that the call
gets as far as its workspace check, and with `need` = its own *_workspace_bytes query:
    (NULL, 0)   (a misaligned address, need)   (an aligned address, need - 1)   (NULL, need)
A row is the entry point's name and one digit n of status -n per workspace (4 = PSNODE_ERR_WORKSPACE).  The check is one shared predicate
(py_psnode_amd/csrc/psnode_launch.h: workspace_ok); the file pins that each entry point still answers what it answered with its own copy.

tests/workspace_check_status.txt is recorded from a build of the commit BEFORE a change to the entry points, never from the changed code:
    PSNODE_LIB_PATH=<that build's libpsnode_hip.so> python tests/test_workspace_check_status.py --record [--commit <its id>]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from py_psnode_amd import _lib  # noqa: E402
from test_entry_status_matrix import DUMMY, _act, _args  # noqa: E402  (the four K0 / K5 args structs with every required pointer set)

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_check_status.txt")
R = ctypes.byref
T, B = 4, 5


def _mlp(m, widths):
    """in -> widths[1:], every weight and bias a dummy"""
    m.n_layers, m.in_dim = len(widths) - 1, widths[0]
    for l, o in enumerate(widths[1:]):
        m.out_dim[l] = o
        m.weight[l] = m.bias[l] = DUMMY


def _set(a, *fields):
    for f in fields:
        v = getattr(a, f)
        if isinstance(v, _lib.ViewF32):
            v.ptr = DUMMY
        elif isinstance(v, ctypes.Array):
            for k in range(len(v)):
                v[k] = DUMMY
        else:
            setattr(a, f, DUMMY)


def _dae_encoded():
    a = _lib.DaeEncodedArgsF32()
    a.method, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = _lib.RK4_38, 4, 2, 2, 2, T, B
    for enc, d in ((a.x_encoder, 4), (a.z_encoder, 2), (a.v_encoder, 2), (a.i_encoder, 2)):
        _mlp(enc, (d, 64, 64))
    _mlp(a.x_decoder, (64, 64, 4))
    _mlp(a.i_decoder, (64, 64, 2))
    _mlp(a.de, (3 * 4 * 64, 64, 64))
    _mlp(a.ae, (7 * 64, 64, 64))
    _set(a, "t", "x", "z", "v", "i", "x0", "x_pred", "i_pred")
    return a


def _latent_bwd_wide():
    a = _lib.LatentBwdWideArgsF32()
    a.method, a.hidden, a.z_dim, a.dae, a.T, a.B = _lib.RK4_38, 32, 32, 0, T, B
    _mlp(a.de, (3 * 2 * 32, 32, 32))
    _set(a, "t", "grad_xs", "grad_x0", "saved_act", "gk", "d1", "d1s")
    return a


def _dae_bwd_wide():
    a = _lib.DaeBwdWideArgsF32()
    xd, zd, vd, idim = 8, 2, 2, 2
    a.method, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = _lib.RK4_38, xd, zd, vd, idim, T, B
    n = xd + zd + vd + idim
    _mlp(a.de, (3 * n, 64, 64, 64, xd))
    _mlp(a.ae, (n + xd + zd + vd, 64, 64, 64, idim))
    _set(a, "t", "z", "v", "all_initial", "xs", "is_", "grad_xs", "carry_x", "ae_act", "ae_delta", "ae_gi", "grad_params_de", "grad_zv",
         "grad_all_initial_de")
    return a


def _head_grads():
    a = _lib.DaeHeadGradsArgsF32()
    a.R, a.B, a.hidden, a.n_zv, a.act_row_stride = 8, B, 64, 0, 64
    _set(a, "act", "delta", "gi", "u", "sa1", "out")
    return a


def _gemm_tn():
    a = _lib.GemmTnArgsF32()
    a.rows, a.M, a.N, a.lda, a.ldb = 8, 4, 4, 4, 4
    _set(a, "A", "B", "C")
    return a


def entry_points(lib):
    """(name, call(workspace, bytes) -> status, need in bytes)"""
    tanh = R(_act("tanh"))          # a non-ELU(1) activation: the K0 / K5 family call path itself, not the plain entry point it forwards to
    ode, dae = _args("ode_fwd", (), True), _args("dae_fwd", (), True)
    ode_b, dae_b = _args("ode_bwd", (), True), _args("dae_bwd", (), True)
    enc, lw, dw, hg, tn = _dae_encoded(), _latent_bwd_wide(), _dae_bwd_wide(), _head_grads(), _gemm_tn()
    return [
        ("ode_integrate_f32", lambda ws, n: lib.psnode_ode_integrate_f32(R(ode), ws, n, None), lib.psnode_workspace_bytes(R(ode.de), None)),
        ("dae_integrate_f32", lambda ws, n: lib.psnode_dae_integrate_f32(R(dae), ws, n, None), lib.psnode_workspace_bytes(R(dae.de), R(dae.ae))),
        ("ode_integrate_act_f32", lambda ws, n: lib.psnode_ode_integrate_act_f32(R(ode), tanh, ws, n, None),
         lib.psnode_workspace_bytes(R(ode.de), None)),
        ("ode_backward_f32", lambda ws, n: lib.psnode_ode_backward_f32(R(ode_b), ws, n, None), lib.psnode_ode_backward_workspace_bytes(R(ode_b))),
        ("dae_backward_f32", lambda ws, n: lib.psnode_dae_backward_f32(R(dae_b.base), ws, n, None),
         lib.psnode_dae_backward_workspace_bytes(R(dae_b.base))),
        ("ode_backward_act_f32", lambda ws, n: lib.psnode_ode_backward_act_f32(R(ode_b), tanh, ws, n, None),
         lib.psnode_ode_backward_workspace_bytes(R(ode_b))),
        ("dae_encoded_integrate_f32", lambda ws, n: lib.psnode_dae_encoded_integrate_f32(R(enc), ws, n, None),
         lib.psnode_dae_encoded_workspace_bytes(R(enc))),
        ("latent_backward_wide_f32", lambda ws, n: lib.psnode_latent_backward_wide_f32(R(lw), ws, n, None),
         lib.psnode_latent_backward_wide_workspace_bytes(lw.hidden)),
        ("dae_backward_wide_f32", lambda ws, n: lib.psnode_dae_backward_wide_f32(R(dw), ws, n, None),
         lib.psnode_dae_backward_wide_workspace_bytes(R(dw))),
        ("dae_head_grads_f32", lambda ws, n: lib.psnode_dae_head_grads_f32(R(hg), ws, n, None), lib.psnode_dae_head_grads_workspace_bytes(R(hg))),
        ("gemm_tn_f32", lambda ws, n: lib.psnode_gemm_tn_f32(R(tn), ws, n, None), lib.psnode_gemm_tn_workspace_bytes(R(tn))),
    ]


def rows():
    out = {}
    for name, call, need in entry_points(_lib.load()):
        assert need > 1, name          # the dims are the entry point's own: its query sizes them
        got = [call(ws, n) for ws, n in ((None, 0), (DUMMY + 16, need), (DUMMY, need - 1), (None, need))]
        out[name] = "".join(str(-rc) if -6 <= rc <= 0 else "?" for rc in got)
    return out


def read_recorded():
    with open(RECORDED) as f:
        return dict(line.split() for line in f if line.strip() and not line.startswith("#"))


def test_every_refused_workspace_gets_the_recorded_status():
    got, want = rows(), read_recorded()
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for name, row in got.items():
        print(name, row)
        assert "0" not in row and "?" not in row, name          # PSNODE_OK would have launched
    assert got == want
    assert set("".join(want.values())) == {"4"}          # every case stops at the workspace check itself


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    with open(RECORDED, "w") as f:
        f.write(f"# tests/test_workspace_check_status.py --record, from the library built at commit {commit}\n")
        f.write("# workspaces: (NULL, 0) (misaligned, need) (aligned, need - 1) (NULL, need); digit n = status -n\n")
        for name, row in rows().items():
            f.write(f"{name} {row}\n")
    print(open(RECORDED).read())
