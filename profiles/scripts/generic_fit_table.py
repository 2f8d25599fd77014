"""Fit table of the generic kernels K0 / K5: what the library's *_supported queries answer over a grid of shapes (no GPU needed).

    python profiles/scripts/generic_fit_table.py LIB.so [OUT.json]

tests/generic_fit_table.json was written by this script from the library of the commit BEFORE K5's fit functions took `pre` as a run-time
argument (each of the four objects had its own, the pre object exported a second fit query); tests/test_generic_fit_table.py compares the
current library with it.  One character per answer: the value the query
returned (0 / 1, or K5's mode 0 / 1 / 2 for the DAE backward).

The C ABI has no plain psnode_{ode,dae}_integrate_supported: the four forward queries are the _act_supported ones with Tanh (K0's act
build) and with SiLU (its pre build); both ask K0's LDS fit, which every shape of this grid passes -- K0's fit (generic_plan,
generic_lds_bytes: compiled once, in the ELU(1) object) is not exercised here."""
import ctypes
import json
import os
import sys

DEPTHS = tuple(range(1, 9))                                   # Linear layers
HIDDEN = (1, 7, 16, 33, 64, 96, 128, 160, 192, 256)
ODE_X, ODE_Z = (1, 8, 20, 24, 32, 64), (0, 2, 8)
DAE_DIMS = ((4, 2, 1, 1), (8, 2, 3, 3), (20, 10, 40, 40), (24, 2, 6, 6))      # x, z, v, i

ODE_QUERIES = ("ode_backward", "ode_backward_act_tanh", "ode_backward_act_silu", "ode_backward_rk_heun2",
               "ode_integrate_act_tanh", "ode_integrate_act_silu")
DAE_QUERIES = ("dae_backward", "dae_backward_act_tanh", "dae_backward_act_silu", "dae_backward_rk_heun2",
               "dae_integrate_act_tanh", "dae_integrate_act_silu")


def ode_shapes():
    return [(L, h, x, z) for L in DEPTHS for h in HIDDEN for x in ODE_X for z in ODE_Z]


def dae_shapes():
    return [(L, h, d) for L in DEPTHS for h in HIDDEN for d in DAE_DIMS]


def _mlp(m, L, hidden, in_dim, out_dim):
    m.n_layers, m.in_dim = L, in_dim
    for k in range(L):
        m.out_dim[k] = hidden if k + 1 < L else out_dim


def answers(_lib):
    """{query name: string of one character per shape}, in the order of ode_shapes() / dae_shapes()."""
    lib = _lib.load()
    R = ctypes.byref

    def act(kind):
        a = _lib.ActF32()
        a.kind, a.alpha, a.beta, a.threshold = kind, 0.0, 1.0, 20.0
        return a

    tanh, silu = act(_lib.ACT_TANH), act(_lib.ACT_SILU)
    heun = _lib.RkTableauF32()
    heun.stages = 2
    heun.a[1][0] = 1.0
    heun.b[0] = heun.b[1] = 0.5
    out = {q: [] for q in ODE_QUERIES + DAE_QUERIES}
    for L, h, x, z in ode_shapes():
        b, f = _lib.OdeBwdArgsF32(), _lib.OdeArgsF32()
        for a in (b, f):
            a.method, a.kernel, a.x_dim, a.z_dim, a.T, a.B = _lib.RK4_38, _lib.KERNEL_GENERIC, x, z, 10, 4
            _mlp(a.de, L, h, 3 * (x + z), x)
        out["ode_backward"].append(lib.psnode_ode_backward_supported(R(b)))
        out["ode_backward_act_tanh"].append(lib.psnode_ode_backward_act_supported(R(b), R(tanh)))
        out["ode_backward_act_silu"].append(lib.psnode_ode_backward_act_supported(R(b), R(silu)))
        out["ode_backward_rk_heun2"].append(lib.psnode_ode_backward_rk_supported(R(b), None, R(heun)))
        out["ode_integrate_act_tanh"].append(lib.psnode_ode_integrate_act_supported(R(f), R(tanh)))
        out["ode_integrate_act_silu"].append(lib.psnode_ode_integrate_act_supported(R(f), R(silu)))
    for L, h, (x, z, v, i) in dae_shapes():
        n = x + z + v + i
        tf, f = _lib.DaeBwdTfArgsF32(), _lib.DaeArgsF32()
        for a in (tf.base, f):
            a.method, a.kernel, a.x_dim, a.z_dim, a.v_dim, a.i_dim, a.T, a.B = _lib.RK4_38, _lib.KERNEL_GENERIC, x, z, v, i, 10, 4
            _mlp(a.de, L, h, 3 * n, x)
            _mlp(a.ae, L, h, n + x + z + v, i)
        b = tf.base
        out["dae_backward"].append(lib.psnode_dae_backward_supported(R(b)))
        out["dae_backward_act_tanh"].append(lib.psnode_dae_backward_act_supported(R(b), R(tanh), R(tanh)))
        out["dae_backward_act_silu"].append(lib.psnode_dae_backward_act_supported(R(b), R(silu), R(silu)))
        out["dae_backward_rk_heun2"].append(lib.psnode_dae_backward_rk_supported(R(tf), None, None, R(heun)))
        out["dae_integrate_act_tanh"].append(lib.psnode_dae_integrate_act_supported(R(f), R(tanh), R(tanh)))
        out["dae_integrate_act_silu"].append(lib.psnode_dae_integrate_act_supported(R(f), R(silu), R(silu)))
    for q, vals in out.items():
        assert all(0 <= v <= 9 for v in vals), (q, sorted(set(vals)))
    return {q: "".join(str(v) for v in vals) for q, vals in out.items()}


def main():
    os.environ["PSNODE_LIB_PATH"] = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from py_psnode_amd import _lib
    table = {"depths": DEPTHS, "hidden": HIDDEN, "ode_x": ODE_X, "ode_z": ODE_Z, "dae_dims": DAE_DIMS, "answers": answers(_lib)}
    text = json.dumps(table, indent=0) + "\n"
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
