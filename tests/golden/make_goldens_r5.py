"""Round-7 goldens, generated from the REAL reference (/root/reference) in the build container -- data only, never source:

  g7_grad_<tag>[.partN].npz: what the reference's `loss.backward()` produces through the direct_encode models (neural_00_ODE_02_direct_encode.py,
  neural_01_DAE_02_direct_encode.py) at hidden widths outside {16, 64} -- the route of K11 / K10 (row MLPs), K3w / K9w (latent integrator):
    ode02_h128, dae02_h128     the scripts' argparse default --hidden 128 (neural_00_ODE_02_direct_encode.py:160-162,
                               neural_01_DAE_02_direct_encode.py:246-248); Euler + RK4 / Euler only (fixture size)
    ode02_h36, dae02_h36,      hidden 36: the K3w class (H % 4 == 0) but no multiple of 16; Euler, Midpoint, RK4
    dae02_z0_h36
    ode02_h30                  hidden 30: no K3w width; K11 with N % 4 != 0 and _pad4's zero columns in K10; Euler, Midpoint, RK4
  Same recipe, shapes (B=8, T=21, two events, per-trajectory clocks) and keys as make_goldens_r2.py:g7, which this script calls with
  other model constructors.  A set larger than a committed file may be is split into <stem>.part0.npz, .part1.npz, ... (disjoint keys;
  tests/helpers.py:load merges them).

    python tests/golden/make_goldens_r5.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens_r2 as r2  # noqa: E402
from make_goldens import OUT  # noqa: E402

PART_BYTES = 960 * 1024         # raw bytes per part: fp32 weights and gradients barely compress, and a committed file stays < 1 MiB


def save_parts(name, **arrs):
    """`name` as one .npz, or as <stem>.part0.npz, .part1.npz, ... of at most PART_BYTES raw bytes each (keys in insertion order)."""
    arrs = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    parts, cur, size = [], {}, 0
    for k, a in arrs.items():
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    stem = os.path.join(OUT, name[:-len(".npz")])
    for old in (f"{stem}.npz", *(f"{stem}.part{k}.npz" for k in range(64))):
        if os.path.exists(old):
            os.remove(old)
    paths = [f"{stem}.npz"] if len(parts) == 1 else [f"{stem}.part{k}.npz" for k in range(len(parts))]
    for path, part in zip(paths, parts):
        np.savez_compressed(path, **part)
        kib = os.path.getsize(path) / 1024
        assert kib < 1024, f"{path}: {kib:.0f} KiB"
        print(f"  wrote {os.path.basename(path)}: {kib:.0f} KiB")


if __name__ == "__main__":
    if not os.path.isdir(r2.REF):
        sys.exit("reference not mounted; goldens can only be regenerated in the build container")
    nd_, mods_ = r2.load_reference()
    xd, zd, vd, idim = 8, 2, 2, 2
    groups = (
        (("euler", "rk4"), lambda o1, o2, d1, d2: (("ode02_h128", 100, lambda z_: o2.ODE_Model(xd, zd, 128)),)),
        (("euler",), lambda o1, o2, d1, d2: (("dae02_h128", 101, lambda z_: d2.DAE_Model(xd, zd, vd, idim, 128)),)),
        (None, lambda o1, o2, d1, d2: (("ode02_h36", 102, lambda z_: o2.ODE_Model(xd, zd, 36)),
                                       ("dae02_h36", 103, lambda z_: d2.DAE_Model(xd, zd, vd, idim, 36)),
                                       ("dae02_z0_h36", 104, lambda z_: d2.DAE_Model(xd, z_, vd, idim, 36)),
                                       ("ode02_h30", 105, lambda z_: o2.ODE_Model(xd, zd, 30)))),
    )
    for methods, cases in groups:
        r2.g7(nd_, mods_, cases, methods=methods, saver=save_parts)
