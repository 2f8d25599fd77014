#!/usr/bin/env python3
"""Record what the REAL reference's ODE_/DAE_Curves_Sample (neural_base.py:10-40,136-166) loads from the synthetic dataset of
tests/test_datapath.py (`_write_npz`, num_sample=9, cut_length=10): every field tensor and item 3, as g9_dataset_<ode|dae>.npz.

    python tests/golden/make_dataset_fixture.py <directory of the reference checkout>

Only the loaded arrays are written; no reference source travels.  test_datapath.py compares this package's dataset mirror and its
device-resident copy against them."""
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)


def main(ref_dir):
    from test_datapath import _write_npz
    from py_psnode_amd import datapath
    ray, rw = types.ModuleType("ray"), types.ModuleType("ray.worker")
    rw.init = lambda *a, **k: None
    ray.worker = rw
    sys.modules.update({"ray": ray, "ray.worker": rw})      # neural_base.py:4 imports an unused symbol from ray
    for k in [k for k in sys.modules if k == "neural_dae" or k.startswith("neural_dae.")]:
        del sys.modules[k]
    sys.path.insert(0, ref_dir)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_nb = importlib.import_module("neural_dae.neural_base")
    assert os.path.abspath(ref_nb.__file__).startswith(os.path.abspath(ref_dir))
    for dae in (False, True):
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "d.npz")
            _write_npz(p, dae=dae, with_mask=dae)
            ds = (ref_nb.DAE_Curves_Sample if dae else ref_nb.ODE_Curves_Sample)(p, "cpu", num_sample=9, cut_length=10)
            out = {k: getattr(ds, k).numpy() for k in datapath.dataset_fields(ds)}
            out.update({f"item3_{j}": a.numpy() for j, a in enumerate(ds[3])})
            out["length"] = np.array(len(ds))
        np.savez(os.path.join(OUT, f"g9_dataset_{'dae' if dae else 'ode'}.npz"), **out)
        print("wrote", f"g9_dataset_{'dae' if dae else 'ode'}.npz", sorted(out))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_dataset_fixture.py <directory of the reference checkout>")
    main(sys.argv[1])
