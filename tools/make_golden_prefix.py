"""Writes the fixture of tests/test_area_fast_loop_gpu.py::test_shared_cdf_builder_outputs_unchanged: paper-mode forward_rows and
loss_and_grad outputs (16 rows of 2048 and of 1025 bins; row losses, mean, the first 64 gradient values per row) as the loaded library
computes them.  Run it on the GPU with the library of the commit BEFORE a change to the shared CDF builder (SOT_LIB_PATH names it):

    SOT_LIB_PATH=/path/to/libsot_hip.so python tools/make_golden_prefix.py [OUT.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sot_amd import _native as nat  # noqa: E402
from test_area_fast_loop_gpu import PREFIX_SHAPES, shared_prefix_outputs  # noqa: E402

nat.load(build_if_missing=False)
out = {}
for n in PREFIX_SHAPES:
    out.update(shared_prefix_outputs(nat, n))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "area_fast_loop_prefix.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes;", nat.library_path(), {k: v.shape for k, v in out.items()})
