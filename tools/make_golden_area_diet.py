"""Writes the fixture of tests/test_area_packed_div_gpu.py::test_rows_unchanged_against_the_build_before: row losses and means of the
plain row loop (2048 bins, p = 1) on the stress rows of that test's small cases, as the loaded library computes them.  Run it on the GPU
with the library of the commit BEFORE a change to the plain loop's arithmetic (SOT_LIB_PATH names it):

    SOT_LIB_PATH=/path/to/libsot_hip.so python tools/make_golden_area_diet.py [OUT.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sot_amd import _native as nat  # noqa: E402
from test_area_packed_div_gpu import golden_outputs  # noqa: E402

nat.load(build_if_missing=False)
out = golden_outputs(nat)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "area_valu_diet.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes;", nat.library_path(), {k: v.tolist() for k, v in out.items()})
