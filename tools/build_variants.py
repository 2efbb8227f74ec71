"""Builds diagnostic variants of the library into tools/ablate_libs/<name>.so:
    python tools/build_variants.py name1:-DFOO=1,-DBAR name2: ...
Run them on the GPU box with tools/ab_probe.py name1 name2 ... (interleaved A/B timing).  VARIANT_PART: the objects (build.OBJECTS,
comma-separated) that are compiled with the flags; the rest are the product's.  Default: the full-row kernels, forward and backward."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sot_amd
LIBDIR = os.path.join(ROOT, "tools", "ablate_libs")
os.makedirs(LIBDIR, exist_ok=True)
ONLY = tuple(os.environ.get("VARIANT_PART", "full_fwd,full_bwd").split(","))

for spec in sys.argv[1:]:
    name, _, flags = spec.partition(":")
    try:
        sot_amd.build.build(extra_flags=[f for f in flags.split(",") if f], only=ONLY, out=os.path.join(LIBDIR, name + ".so"))
        print(name, "ok")
    except RuntimeError as e:
        print(name, "FAILED\n" + str(e)[-2000:])
