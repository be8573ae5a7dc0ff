"""Regenerate tests/golden/reference_surface.json: what the reference's own `model/blocks.py` and `model/transforms.py`
build when they import UNCHANGED against this package's MinkowskiEngine / compressai surfaces.

    python tests/golden/make_reference_surface.py <reference checkout>

The reference files are imported from the checkout named on the command line and never copied; the fixture holds data
only: the surface names they use, and per transform its module tree (shim classes by name) and its state_dict
(key -> shape) at the R2 width.  tests/test_cpu_reference_surface.py checks the build's own modules against it.
"""
import importlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CFG = {"C_in": 4, "C_out": 3, "N1": 128, "N2": 128, "N3": 128, "N4": 128}


def main(ref):
    import unified_point_cloud_compression_amd as upcc
    upcc.install_shims(force=True)
    names = set()
    for rel in ("model/blocks.py", "model/transforms.py", "loss.py"):
        src = open(os.path.join(ref, rel)).read()
        names.update("MinkowskiEngine." + m for m in re.findall(r"\bME\.(\w+)", src))
        for mod, items in re.findall(r"^from (compressai[\w.]*) import ([\w, ]+)$", src, re.M):
            names.update(f"{mod}.{i.strip()}" for i in items.split(","))
    sys.path.insert(0, ref)
    blocks = importlib.import_module("model.blocks")
    transforms = importlib.import_module("model.transforms")
    assert blocks.__file__.startswith(os.path.abspath(ref)) and transforms.__file__.startswith(os.path.abspath(ref))
    out = {"config": CFG, "surface": sorted(names), "transforms": {}}
    for cls in ("AnalysisTransform", "SparseSynthesisTransform"):
        m = getattr(transforms, cls)(CFG)
        shim = {name: f"{type(mod).__module__}.{type(mod).__name__}" for name, mod in m.named_modules()
                if type(mod).__module__.startswith("unified_point_cloud_compression_amd.")}
        out["transforms"][cls] = {"state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()], "shim_modules": shim,
                                  "bias_free": [name for name, mod in m.named_modules() if hasattr(mod, "kernel") and mod.bias is None]}
    g = blocks.MinkowskiGDN(128, inverse=True)
    out["gdn_inverse_128"] = {"inverse": bool(g.inverse), "gamma": list(g.gamma.shape), "kernel_size": g.kernel_size}
    dst = os.path.join(ROOT, "tests", "golden", "reference_surface.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {dst}")


if __name__ == "__main__":
    main(sys.argv[1])
