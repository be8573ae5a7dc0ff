#!/usr/bin/env python3
"""Rates of the inter-frame lossless geometry stream (format 0xA8) on the test clouds of
tests/geom_inter_ref.py, from the numpy reference coder's real stream bytes (no GPU): per cloud the intra bytes, the inter
bytes, the vector list's bytes separately, the share of zero vectors and the node counts of the two symbol populations.
Writes profiles/geometry_inter_rate.json; tests/test_cpu_geometry_inter.py gates only inequalities (inter < intra where the
reference is related, auto <= intra everywhere)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import geom_inter_ref  # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "geometry_inter_rate.json")
    doc = {"what": "inter-frame lossless geometry (DESIGN.md 7e, format 0xA8), numpy reference coder, stream bytes with all framing and "
                   "side information; blocks 16^3, search +-2; ratios are reported, the tests gate inequalities only (no numeric margin)",
           "clouds": geom_inter_ref.rate_report()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, r in doc["clouds"].items():
        print(f"{name:24s} intra {r['intra_bytes']:6d} B  inter {r['inter_bytes']:6d} B  ratio {r['ratio_inter_over_intra']:.3f}  "
              f"vectors {r['vector_bytes']} B  zero vectors {r['zero_vector_share']:.2f}")
    print("wrote", out)


if __name__ == "__main__":
    main()
