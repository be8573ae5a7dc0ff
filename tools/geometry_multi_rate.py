#!/usr/bin/env python3
"""Rates of the geometry stream with several references (format 0xAB, DESIGN.md section 7e "Several references") on the clouds
of tests/geom_multi_ref.py, from the numpy reference coder's real stream bytes (no GPU): per cloud the intra bytes, every slot
alone, all slots together, the blocks per slot and what `mode="auto"` returns.  Writes profiles/geometry_multi_rate.json;
tests/test_cpu_geometry_multi.py gates the inequalities (0xAB at most half the best single slot where each slot shows one part of
the frame; "auto" the single-reference stream where the second slot is useless)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import geom_multi_ref  # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "geometry_multi_rate.json")
    doc = {"what": "geometry with several references (DESIGN.md 7e, format 0xAB), numpy reference coder, stream bytes with all framing and "
                   "side information; blocks 16^3, search +-2; a = surface_cloud(0, bits) floored and made unique, h = 2^(bits-1); "
                   "uncovered: slots a[x < h+8] + (1,0,0) and a[x >= h-8] + (0,-1,1); turn: the half x >= h turned 4 degrees about z "
                   "through (1.5h, h, h), slots a and a warped by that transform; unrelated_second: a + (1,0,0) against a and "
                   "surface_cloud(1, 7); every 0xAB stream was decoded back",
           "clouds": geom_multi_ref.rate_report()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, r in doc["clouds"].items():
        print(f"{name:20s} intra {r['intra_bytes']:6d} B  single {r['single_slot_bytes']}  multi {r['multi_bytes']:6d} B  "
              f"ratio {r['ratio_multi_over_best_single']:.3f}  blocks per slot {r['blocks_per_slot']}  auto {r['auto_bytes']} B")
    print("wrote", out)


if __name__ == "__main__":
    main()
