#!/usr/bin/env python3
"""Timing of the lossless colour coder and the lossless codec on `synth.surface_cloud(0, 9)` and
`(0, 10)`: `encode_attributes_lossless` / `decode_attributes_lossless`, `compress_lossless` / `decompress_lossless`, and in
the same run, alternating inside every repetition, `encode_attributes` / `decode_attributes` at qp 4 (the finest lossy setting)
as the comparison.  Device events, a warm-up, medians of --reps; the encoder's stage times come from its `timings` argument.
Every decode is checked against the input's levels before anything is timed.  Timing is reported, nothing is gated: this path
has no parent.  Not measured here: kernel-level times from a profiler run, any kernel's share of peak, clouds above bits 10,
`predict=False`, and the stored mode."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import anchor, attributes, geometry, lib as L, synth  # noqa: E402
from tools.anchor_rd import alternate  # noqa: E402


def cloud_timing(pc, warmup, reps):
    dev = pc.device
    xyz = pc[:, :3].contiguous()
    cs = geometry.decode_geometry(geometry.encode_geometry(xyz), dev, as_set=True)
    a = attributes.encode_attributes_lossless(pc)
    lossy = attributes.encode_attributes(pc, 4)
    whole = anchor.compress_lossless(pc)
    # exactness first: the decoded levels are the input's, through both interfaces
    levels = torch.round(pc[:, 3:6].to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8)
    rec = anchor.decompress_lossless(whole, dev)
    order = torch.argsort(((xyz[:, 0].long() << 40) | (xyz[:, 1].long() << 20) | xyz[:, 2].long()))
    exact = bool(torch.equal(attributes.decode_attributes_lossless(a, cs), levels[order])
                 and torch.equal(rec[:, :3], xyz[order]) and torch.equal(torch.round(rec[:, 3:].double() * 255).to(torch.uint8), levels[order]))
    if not exact:
        raise SystemExit("lossless_timing.py: a decode did not return the input")
    n = int(cs.n)
    hdr = attributes.parse_lossless_header(a)
    res = {"points": n, "exact": exact, "lossless_colour_bytes": len(a), "lossless_colour_bits_per_point": 8 * len(a) / n,
           "stored": hdr["stored"], "streams": hdr["streams"], "lossless_total_bytes": len(whole), "lossless_total_bits_per_point": 8 * len(whole) / n,
           "qp4_colour_bytes": len(lossy), "qp4_colour_bits_per_point": 8 * len(lossy) / n}
    res["timing"] = alternate({"encode_attributes_lossless": lambda: attributes.encode_attributes_lossless(pc),
                               "decode_attributes_lossless": lambda: attributes.decode_attributes_lossless(a, cs),
                               "encode_attributes_qp4": lambda: attributes.encode_attributes(pc, 4),
                               "decode_attributes_qp4": lambda: attributes.decode_attributes(lossy, cs),
                               "compress_lossless": lambda: anchor.compress_lossless(pc),
                               "decompress_lossless": lambda: anchor.decompress_lossless(whole, dev)}, warmup, reps)
    stages = {}
    for _ in range(reps):
        t = {}
        attributes.encode_attributes_lossless(pc, timings=t)
        for k, v in t["stages_ms"].items():
            stages.setdefault(k, []).append(v)
    res["encode_attributes_lossless_stages_median_ms"] = {k: float(np.median(v)) for k, v in stages.items()}
    res["encode_attributes_lossless_host_reads_beyond_the_level_sets"] = t["host_reads_by_construction"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, nargs="+", default=[9, 10])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossless_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lossless_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    doc = {"device": L.device_info()[1], "warmup": args.warmup, "reps": args.reps, "clouds": {},
           "what": "device events around whole calls, the six forms alternating inside every repetition, medians; stage times from the "
                   "encoder's own events; timing is reported, not gated",
           "not_measured": ["kernel-level times from a profiler run", "any kernel's share of peak", "clouds above surface_cloud(0, 10)",
                            "predict=False", "the stored mode"]}
    for bits in args.bits:
        pc = torch.from_numpy(synth.surface_cloud(0, bits, shuffle=False)).to(dev)
        doc["clouds"][f"surface{bits}"] = cloud_timing(pc, args.warmup, args.reps)
        print(f"surface{bits}", json.dumps(doc["clouds"][f"surface{bits}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
