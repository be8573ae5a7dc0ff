#!/usr/bin/env python3
"""Timing of the inter-frame lossless colour coder ("Inter frames") on `synth.surface_cloud(0, 10)` coded
against itself moved by one voxel with the colours carried along: `encode_attributes_lossless(..., reference=, mode=)` with
mode "inter", "auto" and -- the parent's path, re-measured in the same run -- "intra", and `decode_attributes_lossless` of the
inter and the intra stream.  Device events, a warm-up, medians of --reps, the forms alternating inside every repetition; the
stage times of both sides come from their `timings` argument.  Every decode is checked against the input's levels before anything is
timed.  A report, not a gate: "auto" codes two containers and the decoder re-runs the motion search.  Not measured here:
kernel-level times from a profiler run, any kernel's share of peak, other clouds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import attributes as A, geometry, lib as L, synth  # noqa: E402
from tools.anchor_rd import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossless_inter_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lossless_inter_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    ref = torch.from_numpy(synth.surface_cloud(0, args.bits, shuffle=False)).to(dev)
    ref[:, :3] = torch.floor(ref[:, :3])
    cur = ref.clone()
    cur[:, 0] += 1
    xyz = cur[:, :3].contiguous()
    cs = geometry.decode_geometry(geometry.encode_geometry(xyz), dev, as_set=True)
    enc = {m: (lambda m=m: A.encode_attributes_lossless(cur, reference=ref, mode=m)) for m in ("intra", "inter", "auto")}
    streams = {m: f() for m, f in enc.items()}
    levels = torch.round(cur[:, 3:6].to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8)
    order = torch.argsort((xyz[:, 0].long() << 40) | (xyz[:, 1].long() << 20) | xyz[:, 2].long())
    dec = {m: (lambda m=m: A.decode_attributes_lossless(streams[m], cs, reference=ref)) for m in ("intra", "inter")}
    if not all(torch.equal(f(), levels[order]) for f in dec.values()) or streams["intra"] != A.encode_attributes_lossless(cur):
        raise SystemExit("lossless_inter_timing.py: a decode did not return the input")
    n = int(cs.n)
    hdr = A.parse_lossless_header(streams["inter"])
    doc = {"device": L.device_info()[1], "warmup": args.warmup, "reps": args.reps, "cloud": f"surface{args.bits} moved by (1, 0, 0), colours carried",
           "points": n, "exact": True, "blocks": hdr["blocks"],
           "bytes": {m: len(s) for m, s in streams.items()}, "bits_per_point": {m: 8 * len(s) / n for m, s in streams.items()},
           "auto_is": "inter" if streams["auto"] == streams["inter"] else "intra",
           "what": "device events around whole calls, the five forms alternating inside every repetition, medians; stage times from the "
                   "encoder's and the decoder's own events (encoder stages_ms: the stages of the intra coder; inter_stages_ms: motion search + matching, and the "
                   "select / histogram / member / container passes of the 0xB6 stream); intra is the parent commit's path, mode='intra', "
                   "re-measured in this run; timing is reported, not gated",
           "not_measured": ["kernel-level times from a profiler run", "any kernel's share of peak", "other clouds"]}
    forms = {f"encode_{m}": f for m, f in enc.items()}
    forms.update({f"decode_{m}": f for m, f in dec.items()})
    doc["timing"] = alternate(forms, args.warmup, args.reps)
    for m in ("intra", "inter", "auto"):
        stages = {}
        for _ in range(args.reps):
            t = {}
            A.encode_attributes_lossless(cur, reference=ref, mode=m, timings=t)
            for key in ("stages_ms", "inter_stages_ms"):
                for k, v in t.get(key, {}).items():
                    stages.setdefault(f"{key}.{k}", []).append(v)
        doc[f"encode_{m}_stages_median_ms"] = {k: float(np.median(v)) for k, v in stages.items()}
        if m != "intra":
            doc["mode1_blocks"] = t["mode1_blocks"]
    for m in ("intra", "inter"):
        stages = {}
        for _ in range(args.reps):
            t = {}
            A.decode_attributes_lossless(streams[m], cs, reference=ref, timings=t)
            for k, v in t["stages_ms"].items():
                stages.setdefault(k, []).append(v)
        doc[f"decode_{m}_stages_median_ms"] = {k: float(np.median(v)) for k, v in stages.items()}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
