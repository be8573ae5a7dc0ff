#!/usr/bin/env python3
"""Timing of the inter-frame lossless geometry coder (`geometry.encode_geometry(x, reference=r)` / `decode_geometry`, format
0xA8) on the benchmark frame `synth.surface_cloud(0, 10)`: against itself moved by (1, 0, 0) and against
`synth.surface_cloud(1, 10)`, next to the intra encode and decode of the same frame.

Everything is measured in ONE call, after warm-up, with device events around each call (the calls end in their own
device->host reads), the forms taking turns inside every repetition so that drift hits them alike.  Per form: median, min and
max of --reps repetitions (the spread goes with the figure).  Per phase: the device-event spans `timings=` reports, median of
--reps runs.  Time is recorded, not gated: there is no earlier figure to gate against."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import geometry, lib as L, synth  # noqa: E402


def alternate(forms, warmup, reps):
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}


def phases(fn, reps):
    runs = []
    for _ in range(reps):
        tm = {}
        fn(tm)
        runs.append(tm["inter"])
    return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_inter_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometry_inter_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    frame = torch.from_numpy(np.floor(synth.surface_cloud(0, args.bits, shuffle=False)[:, :3])).to(dev).contiguous()
    refs = {"moved_by_1_0_0": (frame - torch.tensor([1.0, 0.0, 0.0], device=dev)).contiguous(),
            "other_surface": torch.from_numpy(np.floor(synth.surface_cloud(1, args.bits, shuffle=False)[:, :3])).to(dev).contiguous()}
    cells = torch.unique(frame.to(torch.int32), dim=0)
    intra = geometry.encode_geometry(frame)
    doc = {"device": L.device_info()[1], "frame": f"surface_cloud(0, {args.bits})", "voxels": int(cells.shape[0]), "warmup": args.warmup,
           "reps": args.reps, "intra_bytes": len(intra), "references": {}}
    forms = {"intra_encode": lambda: geometry.encode_geometry(frame), "intra_decode": lambda: geometry.decode_geometry(intra, dev)}
    streams = {}
    for name, ref in refs.items():
        tm = {}
        data = geometry.encode_geometry(frame, reference=ref, mode="inter", timings=tm)
        back = geometry.decode_geometry(data, dev, reference=ref)
        assert back.shape == cells.shape and bool((back == cells).all()), f"{name}: round trip"
        streams[name] = data
        doc["references"][name] = {"inter_bytes": len(data), "ratio_inter_over_intra": len(data) / len(intra), "blocks": tm["blocks"],
                                   "zero_vector_share": tm["zero_vectors"] / tm["blocks"],
                                   "encode_host_reads_by_construction": tm["host_reads_by_construction"]}
        forms[f"inter_encode/{name}"] = lambda ref=ref: geometry.encode_geometry(frame, reference=ref, mode="inter")
        forms[f"auto_encode/{name}"] = lambda ref=ref: geometry.encode_geometry(frame, reference=ref, mode="auto")
        forms[f"inter_decode/{name}"] = lambda ref=ref, data=data: geometry.decode_geometry(data, dev, reference=ref)
    doc["timing"] = alternate(forms, args.warmup, args.reps)
    for name, ref in refs.items():
        r = doc["references"][name]
        r["encode_phases_ms"] = phases(lambda tm, ref=ref: geometry.encode_geometry(frame, reference=ref, mode="inter", timings=tm), args.reps)
        r["decode_phases_ms"] = phases(lambda tm, ref=ref, name=name: geometry.decode_geometry(streams[name], dev, reference=ref, timings=tm),
                                       args.reps)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
