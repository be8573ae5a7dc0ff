#!/usr/bin/env python3
"""Timing of the inter-frame RAHT colour coder ("Inter frames") on `synth.surface_cloud(0, 10)` moved by
one voxel with the colours carried along, coded against the unmoved cloud AS DECODED at the same qp:
`encode_attributes(..., reference=, mode=)` with mode "inter", "auto" and -- the parent's path, re-measured in the same run --
"intra", and `decode_attributes` of the inter and the intra stream.  Device events, a warm-up, medians of --reps, the forms
alternating inside every repetition; the stage times of both sides come from their `timings` argument.  The inter decode is
checked for determinism and the intra bytes against a call without a reference before anything is timed.  A report, not a
gate: there is no parent for the new path, "auto" codes two containers and the decoder re-runs the motion search and the
prediction's forward transform.  Not measured here: kernel-level times from a profiler run, any kernel's share of peak, other
clouds."""
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
    ap.add_argument("--qp", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_inter_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor_inter_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    first = torch.from_numpy(synth.surface_cloud(0, args.bits, shuffle=False)).to(dev)
    first[:, :3] = torch.floor(first[:, :3])
    cur = first.clone()
    cur[:, 0] += 1
    rs = geometry.decode_geometry(geometry.encode_geometry(first[:, :3].contiguous()), dev, as_set=True)
    ref_levels = A.decode_attributes(A.encode_attributes(first, args.qp), rs)            # the previous frame as the decoder holds it
    cs = geometry.decode_geometry(geometry.encode_geometry(cur[:, :3].contiguous()), dev, as_set=True)
    ref = {"reference": rs, "reference_attrs": ref_levels}
    enc = {m: (lambda m=m: A.encode_attributes(cur, args.qp, mode=m, **ref)) for m in ("intra", "inter", "auto")}
    streams = {m: f() for m, f in enc.items()}
    dec = {m: (lambda m=m: A.decode_attributes(streams[m], cs, **ref)) for m in ("intra", "inter")}
    if streams["intra"] != A.encode_attributes(cur, args.qp) or not torch.equal(dec["inter"](), dec["inter"]()):
        raise SystemExit("anchor_inter_timing.py: the intra bytes changed or the inter decode is not deterministic")
    n = int(cs.n)
    hdr = A.parse_header(streams["inter"])
    doc = {"device": L.device_info()[1], "warmup": args.warmup, "reps": args.reps, "qp": args.qp,
           "cloud": f"surface{args.bits} moved by (1, 0, 0), colours carried; reference: the unmoved cloud as decoded at qp {args.qp}",
           "points": n, "blocks": hdr["blocks"], "bytes": {m: len(s) for m, s in streams.items()},
           "bits_per_point": {m: 8 * len(s) / n for m, s in streams.items()},
           "auto_is": "inter" if streams["auto"] == streams["inter"] else "intra",
           "what": "device events around whole calls, the five forms alternating inside every repetition, medians; stage times from the "
                   "encoder's and the decoder's own events (stages_ms: the intra coder's stages; inter_stages_ms: motion search + matching, "
                   "prediction fill, the double forward pass with the decision, select / histogram / member choice, member index + "
                   "container, and for auto the intra stream's tail); intra is the parent commit's path, mode='intra', re-measured in this "
                   "run; timing is reported, not gated",
           "not_measured": ["kernel-level times from a profiler run", "any kernel's share of peak", "other clouds"]}
    forms = {f"encode_{m}": f for m, f in enc.items()}
    forms.update({f"decode_{m}": f for m, f in dec.items()})
    doc["timing"] = alternate(forms, args.warmup, args.reps)
    for m in ("intra", "inter", "auto"):
        stages = {}
        for _ in range(args.reps):
            t = {}
            A.encode_attributes(cur, args.qp, mode=m, timings=t, **ref)
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
            A.decode_attributes(streams[m], cs, timings=t, **ref)
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
