#!/usr/bin/env python3
"""Rate / distortion sweep of the octree + RAHT anchor codec (`anchor.compress_anchor / decompress_anchor`, DESIGN.md section
7f): qp 22..46 in steps of 6 on `synth.surface_cloud(0, 9)` and `(0, 10)`, the reference's anchor settings
(`utils.py:505-529`: chroma offset -2, position scale 1).

Per point of the sweep: total bytes and their geometry / colour split, bits per point, `sym_y_psnr` of
`metrics.pointcloud_metrics`, and the encode / decode time from device events (median of --reps after --warmup).  Per cloud,
at --timing-qp: `encode_attributes` and `decode_attributes` beside `encode_geometry` and `decode_geometry`, the four calls
alternating inside every repetition, and the encoder's per-stage device times.  --reference-bits N adds the CPU time of the
numpy reference coder of the test-suite on `surface_cloud(0, N)`, for scale.  Timing is reported, nothing is gated.

--predict: instead of the above, the colour stream with and without the prediction from the parent level (0xB9 against 0xB3,
"Prediction from the parent level" in 7f) on `surface_cloud(0, 10)` unless --bits says otherwise, into
profiles/anchor_pred_rd.json.  Per qp: anchor bytes, colour bytes and `sym_y_psnr` both ways, and `encode_attributes` /
`decode_attributes` both ways, the four calls alternating inside every repetition; at --timing-qp the per-stage device times of
the two encoders and the two decoders."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import anchor, attributes, geometry, lib as L, metrics, synth  # noqa: E402


def alternate(forms, warmup, reps):
    """forms: name -> callable.  Median / min device-event ms per form, the forms taking turns inside every repetition."""
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
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v))} for k, v in ms.items()}


def sweep_point(pc, qp, warmup, reps):
    dev = pc.device
    data = anchor.compress_anchor(pc, qp)
    rec = anchor.decompress_anchor(data, dev)
    _, g, a = anchor.parse_container(data)
    n = int(rec.shape[0])
    res = {"qp": qp, "points": n, "total_bytes": len(data), "geometry_bytes": len(g), "colour_bytes": len(a),
           "bits_per_point": 8 * len(data) / n, "colour_bits_per_point": 8 * len(a) / n,
           "sym_y_psnr": metrics.pointcloud_metrics(pc, rec)["sym_y_psnr"]}
    res["timing"] = alternate({"compress_anchor": lambda: anchor.compress_anchor(pc, qp),
                               "decompress_anchor": lambda: anchor.decompress_anchor(data, dev)}, warmup, reps)
    return res


def coder_timing(pc, qp, warmup, reps):
    dev = pc.device
    xyz = pc[:, :3].contiguous()
    g = geometry.encode_geometry(xyz)
    a = attributes.encode_attributes(pc, qp)
    cs = geometry.decode_geometry(g, dev, as_set=True)
    res = alternate({"encode_geometry": lambda: geometry.encode_geometry(xyz),
                     "decode_geometry": lambda: geometry.decode_geometry(g, dev, as_set=True),
                     "encode_attributes": lambda: attributes.encode_attributes(pc, qp),
                     "decode_attributes": lambda: attributes.decode_attributes(a, cs)}, warmup, reps)
    t = {}
    attributes.encode_attributes(pc, qp, timings=t)
    res["encode_attributes_stages_ms"] = t["stages_ms"]
    res["encode_attributes_host_reads_beyond_the_level_sets"] = t["host_reads_by_construction"]
    res["qp"] = qp
    return res


def predict_point(pc, qp, warmup, reps):
    """One qp of the --predict sweep: the anchor with and without prediction, and the four colour-coder calls taking turns."""
    dev = pc.device
    res = {"qp": qp}
    cs = geometry.decode_geometry(geometry.encode_geometry(pc[:, :3].contiguous()), dev, as_set=True)
    streams = {}
    for name, predict in (("plain", None), ("predicted", True)):
        data = anchor.compress_anchor(pc, qp, predict=predict)
        rec = anchor.decompress_anchor(data, dev)
        _, g, a = anchor.parse_container(data)
        streams[name] = attributes.encode_attributes(pc, qp, predict=predict)
        assert streams[name][0] == a[0] == (0xB9 if predict else 0xB3)
        res[name] = {"total_bytes": len(data), "geometry_bytes": len(g), "colour_bytes": len(a), "points": int(rec.shape[0]),
                     "bits_per_point": 8 * len(data) / int(rec.shape[0]), "sym_y_psnr": metrics.pointcloud_metrics(pc, rec)["sym_y_psnr"]}
    res["timing"] = alternate({"encode_attributes": lambda: attributes.encode_attributes(pc, qp),
                               "encode_attributes_predict": lambda: attributes.encode_attributes(pc, qp, predict=True),
                               "decode_attributes": lambda: attributes.decode_attributes(streams["plain"], cs),
                               "decode_attributes_predict": lambda: attributes.decode_attributes(streams["predicted"], cs)}, warmup, reps)
    return res, streams, cs


def predict_stages(pc, qp, streams, cs):
    out = {}
    for name, predict in (("plain", None), ("predicted", True)):
        te, td = {}, {}
        attributes.encode_attributes(pc, qp, predict=predict, timings=te)
        attributes.decode_attributes(streams[name], cs, timings=td)
        out[name] = {"encode_stages_ms": te["stages_ms"], "decode_stages_ms": td["stages_ms"],
                     "encode_host_reads_beyond_the_level_sets": te["host_reads_by_construction"]}
    return out


def predict_main(args, dev):
    doc = {"device": L.device_info()[1], "warmup": max(args.warmup, 2), "reps": args.reps, "chroma_qp_offset": -2, "position_scale": 1.0,
           "what": "colour stream 0xB3 (plain) against 0xB9 (predicted from the parent level), DESIGN.md 7f; device events, medians; "
                   "the four coder calls alternate inside every repetition; reported, not gated", "clouds": {}}
    for bits in args.bits:
        pc = torch.from_numpy(synth.surface_cloud(0, bits, shuffle=False)).to(dev)
        entry = {"sweep": []}
        for qp in args.qps:
            res, streams, cs = predict_point(pc, qp, max(args.warmup, 2), args.reps)
            if qp == args.timing_qp:
                entry["stages"] = dict(predict_stages(pc, qp, streams, cs), qp=qp)
            entry["sweep"].append(res)
            tm = res["timing"]
            print(f"surface{bits} qp {qp}: colour {res['plain']['colour_bytes']} -> {res['predicted']['colour_bytes']} B, Y-PSNR "
                  f"{res['plain']['sym_y_psnr']:.2f} -> {res['predicted']['sym_y_psnr']:.2f} dB, encode "
                  f"{tm['encode_attributes']['median_ms']:.2f} -> {tm['encode_attributes_predict']['median_ms']:.2f} ms, decode "
                  f"{tm['decode_attributes']['median_ms']:.2f} -> {tm['decode_attributes_predict']['median_ms']:.2f} ms", flush=True)
        if "stages" in entry:
            print(f"surface{bits} stages", json.dumps(entry["stages"]), flush=True)
        doc["clouds"][f"surface{bits}"] = entry
    return doc


def reference_cpu_seconds(bits, qp):
    from tests import raht_ref
    pc = synth.surface_cloud(0, bits)
    lv = raht_ref.levels_of(pc[:, 3:])
    t0 = time.perf_counter()
    data = raht_ref.encode(pc, lv, qp)
    t1 = time.perf_counter()
    raht_ref.decode(data, pc)
    t2 = time.perf_counter()
    return {"bits": bits, "qp": qp, "points": len(pc), "encode_s": t1 - t0, "decode_s": t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, nargs="+", default=None, help="default: 9 10, with --predict: 10")
    ap.add_argument("--qps", type=int, nargs="+", default=list(range(22, 47, 6)))
    ap.add_argument("--timing-qp", type=int, default=28)
    ap.add_argument("--reference-bits", type=int, default=0, help="also time the numpy reference coder on this cloud (0: skip)")
    ap.add_argument("--predict", action="store_true", help="compare the colour stream with and without prediction from the parent level")
    ap.add_argument("--out", default=None, help="default: profiles/anchor_rd.json, with --predict: profiles/anchor_pred_rd.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor_rd.py needs a GPU")
    dev = torch.device("cuda:0")
    args.bits = args.bits or ([10] if args.predict else [9, 10])
    args.out = args.out or os.path.join(ROOT, "profiles", "anchor_pred_rd.json" if args.predict else "anchor_rd.json")
    if args.predict:
        doc = predict_main(args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print("wrote", args.out)
        return
    doc = {"device": L.device_info()[1], "warmup": args.warmup, "reps": args.reps, "chroma_qp_offset": -2, "position_scale": 1.0,
           "clouds": {}}
    for bits in args.bits:
        pc = torch.from_numpy(synth.surface_cloud(0, bits, shuffle=False)).to(dev)
        entry = {"sweep": [sweep_point(pc, qp, args.warmup, args.reps) for qp in args.qps],
                 "coders": coder_timing(pc, args.timing_qp, max(args.warmup, 2), args.reps)}
        doc["clouds"][f"surface{bits}"] = entry
        for p in entry["sweep"]:
            print(f"surface{bits} qp {p['qp']}: {p['total_bytes']} bytes ({p['geometry_bytes']} geometry + {p['colour_bytes']} colour), "
                  f"{p['bits_per_point']:.3f} bpp, Y-PSNR {p['sym_y_psnr']:.2f} dB, encode {p['timing']['compress_anchor']['median_ms']:.1f} ms, "
                  f"decode {p['timing']['decompress_anchor']['median_ms']:.1f} ms", flush=True)
        print(f"surface{bits} coders", json.dumps(entry["coders"]), flush=True)
    if args.reference_bits:
        doc["numpy_reference_cpu"] = reference_cpu_seconds(args.reference_bits, args.timing_qp)
        print("numpy reference", json.dumps(doc["numpy_reference_cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
