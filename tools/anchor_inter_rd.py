#!/usr/bin/env python3
"""Rate / distortion of the anchor codec with inter-frame colour (`anchor.compress_anchor_sequence`, DESIGN.md section 7f,
"Inter frames"): a qp sweep on `synth.surface_cloud(0, bits)` followed by the same cloud moved by one voxel with its colours
carried.  Per qp: the bytes of the second frame coded on its own (`compress_anchor`, the intra anchor) and as the second frame
of the closed-loop sequence (geometry and colour both against the first frame as decoded), their geometry / colour split, and
`sym_y_psnr` of `metrics.pointcloud_metrics` of either decode against the moved cloud.  Rates are reported, nothing is gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import anchor, lib as L, metrics, synth  # noqa: E402


def sweep_point(first, cur, qp):
    dev = cur.device
    intra = anchor.compress_anchor(cur, qp)
    streams = anchor.compress_anchor_sequence([first, cur], qp)
    rec_intra = anchor.decompress_anchor(intra, dev)
    rec_inter = anchor.decompress_anchor_sequence(streams, dev)[1]
    n = int(rec_inter.shape[0])
    res = {"qp": qp, "points": n}
    for name, data, rec in (("intra", intra, rec_intra), ("inter", streams[1], rec_inter)):
        _, g, a = anchor.parse_container(data)
        res[name] = {"total_bytes": len(data), "geometry_bytes": len(g), "colour_bytes": len(a), "colour_magic": hex(a[0]),
                     "bits_per_point": 8 * len(data) / n, "sym_y_psnr": metrics.pointcloud_metrics(cur, rec)["sym_y_psnr"]}
    res["total_ratio_inter_over_intra"] = res["inter"]["total_bytes"] / res["intra"]["total_bytes"]
    res["colour_ratio_inter_over_intra"] = res["inter"]["colour_bytes"] / res["intra"]["colour_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[9, 10])
    ap.add_argument("--qps", type=int, nargs="+", default=list(range(22, 47, 6)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_inter_rd.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor_inter_rd.py needs a GPU")
    dev = torch.device("cuda:0")
    doc = {"device": L.device_info()[1], "chroma_qp_offset": -2, "position_scale": 1.0,
           "what": "frame 2 of a two-frame sequence (surface_cloud(0, bits), then the same cloud moved by (1, 0, 0) with its colours "
                   "carried): coded on its own (intra) and against frame 1 as decoded (inter: compress_anchor_sequence, geometry and "
                   "colour both 'auto'); sym_y_psnr against the moved cloud; reported, not gated",
           "clouds": {}}
    for bits in args.bits:
        first = torch.from_numpy(synth.surface_cloud(0, bits, shuffle=False)).to(dev)
        first[:, :3] = torch.floor(first[:, :3])
        cur = first.clone()
        cur[:, 0] += 1
        doc["clouds"][f"surface{bits}"] = [sweep_point(first, cur, qp) for qp in args.qps]
        for p in doc["clouds"][f"surface{bits}"]:
            print(f"surface{bits} qp {p['qp']}: intra {p['intra']['total_bytes']} B ({p['intra']['colour_bytes']} colour) "
                  f"{p['intra']['sym_y_psnr']:.2f} dB, inter {p['inter']['total_bytes']} B ({p['inter']['colour_bytes']} colour) "
                  f"{p['inter']['sym_y_psnr']:.2f} dB", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
