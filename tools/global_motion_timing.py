#!/usr/bin/env python3
"""Timing and sizes of global motion compensation (`motion.py`, stream format 0xA9, DESIGN.md section 7e "Global motion") on
the benchmark frame `synth.surface_cloud(0, 10)`: the current frame is that cloud rotated by 2 degrees about (1, 1, 0) through
the grid centre and moved by (3.4, -1.2, 0.7), the reference the cloud itself.

Recorded: `estimate_rigid`, `warp_cloud`, the `global_motion="auto"` encode and its decode, the three stream sizes (global,
plain inter as `mode="auto"` returns it, intra), and beside them the plain inter encode and decode of the same pair
(`global_motion=None`: the code path of the parent commit).  Device events around whole calls, the forms taking turns inside
every repetition; median, min and max.  Time is recorded, not gated: nobody has measured any of this before.

`--estimate-report` adds what tests/test_gpu_motion.py bounds the estimator with, on the 7-bit cases: the spread of the numpy
reference's own quantised transform between forward and reversed summation, and the device's distance from it
(profiles/global_motion_estimate.txt).  `--rate` needs no GPU: the numpy reference coder's stream sizes on the tests' cases
(profiles/global_motion_rate.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(forms, warmup, reps):
    import torch
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


def moved(cells, axis, degrees, shift, centre):
    """unique(floor(R (a - centre) + centre + shift + 0.5)) of integer cells: the current frame of the measurement."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.sqrt(k @ k)
    th = np.deg2rad(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    c = np.asarray(centre, dtype=np.float64)
    return np.unique(np.floor((cells.astype(np.float64) - c) @ R.T + c + np.asarray(shift, dtype=np.float64) + 0.5).astype(np.int64), axis=0)


def rate(out):
    from tests import motion_ref as MR
    doc = {"coder": "tests/motion_ref.py (numpy reference)", "reference": "surface_cloud(0, 7) cells; iv: geom_inter_ref f_unrelated",
           "cases": MR.rate_report()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
    print("wrote", out)


def estimate_report(out):
    import torch
    from tests import geom_ref as G, motion_ref as MR
    from unified_point_cloud_compression_amd import geometry, metrics, motion
    dev = torch.device("cuda:0")
    lines = ["entries: M row by row (Q24), then t (Q8 voxels); spread = |forward - reversed| of the numpy reference's quantised",
             "transform (its sums accumulated in forward and in reversed order, on the device's normals); distance = |device - forward|"]
    for name in ("i_rot3", "ii_rot5", "iii_shift"):
        cur, ref = MR.case(name)
        cc, rc = G.unique_cells(cur), G.unique_cells(ref)
        cs = geometry.canonical_rows(torch.from_numpy(cc.astype(np.int32)).to(dev))[0]
        nv = metrics._set_normals(cs, 5.0)[0].cpu().numpy()
        fwd = MR.quantise(*MR.estimate_float(cc, rc, order="forward", cur_normals=nv))
        rev = MR.quantise(*MR.estimate_float(cc, rc, order="reversed", cur_normals=nv))
        got = motion.estimate_rigid(torch.from_numpy(cur).to(dev), torch.from_numpy(ref).to(dev)).ints()
        lines.append(f"{name}: spread {np.abs(np.array(fwd) - np.array(rev)).tolist()} distance {np.abs(np.array(got) - np.array(fwd)).tolist()}")
        tc, tr = torch.from_numpy(cur).to(dev), torch.from_numpy(ref).to(dev)
        sizes = [len(geometry.encode_geometry(tc, reference=tr, global_motion="auto")), len(geometry.encode_geometry(tc, reference=tr, mode="inter")),
                 len(geometry.encode_geometry(tc))]
        lines.append(f"{name}: device streams: global_motion=\"auto\" {sizes[0]} B, plain inter {sizes[1]} B, intra {sizes[2]} B")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_motion_timing.json"))
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--estimate-report", action="store_true")
    args = ap.parse_args()
    if args.rate:
        return rate(os.path.join(ROOT, "profiles", "global_motion_rate.json"))
    import torch
    from unified_point_cloud_compression_amd import geometry, lib as L, motion, synth
    if not torch.cuda.is_available():
        raise SystemExit("global_motion_timing.py needs a GPU")
    if args.estimate_report:
        estimate_report(os.path.join(ROOT, "profiles", "global_motion_estimate.txt"))
    dev = torch.device("cuda:0")
    a = np.unique(np.floor(synth.surface_cloud(0, args.bits, shuffle=False)[:, :3]).astype(np.int64), axis=0)
    half = float(1 << (args.bits - 1))
    cur_np = moved(a, (1, 1, 0), 2.0, (3.4, -1.2, 0.7), (half, half, half))
    cur = torch.from_numpy(cur_np.astype(np.float32)).to(dev).contiguous()
    ref = torch.from_numpy(a.astype(np.float32)).to(dev).contiguous()
    cells = torch.from_numpy(cur_np.astype(np.int32)).to(dev)
    T = motion.estimate_rigid(cur, ref)
    if T is None:
        raise SystemExit("estimate_rigid found no match")
    glob = geometry.encode_geometry(cur, reference=ref, global_motion="auto")
    plain = geometry.encode_geometry(cur, reference=ref)
    plain_inter = geometry.encode_geometry(cur, reference=ref, mode="inter")
    intra = geometry.encode_geometry(cur)
    for data in (glob, plain, plain_inter):
        back = geometry.decode_geometry(data, dev, reference=ref)
        assert back.shape == cells.shape and bool((back == cells).all()), "round trip"
    doc = {"device": L.device_info()[1], "reference": f"surface_cloud(0, {args.bits})", "current": "the reference rotated 2 deg about (1,1,0) "
           "through the grid centre, moved by (3.4, -1.2, 0.7)", "voxels_current": int(cells.shape[0]), "voxels_reference": int(ref.shape[0]),
           "warmup": args.warmup, "reps": args.reps, "transform": T.ints(),
           "bytes": {"global_auto": len(glob), "global_auto_magic": hex(glob[0]), "plain_auto": len(plain), "plain_auto_magic": hex(plain[0]),
                     "plain_inter": len(plain_inter), "intra": len(intra)}}
    forms = {
        "estimate_rigid": lambda: motion.estimate_rigid(cur, ref),
        "warp_cloud": lambda: motion.warp_cloud(ref, T),
        "global_auto_encode": lambda: geometry.encode_geometry(cur, reference=ref, global_motion="auto"),
        "global_given_transform_encode_inter": lambda: geometry.encode_geometry(cur, reference=ref, mode="inter", global_motion=T),
        "global_decode": lambda: geometry.decode_geometry(glob, dev, reference=ref),
        "plain_inter_encode": lambda: geometry.encode_geometry(cur, reference=ref, mode="inter"),
        "plain_auto_encode": lambda: geometry.encode_geometry(cur, reference=ref),
        "plain_inter_decode": lambda: geometry.decode_geometry(plain_inter, dev, reference=ref),
    }
    doc["timing"] = alternate(forms, args.warmup, args.reps)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
