#!/usr/bin/env python3
"""Event timing of the stages of `metrics.pcqm_features` on the benchmark frame (`synth.surface_cloud(0, 10)`, the vox10 frame of
bench.py's configs[1]) against its decoded reconstruction (benchmark model, q = [[0.5, 0.5]], block size 1024), with
r = 0.004 x 1023 and h = 2 r as the evaluation sets them, on the grid path and on the binary-search path.

Per path and stage the median / min of --reps event-timed calls after --warmup calls: the two canonical sets, the two curvature
fields, the nearest-neighbour pairing, the Lab conversion and paired table, the feature kernel, and the whole call.  `restatement`
is the wall time of the numpy restatement (tests/pcqm_ref.py) on the largest test cloud, a CPU figure for scale, not a
comparison at equal size.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import pcqm_ref  # noqa: E402
from unified_point_cloud_compression_amd import lib as L, metrics as M, sparse as S, synth  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcqm_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    model = bench.build_model(dev)
    q = torch.tensor([[0.5, 0.5]], device=dev)
    src = torch.from_numpy(synth.surface_cloud(0, args.bits)).to(dev)
    out = model.compress(src, q, block_size=1024)
    rec = model.decompress(coordinates=out[3], strings=out[0], shape=out[1], k=out[2], q_vals=out[4])
    r = M.PCQM_RADIUS_FRACTION * ((1 << args.bits) - 1)
    h = M.PCQM_RADIUS_FACTOR * r
    res = {"frame": f"synth.surface_cloud(0, {args.bits})", "points": int(src.shape[0]), "decoded": int(rec.shape[0]), "r": r, "h": h,
           "lim_r": M._pcqm_lim(r), "lim_h": M._pcqm_lim(h), "warmup": args.warmup, "reps": args.reps}
    old = S.USE_GRID
    try:
        for name, mode in (("grid", True), ("search", False)):
            S.USE_GRID = mode
            ca, a_pts, (a_rgb,), _ = M._canonical_set(src[:, :3], src[:, 3:6])
            cb, b_pts, (b_rgb,), _ = M._canonical_set(rec[:, :3], rec[:, 3:6])
            nn = M.nearest(a_pts, b_pts)[1].long()
            rho_a, rho_b = M._set_curvature(ca, r), M._set_curvature(cb, r)

            def table():
                la, lb = M.rgb_to_lab(a_rgb), M.rgb_to_lab(b_rgb)[nn]
                return torch.stack([rho_a, rho_b[nn], la[:, 0], lb[:, 0], la[:, 1], lb[:, 1], la[:, 2], lb[:, 2],
                                    torch.hypot(la[:, 1], la[:, 2]), torch.hypot(lb[:, 1], lb[:, 2])], dim=1).contiguous()

            tab = table()
            feats = torch.empty((ca.n, 8), dtype=torch.float64, device=dev)

            def feature_kernel():
                L.call("pcc_pcqm_features", L.ptr(ca.keys), ca.n, *S.grid_args(ca.grid() if mode else None), M._pcqm_lim(h),
                       2.0 / (h * h), L.ptr(tab), L.ptr(feats), L.stream())

            score = M.pcqm_features(src, rec, radius=r)
            res[name] = {
                "pcqm": score["pcqm"], "set_rows": [ca.n, cb.n],
                "canonical_sets": timed(lambda: (M._canonical_set(src[:, :3], src[:, 3:6]), M._canonical_set(rec[:, :3], rec[:, 3:6])),
                                        args.warmup, args.reps),
                "curvature_source": timed(lambda: M._set_curvature(ca, r), args.warmup, args.reps),
                "curvature_reconstruction": timed(lambda: M._set_curvature(cb, r), args.warmup, args.reps),
                "nearest": timed(lambda: M.nearest(a_pts, b_pts), args.warmup, args.reps),
                "lab_and_table": timed(table, args.warmup, args.reps),
                "feature_kernel": timed(feature_kernel, args.warmup, args.reps),
                "pcqm_features": timed(lambda: M.pcqm_features(src, rec, radius=r), args.warmup, args.reps),
            }
    finally:
        S.USE_GRID = old
    big = pcqm_ref.cloud("shell20")
    t0 = time.time()
    pcqm_ref.pcqm(big, pcqm_ref.reconstruction(big), 4.1, 8.2)
    res["restatement"] = {"cloud": "shell20", "points": int(big.shape[0]), "r": 4.1, "h": 8.2, "cpu_wall_ms": (time.time() - t0) * 1e3}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
