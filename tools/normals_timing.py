#!/usr/bin/env python3
"""Event timing of the radius normal estimation (`metrics.estimate_normals`, radius 5 as `evaluate.py:153`) on the benchmark
frame (`synth.surface_cloud(0, 10)`, 787 502 points), on the grid path and on the binary-search path.

Per path: the whole call (canonicalisation of the user rows, the set's grid index, the kernel, the return to the caller's row
order) and the kernel alone (`pcc_normals_grid` over the already canonical set, its grid built), as the median / min of
--reps event-timed calls after --warmup calls.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unified_point_cloud_compression_amd import metrics, sparse as S, synth  # noqa: E402


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
    ap.add_argument("--radius", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    pc = torch.from_numpy(synth.surface_cloud(0, 10)).to(dev)
    xyz = pc[:, :3].contiguous()
    res = {"points": int(xyz.shape[0]), "radius": args.radius, "lim": metrics._normals_lim(args.radius)}
    old = S.USE_GRID
    try:
        for name, mode in (("grid", True), ("search", False)):
            S.USE_GRID = mode
            cs, _, _, _ = metrics._canonical_set(xyz)
            if mode:
                assert cs.grid() is not None, "the benchmark frame's lattice has a grid index"
            res[name] = {"estimate_normals": timed(lambda: metrics.estimate_normals(xyz, args.radius), args.warmup, args.reps),
                         "kernel": timed(lambda: metrics._set_normals(cs, args.radius), args.warmup, args.reps),
                         "set_rows": cs.n}
    finally:
        S.USE_GRID = old
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
