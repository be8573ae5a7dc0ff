#!/usr/bin/env python3
"""Timing of the on-device training batches (`unified_point_cloud_compression_amd/data.py`) on the benchmark frame
(`synth.surface_cloud(0, 10)`, 787 502 points), next to what they feed and what they replace, all in one run:

* slicing      `slice_into_cubes(frame, 128)`, once per frame: event-timed calls.
* assemble     one batch of 8 cubes of 128^3 (more than 300 points) under ColorJitter + RandomRotate(128): events around
               `TrainBatcher.assemble` (upload, the mean reduction, the batch kernel, first-wins de-duplication), over
               pre-drawn batches of one epoch order; also without the de-duplication, and the host wall time of a whole
               iteration step (parameter draws included, ended by a device synchronise).
* train step   `bench.train_step_setup`'s step on one such batch (its batch, q and lambda swapped for the batcher's).
* CPU restatement  the same pipeline (jitter -> rotate -> collate -> first-wins) in numpy on this host (`tests/data_ref.py`),
               thread count printed.  It is NOT the reference's loader (12 worker processes, torchvision), which cannot
               run here; it is the same arithmetic on one CPU process.

Two couplings to files outside tools/, both deliberate and both loud when they break: `rebind` swaps the batch inside the
closure `bench.train_step_setup` returns by the names of its free variables (coords, feats, q, Lam) -- bench.py offers no
other way to hand its step a batch, and a rename there is a KeyError here, not a wrong number; and the CPU restatement is
the test tree's `tests/data_ref.py`, so that the arithmetic timed is the arithmetic the tests check, not a third copy.

One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unified_point_cloud_compression_amd import data as D, synth  # noqa: E402

TRANSFORMS = {"1_ColorJitter": {"key": "ColorJitter"}, "2_Rotate": {"key": "RandomRotate", "block_size": 128}}   # CVPR_inverse_scaling.yaml:32-38
Q_MAP = {"lambda_A_min": 0, "lambda_A_max": 12800, "lambda_G_min": 0, "lambda_G_max": 200, "mode": "quadratic"}


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def event_timed(fns, warmup):
    """Each callable of `fns` once, event-timed, after `warmup` calls cycling through them."""
    for k in range(warmup):
        fns[k % len(fns)]()
    ms = []
    for fn in fns:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def rebind(fn, **values):
    """Replace free variables of a closure (the batch `bench.train_step_setup` captured) by name."""
    cells = dict(zip(fn.__code__.co_freevars, fn.__closure__))
    for name, v in values.items():
        cells[name].cell_contents = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    pc = synth.surface_cloud(0, 10)
    pts, col = torch.from_numpy(pc[:, :3].copy()).to(dev), torch.from_numpy(pc[:, 3:].copy()).to(dev)
    res = {"points": int(pts.shape[0]), "batch": args.batch, "cube_size": 128, "min_points": 300}

    res["slicing"] = event_timed([lambda: D.slice_into_cubes(pts, col, 128)] * 8, 2)
    table = D.slice_into_cubes(pts, col, 128)
    res["cubes"], res["eligible"] = len(table), len(table.indices(300))

    g = torch.Generator().manual_seed(0)
    batcher = D.TrainBatcher(table, args.batch, min_points=300, transforms=D.build_transforms(TRANSFORMS), generator=g)
    order = torch.randperm(len(batcher.eligible), generator=g).tolist()
    drawn = []
    for k in range(args.reps):
        cubes = [batcher.eligible[order[(k * args.batch + j) % len(order)]] for j in range(args.batch)]
        drawn.append((cubes, [batcher.draw() for _ in cubes]))
    res["assemble"] = event_timed([lambda c=c, p=p: batcher.assemble(c, p) for c, p in drawn], args.warmup)
    res["assemble_without_deduplication"] = event_timed([lambda c=c, p=p: batcher.assemble(c, p, deduplicate=False) for c, p in drawn],
                                                         args.warmup)
    rows = [batcher.assemble(c, p) for c, p in drawn[:8]]
    res["rows_per_batch_before_after"] = [int(np.mean([r[2]["rows"] for r in rows])), int(np.mean([r[0].shape[0] for r in rows]))]
    wall = []
    for epoch in range(2):                                 # whole iteration steps, draws included; the first epoch warms up
        it = iter(batcher)
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            item = next(it, None)
            torch.cuda.synchronize()
            if item is None:
                break
            if epoch:
                wall.append((time.perf_counter() - t0) * 1e3)
    res["iteration_step_host_wall"] = stats(wall)

    import bench
    one, info = bench.train_step_setup(dev)
    coords, feats, binfo = batcher.assemble(*drawn[0])
    q, lam = D.Q_Func(Q_MAP)(len(binfo["cubes"]), generator=g, device=dev)
    rebind(one, coords=coords, feats=feats, q=q, Lam=lam)
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.train_steps):
        last = one()
    torch.cuda.synchronize()
    res["train_step"] = {"ms": (time.perf_counter() - t0) / args.train_steps * 1e3, "steps": args.train_steps, "points": int(coords.shape[0]),
                         "loss": last[0], "config": info["config"]}
    res["assemble_share_of_train_step"] = res["assemble"]["median_ms"] / res["train_step"]["ms"]

    from tests import data_ref as R
    cubes_np = {i: (table.cube(i)["points"].cpu().numpy(), table.cube(i)["colors"].cpu().numpy()) for c, _ in drawn[:args.cpu_reps] for i in c}
    cpu = []
    for c, p in drawn[:args.cpu_reps]:
        t0 = time.perf_counter()
        R.batch([cubes_np[i] for i in c], p, np.float32)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res["cpu_restatement"] = dict(stats(cpu), label="CPU restatement (numpy, one process; not the reference's loader)",
                                  torch_threads=torch.get_num_threads(), omp_num_threads=os.environ.get("OMP_NUM_THREADS"))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
