#!/usr/bin/env python3
"""Multi-rate and rate-targeted encoding against one `compress` per quality point, on the benchmark's
frame and model (`bench.py`: synthetic vox10 surface, R2 width, seeded weights) with the reference's 11 x 11 grid of quality
pairs (`rate.q_grid()`).

Variants, taking turns inside every repetition (device-synchronised wall time, median of --reps after --warmup):
  a  121 x `compress`               the only way without this module: the yardstick
  b  `compress_multirate`           one analysis, 121 latent codings
  c  `rate_map`                     one analysis, one sweep launch, no latent coded
  d  `compress_to_size`             at a mid-grid budget (the median real size of the grid), with its `tries`
and the largest relative gap between `predicted_bytes` and the real bytes over the grid.  The benchmark's model has
adaptive_BN false -- q does not reach its latents and the 121 candidates are one and the same -- so the same frame is also run
with adaptive_BN true (the training benchmark's configuration), where the candidates differ.  Reported, nothing is gated."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from unified_point_cloud_compression_amd import lib as L, metrics, rate, synth  # noqa: E402


def build(device, adaptive):
    if not adaptive:
        return bench.build_model(device)
    from unified_point_cloud_compression_amd.MinkowskiEngine.modules import _ConvBase
    from unified_point_cloud_compression_amd.model import UnifiedModel
    torch.manual_seed(0)
    cfg = copy.deepcopy(bench.R2_CONFIG)
    cfg["entropy_model"].update(adaptive_BN=True, entropy_coder="pcc_streams")
    model = UnifiedModel(cfg)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, _ConvBase):
                m.kernel.mul_(3.0)
    model = model.to(device).eval()
    model.update()
    return model


def alternate(forms, warmup, reps):
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}


def run(device, pc, adaptive, warmup, reps):
    model = build(device, adaptive)
    qs = torch.from_numpy(rate.q_grid()).to(device)
    K = qs.shape[0]
    singles = [model.compress(pc, qs[i:i + 1]) for i in range(K)]
    real = [metrics.count_bits(s[0]) // 8 for s in singles]
    multi = model.compress_multirate(pc, qs)
    same = all(bytes(m[0][b][j][0]) == bytes(s[0][b][j][0]) for m, s in zip(multi, singles) for b in range(len(s[0])) for j in (0, 1))
    rm = model.rate_map(pc, qs)
    gaps = [abs(p - r) / r for p, r in zip(rm["predicted_bytes"], real)]
    budget = int(np.median(real))
    info = {}

    def to_size():
        info.update(model.compress_to_size(pc, budget, qs=qs)[1])

    forms = {"a_121_compress": lambda: [model.compress(pc, qs[i:i + 1]) for i in range(K)],
             "b_compress_multirate": lambda: model.compress_multirate(pc, qs),
             "c_rate_map": lambda: model.rate_map(pc, qs),
             "d_compress_to_size": to_size}
    res = {"adaptive_BN": adaptive, "candidates": K, "multirate_equals_singles": bool(same), "timing": alternate(forms, warmup, reps),
           "real_bytes_min": min(real), "real_bytes_max": max(real), "distinct_real_sizes": len(set(real)),
           "fixed_bytes": rm["fixed_bytes"], "largest_relative_gap_predicted_vs_real": max(gaps),
           "largest_gap_bytes": max(abs(p - r) for p, r in zip(rm["predicted_bytes"], real)),
           "compress_to_size": {"budget": budget, "index": info["index"], "bytes": info["bytes"], "predicted_bytes": info["predicted_bytes"],
                                "met": info["met"], "tries": info["tries"]}}
    t = res["timing"]
    print(f"adaptive_BN {adaptive}: a {t['a_121_compress']['median_ms']:.1f} ms, b {t['b_compress_multirate']['median_ms']:.1f} ms, "
          f"c {t['c_rate_map']['median_ms']:.2f} ms, d {t['d_compress_to_size']['median_ms']:.2f} ms ({info['tries']} tries, met {info['met']}); "
          f"real {min(real)}..{max(real)} bytes, largest gap {max(gaps):.3%}; multirate == singles: {same}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, default=bench.BITS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multirate_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multirate_timing.py needs a GPU")
    device = torch.device("cuda:0")
    pc = torch.from_numpy(synth.surface_cloud(seed=0, bits=args.bits)).to(device)
    doc = {"device": L.device_info()[1], "points": int(pc.shape[0]), "warmup": args.warmup, "reps": args.reps,
           "timer": "time.perf_counter around a device-synchronised call; variants alternate inside each repetition",
           "runs": [run(device, pc, adaptive, args.warmup, args.reps) for adaptive in (False, True)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
