#!/usr/bin/env python3
"""Timing of the Shepard's-loss ablation (`configs/CVPR_inverse_scaling_shepard.yaml`) on the configs[3] batch.

Default: rebuilds the training step of `bench.train_step_setup` (4 cubes of 128^3 cut from the benchmark frame, adaptive
bottleneck, offsets, inverse rescaling, STE) and reports
  * ShepardsLoss forward + backward alone (on the prediction of one training forward),
  * the full training step with `ColorLoss` and with `ShepardsLoss`, alternating in one process,
as one JSON line.  `--gather-only`: the interpolation gather alone with the benchmark frame as one batch (ground truth and
queries = the frame), for `rocprofv3 --kernel-trace --stats -- python tools/shepard_timing.py --gather-only`."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import unified_point_cloud_compression_amd.MinkowskiEngine as ME  # noqa: E402
from unified_point_cloud_compression_amd import sparse as S, synth  # noqa: E402
from unified_point_cloud_compression_amd.loss import Loss, ShepardsLoss  # noqa: E402
from unified_point_cloud_compression_amd.model import UnifiedModel  # noqa: E402

BASE_LOSS = {"Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
             "ColorLoss": {"type": "ColorLoss", "loss": "L2"},
             "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0},
             "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0}}
SHEPARD = {"type": "ShepardsLoss", "loss": "L2", "window_size": 9, "p": 8}


def setup(dev):
    cfg = copy.deepcopy(bench.R2_CONFIG)
    cfg["entropy_model"].update(adaptive_BN=True, quantization_offset=True, inverse_rescaling=True)
    torch.manual_seed(0)
    model = UnifiedModel(cfg).to(dev).train()
    pc = synth.surface_cloud(0, 10, shuffle=False)
    cubes = []
    for origin in ((512, 300, 500), (300, 512, 420), (640, 512, 600), (512, 512, 300)):
        o = np.array(origin)
        m = np.all((pc[:, :3] >= o) & (pc[:, :3] < o + 128), axis=1)
        if m.sum() >= 300:
            cubes.append(pc[m])
    coords, feats = ME.utils.sparse_collate([c[:, :3] - c[:, :3].min(0) for c in cubes], [c[:, 3:] for c in cubes])
    nb = len(cubes)
    q = torch.tensor([[0.4, 0.7]] * nb, device=dev)
    Lam = torch.tensor([[5.0, 400.0]] * nb, device=dev)
    opt = torch.optim.Adam([p for nme, p in model.named_parameters() if not nme.endswith(".quantiles")], lr=1e-4)
    opt_aux = torch.optim.Adam([p for nme, p in model.named_parameters() if nme.endswith(".quantiles")], lr=1e-3)
    coords, feats = coords.to(dev), feats.float().to(dev)

    def one(loss_fn):                                   # `bench.train_step_setup`'s step with the given loss
        opt.zero_grad(set_to_none=True)
        opt_aux.zero_grad(set_to_none=True)
        x = ME.SparseTensor(coordinates=coords, features=feats)
        out = model(x, q, Lam)
        total, _ = loss_fn(x, out)
        value = total.item()
        total.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        aux = model.aux_loss()
        aux.item()
        aux.backward()
        opt_aux.step()
        return value

    return model, coords, feats, q, Lam, one


def gather_only(dev, iters):
    pc = synth.surface_cloud(0, 10)
    c = torch.from_numpy(pc[:, :3]).to(dev)
    coords = torch.cat([torch.zeros((c.shape[0], 1), device=dev), c], dim=1)
    gt = ME.SparseTensor(coordinates=coords, features=torch.from_numpy(pc[:, 3:]).to(dev))
    loss = ShepardsLoss(dict(SHEPARD, id="ColorLoss"))
    cs = gt._cset
    feats = torch.cat([torch.ones((cs.n, 1), device=dev), gt._canonical_features()], dim=1).contiguous()
    w = loss._weights_on(dev)
    for _ in range(3):
        S.channelwise_gather(cs, feats, loss._taps, w, cs.keys, cs.n)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        S.channelwise_gather(cs, feats, loss._taps, w, cs.keys, cs.n)
    e1.record()
    torch.cuda.synchronize()
    return {"queries": cs.n, "taps": loss._taps.ntaps, "columns": loss._taps.ncol, "grid": bool(cs.grid()),
            "gather_ms_event": e0.elapsed_time(e1) / iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.gather_only:
        print(json.dumps(gather_only(dev, a.iters)))
        return
    model, coords, feats, q, Lam, one = setup(dev)
    # ---- loss alone: forward + backward on the prediction of one training forward
    x = ME.SparseTensor(coordinates=coords, features=feats)
    with torch.no_grad():
        out = model(x, q, Lam)
    pf = out["prediction"].F.detach().clone().requires_grad_(True)
    pred = ME.SparseTensor(coordinates=out["prediction"].C, features=pf)
    batch = {"prediction": pred, "q_map": Lam}
    shep = ShepardsLoss(dict(SHEPARD, id="ColorLoss"))
    for _ in range(5):
        shep(x, batch).backward()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.iters):
        shep(x, batch).backward()
    e1.record()
    torch.cuda.synchronize()
    loss_ms = e0.elapsed_time(e1) / a.iters
    loss_host_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    # ---- full step, ColorLoss and ShepardsLoss alternating
    fns = {"ColorLoss": Loss(copy.deepcopy(BASE_LOSS)),
           "ShepardsLoss": Loss(dict(copy.deepcopy(BASE_LOSS), ColorLoss=dict(SHEPARD)))}
    for _ in range(a.warmup):
        for f in fns.values():
            one(f)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.steps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one(f)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"points": int(coords.shape[0]), "prediction_rows": int(pred._cset.n),
                      "shepard_fwd_bwd_ms": round(loss_ms, 4), "shepard_fwd_bwd_host_ms": round(loss_host_ms, 4),
                      "step_ms_colorloss": round(med["ColorLoss"], 3), "step_ms_shepardsloss": round(med["ShepardsLoss"], 3),
                      "step_delta_ms": round(med["ShepardsLoss"] - med["ColorLoss"], 3),
                      "step_ms_all": {k: [round(v, 3) for v in vs] for k, vs in times.items()}}))


if __name__ == "__main__":
    main()
