#!/usr/bin/env python3
"""Timing of the training loop's optimiser half and of its whole step on the BASELINE configs[3] workload of `bench.py` (4 cubes of
128^3 cut from the benchmark frame, R2 width, adaptive bottleneck + offsets + inverse rescaling + STE), all in one run:

* optimiser half   clipping to 1.0 + the model optimiser's step + the bottleneck optimiser's step, three ways on the SAME
                   gradients (one backward pass of the benchmark step, cloned; restored before every repeat, outside the
                   timed window): torch default (`clip_grad_norm_` + foreach Adam), torch `fused=True` with `clip_grad_norm_`,
                   and `optim.FusedOptimizer` (clip inside the step).  Device events around each repeat, the three ways
                   alternating inside every round so that drift of the shared machine lands on all of them; median and spread
                   (min, 10th / 90th percentile, max) of the repeats after a warm-up.
* loop step        `train.Training.train_step` on that batch (host clock around work that ends in a synchronise, like
                   `bench.train_step_ms`), next to `bench.train_step_ms` itself -- `train_step_ms` and
                   `train_step_ms_fused_adam` as `python bench.py --full` reports them -- measured in this same run.  bench.py and
                   everything its step runs are the parent commit's, so those two are the parent's figures on this machine.
                   The loop's step reads nothing back; bench's step reads both losses every step, as the reference does.

One coupling to a file outside tools/, deliberate and loud when it breaks: the batch is taken out of the closure
`bench.train_step_setup` returns by the names of its free variables, as tools/data_timing.py does.

One JSON line; --out also writes it to a file (profiles/train_loop_timing.json)."""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "max_ms": float(a.max()), "repeats": int(a.size)}


def _closure(fn):
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


def optimiser_half(device, repeats, warmup):
    import bench
    from unified_point_cloud_compression_amd.optim import FusedOptimizer
    one, info = bench.train_step_setup(device)
    one()                                                # leaves the gradients of a full step in .grad
    model = _closure(one)["model"]
    named = list(model.named_parameters())
    is_q = [nme.endswith(".quantiles") for nme, _ in named]
    grads = [None if p.grad is None else p.grad.detach().clone() for _, p in named]

    def leaves():
        return [p.detach().clone().requires_grad_() for _, p in named]

    def split(ps):
        return [p for p, q in zip(ps, is_q) if not q], [p for p, q in zip(ps, is_q) if q]

    ways = {}
    for name, kw in (("torch_default", {}), ("torch_fused", {"fused": True})):
        ps = leaves()
        m, b = split(ps)
        opt, aux = torch.optim.Adam(m, lr=1e-4, **kw), torch.optim.Adam(b, lr=1e-3, **kw)

        def step(ps=ps, m=m, opt=opt, aux=aux):
            torch.nn.utils.clip_grad_norm_(m, 1.0)        # `train.py:224` (the quantiles have no gradient at that point)
            opt.step()
            aux.step()
        ways[name] = (ps, step)
    ps = leaves()
    m, b = split(ps)
    opt, aux = FusedOptimizer(m, lr=1e-4, max_norm=1.0), FusedOptimizer(b, lr=1e-3, max_norm=None)

    def step(opt=opt, aux=aux):
        opt.step()
        aux.step()
    ways["kernel"] = (ps, step)

    def restore(ps):                                     # clip_grad_norm_ rewrites the gradients: fresh copies every repeat
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()

    times = {k: [] for k in ways}
    for r in range(warmup + repeats):
        for name, (ps, step) in ways.items():
            restore(ps)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    out = {k: _stats(v) for k, v in times.items()}
    out["tensors"] = len(named)
    out["elements"] = int(sum(p.numel() for _, p in named))
    out["chunks"] = int(opt._n_chunks)
    # the three ways ran the same number of steps on the same gradients: their parameters must agree
    ref = ways["torch_default"][0]
    out["max_abs_difference_to_torch_default"] = {
        k: float(max((a.detach() - b.detach()).abs().max() for a, b in zip(ways[k][0], ref) if a.numel())) for k in ("torch_fused", "kernel")}
    return out, info


def loop_step(device, steps, warmup):
    import bench
    from unified_point_cloud_compression_amd import synth
    from unified_point_cloud_compression_amd.ply import write_ply
    from unified_point_cloud_compression_amd.train import Training
    import yaml
    one, _ = bench.train_step_setup(device)
    cv = _closure(one)
    cfg = copy.deepcopy(bench.R2_CONFIG)
    cfg["entropy_model"].update(adaptive_BN=True, quantization_offset=True, inverse_rescaling=True)
    loss_cfg = {"Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
                "ColorLoss": {"type": "ColorLoss", "loss": "L2"},
                "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0}, "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0}}
    with tempfile.TemporaryDirectory() as root:           # `Training` wants a dataset: one small frame; the timed batch is bench's
        os.makedirs(os.path.join(root, "raw", "synth"))
        os.makedirs(os.path.join(root, "dataset"))
        os.makedirs(os.path.join(root, "results"))
        write_ply(os.path.join(root, "raw", "synth", "synth_0000.ply"), torch.from_numpy(synth.surface_cloud(0, 6)).to(device))
        with open(os.path.join(root, "dataset", "config.yaml"), "w") as f:
            yaml.safe_dump({"info": {"cube_size": 128}, "train": {"synth": "0"}, "val": {}}, f)
        tr = Training({"experiment_name": "timing", "results_path": os.path.join(root, "results"), "model": cfg,
                       "data_path": os.path.join(root, "dataset"), "raw_data_path": os.path.join(root, "raw"),
                       "raw_loading": {"relative_paths": {"toy": "{sequence}/{sequence}_{frame_idx:04d}.ply"},
                                       "sequences": {"toy": {"synth": {"start": 0, "end": 0}}}},
                       "min_points_train": 0, "transforms": {"train": {}}, "device": str(device.index or 0), "epochs": 1, "batch_size": 4,
                       "q_map": {"lambda_A_min": 0, "lambda_A_max": 12800, "lambda_G_min": 0, "lambda_G_max": 200, "mode": "quadratic"},
                       "virtual_batches": False, "model_learning_rate": 1e-4, "bottleneck_learning_rate": 1e-3, "optimizer": "Adam",
                       "scheduler_step_size": 150, "scheduler_gamma": 0.1, "clip_grad_norm": 1.0, "loss": loss_cfg})
        tr.model.train()
        batch = (cv["coords"], cv["feats"], cv["q"], cv["Lam"])
        rounds = []
        for r in range(warmup):
            tr.train_step(*batch)
        for _ in range(5):                               # five windows of `steps` steps: their spread is the noise of the figure
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(steps):
                last = tr.train_step(*batch)
            torch.cuda.synchronize()
            rounds.append((time.time() - t0) / steps * 1e3)
        out = {"loop_train_step_ms": _stats(rounds), "steps_per_window": steps, "loss": float(last[0]), "aux_loss": float(last[2])}
    parent = bench.train_step_ms(device, steps=steps, warmup=warmup)
    out["bench_train_step_ms"] = parent["train_step_ms"]
    out["bench_train_step_ms_fused_adam"] = parent["train_step_ms_fused_adam"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_loop_timing.py measures on a GPU; none is visible (no fallback)")
    device = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["optimiser_half"], res["workload"] = optimiser_half(device, args.repeats, args.warmup)
    res.update(loop_step(device, args.steps, max(args.warmup, 6)))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
