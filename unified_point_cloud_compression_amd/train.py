"""The training loop: the reference's `train.py` (`Training`: `train`, `train_epoch`, `val_epoch`, `save_checkpoint`,
`load_checkpoint`, `check_resume`) on the device-side pieces of this package.

    python -m unified_point_cloud_compression_amd.train --config configs/CVPR_inverse_scaling.yaml

Config: the keys of the reference's `configs/CVPR_inverse_scaling.yaml` (`optimizer` "Adam" or "SGD"; `virtual_batches` must
be false; `device` the GPU index) plus
    raw_data_path   directory of the raw PLY frames            raw_loading   yaml in the reference's `raw_loading.yaml` format
    val_every       validate every this many epochs (10)       log_every     read the running sums every this many steps (50)
    seed            seeds both generators (0)
`data_path/config.yaml` is the reference's dataset description: `info.cube_size`, then `train` / `val` mapping a sequence to
a frame-spec string (`parse_frame_spec`).

What differs from the reference:
* data: a frame is read (`read_ply`), sliced into cubes on the GPU (`slice_into_cubes`) and kept there; there is no `.pt`
  cache (slicing is a few ms) and no loader processes (`TrainBatcher` assembles every batch with one kernel).
* one optimiser step is two launches (`optim.FusedOptimizer`): clipping happens inside the model optimiser's step, over the
  optimiser's own parameters -- the quantiles have no gradient at that point (`zero_grad` set it to None and the loss does
  not reach them), so this is the reference's clipping over `model.parameters()`.  The stored gradients keep their
  unclipped values.
* no `empty_cache()` and no per-step `.item()`: running sums stay on the device and are read every `log_every` steps and at
  the end of the epoch.
* randomness: quantisation noise from a device `torch.Generator` (installed as `entropy_model.noise_fn`), batches and the
  quality draw from a CPU generator, both seeded from `seed` (as is torch's global generator, for the initial weights); a
  checkpoint carries both states under `rng` (beside the reference's keys), so a resumed run draws the batches and the
  noise the uninterrupted run would have drawn.
* validation rows are written with the `csv` module (same columns as the reference's DataFrame, index column first).
  Renders of the validation point clouds are NOT built.
"""
import argparse
import csv
import os
import re

import torch
import yaml

from .lib import PccError

QA_FACTORS = {0: 1.0, 1: 2.0, 2: 4.0, 3: 8.0}            # `data/utils/RawLoader.py:50`
VAL_Q = (0.0, 1.0)                                       # `train.py:268-269`
_CKPT = re.compile(r"^ckpt_(\d{3,})\.pt$")


# ------------------------------------------------------------------------------------------------------------------
# pure helpers (no GPU)
# ------------------------------------------------------------------------------------------------------------------
def parse_frame_spec(spec):
    """`"3"`, `"0:5"` (end inclusive), `"0:20:5,31"` -> the frame indices, de-duplicated and ascending
    (`data/dataloader.py:247-275`).  Anything else raises ValueError."""
    if not isinstance(spec, str):
        raise ValueError(f"frame spec must be a string, got {spec!r}")
    frames = set()
    for item in spec.split(","):
        parts = [p.strip() for p in item.split(":")]
        if len(parts) > 3 or any(not re.fullmatch(r"\d+", p) for p in parts):
            raise ValueError(f"malformed frame spec {spec!r}: {item!r} is not 'i', 'a:b' or 'a:b:stride' of non-negative integers")
        v = [int(p) for p in parts]
        if len(v) == 1:
            frames.add(v[0])
            continue
        stride = v[2] if len(v) == 3 else 1
        if stride < 1 or v[1] < v[0]:
            raise ValueError(f"malformed frame spec {spec!r}: {item!r} has an empty range or a zero stride")
        frames.update(range(v[0], v[1] + 1, stride))
    return sorted(frames)


def parse_data_config(config):
    """The dict of `data_path/config.yaml` with every split's frame specs parsed: {"info": ..., split: {sequence: [frames]}}."""
    if "info" not in config or "cube_size" not in config["info"]:
        raise ValueError("dataset config lacks info.cube_size")
    out = {"info": dict(config["info"])}
    for split, seqs in config.items():
        if split != "info":
            out[split] = {seq: parse_frame_spec(spec) for seq, spec in (seqs or {}).items()}
    return out


def optimizer_mode(name):
    """"Adam" / "SGD" (`train.py:67-73`) -> the mode of `optim.FusedOptimizer`; anything else raises ValueError (the reference
    goes on without a model optimiser)."""
    modes = {"Adam": "adam", "SGD": "sgd"}
    if name not in modes:
        raise ValueError(f"optimizer must be 'Adam' or 'SGD', not {name!r}")
    return modes[name]


def check_config(config):
    """Everything that can be refused before a GPU is touched."""
    optimizer_mode(config["optimizer"])
    if config.get("virtual_batches"):
        raise ValueError("virtual_batches is not built: set it to false")
    for key in ("experiment_name", "results_path", "model", "data_path", "raw_data_path", "raw_loading", "min_points_train",
                "q_map", "epochs", "batch_size", "model_learning_rate", "bottleneck_learning_rate", "scheduler_step_size",
                "scheduler_gamma", "clip_grad_norm", "loss"):
        if key not in config:
            raise ValueError(f"config lacks {key!r}")
    for key in ("val_every", "log_every"):
        if int(config.get(key, 1)) < 1:
            raise ValueError(f"{key} must be at least 1")


def checkpoint_path(results_directory, epoch):
    return os.path.join(results_directory, "ckpts", "ckpt_{:03d}.pt".format(epoch))


def latest_checkpoint(results_directory):
    """Path of the checkpoint with the highest epoch number under `ckpts/`, or None.  (The reference sorts the names, which
    agrees up to epoch 999; other files in the directory are ignored.)"""
    folder = os.path.join(results_directory, "ckpts")
    if not os.path.isdir(folder):
        return None
    found = [(int(m.group(1)), name) for name in os.listdir(folder) for m in [_CKPT.match(name)] if m]
    return os.path.join(folder, max(found)[1]) if found else None


def lr_at_epoch(config, epoch):
    """The model learning rate during `epoch` (0-based) under StepLR: lr * gamma ** (epoch // step_size)."""
    return config["model_learning_rate"] * config["scheduler_gamma"] ** (epoch // config["scheduler_step_size"])


class RawFrames:
    """Where raw frames live (`data/utils/RawLoader.py`): `raw_loading` (a path or its dict) holds
    `relative_paths[dataset]` with `{sequence}` / `{frame_idx}` fields and `sequences[dataset][sequence]{start, end}`."""

    def __init__(self, raw_data_path, raw_loading):
        self.raw_data_path = raw_data_path
        if not isinstance(raw_loading, dict):
            with open(raw_loading, "r") as f:
                raw_loading = yaml.safe_load(f)
        self.config = raw_loading

    def dataset_of(self, sequence):
        for key, seqs in self.config["sequences"].items():
            if sequence in (seqs or {}):
                return key
        raise ValueError(f"sequence {sequence!r} is in no dataset of the raw_loading config")

    def path(self, sequence, frame_idx):
        key = self.dataset_of(sequence)
        rng = self.config["sequences"][key][sequence]
        if not rng["start"] <= frame_idx <= rng["end"]:
            raise ValueError(f"frame {frame_idx} of {sequence} is outside [{rng['start']}:{rng['end']}]")
        return os.path.join(self.raw_data_path, self.config["relative_paths"][key].format(sequence=sequence, frame_idx=frame_idx))

    def load(self, sequence, frame_idx, device):
        """The frame as a [N, 6] fp32 device tensor (xyz, rgb in [0, 1]); a `QA` frame down-scaled as the reference does."""
        from . import ply, voxelize
        cloud = ply.read_ply(self.path(sequence, frame_idx), device, normals=False).cloud
        if cloud.shape[1] != 6:
            raise PccError(f"{sequence} frame {frame_idx}: the PLY file has no colours")
        if self.dataset_of(sequence) == "QA":
            cloud = voxelize.downscale(cloud, QA_FACTORS[frame_idx])
        return cloud


# ------------------------------------------------------------------------------------------------------------------
# training
# ------------------------------------------------------------------------------------------------------------------
class Training:
    """Training class for unified geometry and colour compression (`train.py:43-350`)."""

    def __init__(self, config_or_path):
        self.load_config(config_or_path)
        check_config(self.config)
        self.setup_folders()
        from . import data
        from .loss import Loss
        from .model.model import UnifiedModel
        from .optim import FusedOptimizer
        cfg = self.config
        self.device = torch.device("cuda", int(cfg.get("device", 0)))
        torch.cuda.set_device(self.device)

        seed = int(cfg.get("seed", 0))
        torch.manual_seed(seed)                          # the initial weights (`train.py:29`)
        self.model = UnifiedModel(cfg["model"]).to(self.device)
        model_parameters = [p for n, p in self.model.named_parameters() if not n.endswith(".quantiles")]
        bottleneck_parameters = [p for n, p in self.model.named_parameters() if n.endswith(".quantiles")]
        self.model_optimizer = FusedOptimizer(model_parameters, lr=cfg["model_learning_rate"], mode=optimizer_mode(cfg["optimizer"]),
                                              momentum=0.9, max_norm=cfg["clip_grad_norm"])
        self.bottleneck_optimizer = FusedOptimizer(bottleneck_parameters, lr=cfg["bottleneck_learning_rate"], mode="adam",
                                                   max_norm=None)
        self.model_scheduler = torch.optim.lr_scheduler.StepLR(self.model_optimizer, step_size=cfg["scheduler_step_size"],
                                                               gamma=cfg["scheduler_gamma"])
        self.loss = Loss(cfg["loss"])

        self.batch_generator = torch.Generator().manual_seed(seed)                 # batches, transforms, the quality draw
        self.noise_generator = torch.Generator(self.device).manual_seed(seed)      # quantisation noise
        self.model.entropy_model.noise_fn = self._noise

        self.load_data()
        transforms = data.build_transforms((cfg.get("transforms") or {}).get("train"))
        self.batcher = data.TrainBatcher(self.train_table, cfg["batch_size"], min_points=cfg["min_points_train"],
                                         transforms=transforms, generator=self.batch_generator, shuffle=True)
        self.q_func = data.Q_Func(cfg["q_map"])
        self.val_every, self.log_every = int(cfg.get("val_every", 10)), int(cfg.get("log_every", 50))
        self.log = print

        self.results = []
        self.epoch = 0
        self.check_resume()

    def _noise(self, tag, like):
        return torch.empty_like(like).uniform_(-0.5, 0.5, generator=self.noise_generator)

    def load_config(self, config_or_path):
        if isinstance(config_or_path, dict):
            self.config = config_or_path
        else:
            with open(config_or_path, "r") as config_file:
                self.config = yaml.safe_load(config_file)

    def setup_folders(self):
        self.results_directory = os.path.join(self.config["results_path"], self.config["experiment_name"])
        os.makedirs(os.path.join(self.results_directory, "ckpts"), exist_ok=True)
        with open(os.path.join(self.results_directory, "config.yaml"), "w") as config_file:
            yaml.safe_dump(self.config, config_file)

    def load_data(self):
        """Training frames sliced into one device-resident cube table; validation frames kept whole."""
        from . import data
        cfg = self.config
        with open(os.path.join(cfg["data_path"], "config.yaml"), "r") as f:
            dcfg = parse_data_config(yaml.safe_load(f))
        raw = RawFrames(cfg["raw_data_path"], cfg["raw_loading"])
        cube_size = dcfg["info"]["cube_size"]
        tables = []
        for sequence, frames in dcfg.get("train", {}).items():
            for frame_idx in frames:
                cloud = raw.load(sequence, frame_idx, self.device)
                tables.append(data.slice_into_cubes(cloud[:, :3].contiguous(), cloud[:, 3:].contiguous(), cube_size))
        if not tables:
            raise ValueError("the dataset config names no training frame")
        self.train_table = data.CubeTable.concat(tables)
        self.val_frames = [(sequence, frame_idx, raw.load(sequence, frame_idx, self.device))
                           for sequence, frames in dcfg.get("val", {}).items() for frame_idx in frames]

    def check_resume(self):
        """Resume from the latest checkpoint of this experiment, if there is one."""
        path = latest_checkpoint(self.results_directory)
        if path is not None:
            self.load_checkpoint(path)

    # ---- training ----------------------------------------------------------------------------------------------------
    def train(self):
        path = os.path.join(self.results_directory, "weights.pt")
        for epoch in range(self.epoch, self.config["epochs"]):
            self.train_epoch(epoch)
            if (epoch + 1) % self.val_every == 0:
                self.val_epoch(epoch)
            self.model_scheduler.step()
            self.model.update()
            self.save_checkpoint(epoch + 1)
            torch.save(self.model.state_dict(), path)
        self.model.update()
        torch.save(self.model.state_dict(), path)

    def draw_q(self, n_cubes):
        """(q, Lambda) of one step: one (q_g, q_a) pair from the batch generator, broadcast over the batch."""
        return self.q_func(n_cubes, generator=self.batch_generator, device=self.device)

    def train_step(self, coords, feats, q, Lambda):
        """`train.py:196-234` for one batch; returns (loss, loss parts, aux loss) as device tensors, nothing read back."""
        import unified_point_cloud_compression_amd.MinkowskiEngine as ME
        self.model_optimizer.zero_grad()
        self.bottleneck_optimizer.zero_grad()
        x = ME.SparseTensor(features=feats, coordinates=coords, device=self.device)
        output = self.model(x, q, Lambda)
        loss_value, loss_dict = self.loss(x, output)
        loss_value.backward()
        self.model_optimizer.step()                      # clips to clip_grad_norm inside the step
        aux_loss = self.model.aux_loss()
        aux_loss.backward()
        self.bottleneck_optimizer.step()
        return loss_value.detach(), loss_dict, aux_loss.detach()

    def train_epoch(self, epoch):
        self.model.train()
        sums = torch.zeros(2, dtype=torch.float64, device=self.device)          # loss, aux loss: summed on the device
        steps, n_steps = 0, len(self.batcher)
        for coords, feats, info in self.batcher:
            q, Lambda = self.draw_q(len(info["cubes"]))
            loss_value, _, aux_loss = self.train_step(coords, feats, q, Lambda)
            sums += torch.stack([loss_value, aux_loss]).double()
            steps += 1
            if steps % self.log_every == 0 or steps == n_steps:
                loss_avg, aux_avg = (sums / steps).tolist()
                self.log("[Train] [{}: {:03d}/{:03d}] step {}/{} lr {:.2e} Loss {:.2e} Aux_Loss {:.2e}".format(
                    self.config["experiment_name"], epoch + 1, self.config["epochs"], steps, n_steps,
                    self.model_optimizer.param_groups[0]["lr"], loss_avg, aux_avg))
        return (sums / max(steps, 1)).tolist()

    # ---- validation --------------------------------------------------------------------------------------------------
    def val_epoch(self, epoch):
        """Every validation frame through compress -> decompress at the four corners of the quality square."""
        from . import metrics
        self.model.eval()
        self.model.update()
        with torch.no_grad():
            for sequence, frame_idx, source in self.val_frames:
                N = source.shape[0]
                for q_a in VAL_Q:
                    for q_g in VAL_Q:
                        Q_map = torch.tensor([[q_g, q_a]], device=self.device)
                        strings, shapes, k, coordinates, q_vals = self.model.compress(source, Q_map)
                        reconstruction = self.model.decompress(coordinates=coordinates, strings=strings, shape=shapes, k=k,
                                                               q_vals=q_vals)
                        results = dict(metrics.pointcloud_metrics(source, reconstruction))
                        results["bpp"] = metrics.count_bits(strings) / N
                        results["sequence"] = sequence
                        results["frameIdx"] = frame_idx
                        results["q_a"] = q_a
                        results["q_g"] = q_g
                        self.results.append(results)
        self.write_results()

    def write_results(self):
        """`val.csv`, rewritten whole: an index column, then every key in order of first appearance."""
        keys = []
        for row in self.results:
            keys += [k for k in row if k not in keys]
        with open(os.path.join(self.results_directory, "val.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow([""] + keys)
            for i, row in enumerate(self.results):
                w.writerow([i] + [row.get(k, "") for k in keys])

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def save_checkpoint(self, epoch):
        self.model.update()
        checkpoint = {
            "epoch": epoch,
            "results": self.results,
            "model": self.model.state_dict(),
            "model_optimizer": self.model_optimizer.state_dict(),
            "model_scheduler": self.model_scheduler.state_dict(),
            "bottleneck_optimizer": self.bottleneck_optimizer.state_dict(),
            "rng": {"batch": self.batch_generator.get_state(), "noise": self.noise_generator.get_state()},
        }
        torch.save(checkpoint, checkpoint_path(self.results_directory, epoch))

    def load_checkpoint(self, path):
        checkpoint = torch.load(path, map_location=self.device, weights_only=False)
        self.epoch = checkpoint["epoch"]
        self.results = checkpoint["results"]
        self.model.load_state_dict(checkpoint["model"])
        self.model_optimizer.load_state_dict(checkpoint["model_optimizer"])
        self.model_scheduler.load_state_dict(checkpoint["model_scheduler"])
        self.bottleneck_optimizer.load_state_dict(checkpoint["bottleneck_optimizer"])
        rng = checkpoint.get("rng")                      # absent in a checkpoint written by the reference
        if rng is not None:
            self.batch_generator.set_state(rng["batch"].cpu())
            self.noise_generator.set_state(rng["noise"].cpu())
        lr, want = self.model_optimizer.param_groups[0]["lr"], lr_at_epoch(self.config, self.epoch)
        if abs(lr - want) > 1e-9 * want:                 # the checkpoint's schedule wins; say so when the config moved
            self.log(f"[Resume] lr {lr:.3e} from {os.path.basename(path)}; this config's schedule gives {want:.3e} at epoch {self.epoch}")


def parse_options(argv=None):
    parser = argparse.ArgumentParser(description="Train the unified point-cloud codec on one GPU.")
    parser.add_argument("--config", type=str, required=True, help="Configuration for training")
    return parser.parse_args(argv)


def main(argv=None):
    Training(parse_options(argv).config).train()


if __name__ == "__main__":
    main()
