"""Training losses: counterpart of the reference's `loss.py` (BASELINE config 4).

`Loss(config)(gt, pred)` with the reference's config keys: `BPPLoss` (`loss.py:63-81`), `ColorLoss` (`:84-111`),
`Multiscale_FocalLoss` (`:115-157`), `ShepardsLoss` (the colour-loss ablation `configs/CVPR_inverse_scaling_shepard.yaml`,
`:161-274`).  Coordinate membership tests use exact packed keys on the device (the reference flattens coordinates with
float-scaled weights and torch.isin).
"""
import math

import torch

from . import lib as L
from . import sparse as S

FUSED_FOCAL = True    # focal loss rows as one kernel per level (training step)


def _lookup_rows32(cset, query_keys, nq):
    rows = torch.empty(max(nq, 1), dtype=torch.int32, device=cset.device)
    if nq:
        L.call("pcc_lookup_rows", L.ptr(cset.keys), cset.n, L.ptr(query_keys), nq, L.ptr(rows), L.stream())
    return rows[:nq]


def _lookup_rows(cset, query_keys, nq):
    return _lookup_rows32(cset, query_keys, nq).long()


class BPPLoss:
    def __init__(self, config):
        self.weight, self.identifier, self.key = config["weight"], config["id"], config["key"]

    def __call__(self, gt, pred):
        lik = pred["likelihoods"][self.key]
        return (torch.log(lik).sum() / (-math.log(2) * gt.C.shape[0])) * self.weight


class ColorLoss:
    def __init__(self, config):
        self.identifier = config["id"]
        self.l2 = config["loss"] == "L2"

    def __call__(self, gt, pred):
        prediction, q_map = pred["prediction"], pred["q_map"]
        gcs, pcs = gt._cset, prediction._cset
        # The overlapping voxels are enumerated from the PREDICTION side: the ground-truth row of every decoded voxel (-1: none),
        # the ground-truth colours gathered (no gradient), the prediction's own rows used in place -- so the backward pass has no
        # scatter in it.  A 0/1 weight replaces boolean-mask indexing (which makes torch count the mask on the host, in both
        # directions).  Same pairs and weights as `loss.py:84-111`; mean over overlapping voxels x channels.
        rows = _lookup_rows(gcs, pcs.keys, pcs.n)
        ov = (rows >= 0).to(torch.float32).unsqueeze(1)
        gt_colors = gt._canonical_features().index_select(0, rows.clamp(min=0))
        pred_colors = prediction._canonical_features()
        batch = pcs.keys[:pcs.n] >> 48
        d = (gt_colors - pred_colors) * ov
        e = d * d if self.l2 else d.abs()
        return (e * q_map[batch, 1].unsqueeze(1)).sum() / (ov.sum() * gt_colors.shape[1])


class Multiscale_FocalLoss:
    def __init__(self, config):
        self.identifier, self.alpha, self.gamma = config["id"], config["alpha"], config["gamma"]

    def __call__(self, gt, pred):
        predictions, points, q_map = list(pred["occ_predictions"]), list(pred["points"]), pred["q_map"]
        predictions.reverse()
        points.reverse()
        loss = 0.0
        for prediction, coords in zip(predictions, points):
            pcs, gcs = prediction._cset, coords._cset
            logit = prediction._canonical_features()[:, 0]
            if FUSED_FOCAL and logit.is_cuda and pcs.n > 0:        # one kernel + one sum per level (`autograd.FocalRowsFn`)
                from .autograd import FocalRowsFn
                occ_row = _lookup_rows32(gcs, pcs.keys, pcs.n)
                loss = loss + FocalRowsFn.apply(logit, occ_row, pcs.keys, q_map, self.alpha, self.gamma) / pcs.n
                continue
            occ = _lookup_rows(gcs, pcs.keys, pcs.n) >= 0           # predicted voxel is occupied in the ground truth
            p = torch.sigmoid(prediction._canonical_features()[:, 0])
            pt = torch.clip(torch.where(occ, p, 1 - p), 1e-2, 1)
            alpha = torch.where(occ, self.alpha, 1 - self.alpha)
            focal = -alpha * (1 - pt) ** self.gamma * torch.log(pt)
            batch = pcs.keys[:pcs.n] >> 48
            loss = loss + (focal * q_map[batch, 0]).mean()
        return loss


class ShepardsLoss:
    """Colour loss against the ground truth interpolated onto the predicted voxels by inverse-distance weighting over a ball
    (`loss.py:161-274`).  The window is built exactly as `create_window_3D`; it is constant, so its non-zero taps (257 of 729
    for window_size 9, p = 8) and their column table are computed once, here.  The interpolation is ONE gather kernel
    (`sparse.channelwise_gather`, `pcc_chconv_fwd`) with the ground-truth set as input, features [1 | gt.F] and the predicted
    keys as queries: the reference's combined tensor has zero features off the ground truth, so its window sum over the union
    set equals this sum over ground-truth voxels of the same batch (no union set is built).  Zero taps are skipped, which gives
    the same result for finite ground-truth features."""

    def __init__(self, config):
        self.identifier = config["id"]
        if config["loss"] not in ("L1", "L2"):
            raise L.PccError(f"ShepardsLoss: loss {config['loss']!r} is neither L1 nor L2")
        self.l2 = config["loss"] == "L2"
        self.p = config["p"]
        self.window_size = config["window_size"]
        ks = int(self.window_size)
        if ks < 1 or ks % 2 == 0 or ks > 9:
            raise L.PccError(f"ShepardsLoss: window_size {ks} unsupported (odd, at most 9)")
        self.window = self.create_window_3D(self.window_size)
        self.conv_sum = self._init_minkowski_conv(4, self.window_size, self.window)
        w = self.window.view(-1)
        nz = torch.nonzero(w)[:, 0].tolist()                  # x-fastest offset ids of the non-zero taps (host, once)
        r = ks // 2
        self._taps = S.ChannelwiseTaps([(k % ks - r, (k // ks) % ks - r, k // (ks * ks) - r) for k in nz], ks)
        self._weights = w[nz].reshape(-1, 1).contiguous()      # [T, 1] float32
        self._dev_weights = {}

    def _init_minkowski_conv(self, in_channels, kernel_size, kernel):
        from .MinkowskiEngine.modules import MinkowskiChannelwiseConvolution
        conv = MinkowskiChannelwiseConvolution(in_channels=in_channels, kernel_size=kernel_size, stride=1, dimension=3)
        conv.kernel = torch.nn.Parameter(kernel)
        conv.kernel.requires_grad = False
        return conv

    def create_window_3D(self, window_size):
        """`loss.py:192-219`: 1 / (d^p + 1e-5) over the (window_size)^3 cube, zero where d > window_size // 2; [K, 1] float32,
        x fastest."""
        radius = window_size // 2
        z, y, x = torch.meshgrid(torch.arange(window_size) - radius, torch.arange(window_size) - radius,
                                 torch.arange(window_size) - radius, indexing="ij")
        distance = torch.sqrt(x ** 2 + y ** 2 + z ** 2)
        window = 1 / (distance ** self.p + 1e-5)
        window[distance > radius] = 0
        return window.view(-1, 1)

    def _weights_on(self, device):
        w = self._dev_weights.get(str(device))
        if w is None:
            w = self._dev_weights[str(device)] = self._weights.to(device)
        return w

    def _gt_on_pred(self, gt, prediction):
        """Ground-truth features at the predicted voxels in the prediction's canonical row order: the voxel's own colour where
        the ground truth has it, else the inverse-distance-weighted mean over the window (0/0 = NaN when the ball is empty)."""
        gcs, pcs = gt._cset, prediction._cset
        gf = gt._canonical_features().detach()
        feats = torch.cat([torch.ones((gf.shape[0], 1), dtype=torch.float32, device=gf.device), gf.to(torch.float32)], dim=1)
        acc = S.channelwise_gather(gcs, feats, self._taps, self._weights_on(gf.device), pcs.keys, pcs.n)
        rows = _lookup_rows(gcs, pcs.keys, pcs.n)
        own = gf.index_select(0, rows.clamp(min=0))
        return torch.where((rows >= 0).unsqueeze(1), own, acc[:, 1:] / acc[:, :1])

    def interpolate_gt_to_pred(self, gt, prediction, interpolate_q_map=False):
        """`loss.py:236-273`: a SparseTensor on the prediction's coordinates carrying the interpolated ground truth."""
        want = 2 if interpolate_q_map else 3
        if gt.F.shape[1] != want:
            raise L.PccError(f"interpolate_gt_to_pred: ground truth has {gt.F.shape[1]} channels, expected {want}")
        return prediction._like(self._gt_on_pred(gt, prediction))

    def __call__(self, gt, pred):
        # Rows whose interpolation is not finite are dropped by `torch.where` on the difference (no boolean-mask indexing, no
        # host read), so a non-finite prediction in such a row reaches neither the value nor the gradient (`loss.py:226-232`).
        prediction, q_map = pred["prediction"], pred["q_map"]
        pcs = prediction._cset
        gt_on_pred = self._gt_on_pred(gt, prediction)
        pred_colors = prediction._canonical_features()
        valid = torch.isfinite(gt_on_pred).all(dim=1, keepdim=True)
        d = torch.where(valid, gt_on_pred - pred_colors, 0.0)
        e = d * d if self.l2 else d.abs()
        batch = pcs.keys[:pcs.n] >> 48
        return (e * q_map[batch, 1].unsqueeze(1)).sum() / (valid.sum() * gt_on_pred.shape[1])


class Loss:
    def __init__(self, config):
        self.losses = {}
        for ident, setting in config.items():
            setting = dict(setting, id=ident)
            kind = setting["type"]
            if kind == "BPPLoss":
                self.losses[ident] = BPPLoss(setting)
            elif kind == "ColorLoss":
                self.losses[ident] = ColorLoss(setting)
            elif kind == "Multiscale_FocalLoss":
                self.losses[ident] = Multiscale_FocalLoss(setting)
            elif kind == "ShepardsLoss":
                self.losses[ident] = ShepardsLoss(setting)
            else:
                raise L.PccError(f"loss {kind!r} is out of scope (ablation only)")

    def __call__(self, gt, pred):
        total, parts = 0, {}
        for loss in self.losses.values():
            item = loss(gt, pred)
            parts[loss.identifier] = item
            total = total + item
        return total, parts
