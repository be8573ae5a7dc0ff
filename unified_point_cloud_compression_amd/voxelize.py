"""Voxel-grid down-sampling with averaged attributes on the device: the step of the reference's data preparation that
merges the points of a cell (`data/utils/RawLoader.py:48-57`: Open3D's `voxel_down_sample(factor)`, then the division by
the factor and the rounding).  Everywhere else in this package points that share a cell are merged first-wins
(`sparse_quantize`, the `SparseTensor` constructor, `compress(scaling_factor=)`); here a cell keeps the MEAN of its points,
colours and whatever else the caller packs.

Arithmetic (restated by `tests/voxel_ref.py` in numpy float64):

* index     idx = floor((float64(p) - origin) / voxel_size) per axis: one fp64 subtraction, one true fp64 division.
* origin    `origin=None` is Open3D's rule, min_bound - voxel_size / 2 per axis: the minimum is exact (`torch.aminmax`
            of fp32 values), the subtraction is float64 on the host.
* order     voxels in ascending (ix, iy, iz) order; |idx| < 2^15 per axis (the 16-bit key fields of `pcc_cube_keys`).
* mean      fp64 sums of the fp32 values, one fp64 division by the count, rounded once to fp32.  No floating-point
            atomics; the order of the additions is a function of the row count and the run layout only, so equal inputs
            give equal bits on every run.  (`index_add_`, the usual torch route, sums fp32 with atomics.)
* normals   the plain mean, NOT renormalised.

UNPINNED: the origin rule, the plain mean of normals and the tie rule of `downscale` are restated from knowledge of
Open3D / numpy, not checked against Open3D (SURVEY section 8c's sense of the word).

The pipeline is `slice_into_cubes`' own: keys per point (`pcc_voxel_keys`), the stable `pcc_sort_keys` with its
permutation, `pcc_unique_sorted` for the run starts, then one reduction over the runs (`pcc_voxel_means`).  No CPU
fallback (`PccError` on CPU tensors); arguments are checked before the GPU is touched.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import lib as L

PccError = L.PccError

MAX_ATTRS, WAVE_RUN, SPLIT_RUN, TILE_ROWS = 32, 32, 2048, 1024      # PCC_VOXEL_* of include/pcc_hip.h
_stage_hook = None      # measurement only (tools/voxel_timing.py): called with a stage's name once the stage is queued

VoxelGrid = namedtuple("VoxelGrid", "index points attrs counts origin voxel_size")
VoxelGrid.__doc__ = """`index` [M, 3] int32 voxel indices in ascending (ix, iy, iz) order, `points` [M, 3] and `attrs` [M, c] fp32
means (`attrs` is None without attributes), `counts` [M] int32 points per voxel, `origin` (three floats) and `voxel_size`:
voxel idx covers origin + idx * voxel_size <= p < origin + (idx + 1) * voxel_size per axis."""


def _need_tensor(t, what):
    if not torch.is_tensor(t):
        raise PccError(f"{what}: tensor required, got {type(t).__name__}")


def _need_gpu(t, what):
    if not t.is_cuda:
        raise PccError(f"{what}: GPU tensor required (no CPU fallback)")


def _voxel_size(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise PccError(f"{what}: voxel size must be a number, got {v!r}") from None
    if not math.isfinite(v) or v <= 0.0:
        raise PccError(f"{what}: voxel size must be finite and positive, got {v}")
    return v


def _origin(origin, what):
    try:
        o = tuple(float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin))
    except (TypeError, ValueError):
        raise PccError(f"{what}: origin must be three numbers, got {origin!r}") from None
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise PccError(f"{what}: origin must be three finite numbers, got {origin!r}")
    return o


def _bounds(points, what):
    """(min [3], max [3]) as float64 numpy: the one host read of the bounds (exact: fp32 values compared, not rounded)."""
    lo, hi = torch.aminmax(points, dim=0)
    b = torch.stack([lo, hi]).cpu().numpy().astype(np.float64)
    if not np.all(np.isfinite(b)):
        raise PccError(f"{what}: a point is not finite")
    return b[0], b[1]


def _check_cloud(cloud, what, cols=(6,)):
    _need_tensor(cloud, what)
    if cloud.dim() != 2 or cloud.shape[1] not in cols:
        raise PccError(f"{what}: cloud must be [N, {' or '.join(str(c) for c in cols)}], got {tuple(cloud.shape)}")


def voxel_grid(points, attrs=None, voxel_size=1.0, origin=None):
    """The voxel grid of `points` [N, 3] with mean positions and mean `attrs` [N, c], 1 <= c <= 32 (colours, normals,
    anything packed into columns): a `VoxelGrid`.  `origin=None`: min_bound - voxel_size / 2 (see the module docstring).
    At most two small host reads: the bounds (only for origin=None), then the voxel count and the range flag together.
    N = 0 returns an empty grid without a launch.  PccError when a point is not finite or an index leaves [-2^15, 2^15)."""
    what = "voxel_grid"
    _need_tensor(points, what)
    if points.dim() != 2 or points.shape[1] != 3:
        raise PccError(f"{what}: points must be [N, 3], got {tuple(points.shape)}")
    c = 0
    if attrs is not None:
        _need_tensor(attrs, what)
        if attrs.dim() != 2 or attrs.shape[0] != points.shape[0] or not 1 <= attrs.shape[1] <= MAX_ATTRS:
            raise PccError(f"{what}: attrs must be [N, 1..{MAX_ATTRS}] with the points' N, got {tuple(attrs.shape)}")
        c = attrs.shape[1]
    vs = _voxel_size(voxel_size, what)
    if origin is not None:
        origin = _origin(origin, what)
    _need_gpu(points, what)                                # last of the checks: the others name what is wrong on any device
    if c:
        _need_gpu(attrs, what)
        if attrs.device != points.device:
            raise PccError(f"{what}: points and attrs are on different devices")
    n, dev = points.shape[0], points.device
    if n >= (1 << 31) - 2 * TILE_ROWS:
        raise PccError(f"{what}: {n} points are too many")
    if n == 0:
        e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)      # noqa: E731
        return VoxelGrid(e(0, 3, dt=torch.int32), e(0, 3), e(0, c) if c else None, e(0, dt=torch.int32),
                         origin or (0.0, 0.0, 0.0), vs)
    pts = points.to(torch.float32).contiguous()
    att = attrs.to(torch.float32).contiguous() if c else None
    if origin is None:
        lo, _ = _bounds(pts, what)
        origin = tuple(float(x) for x in lo - vs / 2)                  # float64 on the host
    with torch.cuda.device(dev):
        lib, st = L.load(), L.stream()
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        head = L.counter(2)                                   # [0] number of voxels, [1] (int32) a point outside the key range
        mark = _stage_hook or (lambda name: None)
        mark("start")
        L.call("pcc_voxel_keys", L.ptr(pts), n, origin[0], origin[1], origin[2], vs, L.ptr(keys), L.cptr(head) + 8, st)
        mark("keys")
        skeys = torch.empty(n, dtype=torch.int64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.pcc_sort_ws_bytes(n), dev)
        L.call("pcc_sort_keys", L.ptr(keys), n, (1 << 48) - 1, L.ptr(skeys), L.ptr(perm), L.ptr(ws), ws.numel(), st)
        mark("sort")
        ukeys = keys                                          # the unsorted keys are no longer needed
        first = torch.empty(n, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.pcc_unique_ws_bytes(n), dev)
        L.call("pcc_unique_sorted", L.ptr(skeys), n, L.ptr(ukeys), L.ptr(first), L.cptr(head), L.ptr(ws), ws.numel(), st)
        mark("unique")
        index = torch.empty((n, 3), dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        mean_p = torch.empty((n, 3), dtype=torch.float32, device=dev)
        mean_a = torch.empty((n, c), dtype=torch.float32, device=dev) if c else None
        ws = L.workspace(lib.pcc_voxel_means_ws_bytes(n, c), dev)
        L.call("pcc_voxel_means", L.ptr(pts), L.ptr(att), c, n, L.ptr(perm), L.ptr(ukeys), L.ptr(first), L.cptr(head),
               L.ptr(index), L.ptr(counts), L.ptr(mean_p), L.ptr(mean_a), L.ptr(ws), ws.numel(), st)
        mark("means")
        m, bad = L.read(head)
    if bad:
        raise PccError(f"{what}: a point is not finite or its voxel index does not fit 16 bits (voxel size {vs}, origin {origin})")
    return VoxelGrid(index[:m], mean_p[:m], mean_a[:m] if c else None, counts[:m], origin, vs)


def voxel_down_sample(cloud, voxel_size, normals=None, origin=None, return_counts=False):
    """Open3D's `PointCloud.voxel_down_sample(voxel_size)` for a cloud [N, 6] fp32 (xyz, rgb: the layout of `read_ply` and
    `compress`): [M, 6] with the mean position and the mean colour of every occupied voxel, in ascending voxel order.  With
    `normals` [N, 3] the result is `(cloud, normals)` and the normals are plain means, not renormalised; with
    `return_counts` the points per voxel [M] int32 come last."""
    what = "voxel_down_sample"
    _check_cloud(cloud, what)
    if normals is not None:
        _need_tensor(normals, what)
        if normals.shape != (cloud.shape[0], 3):
            raise PccError(f"{what}: normals must be [N, 3] with the cloud's N, got {tuple(normals.shape)}")
    _voxel_size(voxel_size, what)
    _need_gpu(cloud, what)
    attrs = cloud[:, 3:]
    if normals is not None:
        _need_gpu(normals, what)
        attrs = torch.cat([attrs.to(torch.float32), normals.to(torch.float32)], dim=1)
    g = voxel_grid(cloud[:, :3], attrs, voxel_size, origin)
    out = (torch.cat([g.points, g.attrs[:, :3]], dim=1),)
    if normals is not None:
        out += (g.attrs[:, 3:].contiguous(),)
    if return_counts:
        out += (g.counts,)
    return out[0] if len(out) == 1 else out


def downscale(cloud, factor):
    """The QA branch of the reference's `RawLoader` (`data/utils/RawLoader.py:48-57`) for a cloud [N, 6]:
    `voxel_down_sample(cloud, factor)`, then xyz divided by the factor in float64 and rounded half to even (`np.round`),
    colours kept.  Rounding can make rows collide (two neighbouring voxels' means may round to the same integer point): the
    reference leaves those duplicates to `sparse_quantize`, first wins, and so does this function -- hand the result to
    `compress` / `SparseTensor` as it is."""
    what = "downscale"
    _check_cloud(cloud, what)
    f = _voxel_size(factor, what)
    _need_gpu(cloud, what)
    out = voxel_down_sample(cloud, f)
    out[:, :3] = torch.round(out[:, :3].double() / f).to(torch.float32)     # torch.round: half to even
    return out


def voxelize(cloud, bits=None, voxel_size=None, origin=(0.0, 0.0, 0.0)):
    """A cloud [N, 6] (or [N, 3]) on a grid, as a codec wants it: `(vox, origin, voxel_size)` where `vox` [M, 6] (or [M, 3])
    holds the integer voxel indices as fp32 -- unique by construction, ascending -- and the mean colour of every voxel.
    Give exactly one of

    * `voxel_size`  cells of that size from `origin` (default the coordinate origin; None: the cloud's minimum per axis);
    * `bits`        a grid of 2^bits cells along the longest axis: `origin=None` is the cloud's minimum per axis, the
                    extent is the largest of max - origin over the axes (no point may lie below the origin), and
                    voxel_size = extent / 2^bits, then raised to the next float64 until floor(extent / voxel_size) <
                    2^bits -- the farthest point would otherwise open cell 2^bits; after the nudge it lands in the last
                    cell, 2^bits - 1.  A cloud without extent takes voxel_size 1.

    `devoxelize(vox, origin, voxel_size)` maps indices back to cell centres."""
    what = "voxelize"
    _check_cloud(cloud, what, cols=(3, 6))
    if (bits is None) == (voxel_size is None):
        raise PccError(f"{what}: give exactly one of bits and voxel_size")
    if bits is not None:
        if int(bits) != bits or not 1 <= int(bits) <= 15:
            raise PccError(f"{what}: bits must be an integer in 1..15, got {bits!r}")
    else:
        voxel_size = _voxel_size(voxel_size, what)
    if origin is not None:
        origin = _origin(origin, what)
    _need_gpu(cloud, what)
    cols = cloud.shape[1]
    if cloud.shape[0] == 0:
        return (torch.empty((0, cols), dtype=torch.float32, device=cloud.device), origin or (0.0, 0.0, 0.0),
                1.0 if voxel_size is None else voxel_size)
    pts = cloud[:, :3].to(torch.float32).contiguous()
    if bits is not None or origin is None:
        lo, hi = _bounds(pts, what)
        if origin is None:
            origin = tuple(float(x) for x in lo)
        if bits is not None:
            if np.any(lo < np.asarray(origin)):
                raise PccError(f"{what}: with bits no point may lie below the origin {origin}; the minimum is {tuple(lo)}")
            cells = 1 << int(bits)
            extent = float(np.max(hi - np.asarray(origin)))
            voxel_size = extent / cells if extent > 0 else 1.0
            while math.floor(extent / voxel_size) >= cells:
                voxel_size = float(np.nextafter(voxel_size, np.inf))
    g = voxel_grid(pts, cloud[:, 3:] if cols == 6 else None, voxel_size, origin)
    idx = g.index.to(torch.float32)
    return (torch.cat([idx, g.attrs], dim=1) if cols == 6 else idx), origin, voxel_size


def devoxelize(cloud, origin, voxel_size):
    """Voxel indices back to points: xyz = origin + (idx + 0.5) * voxel_size, the centre of every cell, evaluated in float64
    and rounded to fp32; further columns (colours) are kept.  `cloud`: what `voxelize` returned, or a decoded copy of it."""
    what = "devoxelize"
    _check_cloud(cloud, what, cols=(3, 6))
    vs, o = _voxel_size(voxel_size, what), _origin(origin, what)
    _need_gpu(cloud, what)
    out = cloud.to(torch.float32).clone()
    o = torch.tensor(o, dtype=torch.float64, device=cloud.device)
    out[:, :3] = (o + (cloud[:, :3].double() + 0.5) * vs).to(torch.float32)
    return out
