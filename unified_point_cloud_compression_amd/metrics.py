"""Rate / distortion figures the reference's harness reports (`evaluate.py:165-166`): the `PointCloudMetric` report
(`metrics/metric.py:6-188`) and bits per input point (`utils.py:471`, `utils.py:30-48`).

The nearest-neighbour association -- two Open3D KD-trees and a Python loop per point in the reference -- runs on the
GPU (`pcc_nn_sorted_x`); the per-point arithmetic after it is a handful of float64 tensor ops on the device.

The point-to-plane (D2) figures the reference reads back from MPEG `pc_error` (`utils.py:189-267`) use normals estimated
with a radius search (`evaluate.py:153`); `estimate_normals` computes them on the GPU (`pcc_normals_grid`)."""
import math

import torch

from . import lib as L
from . import sparse as S

_YUV = ((0.2126, 0.7152, 0.0722), (-0.1146, -0.3854, 0.5), (0.5, -0.4542, -0.0458))     # BT.709, `metric.py:179-181`


def _canonical_set(xyz, *rows):
    """Voxel cloud -> (its CoordSet at pitch 1, int32 xyz sorted by (x,y,z), [each of `rows` in the same order as float64,
    or None], the [N, 4] coordinates when the user rows were not already canonical, else None), duplicates dropped (first
    wins), like `remove_duplicated_points` at `metrics/metric.py:19-21`."""
    xyz = torch.as_tensor(xyz)
    if not xyz.is_cuda:
        raise L.PccError("metrics: GPU tensors required (no CPU fallback)")
    n = xyz.shape[0]
    coords = torch.cat([torch.zeros((n, 1), device=xyz.device, dtype=xyz.dtype), xyz[:, :3]], dim=1)
    cs, perm, keep = S.coordset_from_coords(coords, 1)
    pts = cs.coords()[:, 1:].contiguous()
    out = []
    for r in rows:
        if r is not None:
            r = torch.as_tensor(r, device=xyz.device)
            if r.shape[0] != n:
                raise L.PccError(f"metrics: {r.shape[0]} attribute rows for {n} points")
            if keep is not None:
                r = r[keep]
            if perm is not None:    # perm: canonical position -> row of the de-duplicated user-order tensor
                r = r[perm]
            r = r.to(torch.float64)
        out.append(r)
    return cs, pts, out, (coords if perm is not None or keep is not None else None)


def _canonical(xyz, rgb=None):
    """Voxel cloud -> (int32 xyz sorted by (x,y,z), rgb in the same order), duplicates dropped (first wins), like
    `remove_duplicated_points` at `metrics/metric.py:19-21`."""
    _, pts, (rgb,), _ = _canonical_set(xyz, rgb)
    return pts, rgb


def nearest(a_xyz, b_xyz_sorted):
    """For every row of a (int32 [n,3]) the squared distance to, and the row of, its nearest point of b (sorted by x)."""
    a = a_xyz.to(torch.int32).contiguous()
    b = b_xyz_sorted.to(torch.int32).contiguous()
    d2 = torch.empty(a.shape[0], dtype=torch.int64, device=a.device)
    nn = torch.empty(a.shape[0], dtype=torch.int32, device=a.device)
    L.call("pcc_nn_sorted_x", L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], L.ptr(d2), L.ptr(nn), L.stream())
    return d2, nn


NORMALS_MAX_RADIUS = 8.0


def _normals_lim(radius):
    """Largest integer |d|^2 inside a radius search of `radius` (strict dist^2 < r^2, as the FLANN / nanoflann radius result
    sets under Open3D's SearchRadius; an assumption, Open3D is not checked here): ceil(r^2) - 1."""
    r = float(radius)
    if not (0.0 < r <= NORMALS_MAX_RADIUS):
        raise L.PccError(f"estimate_normals: radius {radius} unsupported (0 < radius <= {NORMALS_MAX_RADIUS:g})")
    return math.ceil(r * r) - 1


def _set_normals(cs, radius, with_counts=False):
    """fp32 [n, 3] normals (and int32 [n] neighbourhood sizes) of a canonical pitch-1 set, in canonical order."""
    lim = _normals_lim(radius)
    normals = torch.empty((cs.n, 3), dtype=torch.float32, device=cs.device)
    counts = torch.empty(cs.n, dtype=torch.int32, device=cs.device) if with_counts else None
    if cs.n:
        bits, _, h = S.grid_args(cs.grid() if S.USE_GRID else None)
        L.call("pcc_normals_grid", L.ptr(cs.keys), cs.n, bits, h, lim, L.ptr(normals),
               L.ptr(counts) if counts is not None else None, L.stream())
    return normals, counts


def estimate_normals(xyz, radius=5.0, return_counts=False):
    """Unoriented normals of a voxel cloud by radius search: Open3D's `estimate_normals(KDTreeSearchParamRadius(radius))`
    as the reference calls it on the reconstruction (`evaluate.py:153`).  xyz: GPU [N, >= 3] voxel coordinates.

    The neighbourhood of a point is every point at squared distance < radius^2, itself included; the normal is the
    eigenvector of the smallest eigenvalue of the neighbourhood's covariance (exact integer moments, fp64 solve), flipped
    so that its largest-magnitude component is positive (Open3D leaves the sign open; D2 does not depend on it).  Fewer
    than 3 neighbours give (0, 0, 1).  0 < radius <= 8.  Returns float32 [N, 3] in the caller's row order (duplicate rows
    get the normal of their cell), and with return_counts also the neighbourhood sizes, int32 [N]."""
    _normals_lim(radius)                                  # (raises before any work)
    cs, _, _, coords = _canonical_set(xyz)
    normals, counts = _set_normals(cs, radius, return_counts)
    if coords is not None:                                # user row -> canonical row of its cell
        rows = torch.searchsorted(cs.keys[:cs.n], S.pack_keys(coords)[:coords.shape[0]])
        normals = normals[rows]
        counts = counts[rows] if counts is not None else None
    return (normals, counts) if return_counts else normals


# The reference rounds colours to k/255 (`metric.py:152-153`) and then truncates k/255*255 to uint8 (`metric.py:175`).
# Under IEEE double division that product truncates back to k for every 8-bit level (checked here), so the level IS k.
# (Dividing a GPU tensor by the scalar 255 multiplies by its reciprocal instead, which lands below k for some levels:
# the integer level is used directly rather than re-deriving it through that arithmetic.)
assert all(int(float(k) / 255.0 * 255.0) == k for k in range(256))


def rgb_to_yuv(rgb):
    """`convert_rgb_to_yuv(clip(round(rgb*255)/255, 0, 1))` (`metrics/metric.py:152-153,170-188`): 8-bit levels with
    the reference's truncation, BT.709, chroma + 0.5."""
    c = torch.round(rgb.to(torch.float64) * 255.0).clamp(0, 255).to(torch.float32)
    m = torch.tensor(_YUV, dtype=torch.float32, device=rgb.device)
    yuv = (c @ m.t()) / 255.0
    yuv[:, 1:] += 0.5
    return yuv


def _d2_mse(a_pts, b_pts, b_normals, nn):
    """Point-to-plane mse of a -> b: mean over a of ((a - b[nn]) . n_b[nn])^2, in float64 (`pc_error`'s D2 sums the
    squared projection over the axes, it is not divided by 3)."""
    if a_pts.shape[0] == 0:
        return math.nan
    nnl = nn.long()
    e = (a_pts.to(torch.float64) - b_pts[nnl].to(torch.float64))
    proj = (e * b_normals[nnl].to(torch.float64)).sum(dim=1)
    return float((proj * proj).mean())


def _d2_psnr(mse, resolution):
    return math.inf if mse == 0 else 10 * math.log10(3 * resolution ** 2 / mse)


def _one_direction(prefix, a_pts, a_rgb, b_pts, b_rgb, resolution, b_normals=None):
    d2, nn = nearest(a_pts, b_pts)
    if b_normals is not None:
        mse = _d2_mse(a_pts, b_pts, b_normals, nn)
        d2_keys = {prefix + "d2_mse": mse, prefix + "d2_psnr": _d2_psnr(mse, resolution)}
    l2 = d2.to(torch.float64) / 3.0                                  # mean over the three axes, `metric.py:121`
    r = {prefix + "mse": float(l2.mean()), prefix + "hausdorff": float(l2.max())}
    for k in ("mse", "hausdorff"):
        v = r[prefix + k]
        r[prefix + "psnr_" + k] = math.inf if v == 0 else 10 * math.log10(resolution ** 2 / v)
    if a_rgb is not None and b_rgb is not None:
        ya, yb = rgb_to_yuv(a_rgb), rgb_to_yuv(b_rgb[nn.long()])
        e = ((ya - yb) ** 2).to(torch.float64).mean(dim=0)
        for i, ch in enumerate("yuv"):
            r[prefix + ch + "_mse"] = float(e[i])
            r[prefix + ch + "_psnr"] = math.inf if e[i] == 0 else 10 * math.log10(1 / float(e[i]))
        m = float(e.mean())
        r[prefix + "yuv_mse"] = m
        r[prefix + "yuv_psnr"] = math.inf if m == 0 else 10 * math.log10(1 / m)
    if b_normals is not None:
        r.update(d2_keys)
    return r


def pointcloud_metrics(source, reconstruction, resolution=1023, point_to_plane=False, normal_radius=5.0, source_normals=None,
                       reconstruction_normals=None):
    """`PointCloudMetric(source, reconstruction, resolution).compute_pointcloud_metrics(drop_duplicates=True)`:
    source / reconstruction are [N, 3] or [N, 6] (xyz then rgb in [0,1]) GPU tensors of voxel coordinates.
    Ties between equidistant neighbours resolve to the smallest canonical row (a KD-tree's choice is unspecified).

    point_to_plane=True adds the D2 keys the reference parses from `pc_error` (`utils.py:248-252`):
    `AB_d2_mse` = mean over the points a of A of ((a - b) . n_b)^2, with b the same nearest neighbour as D1 and n_b the
    normal at b, a point of the target cloud B (MPEG D2; Tian et al., ICIP 2017); `AB_d2_psnr` = 10 log10(3 resolution^2 /
    AB_d2_mse); the same for `BA_`; `sym_d2_mse` = the max of the two directions and `sym_d2_psnr` the min -- `pc_error`'s
    symmetric rule, unlike the min-of-mse rule of the `sym_` D1 keys, which follow `PointCloudMetric`.  Three of these are
    restated, not checked against `pc_error` (not available here): the target cloud's normal, the squared projection summed
    over the axes with the factor 3 in the PSNR (the D1 `AB_mse` is the mean over the axes), and max for `sym_d2_mse`.
    Normals are estimated on both clouds with `estimate_normals(..., normal_radius)` (`evaluate.py:153`) unless given as
    source_normals / reconstruction_normals ([N, 3], in the caller's row order; a duplicate row's cell takes the normal
    of its first row).  With point_to_plane=False the result is exactly the D1 / colour report."""
    sa = torch.as_tensor(source)
    sb = torch.as_tensor(reconstruction)
    ca, a_pts, (a_rgb, a_nrm), _ = _canonical_set(sa[:, :3], sa[:, 3:6] if sa.shape[1] >= 6 else None,
                                                  source_normals if point_to_plane else None)
    cb, b_pts, (b_rgb, b_nrm), _ = _canonical_set(sb[:, :3], sb[:, 3:6] if sb.shape[1] >= 6 else None,
                                                  reconstruction_normals if point_to_plane else None)
    if point_to_plane:
        a_nrm = a_nrm if a_nrm is not None else _set_normals(ca, normal_radius)[0]
        b_nrm = b_nrm if b_nrm is not None else _set_normals(cb, normal_radius)[0]
    r = {}
    r.update(_one_direction("AB_", a_pts, a_rgb, b_pts, b_rgb, resolution, b_nrm))
    r.update(_one_direction("BA_", b_pts, b_rgb, a_pts, a_rgb, resolution, a_nrm))
    keys = ["mse", "hausdorff", "psnr_mse", "psnr_hausdorff"]
    if a_rgb is not None and b_rgb is not None:
        keys += [c + s for c in "yuv" for s in ("_mse", "_psnr")]
    for k in keys:                                                   # `metric.py:72-83`: min over the two directions
        r["sym_" + k] = min(r["AB_" + k], r["BA_" + k])
    if point_to_plane:                                               # `pc_error`: the worse direction
        r["sym_d2_mse"] = max(r["AB_d2_mse"], r["BA_d2_mse"])
        r["sym_d2_psnr"] = min(r["AB_d2_psnr"], r["BA_d2_psnr"])
    return r


def d1_psnr(a_xyz, b_xyz, resolution=1023):
    """Point-to-point geometry PSNR (`metrics/metric.py:113-119,74`): (A->B, B->A, symmetric = min)."""
    a, _ = _canonical(torch.as_tensor(a_xyz)[:, :3])
    b, _ = _canonical(torch.as_tensor(b_xyz)[:, :3])
    ab = _one_direction("", a, None, b, None, resolution)["psnr_mse"]
    ba = _one_direction("", b, None, a, None, resolution)["psnr_mse"]
    return ab, ba, min(ab, ba)


def d2_psnr(a_xyz, b_xyz, resolution=1023, radius=5.0):
    """Point-to-plane geometry PSNR (`pc_error` D2, see `pointcloud_metrics`), normals estimated on both clouds with
    `radius`: (A->B, B->A, symmetric = min)."""
    ca, a, _, _ = _canonical_set(torch.as_tensor(a_xyz)[:, :3])
    cb, b, _, _ = _canonical_set(torch.as_tensor(b_xyz)[:, :3])
    na, nb = _set_normals(ca, radius)[0], _set_normals(cb, radius)[0]
    ab = _d2_psnr(_d2_mse(a, b, nb, nearest(a, b)[1]), resolution)
    ba = _d2_psnr(_d2_mse(b, a, na, nearest(b, a)[1]), resolution)
    return ab, ba, min(ab, ba)


def count_bits(strings):
    """`utils.count_bits` (`utils.py:30-48`)."""
    return sum(count_bits(s) if isinstance(s, list) else len(s) * 8 for s in strings)
