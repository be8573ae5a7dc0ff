"""Rate / distortion figures the reference's harness reports (`evaluate.py:165-166`): the `PointCloudMetric` report
(`metrics/metric.py:6-188`) and bits per input point (`utils.py:471`, `utils.py:30-48`).

The nearest-neighbour association -- two Open3D KD-trees and a Python loop per point in the reference -- runs on the
GPU (`pcc_nn_sorted_x`); the per-point arithmetic after it is a handful of float64 tensor ops on the device.

The point-to-plane (D2) figures the reference reads back from MPEG `pc_error` (`utils.py:189-267`) use normals estimated
with a radius search (`evaluate.py:153`); `estimate_normals` computes them on the GPU (`pcc_normals_grid`).

PCQM, which the reference reads back from another external binary (`utils.py:270-322`), is restated on the voxel lattice:
`pcqm` / `pcqm_features` (`pcc_curvature_grid`, `pcc_pcqm_features`)."""
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


# ---- PCQM -----------------------------------------------------------------------------------------------------------------
# Constants of the published metric (Meynet, Nehme, Digne, Lavoue, "PCQM: a full-reference quality metric for colored 3D
# point clouds", QoMEX 2020), restated from the paper.  The binary the reference shells out to (`utils.py:270-322`) and its
# source are not available here, so none of them is read from it: they are unpinned.
PCQM_MAX_RADIUS = 17.0                                   # of h; a z field of the feature kernel is then <= 33 bits
PCQM_RADIUS_FRACTION = 0.004                             # the reference's `-r 0.004`
PCQM_RADIUS_FACTOR = 2.0                                 # the reference's `-rx 2.0`
PCQM_K, PCQM_C1, PCQM_C2, PCQM_C3, PCQM_C4, PCQM_C5 = 1.0, 0.002, 0.1, 0.1, 0.002, 0.008    # (pcc_pcqm.hip holds the same)
PCQM_WEIGHTS = {"f3": 0.0057, "f4": 0.9771, "f6": 0.0172}
_SRGB_TO_XYZ = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))
_D65_WHITE = (0.95047, 1.0, 1.08883)


def rgb_to_lab(rgb):
    """8-bit levels round(rgb * 255) (clamped) -> CIE Lab, float64 [n, 3]: sRGB -> linear (0.04045 / 12.92 / 2.4 form) ->
    XYZ (D65) -> Lab with white (0.95047, 1, 1.08883)."""
    c = torch.round(rgb.to(torch.float64) * 255.0).clamp(0, 255) / 255.0
    lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    xyz = lin @ torch.tensor(_SRGB_TO_XYZ, dtype=torch.float64, device=rgb.device).t()
    t = xyz / torch.tensor(_D65_WHITE, dtype=torch.float64, device=rgb.device)
    f = torch.where(t > (6.0 / 29.0) ** 3, t.clamp_min(0).pow(1.0 / 3.0), t / (3.0 * (6.0 / 29.0) ** 2) + 4.0 / 29.0)
    return torch.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], dim=1)


def _pcqm_radii(radius, radius_fraction, radius_factor, extent=None):
    """(r, h) of a PCQM call, checked: 0 < r <= h <= 17.  radius None: r = radius_fraction x extent."""
    r = float(radius) if radius is not None else float(radius_fraction) * float(extent)
    h = float(radius_factor) * r
    if not (0.0 < r <= h <= PCQM_MAX_RADIUS):                      # (also refuses NaN)
        raise L.PccError(f"pcqm: radii r = {r:g}, h = {h:g} unsupported (0 < r <= h <= {PCQM_MAX_RADIUS:g})")
    return r, h


def _pcqm_lim(radius):
    """The integer neighbourhood rule of `estimate_normals`: |d|^2 <= ceil(radius^2) - 1."""
    return math.ceil(radius * radius) - 1


def _set_curvature(cs, radius):
    """float64 [n]: the curvature field of a canonical pitch-1 set at `radius`, in canonical order (`pcc_curvature_grid`)."""
    out = torch.empty(cs.n, dtype=torch.float64, device=cs.device)
    if cs.n:
        L.call("pcc_curvature_grid", L.ptr(cs.keys), cs.n, *S.grid_args(cs.grid() if S.USE_GRID else None),
               _pcqm_lim(radius), L.ptr(out), L.stream())
    return out


def curvature(xyz, radius):
    """The curvature field PCQM compares (step 1 of `pcqm_features`): float64 [N] in the caller's row order, a duplicate
    row taking the value of its cell.  xyz: GPU [N, >= 3] voxel coordinates; 0 < radius <= 17."""
    _pcqm_radii(radius, None, 1.0)
    cs, _, _, coords = _canonical_set(torch.as_tensor(xyz)[:, :3])
    rho = _set_curvature(cs, float(radius))
    if coords is not None:
        rho = rho[torch.searchsorted(cs.keys[:cs.n], S.pack_keys(coords)[:coords.shape[0]])]
    return rho


def pcqm_features(source, reconstruction, radius=None, radius_fraction=PCQM_RADIUS_FRACTION, radius_factor=PCQM_RADIUS_FACTOR,
                  per_point=False):
    """PCQM (Meynet, Nehme, Digne, Lavoue, QoMEX 2020) of a reconstruction D against its source R, the figure the
    reference's evaluation prints first (`evaluate.py:168-171`), with its eight features.  source / reconstruction: GPU
    [N, 6] tensors, voxel xyz then rgb in [0, 1]; duplicates are dropped, the first row of a cell wins.

    This is the published metric RESTATED on a voxel lattice, not the binary the reference calls (`utils.py:270-322`), which
    is not available here: the constants and weights below are taken from the paper, not read from that binary, and so are
    unpinned; a figure of this function is not comparable digit for digit with one the reference printed.

    r = `radius` in voxels when given, else radius_fraction x the largest extent of R's bounding box (the reference's
    `-r 0.004`); h = radius_factor x r (`-rx 2.0`); 0 < r <= h <= 17, else PccError.  All neighbourhoods follow the integer
    rule of `estimate_normals`: the offsets d with |d|^2 <= ceil(rho^2) - 1, the centre included.
      1. Curvature field of each cloud over N(q, r): the normal of `estimate_normals` kept in fp64; in-plane axes u =
         normalise(e x n), e the axis where |n| is smallest (first on a tie), v = n x u; an unweighted least-squares fit of
         z = a x^2 + b xy + c y^2 + d x + e y + f to the offsets in that frame (6 x 6 normal equations in fp64, summed in
         the order dx, dy, dz ascending, Cholesky); the value is |((1 + e^2) a - d e b + (1 + d^2) c) / (1 + d^2 + e^2)^1.5|,
         the absolute mean curvature of the fitted surface at q's foot, and 0 with fewer than 6 neighbours or a pivot
         <= 1e-12 x the largest diagonal entry.
      2. Correspondence: nn(q) = the nearest point of D to q (`nearest`, ties to the smallest canonical row).  A DEPARTURE
         from the published method, which projects q onto a quadric fitted to D: on a lattice the distorted samples are
         lattice points, so the nearest one stands for the projection.
      3. Colour: `rgb_to_lab` of the 8-bit levels.
      4. Per point q of R the pairs (R's value at q, D's value at nn(q)) of curvature, L, a, b and C = hypot(a, b).
      5. At every point p of R, over N_R(p, h) with weights exp(-|d|^2 / (2 sigma^2)), sigma = h / 2: means, standard
         deviations (variance clamped at 0) and covariance of the curvature and L pairs, means of the a, b, C pairs (every
         attribute shifted by p's own value before it is summed; `pcc_pcqm_features`).
      6. f1 = |mu_R - mu_D| / (max(mu_R, mu_D) + k), f2 the same of sigma, f3 = |sigma_R sigma_D - sigma_RD| /
         (sigma_R sigma_D + k) on curvature; f4 = 1 - 1 / (c1 (muL_R - muL_D)^2 + 1), f5 = 1 - (2 sL_R sL_D + c2) /
         (sL_R^2 + sL_D^2 + c2), f6 = 1 - (sL_RD + c3) / (sL_R sL_D + c3) on lightness; f7 = 1 - 1 / (c4 dC^2 + 1),
         f8 = 1 - 1 / (c5 dH^2 + 1), dH^2 = max(0, da^2 + db^2 - dC^2) on the chroma means.
      7. Each feature is averaged over R's points; PCQM = 0.0057 f3 + 0.9771 f4 + 0.0172 f6.
    Not covered: a symmetric variant, float positions.

    Returns {"pcqm", "f1" .. "f8", "r", "h", "n"}; with per_point also "features", float64 [N, 8] in the caller's row order
    of R (a duplicate row takes the values of its cell)."""
    if radius is not None:
        _pcqm_radii(radius, radius_fraction, radius_factor)          # (raises before any work)
    sa, sb = torch.as_tensor(source), torch.as_tensor(reconstruction)
    if sa.dim() != 2 or sb.dim() != 2 or sa.shape[1] < 6 or sb.shape[1] < 6:
        raise L.PccError("pcqm: both clouds need colour ([N, 6]: voxel xyz, then rgb in [0, 1])")
    if sa.shape[0] == 0 or sb.shape[0] == 0:
        raise L.PccError("pcqm: empty cloud")
    if not (sa.is_cuda and sb.is_cuda):
        raise L.PccError("pcqm: GPU tensors required (no CPU fallback)")
    ca, a_pts, (a_rgb,), a_coords = _canonical_set(sa[:, :3], sa[:, 3:6])
    cb, b_pts, (b_rgb,), _ = _canonical_set(sb[:, :3], sb[:, 3:6])
    extent = None
    if radius is None:
        extent = int((a_pts.max(dim=0).values - a_pts.min(dim=0).values).max())
    r, h = _pcqm_radii(radius, radius_fraction, radius_factor, extent)
    nn = nearest(a_pts, b_pts)[1].long()
    lab_a, lab_b = rgb_to_lab(a_rgb), rgb_to_lab(b_rgb)[nn]
    table = torch.stack([_set_curvature(ca, r), _set_curvature(cb, r)[nn], lab_a[:, 0], lab_b[:, 0], lab_a[:, 1], lab_b[:, 1],
                         lab_a[:, 2], lab_b[:, 2], torch.hypot(lab_a[:, 1], lab_a[:, 2]), torch.hypot(lab_b[:, 1], lab_b[:, 2])],
                        dim=1).contiguous()
    feats = torch.empty((ca.n, 8), dtype=torch.float64, device=table.device)
    L.call("pcc_pcqm_features", L.ptr(ca.keys), ca.n, *S.grid_args(ca.grid() if S.USE_GRID else None), _pcqm_lim(h),
           2.0 / (h * h), L.ptr(table), L.ptr(feats), L.stream())
    means = feats.mean(dim=0).tolist()
    out = {"f%d" % (k + 1): means[k] for k in range(8)}
    out["pcqm"] = sum(w * out[f] for f, w in PCQM_WEIGHTS.items())
    out.update(r=r, h=h, n=ca.n)
    if per_point:
        if a_coords is not None:
            feats = feats[torch.searchsorted(ca.keys[:ca.n], S.pack_keys(a_coords)[:a_coords.shape[0]])]
        out["features"] = feats
    return out


def pcqm(source, reconstruction, radius=None, radius_fraction=PCQM_RADIUS_FRACTION, radius_factor=PCQM_RADIUS_FACTOR):
    """The PCQM score of `pcqm_features` (0 = identical; larger = worse)."""
    return pcqm_features(source, reconstruction, radius, radius_fraction, radius_factor)["pcqm"]


def count_bits(strings):
    """`utils.count_bits` (`utils.py:30-48`)."""
    return sum(count_bits(s) if isinstance(s, list) else len(s) * 8 for s in strings)
