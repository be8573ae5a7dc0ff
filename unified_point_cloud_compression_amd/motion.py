"""Global motion of the inter-frame coders: `RigidTransform`, `warp_cloud`, `estimate_rigid` (DESIGN.md section 7e "Global
motion").

One transform per frame takes the reference cloud onto the current frame before the block motion of the inter coders looks at
it.  The decoder repeats the warp, so the warp is integers only: T = (M, t), M[3][3] in Q24 and t[3] in Q8 voxels, and a voxel p
goes to

    q_i = (sum_j M_ij p_j + (t_i << 16) + 2^23) >> 24            (int64, the shift floors)

(`pcc_motion_warp`).  A voxel that leaves the range a coordinate set holds is dropped.  Several sources may land in one cell:
the warped cloud is the set of distinct cells, and a cell carries the attributes of the source of lowest canonical rank -- a
stable sort of the warped keys with the canonical row as payload and the first row of every run (`pcc_sort_keys`,
`pcc_unique_sorted`, `pcc_motion_gather`), never arrival order.

The estimator runs on the encoder only and may be as approximate as it likes -- the transform travels in the stream.  It is a
plain point-to-plane ICP in fp64: every iteration is one `pcc_motion_icp_terms` launch over the reference voxels (nearest
current voxel inside `radius` through the current frame's grid index, the current frame's `pcc_normals_grid` normals) and one
read of 29 sums; the 6 x 6 solve is numpy on the host.  It is a local method: what is left of the motion once the centroids are
aligned has to lie inside `radius`.
"""
import ctypes as C
import struct

import numpy as np
import torch

from . import lib as L
from . import sparse as S

MAX_M = 1 << 25           # |M_ij| <= 2^25 (Q24: entries up to 2 in magnitude)
MAX_T = 1 << 24           # |t_i| < 2^24 (Q8: 65536 voxels)
ONE = 1 << 24
MAX_ATTRS = 8
MAX_RADIUS = 4.0
N_SUMS = 29
RIDGE = 1e-9
PACKED = struct.Struct("<12i")
LO, HI = -S.BIAS + 64, S.BIAS - 64        # a coordinate set holds coordinates in [LO, HI) (`sparse.Bounds`)
DROPPED = (1 << 63) - 1                   # PCC_MOTION_DROPPED


class RigidTransform:
    """The 12 integers of a global motion: M (3 x 3, Q24) and t (3, Q8 voxels).  Not necessarily a rotation: any matrix within
    the ranges is a valid transform, the warp is defined for all of them."""

    __slots__ = ("M", "t")

    def __init__(self, M, t):
        M = [int(v) for row in M for v in (row if hasattr(row, "__len__") else [row])]
        t = [int(v) for v in t]
        if len(M) != 9 or len(t) != 3:
            raise L.PccError("RigidTransform: a 3 x 3 matrix and 3 translation entries are required")
        if any(abs(v) > MAX_M for v in M):
            raise L.PccError(f"RigidTransform: a matrix entry outside +-2^25 (Q24): {M}")
        if any(abs(v) >= MAX_T for v in t):
            raise L.PccError(f"RigidTransform: a translation entry outside +-2^24 (Q8 voxels): {t}")
        self.M = tuple(tuple(M[3 * i:3 * i + 3]) for i in range(3))
        self.t = tuple(t)

    @classmethod
    def identity(cls):
        return cls([[ONE, 0, 0], [0, ONE, 0], [0, 0, ONE]], [0, 0, 0])

    @classmethod
    def from_float(cls, R, t):
        """Quantise a float matrix and translation (voxels): round half up, floor(v * 2^q + 0.5)."""
        R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            raise L.PccError("RigidTransform: the transform is not finite")
        return cls(np.floor(R * float(ONE) + 0.5).astype(np.int64).tolist(), np.floor(t * 256.0 + 0.5).astype(np.int64).tolist())

    def ints(self):
        return [v for row in self.M for v in row] + list(self.t)

    def is_identity(self):
        return self.ints() == RigidTransform.identity().ints()

    def pack(self):
        """48 bytes: the 12 integers as little-endian int32, M row by row, then t."""
        return PACKED.pack(*self.ints())

    @classmethod
    def unpack(cls, data):
        if len(data) != PACKED.size:
            raise L.PccError(f"RigidTransform: {len(data)} bytes, a packed transform has {PACKED.size}")
        v = PACKED.unpack(bytes(data))
        return cls(v[:9], v[9:])

    def __eq__(self, other):
        return isinstance(other, RigidTransform) and self.ints() == other.ints()

    def __hash__(self):
        return hash(tuple(self.ints()))

    def __repr__(self):
        return f"RigidTransform(M={self.M}, t={self.t})"


def _corner_bounds(T, lo, hi):
    """[min, max] per axis of the warp over the box lo..hi, exactly: the form is linear per axis and the shift is monotonic."""
    out_lo, out_hi = [], []
    for i in range(3):
        a = b = (T.t[i] << 16) + (1 << 23)
        for j in range(3):
            m = T.M[i][j]
            a += min(m * lo[j], m * hi[j])
            b += max(m * lo[j], m * hi[j])
        out_lo.append(a >> 24)
        out_hi.append(b >> 24)
    return out_lo, out_hi


def _warp_keys(keys, n, T, box, want_rows, check=None):
    """The warp of a pitch-1 key array (any order): (canonical CoordSet of the distinct kept cells with exact bounds, perm,
    first).  box: (lo, hi) that holds the input, or None.  check: device int32 [2], the least and the largest coordinate of
    rows nobody has looked at yet.  ONE device->host read: the distinct count, the dropped count, the bounds of the result
    (and `check`: keys packed from coordinates outside the key range mean nothing, and nothing is returned for them)."""
    dev = keys.device
    lib = L.load()
    empty = S.CoordSet(torch.empty(1, dtype=torch.int64, device=dev), 0, 1, S.Bounds(0, (0, 0, 0), (0, 0, 0)), on_lattice=True)
    if n == 0:
        return empty, None, None
    mask = 0xFFFFFFFFFFFFFFFF
    if box is not None:            # no row can be dropped: only the digits the warped box spans are sorted
        wlo, whi = _corner_bounds(T, *box)
        if min(wlo) >= LO and max(whi) < HI:
            mask = S.Bounds(0, wlo, whi).bit_mask()
    with torch.cuda.device(dev):
        imax, imin = 2 ** 31 - 1, -2 ** 31
        info = torch.tensor([imax, imax, imax, imin, imin, imin, 0, 0, 0, 0], dtype=torch.int32, device=dev)   # [8:10]: the count (int64)
        wkeys = torch.empty(n, dtype=torch.int64, device=dev)
        L.call("pcc_motion_warp", L.ptr(keys), n, (C.c_int32 * 12)(*T.ints()), L.ptr(wkeys), L.ptr(info), L.stream())
        skeys = torch.empty(n, dtype=torch.int64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
        ws = L.workspace(lib.pcc_sort_ws_bytes(n), dev)
        L.call("pcc_sort_keys", L.ptr(wkeys), n, mask, L.ptr(skeys), L.ptr(perm), L.ptr(ws), ws.numel(), L.stream())
        ukeys = torch.empty(n, dtype=torch.int64, device=dev)
        first = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
        ws = L.workspace(lib.pcc_unique_ws_bytes(n), dev)
        L.call("pcc_unique_sorted", L.ptr(skeys), n, L.ptr(ukeys), L.ptr(first), info.data_ptr() + 32, L.ptr(ws), ws.numel(), L.stream())
        v = (info if check is None else torch.cat([info, check])).tolist()      # the warp's one device->host read
    if check is not None and (v[10] < LO or v[11] >= HI):
        raise L.PccError("warp_cloud: coordinates out of the 16-bit key range")
    runs, dropped = v[8] | (v[9] << 32), v[6]
    m = runs - (1 if dropped else 0)                               # the dropped rows are one run, behind every key
    if not 0 <= m <= n or dropped > n:
        raise L.PccError(f"warp_cloud: {runs} runs and {dropped} dropped rows of {n}")
    if m == 0:
        return empty, None, None
    return S.CoordSet(ukeys, m, 1, S.Bounds(0, v[0:3], v[3:6]), on_lattice=True), perm, first


def _levels(rgb):
    return torch.round(rgb.to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8)


def _canonical_with_rows(x, rows, what):
    """(canonical set, rows in canonical order -- of a repeated voxel the first row's)."""
    from .geometry import canonical_rows
    cs, perm, keep = canonical_rows(x, what)
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.dtype != torch.uint8 or not 1 <= rows.shape[1] <= MAX_ATTRS:
            raise L.PccError(f"{what}: attrs is a uint8 [N, 1..{MAX_ATTRS}] tensor")
        if rows.shape[0] != (cs.n if isinstance(x, S.CoordSet) else x.shape[0]):
            raise L.PccError(f"{what}: {rows.shape[0]} attribute rows for {x.n if isinstance(x, S.CoordSet) else x.shape[0]} voxels")
        if keep is not None:
            rows = rows[keep]
        if perm is not None:
            rows = rows[perm]
        rows = rows.contiguous()
    return cs, rows


@torch.no_grad()
def warp_set(cloud, T):
    """The geometry of `warp_cloud` alone (what the geometry coder needs of a reference, colours or not): the canonical set of
    the distinct warped cells.  That set does not depend on which source wins a cell nor on the order of the input rows, so
    tensor rows are warped as they are, without canonicalising them first: ONE device->host read in all."""
    what = "warp_cloud"
    if not isinstance(T, RigidTransform):
        raise L.PccError(f"{what}: T is a RigidTransform")
    if isinstance(cloud, S.CoordSet):
        if cloud.ts != 1 or cloud.bounds.bmax > 0:
            raise L.PccError(f"{what}: a pitch-1 single-batch coordinate set is required")
        return _warp_keys(cloud.keys, cloud.n, T, (cloud.bounds.lo, cloud.bounds.hi), False)[0]
    if not torch.is_tensor(cloud) or cloud.dim() != 2 or cloud.shape[1] < 3:
        raise L.PccError(f"{what}: an [N, >= 3] tensor or a CoordSet is required")
    if not cloud.is_cuda:
        raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
    xyz = cloud[:, :3]
    xyz = torch.floor(xyz).to(torch.int32) if xyz.dtype.is_floating_point else xyz.to(torch.int32)
    c4 = torch.cat([torch.zeros((xyz.shape[0], 1), dtype=torch.int32, device=xyz.device), xyz], dim=1).contiguous()
    check = torch.stack([xyz.min(), xyz.max()]) if xyz.shape[0] else None
    return _warp_keys(S.pack_keys(c4), c4.shape[0], T, None, False, check)[0]


@torch.no_grad()
def warp_cloud(cloud, T, attrs=None):
    """The reference cloud as every side of a stream sees it under the transform T.

    cloud: a pitch-1 CoordSet, or a GPU [N, >= 3] tensor of voxels (any row order, duplicates allowed, floats floored).
    Returns the canonical pitch-1 CoordSet of the distinct warped cells (exact bounds).  attrs (uint8 [N, 1..8], row i the
    attributes of voxel i; for a CoordSet in canonical order): returns (set, uint8 [n, C]) -- every cell carries the row of the
    source voxel of lowest canonical rank among those that landed in it.  An [N, 6] tensor (xyz, rgb in [0, 1]) carries its
    colour levels round(255 c) and comes back as a float32 [n, 6] tensor (xyz, level / 255) in canonical order.
    The result depends on the set of input voxels (and their attributes) alone, not on row order or repeated rows (of a
    repeated voxel the first row's attributes count, as everywhere in the coders)."""
    if not isinstance(T, RigidTransform):
        raise L.PccError("warp_cloud: T is a RigidTransform")
    what = "warp_cloud"
    coloured = attrs is None and torch.is_tensor(cloud) and cloud.dim() == 2 and cloud.shape[1] == 6
    if coloured:
        attrs = _levels(cloud[:, 3:6])
    if attrs is None:
        return warp_set(cloud, T)
    cs, rows = _canonical_with_rows(cloud, attrs, what)
    ws, perm, first = _warp_keys(cs.keys, cs.n, T, (cs.bounds.lo, cs.bounds.hi), True)
    out = torch.empty((ws.n, rows.shape[1]), dtype=torch.uint8, device=cs.device)
    if ws.n:
        with torch.cuda.device(cs.device):
            L.call("pcc_motion_gather", L.ptr(rows), rows.shape[1], cs.n, L.ptr(perm), L.ptr(first), ws.n, L.ptr(out), L.stream())
    if not coloured:
        return ws, out
    rgb = out.to(torch.float64) / torch.tensor(255.0, dtype=torch.float64, device=cs.device)
    return torch.cat([ws.coords()[:ws.n, 1:].to(torch.float64), rgb], dim=1).to(torch.float32)


def icp_terms(cur, normals, ref, R, t, centre, radius, want_match=False):
    """One launch of `pcc_motion_icp_terms`: (device fp64 [29] sums, int32 [ref.n] matches or None).  cur / ref: canonical
    pitch-1 sets, normals: fp32 [cur.n, 3]; R (3 x 3), t, centre: host floats."""
    dev = ref.device
    lib = L.load()
    with torch.cuda.device(dev):
        out = torch.empty(N_SUMS, dtype=torch.float64, device=dev)
        match = torch.empty(max(ref.n, 1), dtype=torch.int32, device=dev) if want_match else None
        rt = (C.c_double * 12)(*[float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)], *[float(v) for v in t])
        g = (C.c_double * 3)(*[float(v) for v in centre])
        ws = L.workspace(lib.pcc_motion_icp_ws_bytes(ref.n), dev)
        L.call("pcc_motion_icp_terms", L.ptr(ref.keys), ref.n, L.ptr(cur.keys), cur.n, *S.grid_args(cur.grid() if (S.USE_GRID and cur.n) else None),
               L.ptr(normals), rt, g, float(radius), L.ptr(out), L.ptr(match), L.ptr(ws), ws.numel(), L.stream())
    return out, (match[:ref.n] if want_match else None)


def rodrigues(w):
    """The rotation matrix exp([w]x) of a rotation vector (numpy fp64)."""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.sqrt(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def solve_step(sums, R, t, g):
    """One Gauss-Newton step from the 29 sums: the new (R, t).  6 x 6 system with a ridge of 1e-9 * trace / 6; dR by Rodrigues
    from the first three unknowns, dt = w[3:] + g - dR g."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    w = np.linalg.solve(A + (RIDGE * np.trace(A) / 6.0) * np.eye(6), sums[21:27])
    dR = rodrigues(w[:3])
    dt = w[3:] + g - dR @ g
    return dR @ R, dR @ t + dt


def _integer_sums(cs):
    """Exact (sum x, sum y, sum z) of a canonical set as a device int64 [3] tensor."""
    return cs.coords()[:cs.n, 1:].to(torch.int64).sum(dim=0)


@torch.no_grad()
def estimate_rigid(cur, ref, iterations=8, radius=3.0, normal_radius=5.0):
    """A RigidTransform that takes `ref` onto `cur` (both: what `warp_cloud` takes), or None when no reference voxel finds a
    current voxel inside `radius` in some iteration.  Point-to-plane ICP from R = I, t = mean(cur) - mean(ref) (exact integer
    sums); per iteration one `pcc_motion_icp_terms` launch and one read of its 29 sums; quantised once, at the end.
    Two calls give the same integers, and so do permuted or repeated input rows: every sum is in canonical order."""
    from .geometry import canonical_rows
    from .metrics import _set_normals
    if not 0.0 < float(radius) <= MAX_RADIUS:
        raise L.PccError(f"estimate_rigid: radius {radius} outside (0, {MAX_RADIUS:g}] (the candidate cube grows with its cube)")
    if int(iterations) < 1:
        raise L.PccError(f"estimate_rigid: {iterations} iterations")
    cs, rs = canonical_rows(cur, "estimate_rigid")[0], canonical_rows(ref, "estimate_rigid (reference)")[0]
    if cs.n == 0 or rs.n == 0:
        return None
    sums = torch.cat([_integer_sums(cs), _integer_sums(rs)]).tolist()           # one read
    g = np.array([sums[k] / cs.n for k in range(3)], dtype=np.float64)
    R, t = np.eye(3), np.array([sums[k] / cs.n - sums[3 + k] / rs.n for k in range(3)], dtype=np.float64)
    normals = _set_normals(cs, normal_radius)[0]
    for _ in range(int(iterations)):
        s = icp_terms(cs, normals, rs, R, t, g, radius)[0].cpu().numpy()         # one read per iteration
        if s[27] == 0:
            return None
        R, t = solve_step(s, R, t, g)
    return RigidTransform.from_float(R, t)
