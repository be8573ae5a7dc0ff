"""Training batches on the device: the reference's `data/` package (`data/dataloader.py`, `data/transform.py`,
`data/q_func.py`) and the loader loop of `train.py:84-101,195-213`, turned round: a frame is sliced into cubes ONCE on
the GPU and stays there (`slice_into_cubes` -> `CubeTable`), and every step's batch is assembled by one kernel from a
few dozen host-drawn parameters (`TrainBatcher`) -- the reference deep-copies, jitters, rotates and de-duplicates every
cube in 12 CPU worker processes and ships the result to the GPU.

Arithmetic (restated by `tests/data_ref.py` in numpy):

* slicing      cube index = floor(p / cube_size) per axis (fp32 division), cube-local point = p - index * cube_size;
               cubes in ascending (ix, iy, iz) order (`torch.unique(dim=0)`), rows of a cube in frame order (a boolean
               mask) -- first-wins de-duplication later depends on row order.
* rotation     phi, theta = rand * 2 * 3.141592653589793 (two draws, that order), R = R_y(theta) R_x(phi) in fp32 on the
               host, out = (p - c) R^T + c with c = block_size / 2, evaluated per axis as
               ((dx R[j][0] + dy R[j][1]) + dz R[j][2]) + c with every product and sum rounded to fp32 SEPARATELY (no
               FMA), then floor: the voxel of a point is a defined function of its inputs, reproducible bit for bit.
* colour       torchvision's ColorJitter(0.3, 0.3, 0.3, 0.3) on the [3, N, 1] image of a cube's colours, restated
               from torchvision's `functional_tensor` code and not checked against it: UNPINNED in the same sense as
               the rest of this project's parity.
               order = randperm(4), then b, c, s ~ U(0.7, 1.3), h ~ U(-0.3, 0.3); steps in `order`, 0 brightness,
               1 contrast, 2 saturation, 3 hue.  blend(x, y, r) = clamp(r x + (1 - r) y, 0, 1),
               grey(x) = 0.2989 r + 0.587 g + 0.114 b.  brightness blend(x, 0, b); contrast blend(x, mean over the
               cube's rows of grey(x), c); saturation blend(x, grey(x), s); hue: RGB -> HSV, h <- (h + hue) mod 1,
               HSV -> RGB.  fp32 throughout; the contrast mean is an fp64 sum in a fixed order, rounded once.
               The mean runs over all rows of the cube as the table holds them (in the reference's configuration the
               jitter precedes the rotation, so that is what it sees too).

No CPU fallback (`PccError` on CPU tensors).  Draws come from a `torch.Generator`; no global RNG state is touched.
"""
import math

import numpy as np
import torch

from . import lib as L
from . import sparse as S

PccError = L.PccError

SLOT_WORDS, BLOCK_ROWS, MAX_SLOTS = 32, 1024, 4096       # PCC_AUG_* of include/pcc_hip.h
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
_KEY_BIAS = 1 << 15


def _need_gpu(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise PccError(f"{what}: GPU tensor required (no CPU fallback)")


# ------------------------------------------------------------------------------------------------------------------
# cube table
# ------------------------------------------------------------------------------------------------------------------
class CubeTable:
    """Cubes of one or more frames, device resident: `points` / `colors` [N, 3] fp32 with every cube one contiguous run,
    `offsets` [n_cubes + 1] and `origin` [n_cubes, 3] (the reference's `cube_shift`) on the device and, read back once,
    on the host (`h_offsets`, `h_origin`: numpy int64); `frame` [n_cubes]: which frame of a `concat` a cube came from;
    `extent` (lo [3], hi [3]): smallest and largest point coordinate per axis, read once here unless given -- the batcher
    bounds every step's output coordinates from it on the host instead of reading them back."""

    def __init__(self, points, colors, h_offsets, h_origin, cube_size, frame=None, extent=None):
        self.points, self.colors, self.cube_size = points, colors, int(cube_size)
        self.h_offsets = np.asarray(h_offsets, dtype=np.int64)
        self.h_origin = np.asarray(h_origin, dtype=np.int64).reshape(-1, 3)
        self.frame = np.zeros(len(self.h_origin), dtype=np.int64) if frame is None else np.asarray(frame, dtype=np.int64)
        if (len(self.h_offsets) != len(self.h_origin) + 1 or self.h_offsets[0] != 0 or self.h_offsets[-1] != points.shape[0]
                or np.any(np.diff(self.h_offsets) <= 0)):
            raise PccError("CubeTable: offsets must rise from 0 to the row count, one entry per cube and one more")
        if extent is None:
            lo, hi = torch.aminmax(points.to(torch.float32), dim=0)
            extent = torch.stack([lo, hi]).cpu().numpy()
        self.extent = np.asarray(extent, dtype=np.float64).reshape(2, 3)
        if not np.all(np.isfinite(self.extent)):
            raise PccError("CubeTable: points must be finite")
        self.offsets = torch.from_numpy(self.h_offsets).to(points.device)
        self.origin = torch.from_numpy(self.h_origin).to(points.device)

    def __len__(self):
        return len(self.h_origin)

    @property
    def device(self):
        return self.points.device

    @property
    def num_points(self):
        return np.diff(self.h_offsets)

    def cube(self, i):
        """The reference's cube dict (`dataloader.py:199-204`), as views into the table."""
        if not 0 <= i < len(self):
            raise ValueError(f"cube index {i} outside 0..{len(self) - 1}")
        a, b = int(self.h_offsets[i]), int(self.h_offsets[i + 1])
        return {"points": self.points[a:b], "colors": self.colors[a:b], "offset": self.origin[i],
                "num_points": torch.tensor(b - a)}

    def indices(self, min_points=0):
        """Cubes with num_points > min_points (`dataloader.py:221`, strict)."""
        return [int(i) for i in np.nonzero(self.num_points > min_points)[0]]

    @classmethod
    def concat(cls, tables):
        tables = list(tables)
        if not tables:
            raise ValueError("CubeTable.concat: no tables")
        if len({t.cube_size for t in tables}) != 1 or len({t.device for t in tables}) != 1:
            raise ValueError("CubeTable.concat: tables differ in cube size or device")
        offs, base, frames, nf = [np.zeros(1, dtype=np.int64)], 0, [], 0
        for t in tables:
            offs.append(t.h_offsets[1:] + base)
            base += int(t.h_offsets[-1])
            frames.append(t.frame + nf)
            nf += int(t.frame.max()) + 1 if len(t) else 0
        return cls(torch.cat([t.points for t in tables]), torch.cat([t.colors for t in tables]), np.concatenate(offs),
                   np.concatenate([t.h_origin for t in tables]), tables[0].cube_size, np.concatenate(frames),
                   np.stack([np.min([t.extent[0] for t in tables], axis=0), np.max([t.extent[1] for t in tables], axis=0)]))


def slice_into_cubes(points, colors, cube_size=64):
    """`StaticDataset.slice_into_cubes` (`data/dataloader.py:168-208`) on the GPU: keys per point, the stable key sort and
    run starts that coordinate sets use, one regrouping pass.  Three small host reads, once per frame."""
    _need_gpu(points, "slice_into_cubes"), _need_gpu(colors, "slice_into_cubes")
    if points.dim() != 2 or points.shape[1] != 3 or colors.shape != points.shape:
        raise PccError("slice_into_cubes: points and colors must both be [N, 3]")
    cube_size = int(cube_size)
    n, dev = points.shape[0], points.device
    if n == 0:
        raise PccError("slice_into_cubes: empty frame")
    pts, col = points.to(torch.float32).contiguous(), colors.to(torch.float32).contiguous()
    lib, st = L.load(), L.stream()
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    local = torch.empty((n, 3), dtype=torch.float32, device=dev)
    head = L.counter(2)                                   # [0] number of cubes, [1] (int32) a point outside the key range
    L.call("pcc_cube_keys", L.ptr(pts), n, cube_size, L.ptr(keys), L.ptr(local), L.cptr(head) + 8, st)
    skeys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.pcc_sort_ws_bytes(n), dev)
    L.call("pcc_sort_keys", L.ptr(keys), n, (1 << 48) - 1, L.ptr(skeys), L.ptr(perm), L.ptr(ws), ws.numel(), st)
    ukeys = torch.empty(n, dtype=torch.int64, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.pcc_unique_ws_bytes(n), dev)
    L.call("pcc_unique_sorted", L.ptr(skeys), n, L.ptr(ukeys), L.ptr(first), L.cptr(head), L.ptr(ws), ws.numel(), st)
    out_p, out_c = torch.empty_like(local), torch.empty_like(col)
    L.call("pcc_cube_regroup", L.ptr(local), L.ptr(col), L.ptr(perm), n, L.ptr(out_p), L.ptr(out_c), st)
    nu, bad = L.read(head)
    if bad:
        raise PccError("slice_into_cubes: a point is not finite or its cube index does not fit 16 bits")
    tab = torch.cat([ukeys[:nu], first[:nu].long()]).cpu().numpy()       # the second (and last) read
    uk = tab[:nu]
    idx = np.stack([(uk >> 32) & 0xFFFF, (uk >> 16) & 0xFFFF, uk & 0xFFFF], axis=1) - _KEY_BIAS
    return CubeTable(out_p, out_c, np.concatenate([tab[nu:], [n]]), idx * cube_size, cube_size)


# ------------------------------------------------------------------------------------------------------------------
# transforms (parameter objects) and the quality draw
# ------------------------------------------------------------------------------------------------------------------
class ColorJitter:
    """`data/transform.py:32-54`: torchvision.transforms.ColorJitter(0.3, 0.3, 0.3, 0.3); see the module docstring."""
    brightness = contrast = saturation = (0.7, 1.3)
    hue = (-0.3, 0.3)

    def draw(self, generator):
        """torchvision's `get_params`: the step order, then the four factors (each an fp32 draw, as `.uniform_` makes it)."""
        order = torch.randperm(4, generator=generator).tolist()
        f = [float(torch.empty(1).uniform_(lo, hi, generator=generator)) for lo, hi in
             (self.brightness, self.contrast, self.saturation, self.hue)]
        return {"steps": order, "factors": tuple(f)}


class RandomRotate:
    """`data/transform.py:57-123` without the crop (which `build_transforms` never enables)."""

    def __init__(self, block_size, crop=False):
        if crop:
            raise PccError("RandomRotate(crop=True) is not built: data/transform.py:24 constructs RandomRotate(block_size) "
                           "only, so the crop branch of :86-89 is unreachable through build_transforms")
        self.block_size = block_size

    @staticmethod
    def rotation_matrix_3d(phi, theta):
        """R = R_y(theta) R_x(phi) in fp32 (`transform.py:108-123`); phi, theta: fp32 tensors of one element."""
        phi, theta = torch.as_tensor(phi, dtype=torch.float32).reshape(()), torch.as_tensor(theta, dtype=torch.float32).reshape(())
        one, zero = torch.ones(()), torch.zeros(())
        cp, sp, ct, st = torch.cos(phi), torch.sin(phi), torch.cos(theta), torch.sin(theta)
        r_x = torch.stack([one, zero, zero, zero, cp, -sp, zero, sp, cp]).reshape(3, 3)
        r_y = torch.stack([ct, zero, st, zero, one, zero, -st, zero, ct]).reshape(3, 3)
        return torch.mm(r_y, r_x)

    def params(self, phi, theta):
        """Parameters of given angles (what `draw` returns for drawn ones)."""
        return {"phi": float(phi), "theta": float(theta), "matrix": self.rotation_matrix_3d(phi, theta),
                "centre": self.block_size / 2}

    def draw(self, generator):
        phi = torch.rand(1, generator=generator) * 2 * 3.141592653589793       # random roll
        theta = torch.rand(1, generator=generator) * 2 * 3.141592653589793     # random pitch
        return self.params(phi, theta)


def build_transforms(config):
    """`data/transform.py:9-30`: entries in sorted key order; `key` names the transform."""
    transforms = []
    if not config:
        return transforms
    for name in sorted(config):
        key = config[name]["key"]
        if key == "RandomRotate":
            transforms.append(RandomRotate(config[name]["block_size"]))
        elif key == "ColorJitter":
            transforms.append(ColorJitter())
        else:
            raise ValueError(f"Transform {key} not defined.")
    return transforms


class Q_Func:
    """`data/q_func.py`: one (q_g, q_a) pair per step, broadcast over the batch, and its lambdas."""

    def __init__(self, config):
        self.mode = config["mode"]
        if self.mode == "exponential":
            self.a_A = math.log2(config["lambda_A_max"] + config["lambda_A_min"])
            self.b_A = config["lambda_A_min"] - 1
            self.a_G = math.log2(config["lambda_G_max"] + config["lambda_G_min"])
            self.b_G = config["lambda_G_min"] - 1
        elif self.mode == "quadratic":
            self.a_A = config["lambda_A_max"] - config["lambda_A_min"]
            self.b_A = config["lambda_A_min"]
            self.a_G = config["lambda_G_max"] - config["lambda_G_min"]
            self.b_G = config["lambda_G_min"]
        else:
            raise ValueError("Unknown mapping mode")

    def __call__(self, batch, generator=None, device=None):
        """batch: the number of cubes, or a sparse tensor (its largest batch index + 1, one host read).  The two draws are
        fp64 uniforms of `generator` (the reference takes them from Python's global `random`)."""
        if isinstance(batch, int):
            nb = batch
        else:
            nb, device = int(batch.C[:, 0].max()) + 1, batch.C.device if device is None else device
        q = torch.rand(2, generator=generator, dtype=torch.float64).to(torch.float32)
        q_vals = q.reshape(1, 2).repeat(nb, 1)
        if device is not None:
            q_vals = q_vals.to(device)
        return q_vals, self.scale_q_vals(q_vals)

    def scale_q_vals(self, q_vals):
        lambda_vals = q_vals.clone()
        if self.mode == "exponential":
            lambda_vals[:, 0] = 2 ** (lambda_vals[:, 0] * self.a_G) + self.b_G
            lambda_vals[:, 1] = 2 ** (lambda_vals[:, 1] * self.a_A) + self.b_A
        elif self.mode == "quadratic":
            lambda_vals[:, 0] = lambda_vals[:, 0] ** 2 * self.a_G + self.b_G
            lambda_vals[:, 1] = lambda_vals[:, 1] ** 2 * self.a_A + self.b_A
        else:
            raise ValueError("Unknown mapping mode")
        return lambda_vals


# ------------------------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------------------------
_IDENTITY = np.eye(3, dtype=np.float32).reshape(-1)


def _slot_tables(table, cube_indices, params):
    """Descriptors [nslots, SLOT_WORDS] and block table [nblocks, 2] as int32 numpy arrays (layout: include/pcc_hip.h),
    checked against the table here, before anything is uploaded; also the row count and the box (lo, hi) of the batch.
    A slot's box bounds its output coordinates rigorously: |out_j - c| <= sum_i |R[j][i]| max|p_i - c| over the table's
    extent, widened by 1e-5 of itself for the four fp32 roundings and by one voxel."""
    ns = len(cube_indices)
    if not 1 <= ns <= MAX_SLOTS:
        raise ValueError(f"a batch holds 1..{MAX_SLOTS} cubes, not {ns}")
    if len(params) != ns:
        raise ValueError(f"{ns} cubes but {len(params)} parameter sets")
    desc = np.zeros((ns, SLOT_WORDS), dtype=np.int32)
    fdesc = desc.view(np.float32)
    blocks, out = [], 0
    for s, (ci, p) in enumerate(zip(cube_indices, params)):
        if not 0 <= int(ci) < len(table):
            raise ValueError(f"cube index {ci} outside 0..{len(table) - 1}")
        a, rows = int(table.h_offsets[ci]), int(table.h_offsets[ci + 1] - table.h_offsets[ci])
        jit, rot = (p or {}).get("jitter"), (p or {}).get("rotate")
        steps = list(jit["steps"]) if jit else []
        if len(steps) > 4 or len(set(steps)) != len(steps) or any(k not in (0, 1, 2, 3) for k in steps):
            raise ValueError(f"slot {s}: colour steps must be distinct members of 0..3, got {steps}")
        nb = -(-rows // BLOCK_ROWS)
        desc[s, 0:4] = (a, rows, out, len(steps))
        desc[s, 4:4 + len(steps)] = steps
        fdesc[s, 8:12] = jit["factors"] if jit else (1.0, 1.0, 1.0, 0.0)
        fdesc[s, 12:21] = rot["matrix"].numpy().reshape(-1) if rot else _IDENTITY
        fdesc[s, 21] = rot["centre"] if rot else 0.0
        m, c = fdesc[s, 12:21].astype(np.float64).reshape(3, 3), float(fdesc[s, 21])
        reach = np.abs(m) @ np.maximum(np.abs(table.extent[0] - c), np.abs(table.extent[1] - c)) * (1 + 1e-5) + 1.0
        if not np.all(np.isfinite(reach)) or np.any(c - reach <= -_KEY_BIAS + 64) or np.any(c + reach >= _KEY_BIAS - 64):
            raise ValueError(f"slot {s}: rotated coordinates would leave the 16-bit key range (or the matrix is not finite)")
        desc[s, 24:27], desc[s, 27:30] = np.floor(c - reach), np.ceil(c + reach)
        desc[s, 22:24] = (len(blocks), nb)
        blocks.extend((s, b * BLOCK_ROWS) for b in range(nb))
        out += rows
    if out >= 1 << 31:
        raise ValueError("batch too large")
    return desc, np.asarray(blocks, dtype=np.int32).reshape(-1, 2), out, (desc[:, 24:27].min(axis=0), desc[:, 27:30].max(axis=0))


class TrainBatcher:
    """One epoch of training batches over the eligible cubes of a table (`train.py:84-101,195-208`): iterating yields
    `(coords int32 [n, 4], feats fp32 [n, 3], info)` -- `sparse_collate` followed by `sparse_quantize(quantization_size=1.0)`
    of the transformed cubes: batch index first, duplicates removed first-wins in (batch slot, cube row) order, surviving
    rows in that order -- ready for `ME.SparseTensor(features=feats, coordinates=coords)`.  `len()` counts full and partial
    batches (a DataLoader with drop_last=False).  Per step the host uploads the slot descriptors once (from pinned memory)
    and makes ONE device->host read, the row count of the de-duplication (`sparse.coordset_from_coords`, whose lattice is
    sized from the host-side box of the batch, not from coordinates read back)."""

    def __init__(self, table, batch_size, min_points=0, transforms=(), generator=None, shuffle=True):
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if not isinstance(table, CubeTable):
            raise PccError("TrainBatcher: table must be a CubeTable (slice_into_cubes)")
        _need_gpu(table.points, "TrainBatcher")
        for t in transforms:
            if not isinstance(t, (ColorJitter, RandomRotate)):
                raise ValueError(f"Transform {t!r} not defined.")
        self.table, self.batch_size, self.transforms, self.shuffle = table, int(batch_size), list(transforms), shuffle
        self.eligible = table.indices(min_points)
        if generator is None:
            generator = torch.Generator()
            generator.seed()
        self.generator = generator
        self._staging = L.PinnedStaging(torch.int32)    # pinned staging buffers, each with the event of its last copy

    def __len__(self):
        return -(-len(self.eligible) // self.batch_size)

    def draw(self):
        """Parameters of one cube: every transform's draw, in transform order (as a loader worker makes them)."""
        p = {}
        for t in self.transforms:
            p["jitter" if isinstance(t, ColorJitter) else "rotate"] = t.draw(self.generator)
        return p

    def __iter__(self):
        ne = len(self.eligible)
        order = torch.randperm(ne, generator=self.generator).tolist() if self.shuffle else list(range(ne))
        flags = []
        for a in range(0, ne, self.batch_size):
            cubes = [self.eligible[i] for i in order[a:a + self.batch_size]]
            item = self.assemble(cubes, [self.draw() for _ in cubes])
            flags.append(item[2]["outside"])
            yield item
        if flags and bool(torch.cat(flags).any()):         # one read per epoch, after its last batch
            raise PccError("TrainBatcher: coordinates left the box computed from the table's extent during this epoch and "
                           "were moved onto it -- the table's points were changed after the table was built")

    def _upload(self, desc, blocks):
        """Both tables through a pinned staging buffer and one asynchronous copy.  Two buffers take turns, and each carries
        the event recorded behind its last copy: a buffer is rewritten only after that event has completed, so the device
        copy the kernels index by is always the host copy that was validated, however much work the stream still holds and
        whether or not the step reads anything back."""
        h = self._staging.acquire(desc.size + blocks.size)
        hn = h.numpy()
        hn[:desc.size] = desc.reshape(-1)
        hn[desc.size:] = blocks.reshape(-1)
        return h, self._staging.upload(h, self.table.device)

    def assemble(self, cube_indices, params, deduplicate=True):
        """The batch of the given cubes under the given parameters: one dict per slot with optional entries "jitter"
        ({"steps": up to four distinct step kinds in order, "factors": (b, c, s, hue)}) and "rotate" ({"matrix": 3x3 fp32
        CPU tensor, "centre": block_size / 2}); a missing entry leaves colours / points as they are.  deduplicate=False
        returns the collated rows as the kernel wrote them (all rows of slot 0, then slot 1, ...)."""
        cube_indices = [int(i) for i in cube_indices]
        desc, blocks, rows, (lo, hi) = _slot_tables(self.table, cube_indices, params)
        tb, dev, st = self.table, self.table.device, L.stream()
        ns, nb = len(desc), len(blocks)
        h, d = self._upload(desc, blocks)
        hs, hb = h.data_ptr(), h.data_ptr() + desc.size * 4
        ds, db = d.data_ptr(), d.data_ptr() + desc.size * 4
        coords = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        feats = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        means, outside = None, torch.empty(1, dtype=torch.int32, device=dev)
        if desc[:, 3].any():                               # rotation-only batches launch no reduction
            partials = torch.empty(nb, dtype=torch.float64, device=dev)
            means = torch.empty(ns, dtype=torch.float32, device=dev)
            L.call("pcc_aug_gray_sums", L.ptr(tb.colors), tb.colors.shape[0], hs, ds, ns, hb, db, nb, L.ptr(partials),
                   L.ptr(means), st)
        L.call("pcc_aug_batch", L.ptr(tb.points), L.ptr(tb.colors), tb.points.shape[0], hs, ds, ns, hb, db, nb, L.ptr(means),
               L.ptr(coords), L.ptr(feats), rows, L.ptr(outside), st)
        if deduplicate:                                    # first wins; keep = surviving rows in their order, or None
            hint = (S.pack_keys(coords), S.Bounds(ns - 1, lo, hi), False)
            _, _, keep = S.coordset_from_coords(S.FrameRows(rows, dev, hint), 1)
            if keep is not None:
                coords, feats = coords[keep], feats[keep]
        # "outside": device int32 [1], non-zero if a coordinate had to be moved onto its slot's box (never, unless the
        # table was changed after its extent was taken); left on the device so that no step waits for it -- iterating
        # reads the flags of an epoch once, at its end, and raises
        return coords, feats, {"cubes": cube_indices, "params": list(params), "rows": rows, "outside": outside}
