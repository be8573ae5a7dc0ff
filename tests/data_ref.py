"""CPU restatements of the training-batch pipeline (unified_point_cloud_compression_amd/data.py), numpy / torch-CPU only:
what the reference's loader computes (`data/dataloader.py:168-208`, `data/transform.py:32-123`, `train.py:199-208`), written
out literally.  The colour steps exist in fp32 (the reference's own arithmetic) and in float64 (the yardstick)."""
import numpy as np
import torch


def slice_into_cubes(points, colors, cube_size):
    """`StaticDataset.slice_into_cubes`, line for line (torch CPU tensors in, list of cube dicts out)."""
    min_boundary = torch.tensor([0, 0, 0])
    cube_indices = ((points - min_boundary) / cube_size).floor().long()
    unique_cube_indices, inverse_indices = torch.unique(cube_indices, dim=0, return_inverse=True)
    cubes = []
    for idx in range(unique_cube_indices.size(0)):
        mask = inverse_indices == idx
        cube_points = points[mask]
        cube_shift = unique_cube_indices[idx] * cube_size
        cube = {"points": cube_points - cube_shift, "colors": colors[mask], "offset": cube_shift,
                "num_points": torch.tensor(len(cube_points))}
        if cube["num_points"] > 0:
            cubes.append(cube)
    return cubes


def rotate_ordered(points, R, c):
    """((dx R[j][0] + dy R[j][1]) + dz R[j][2]) + c, every product and sum rounded to fp32 on its own, then floor."""
    p, R, c = np.asarray(points, np.float32), np.asarray(R, np.float32), np.float32(c)
    d = p - c
    out = np.stack([((d[:, 0] * R[j, 0] + d[:, 1] * R[j, 1]) + d[:, 2] * R[j, 2]) + c for j in range(3)], axis=1)
    assert out.dtype == np.float32
    return np.floor(out).astype(np.int32)


def rotate_f64(points, R, c):
    """The same rotation (the same fp32 matrix entries) carried out in float64."""
    p, R = np.asarray(points, np.float64), np.asarray(R, np.float64)
    return np.floor((p - c) @ R.T + c).astype(np.int32)


def _grey(x, dt):
    return (dt(0.2989) * x[:, 0] + dt(0.587) * x[:, 1]) + dt(0.114) * x[:, 2]


def _blend(x, y, r, dt):
    r = dt(r)
    return np.clip(r * x + (dt(1.0) - r) * y, dt(0.0), dt(1.0))


def _hue(x, shift, dt):
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    one = dt(1.0)
    maxc, minc = x.max(axis=1), x.min(axis=1)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, one, maxc)
    div = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = np.where(maxc == r, bc - gc, dt(0.0))
    hg = np.where((maxc == g) & (maxc != r), (dt(2.0) + rc) - bc, dt(0.0))
    hb = np.where((maxc != g) & (maxc != r), (dt(4.0) + gc) - rc, dt(0.0))
    h = (hr + hg) + hb
    h = np.fmod(h / dt(6.0) + one, one)
    h = np.mod(h + dt(shift), one)                       # floored modulo
    v = maxc
    h6 = h * dt(6.0)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int32) % 6
    p = np.clip(v * (one - s), dt(0.0), one)
    q = np.clip(v * (one - s * f), dt(0.0), one)
    t = np.clip(v * (one - s * (one - f)), dt(0.0), one)
    pick = lambda *six: np.choose(i, six)
    out = np.stack([pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)], axis=1)
    assert out.dtype == dt
    return out


def jitter(colors, steps, factors, dt=np.float32):
    """torchvision ColorJitter's steps in the given order on [n, 3] colours; the contrast mean runs over all rows."""
    x = np.asarray(colors, np.float32).astype(dt)
    for st in steps:
        if st == 0:
            x = _blend(x, dt(0.0), factors[0], dt)
        elif st == 1:
            x = _blend(x, _grey(x, dt).mean(dtype=dt), factors[1], dt)
        elif st == 2:
            x = _blend(x, _grey(x, dt)[:, None], factors[2], dt)
        elif st == 3:
            x = _hue(x, factors[3], dt)
        else:
            raise ValueError(st)
        assert x.dtype == dt
    return x


def first_wins(coords):
    """Rows of int [n, 4] coordinates that survive `sparse_quantize` (first occurrence kept, original order)."""
    c = np.asarray(coords, np.int64) + (1 << 15)
    keys = (c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]
    _, first = np.unique(keys, return_index=True)
    return np.sort(first)


def batch(cubes, params, dt=np.float32, deduplicate=True):
    """jitter -> rotate -> collate -> quantize (first wins) of a list of (points, colors) numpy cubes under per-slot
    parameter dicts as `TrainBatcher.assemble` takes them.  Returns (coords int32 [n, 4], feats dt [n, 3])."""
    Cs, Fs = [], []
    for s, ((pts, col), p) in enumerate(zip(cubes, params)):
        jit, rot = p.get("jitter"), p.get("rotate")
        f = jitter(col, jit["steps"], jit["factors"], dt) if jit else np.asarray(col, np.float32).astype(dt)
        xyz = rotate_ordered(pts, rot["matrix"].numpy(), rot["centre"]) if rot else np.floor(pts).astype(np.int32)
        Cs.append(np.concatenate([np.full((len(xyz), 1), s, np.int32), xyz], axis=1))
        Fs.append(f)
    C, F = np.concatenate(Cs), np.concatenate(Fs)
    if deduplicate:
        keep = first_wins(C)
        C, F = C[keep], F[keep]
    return C, F
