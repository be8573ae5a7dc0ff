"""GPU suite of voxel-grid down-sampling (`voxelize.py` over `csrc/pcc_voxel.hip`) against the numpy float64 restatement
`tests/voxel_ref.py`.

Tolerances.  Voxel indices and counts are integers: exact.  On the voxelised cloud every summand is an integer below 2^8 or
an fp32 k / 255 (a multiple of 2^-31 below 2), in runs far below 2^21 rows: every partial sum is exact in fp64 whatever the
order, so the means agree bit for bit.  On float clouds the device adds in another order than `np.add.reduceat`; the fp64
sums then differ by a few units of 2^-53 relative to the sum of magnitudes, the quotients likewise, and two fp64 values that
close round to the same fp32 or to neighbours: one fp32 ulp.  Two runs of the device agree bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import voxel_ref as R
from tests.util import dev, n as to_np
from unified_point_cloud_compression_amd import data, ply, sparse as S, voxelize as V
from unified_point_cloud_compression_amd.lib import PccError

pytestmark = pytest.mark.gpu


def t(a):
    return torch.from_numpy(np.array(a)).to(dev())        # a copy: the cached clouds are read-only


def bits_equal(got, want):
    got, want = (to_np(x) if torch.is_tensor(x) else np.asarray(x) for x in (got, want))
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def within_one_ulp(got, want):
    got, want = to_np(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    worst = float((err / ulp).max()) if err.size else 0.0
    print(f"largest error {worst:.2f} ulp over {err.size} entries, {int((err > 0).sum())} differ")
    return worst <= 1.0


def check_grid(g, ref, exact):
    """A VoxelGrid against the restatement's tuple."""
    index, pts, attrs, counts, origin = ref
    assert bits_equal(g.index, index) and bits_equal(g.counts, counts)
    assert tuple(g.origin) == tuple(float(x) for x in origin)
    same = bits_equal if exact else within_one_ulp
    assert same(g.points, pts)
    assert (g.attrs is None) == (attrs is None)
    if attrs is not None:
        assert same(g.attrs, attrs)


# ---------------------------------------------------------------------------------------------------------------------
# voxelised input: exact
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_cloud():
    """64^3 Bernoulli(0.05) block of integer points offset by 100 with 8-bit colour levels: 12 997 rows in (x, y, z) order."""
    rng = np.random.default_rng(0)
    xyz = np.argwhere(rng.random((64, 64, 64)) < 0.05) + 100
    col = rng.integers(0, 256, (len(xyz), 3)).astype(np.float32) / np.float32(255)
    cloud = np.concatenate([xyz.astype(np.float32), col], axis=1)
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def block_ref(factor):
    out, counts = R.voxel_down_sample(block_cloud(), factor)
    return out, counts, R.downscale(block_cloud(), factor)


def shuffled(cloud, seed):
    return cloud[np.random.default_rng(seed).permutation(len(cloud))]


def test_factor_one_returns_the_same_rows():
    cloud = block_cloud()
    out, counts = V.voxel_down_sample(t(shuffled(cloud, 1)), 1, return_counts=True)
    assert bits_equal(out, cloud)                                    # argwhere order is ascending (x, y, z) order
    assert bits_equal(counts, np.ones(len(cloud), np.int32))


@pytest.mark.parametrize("factor", [2, 4, 8])
def test_voxelised_input_matches_the_restatement_bit_for_bit(factor):
    cloud = block_cloud()
    want, want_counts, want_down = block_ref(factor)
    assert len(want) == {2: 11031, 4: 4390, 8: 729}[factor]
    x = t(cloud)
    out, counts = V.voxel_down_sample(x, factor, return_counts=True)
    assert bits_equal(out, want) and bits_equal(counts, want_counts)
    g = V.voxel_grid(x[:, :3], x[:, 3:], factor)
    check_grid(g, R.voxel_grid(cloud[:, :3], cloud[:, 3:], factor), exact=True)
    down = V.downscale(x, factor)
    if factor == 2:                                                  # most rows sit on a rounding tie: half to even is tested
        q = want[:, :3].astype(np.float64) / 2
        assert int(np.any(q - np.floor(q) == 0.5, axis=1).sum()) == 8938
    assert bits_equal(down, want_down)
    # shuffling the rows changes no output bit
    out_s, counts_s = V.voxel_down_sample(t(shuffled(cloud, factor)), factor, return_counts=True)
    assert bits_equal(out_s, want) and bits_equal(counts_s, want_counts)


def test_normals_get_the_plain_mean():
    cloud = block_cloud()
    rng = np.random.default_rng(5)
    nrm = rng.integers(-8, 9, (len(cloud), 3)).astype(np.float32) / np.float32(8)       # exact sums
    out, normals, counts = V.voxel_down_sample(t(cloud), 4, normals=t(nrm), return_counts=True)
    ref = R.voxel_grid(cloud[:, :3], np.concatenate([cloud[:, 3:], nrm], axis=1), 4)
    assert bits_equal(out, np.concatenate([ref[1], ref[2][:, :3]], axis=1))
    assert bits_equal(normals, np.ascontiguousarray(ref[2][:, 3:])) and bits_equal(counts, ref[3])
    assert float(np.abs(np.linalg.norm(to_np(normals), axis=1) - 1).max()) > 0.1        # not renormalised


# ---------------------------------------------------------------------------------------------------------------------
# float input: one ulp, and the same bits on every run
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_cloud(c):
    rng = np.random.default_rng(11)
    pts = (rng.random((20000, 3)) * 64).astype(np.float32)
    attrs = rng.standard_normal((20000, 32)).astype(np.float32)[:, :c]
    pts.setflags(write=False)
    return pts, np.ascontiguousarray(attrs)


@pytest.mark.parametrize("voxel_size", [2.5, 0.37])
@pytest.mark.parametrize("c", [1, 3, 9, 32])
def test_float_input(c, voxel_size):
    pts, attrs = float_cloud(c)
    g = V.voxel_grid(t(pts), t(attrs), voxel_size)
    check_grid(g, R.voxel_grid(pts, attrs, voxel_size), exact=False)
    again = V.voxel_grid(t(pts), t(attrs), voxel_size)
    for a, b in zip(g[:4], again[:4]):
        assert bits_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# run-length regimes
# ---------------------------------------------------------------------------------------------------------------------
def runs_cloud(lengths, c, seed):
    """One cell of the x axis per run (voxel size 1 from the origin, cells from x = -3 on), `lengths[i]` points in cell i,
    rows shuffled.  Positive attributes: no cancellation in the sums."""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.arange(len(lengths)) - 3, lengths)
    pts = rng.random((len(cell), 3)).astype(np.float32) * np.float32(0.999)
    pts[:, 0] += cell.astype(np.float32)
    attrs = rng.random((len(cell), c)).astype(np.float32) if c else None
    order = rng.permutation(len(cell))
    return pts[order], None if attrs is None else attrs[order]


def check_runs(lengths, c, seed=0):
    pts, attrs = runs_cloud(lengths, c, seed)
    ref = R.voxel_grid(pts, attrs, 1.0, origin=(0, 0, 0))
    assert ref[3].tolist() == list(lengths)
    x, a = t(pts), None if attrs is None else t(attrs)
    g = V.voxel_grid(x, a, 1.0, origin=(0, 0, 0))
    check_grid(g, ref, exact=False)
    again = V.voxel_grid(x, a, 1.0, origin=(0, 0, 0))
    assert bits_equal(g.points, again.points) and (a is None or bits_equal(g.attrs, again.attrs))


RUN_LENGTHS = sorted({1, 63, 64, 65, V.WAVE_RUN - 1, V.WAVE_RUN, V.WAVE_RUN + 1, V.SPLIT_RUN - 1, V.SPLIT_RUN, V.SPLIT_RUN + 1})


@pytest.mark.parametrize("c", [0, 3, 32])
@pytest.mark.parametrize("length", RUN_LENGTHS)
def test_run_of_every_regime_first_middle_and_last(length, c):
    """The run first in key order, between single rows, and last."""
    check_runs([length, 1, 1, 1, length, 1, 1, length], c)
    check_runs([1, 1, length, 1], c, seed=1)


@pytest.mark.parametrize("c", [0, 3, 9])
def test_runs_over_several_workgroups(c):
    """Split runs next to each other (a tile of the split pass then holds the tail of one and the head of the next), one over
    five tiles, runs of every regime between them, and the sixteen runs of one wave all long."""
    s, tile = V.SPLIT_RUN, V.TILE_ROWS
    check_runs([s + 52, s + 52, 1, 5 * tile + 17, s, 3, tile - 1, 1, s + tile, 40], c)
    check_runs([1, 7, 5 * tile, 2 * tile, 1], c, seed=2)                 # split runs that start and end on tile boundaries
    check_runs([V.WAVE_RUN + i for i in range(16)] + [3] * 16 + [200] * 17, c, seed=3)


@pytest.mark.parametrize("c", [0, 3, 32])
def test_whole_cloud_in_one_voxel(c):
    pts, attrs = runs_cloud([100003], c, 4)
    ref = R.voxel_grid(pts, attrs, 1.0, origin=(-3, 0, 0))
    assert ref[3].tolist() == [100003]
    g = V.voxel_grid(t(pts), None if attrs is None else t(attrs), 1.0, origin=(-3, 0, 0))
    check_grid(g, ref, exact=False)
    # and through the default origin with a voxel that holds everything
    g = V.voxel_grid(t(pts), None if attrs is None else t(attrs), 64.0)
    check_grid(g, R.voxel_grid(pts, attrs, 64.0), exact=False)
    assert g.counts.tolist() == [100003]


# ---------------------------------------------------------------------------------------------------------------------
# sizes, origin, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_sizes_zero_and_one():
    e = V.voxel_grid(torch.empty((0, 3), device=dev()), torch.empty((0, 5), device=dev()), 2.0)
    assert e.index.shape == (0, 3) and e.points.shape == (0, 3) and e.attrs.shape == (0, 5) and e.counts.shape == (0,)
    assert e.index.dtype == torch.int32 and e.counts.dtype == torch.int32 and e.index.is_cuda
    assert V.voxel_down_sample(torch.empty((0, 6), device=dev()), 1.0).shape == (0, 6)
    assert V.downscale(torch.empty((0, 6), device=dev()), 2).shape == (0, 6)
    assert V.voxelize(torch.empty((0, 6), device=dev()), bits=10)[0].shape == (0, 6)
    one = np.float32([[7.25, -3.5, 100.0, 0.25, 0.5, 0.75]])
    g = V.voxel_grid(t(one[:, :3]), t(one[:, 3:]), 2.0)
    check_grid(g, R.voxel_grid(one[:, :3], one[:, 3:], 2.0), exact=True)
    assert g.index.tolist() == [[0, 0, 0]] and g.counts.tolist() == [1] and bits_equal(g.points, one[:, :3])
    assert bits_equal(V.downscale(t(one), 2), R.downscale(one, 2))


def test_origin_rule_and_negative_indices():
    pts, attrs = float_cloud(3)
    x, a = t(pts), t(attrs)
    implicit = V.voxel_grid(x, a, 2.5)
    origin = pts.min(axis=0).astype(np.float64) - 2.5 / 2
    assert implicit.origin == tuple(origin.tolist())
    explicit = V.voxel_grid(x, a, 2.5, origin=origin)
    for u, v in zip(implicit[:4], explicit[:4]):
        assert bits_equal(u, v)
    g = V.voxel_grid(x, a, 2.5, origin=(40.0, 70.5, 31.0))
    ref = R.voxel_grid(pts, attrs, 2.5, origin=(40.0, 70.5, 31.0))
    assert ref[0][:, 0].min() == -16 and ref[0][:, 1].max() < 0 and ref[0][:, 2].max() > 0
    check_grid(g, ref, exact=False)


def test_refusals():
    def grid(z, **kw):
        return V.voxel_grid(t(np.float32([[0, 0, 0], [1, 2, z], [3, 1, 0]])), None, 1.0, **kw)
    lim = float(1 << 15)                # indices live in [-2^15, 2^15): 2^15 and -2^15 - 1 are the first ones outside
    for z in (lim, -lim - 1, 3e9, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(PccError, match="not finite or its voxel index"):
            grid(z, origin=(0, 0, 0))
    for z in (float("inf"), float("nan")):
        with pytest.raises(PccError, match="not finite"):
            grid(z)                                                   # the bounds of the default origin already show it
    with pytest.raises(PccError, match="voxel index"):
        V.voxel_grid(t(np.float32([[0, 0, 0], [1, 1, 1]])), None, 1e-5)
    with pytest.raises(PccError, match="not finite"):
        V.voxel_down_sample(t(np.float32([[0, 0, float("inf"), 0, 0, 0]])), 1.0)
    # the last indices inside the range, and the library is as usable as before
    g = grid(lim - 1, origin=(0, 0, 0))
    assert g.index.tolist() == [[0, 0, 0], [1, 2, int(lim) - 1], [3, 1, 0]]
    g = grid(-lim, origin=(0, 0, 0))
    assert g.index.tolist() == [[0, 0, 0], [1, 2, -int(lim)], [3, 1, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# voxelize / devoxelize, and the data pipeline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(bits=6, origin=None), dict(bits=7), dict(voxel_size=0.75), dict(voxel_size=1.5, origin=None)],
                         ids=["bits6_min", "bits7_zero", "size_zero", "size_min"])
def test_voxelize_end_to_end(kw):
    pts, attrs = float_cloud(3)
    cloud = np.concatenate([pts, np.abs(attrs) % 1], axis=1).astype(np.float32)
    vox, origin, vs = V.voxelize(t(cloud), **kw)
    m = vox.shape[0]
    ref = R.voxel_grid(pts, cloud[:, 3:], vs, origin=origin)
    assert bits_equal(vox[:, :3], ref[0].astype(np.float32)) and within_one_ulp(vox[:, 3:], ref[2])
    if "bits" in kw:                                                  # the farthest point lands in the last cell
        assert int(vox[:, :3].max()) == (1 << kw["bits"]) - 1 and int(vox[:, :3].min()) == 0
        extent = float((pts.astype(np.float64).max(axis=0) - np.asarray(origin)).max())
        assert vs >= extent / (1 << kw["bits"]) and vs <= extent / (1 << kw["bits"]) * (1 + 1e-12)
    # no duplicate coordinates: the canonical set keeps all rows
    coords = torch.cat([torch.zeros((m, 1), dtype=torch.int32, device=dev()), vox[:, :3].to(torch.int32)], dim=1).contiguous()
    cs, _, keep = S.coordset_from_coords(coords, 1)
    assert cs.n == m and keep is None
    # cell centres: within half a voxel (and the fp32 rounding of the centre) of EVERY input point of the cell, per axis
    back = to_np(V.devoxelize(vox, origin, vs))
    assert bits_equal(back[:, 3:], to_np(vox[:, 3:]))
    idx = R.indices(pts, vs, origin).astype(np.int64)
    row = {tuple(r): i for i, r in enumerate(ref[0].tolist())}
    centre = back[[row[tuple(r)] for r in idx.tolist()], :3].astype(np.float64)
    slack = vs / 2 * (1 + 2.0 ** -40) + np.spacing(np.float32(np.abs(pts).max() + vs))
    assert float(np.abs(centre - pts.astype(np.float64)).max()) <= slack


def test_with_the_data_pipeline(tmp_path):
    cloud = block_cloud()
    path = str(tmp_path / "block.ply")
    ply.write_ply(path, t(cloud))
    got = ply.read_ply(path, dev()).cloud
    assert bits_equal(got, cloud)
    down = V.downscale(got, 2)
    assert bits_equal(down, block_ref(2)[2])
    table = data.slice_into_cubes(down[:, :3].contiguous(), down[:, 3:].contiguous(), 16)
    assert table.points.shape[0] == down.shape[0] == 11031 and int(table.h_offsets[-1]) == 11031
    assert len(table) > 1 and int(table.num_points.sum()) == 11031
