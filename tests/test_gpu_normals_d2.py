"""GPU suite: radius normal estimation (`pcc_normals_grid`, reference `evaluate.py:153`) and the point-to-plane (D2) report
(`pc_error`'s d2 keys, reference `utils.py:189-267`) against a numpy float64 restatement: brute-force neighbourhood over
the integer offsets with |d|^2 <= ceil(r^2) - 1, exact moments, `np.linalg.eigh` -- every normals case with the grid index
and with binary search."""
import math

import numpy as np
import pytest
import torch

from tests.util import dev, t, n

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[True, False], ids=["grid", "bsearch"])
def lookup_mode(request):
    from unified_point_cloud_compression_amd import sparse as S
    old = S.USE_GRID
    S.USE_GRID = request.param
    yield request.param
    S.USE_GRID = old


# ---- float64 restatement ------------------------------------------------------------------------------------------------
def _lim(radius):
    return math.ceil(radius * radius) - 1


def _offsets(lim):
    R = math.isqrt(lim)
    g = np.arange(-R, R + 1)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return d[(d * d).sum(1) <= lim]


def _enc(p):
    p = np.asarray(p, dtype=np.int64) + (1 << 20)
    return (p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2]


def _ref_moments(cloud, queries, radius):
    """Neighbourhood sizes and M = n S2 - S1 S1^T (int64 [m, 3, 3]) of every query point over the unique points of cloud."""
    keys = np.unique(_enc(cloud))
    q = np.asarray(queries, dtype=np.int64)
    cnt = np.zeros(len(q), dtype=np.int64)
    s1 = np.zeros((len(q), 3), dtype=np.int64)
    s2 = np.zeros((len(q), 3, 3), dtype=np.int64)
    for d in _offsets(_lim(radius)):
        k = _enc(q + d)
        i = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        hit = (keys[i] == k).astype(np.int64)
        cnt += hit
        s1 += hit[:, None] * d[None, :]
        s2 += hit[:, None, None] * np.outer(d, d)[None]
    M = cnt[:, None, None] * s2 - s1[:, :, None] * s1[:, None, :]
    return cnt, M


def _check_normals(got, cnt, M, where=""):
    """The accuracy bar: counts < 3 give exactly (0, 0, 1); with an eigen gap (l2 - l1) >= 1e-3 l3 the normal is the
    restatement's up to sign (1 - |n.n_ref| <= 1e-6); otherwise a unit vector with |M n - l1 n| <= 1e-6 l3.  Every normal
    has its largest-magnitude component positive (first axis on a tie)."""
    got = np.asarray(got, dtype=np.float32)
    assert np.isfinite(got).all(), where
    small = cnt < 3
    assert (got[small] == np.array([0, 0, 1], np.float32)).all(), where
    g64 = got[~small].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(g64, axis=1) - 1) <= 1e-6), where
    if (~small).any():
        w, V = np.linalg.eigh(M[~small].astype(np.float64))
        l1, l2, l3 = w[:, 0], w[:, 1], w[:, 2]
        gap = (l2 - l1) >= 1e-3 * l3
        dot = np.abs((g64 * V[:, :, 0]).sum(1))
        assert np.all(1 - dot[gap] <= 1e-6), (where, float((1 - dot[gap]).max()))
        res = np.linalg.norm(np.einsum("nij,nj->ni", M[~small][~gap].astype(np.float64), g64[~gap]) - l1[~gap, None] * g64[~gap],
                             axis=1)
        assert np.all(res <= 1e-6 * l3[~gap]), where
    a = np.abs(got)
    j = np.argmax(a, axis=1)                              # first maximum
    assert (got[np.arange(len(got)), j] > 0).all(), where


def _normals(xyz, radius):
    from unified_point_cloud_compression_amd import metrics
    nr, c = metrics.estimate_normals(t(np.ascontiguousarray(xyz, dtype=np.int32)), radius, return_counts=True)
    return n(nr), n(c)


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def _blob(seed, size=12, p=0.35, shift=(0, 0, 0)):
    """Random voxels of a box with its 8 corners and points on each of its 6 faces included, shifted (negative coordinates)."""
    rng = np.random.default_rng(seed)
    occ = rng.random((size, size, size)) < p
    e = size - 1
    for c in ((0, 0, 0), (e, 0, 0), (0, e, 0), (0, 0, e), (e, e, 0), (e, 0, e), (0, e, e), (e, e, e)):
        occ[c] = True
    m = size // 2
    for c in ((0, m, m), (e, m, m), (m, 0, m), (m, e, m), (m, m, 0), (m, m, e)):
        occ[c] = True
    xyz = np.argwhere(occ) + np.array(shift)
    return xyz[rng.permutation(len(xyz))]


def _surface(seed=0, bits=7):
    from unified_point_cloud_compression_amd import synth
    return synth.surface_cloud(seed, bits)[:, :3].astype(np.int64)


CLOUDS = {
    "blob": lambda: _blob(1),
    "blob_negative": lambda: _blob(2, shift=(-40, -3, -17)),
    "blob_sparse": lambda: _blob(3, size=16, p=0.08, shift=(-7, 5, -1)),
    "surface": lambda: _surface(0, 7),
}


# ---- 1 + 2: exact neighbourhoods and normals --------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1.0, 1.5, 5.0, 5.0000001, 8.0])
@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_neighbourhoods_and_normals_match_restatement(cloud, radius, lookup_mode):
    xyz = CLOUDS[cloud]()
    got, cnt = _normals(xyz, radius)
    ref_cnt, M = _ref_moments(xyz, xyz, radius)
    assert np.array_equal(cnt, ref_cnt), (cloud, radius)
    if radius == 1.0:
        assert (cnt == 1).all() and (got == np.array([0, 0, 1], np.float32)).all()
    _check_normals(got, ref_cnt, M, (cloud, radius))


def test_radius_limits():
    from unified_point_cloud_compression_amd import lib as L, metrics
    x = t(_blob(4).astype(np.int32))
    for r in (8.0001, 9.0, 0.0, -1.0):
        with pytest.raises(L.PccError):
            metrics.estimate_normals(x, r)
    _, M5 = _ref_moments(_blob(4), _blob(4), 5.0000001)
    assert _lim(5.0000001) == 25 and _lim(5.0) == 24 and _lim(8.0) == 63 and _lim(1.5) == 2 and _lim(1.0) == 0
    assert M5.shape[0] == _blob(4).shape[0]


def test_plane_normals_are_exact(lookup_mode):
    g = np.arange(20)
    X, Y = np.meshgrid(g, g, indexing="ij")
    plane = np.stack([X.ravel(), Y.ravel(), np.full(X.size, 7)], 1)
    for r in (1.5, 5.0, 8.0):
        got, cnt = _normals(plane, r)
        assert (cnt >= 3).all() and (got == np.array([0, 0, 1], np.float32)).all(), r
    diag = np.stack([X.ravel(), X.ravel(), Y.ravel() - 5], 1)        # the plane x = y
    got, cnt = _normals(diag, 5.0)
    ref = np.array([1, -1, 0]) / math.sqrt(2)
    err = np.minimum(np.abs(got - ref).max(1), np.abs(got + ref).max(1))
    assert (err <= 1e-6).all(), float(err.max())


def test_sphere_normals_are_near_radial(lookup_mode):
    R = 100
    g = np.arange(-R - 1, R + 2)
    pts = []
    for x in g:                                          # voxels whose centre lies within half a voxel of the sphere
        Y, Z = np.meshgrid(g, g, indexing="ij")
        rr = np.sqrt(x * x + Y * Y + Z * Z)
        m = np.abs(rr - R) < 0.5
        pts.append(np.stack([np.full(m.sum(), x), Y[m], Z[m]], 1))
    sph = np.concatenate(pts)
    got, cnt = _normals(sph, 5.0)
    rng = np.random.default_rng(7)
    s = rng.choice(len(sph), 4000, replace=False)
    ref_cnt, M = _ref_moments(sph, sph[s], 5.0)
    assert np.array_equal(cnt[s], ref_cnt)
    _check_normals(got[s], ref_cnt, M, "sphere")
    radial = sph / np.linalg.norm(sph, axis=1, keepdims=True)
    w, V = np.linalg.eigh(M.astype(np.float64))
    bound = float((1 - np.abs((V[:, :, 0] * radial[s]).sum(1))).max())   # how far from radial the restatement is
    dev_got = 1 - np.abs((got.astype(np.float64) * radial).sum(1))
    assert bound < 0.05 and float(dev_got[s].max()) <= bound + 1e-6


def test_degenerate_neighbourhoods(lookup_mode):
    pts = np.array([[0, 0, 0],                                        # isolated
                    [100, 0, 0], [101, 0, 0],                         # a pair
                    [200, 0, 0], [201, 0, 0], [202, 0, 0],            # collinear along x
                    [300, 300, 300], [301, 301, 301], [302, 302, 302],  # collinear along a diagonal
                    [400, 10, 5], [401, 12, 6], [402, 14, 7]])        # collinear, skew
    got, cnt = _normals(pts, 5.0)
    assert list(cnt) == [1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3]
    ref_cnt, M = _ref_moments(pts, pts, 5.0)
    assert np.array_equal(cnt, ref_cnt)
    _check_normals(got, ref_cnt, M, "degenerate")


def test_empty_single_and_duplicate_rows(lookup_mode):
    from unified_point_cloud_compression_amd import metrics
    e, c = metrics.estimate_normals(torch.zeros((0, 3), dtype=torch.int32, device=dev()), 5.0, return_counts=True)
    assert e.shape == (0, 3) and e.dtype == torch.float32 and c.shape == (0,)
    one, c = metrics.estimate_normals(t(np.array([[3, -4, 5]], np.int32)), 5.0, return_counts=True)
    assert n(one).tolist() == [[0.0, 0.0, 1.0]] and n(c).tolist() == [1]
    xyz = _blob(5)
    rng = np.random.default_rng(5)
    dup = np.concatenate([xyz, xyz[rng.choice(len(xyz), len(xyz) // 2)]])
    dup = dup[rng.permutation(len(dup))]
    base, bcnt = _normals(xyz, 5.0)
    got, cnt = _normals(dup, 5.0)
    where = {tuple(p): i for i, p in enumerate(xyz)}
    rows = np.array([where[tuple(p)] for p in dup])
    assert np.array_equal(got.view(np.int32), base[rows].view(np.int32)) and np.array_equal(cnt, bcnt[rows])
    gf = n(metrics.estimate_normals(t(dup.astype(np.float32) + 0.25), 5.0))   # float voxel coordinates floor to the same cells
    assert np.array_equal(gf.view(np.int32), got.view(np.int32))


# ---- 3: same bits ------------------------------------------------------------------------------------------------------------
def test_grid_and_search_paths_give_the_same_bits():
    from unified_point_cloud_compression_amd import metrics, sparse as S
    xyz = t(_surface(1, 8).astype(np.int32))
    old = S.USE_GRID
    try:
        out = {}
        for mode in (True, False):
            S.USE_GRID = mode
            a, ca = metrics.estimate_normals(xyz, 5.0, return_counts=True)
            b, cb = metrics.estimate_normals(xyz, 5.0, return_counts=True)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
            out[mode] = (a, ca)
    finally:
        S.USE_GRID = old
    assert torch.equal(out[True][0].view(torch.int32), out[False][0].view(torch.int32))
    assert torch.equal(out[True][1], out[False][1])


# ---- 4: D2 -------------------------------------------------------------------------------------------------------------------
def _plane(extent=20, z=0):
    g = np.arange(extent)
    X, Y = np.meshgrid(g, g, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1)


def _pm(a, b, **kw):
    from unified_point_cloud_compression_amd import metrics
    return metrics.pointcloud_metrics(t(np.ascontiguousarray(a, dtype=np.float32)), t(np.ascontiguousarray(b, dtype=np.float32)), **kw)


def test_d2_identical_and_shifted_planes():
    from unified_point_cloud_compression_amd import metrics
    a = _blob(6)
    r = _pm(a, a, point_to_plane=True)
    for p in ("AB_", "BA_", "sym_"):
        assert r[p + "d2_mse"] == 0 and r[p + "d2_psnr"] == math.inf
    p0 = _plane()
    r = _pm(p0, p0 + np.array([0, 0, 1]), point_to_plane=True)       # along the normal
    assert r["AB_d2_mse"] == 1.0 and r["BA_d2_mse"] == 1.0 and r["sym_d2_mse"] == 1.0
    assert r["AB_d2_psnr"] == 10 * math.log10(3 * 1023 ** 2)
    r = _pm(p0, p0 + np.array([1, 0, 0]), point_to_plane=True)       # within the plane
    assert r["AB_d2_mse"] == 0 and r["BA_d2_mse"] == 0 and r["AB_mse"] > 0 and r["BA_mse"] > 0
    ab, ba, sym = metrics.d2_psnr(t(p0.astype(np.float32)), t((p0 + np.array([0, 0, 1])).astype(np.float32)))
    assert ab == ba == sym == 10 * math.log10(3 * 1023 ** 2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_d2_matches_restatement(seed):
    """Same association (`nearest`), the build's own fp32 normals: the projection, the mean and the PSNR in float64."""
    from unified_point_cloud_compression_amd import metrics
    rng = np.random.default_rng(seed)
    a = _blob(10 + seed, size=16, p=0.3)
    b = a[rng.random(len(a)) < 0.7]
    b = b + rng.integers(-1, 2, b.shape)
    res = 511
    r = _pm(a, b, point_to_plane=True, resolution=res)
    ca, _ = metrics._canonical(t(a.astype(np.float32)))
    cb, _ = metrics._canonical(t(b.astype(np.float32)))
    na, nb = n(metrics.estimate_normals(ca, 5.0)).astype(np.float64), n(metrics.estimate_normals(cb, 5.0)).astype(np.float64)
    for pre, (P, Q, NQ) in (("AB_", (ca, cb, nb)), ("BA_", (cb, ca, na))):
        d2, nn = metrics.nearest(P, Q)
        nn = n(nn)
        PP, QQ = n(P).astype(np.float64), n(Q).astype(np.float64)
        proj = ((PP - QQ[nn]) * NQ[nn]).sum(1)
        mse = float((proj ** 2).mean())
        assert abs(r[pre + "d2_mse"] - mse) <= 1e-12 * mse, pre
        assert abs(r[pre + "d2_psnr"] - 10 * math.log10(3 * res ** 2 / mse)) <= 1e-9
        assert r[pre + "d2_mse"] <= 3 * r[pre + "mse"] * (1 + 1e-6)
        assert abs(3 * r[pre + "mse"] - float(n(d2).astype(np.float64).mean())) <= 1e-12 * 3 * r[pre + "mse"]
    assert r["sym_d2_mse"] == max(r["AB_d2_mse"], r["BA_d2_mse"])
    assert r["sym_d2_psnr"] == min(r["AB_d2_psnr"], r["BA_d2_psnr"])


def test_d2_user_normals():
    from unified_point_cloud_compression_amd import metrics
    rng = np.random.default_rng(3)
    a = _blob(20, size=14, p=0.3)
    b = a[rng.random(len(a)) < 0.8]
    b = b + rng.integers(-1, 2, b.shape)
    ex = np.array([[1, 0, 0]], np.float32)
    r = _pm(a, b, point_to_plane=True, source_normals=t(np.repeat(ex, len(a), 0)), reconstruction_normals=t(np.repeat(ex, len(b), 0)))
    ca, _ = metrics._canonical(t(a.astype(np.float32)))
    cb, _ = metrics._canonical(t(b.astype(np.float32)))
    for pre, (P, Q) in (("AB_", (ca, cb)), ("BA_", (cb, ca))):
        _, nn = metrics.nearest(P, Q)
        e = P[:, 0].to(torch.float64) - Q[nn.long(), 0].to(torch.float64)
        assert r[pre + "d2_mse"] == float((e * e).mean()), pre
    # the normals estimate_normals returns, in the caller's (shuffled, duplicated) row order == internal estimation
    ad = np.concatenate([a, a[:30]])[rng.permutation(len(a) + 30)]
    ta, tb = t(ad.astype(np.float32)), t(b.astype(np.float32))
    r_int = metrics.pointcloud_metrics(ta, tb, point_to_plane=True)
    r_usr = metrics.pointcloud_metrics(ta, tb, point_to_plane=True, source_normals=metrics.estimate_normals(ta),
                                       reconstruction_normals=metrics.estimate_normals(tb))
    assert r_int.keys() == r_usr.keys() and all(r_int[k] == r_usr[k] or (math.isnan(r_int[k]) and math.isnan(r_usr[k]))
                                                 for k in r_int)


def test_point_to_plane_off_is_the_d1_report():
    from oracle import metrics as ometrics
    from unified_point_cloud_compression_amd import metrics
    rng = np.random.default_rng(9)
    a = _blob(30, size=14).astype(np.float32)
    b = (a[rng.random(len(a)) < 0.8] + rng.integers(-1, 2, (1, 3))).astype(np.float32)
    pa = np.concatenate([a, rng.random((len(a), 3), dtype=np.float32)], 1)
    pb = np.concatenate([b, rng.random((len(b), 3), dtype=np.float32)], 1)
    off = metrics.pointcloud_metrics(t(pa), t(pb), resolution=63)
    on = metrics.pointcloud_metrics(t(pa), t(pb), resolution=63, point_to_plane=True)
    assert not any("d2" in k for k in off)
    assert list(off) == [k for k in on if "d2" not in k]
    assert all(off[k] == on[k] for k in off)
    ref = ometrics.pointcloud_metrics(pa, pb, 63)                    # the tolerance of test_gpu_codec's report check
    assert set(off) == set(ref)
    for k in ref:
        assert abs(off[k] - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])), k
    assert metrics.d1_psnr(t(a), t(b), 63) == (off["AB_psnr_mse"], off["BA_psnr_mse"], off["sym_psnr_mse"])


# ---- 5: full size --------------------------------------------------------------------------------------------------------------
def test_fullsize_normals_and_d2():
    import bench
    from unified_point_cloud_compression_amd import metrics, sparse as S, synth
    pc_np = synth.surface_cloud(0, 10)
    xyz = pc_np[:, :3].astype(np.int64)
    pc = t(pc_np)
    got, cnt = metrics.estimate_normals(pc[:, :3], 5.0, return_counts=True)
    got, cnt = n(got), n(cnt)
    assert got.shape == (787502, 3)
    assert np.isfinite(got).all() and np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) <= 1e-6)
    s = np.random.default_rng(20000).choice(len(xyz), 20000, replace=False)
    ref_cnt, M = _ref_moments(xyz, xyz[s], 5.0)
    assert np.array_equal(cnt[s], ref_cnt)
    _check_normals(got[s], ref_cnt, M, "bench frame")
    old = S.USE_GRID
    try:
        S.USE_GRID = False
        srch = n(metrics.estimate_normals(pc[:, :3], 5.0))
    finally:
        S.USE_GRID = old
    assert np.array_equal(srch.view(np.int32), got.view(np.int32))
    model = bench.build_model(dev(), coder="symbols")
    q = torch.tensor([[0.5, 0.5]], device=dev())
    out = model.compress(pc, q, block_size=1024)
    rec = model.decompress(coordinates=out[3], strings=out[0], shape=out[1], k=out[2], q_vals=out[4])
    r = metrics.pointcloud_metrics(pc, rec, 1023, point_to_plane=True)
    assert math.isfinite(r["sym_d2_psnr"]) and r["sym_d2_psnr"] >= r["sym_psnr_mse"] - 1e-6
    for p in ("AB_", "BA_"):
        assert r[p + "d2_mse"] <= 3 * r[p + "mse"] * (1 + 1e-6)
