"""CPU suite: the argument checks of `metrics.pcqm` (they raise before any launch), and the numpy restatement of the metric
(tests/pcqm_ref.py, the oracle of tests/test_gpu_pcqm.py) against the properties the definition must have."""
import numpy as np
import pytest
import torch

from tests import pcqm_ref as P


def _cloud(n=8, colour=True):
    g = torch.Generator().manual_seed(3)
    xyz = torch.randint(0, 16, (n, 3), generator=g).to(torch.float32)
    return torch.cat([xyz, torch.rand((n, 3), generator=g)], dim=1) if colour else xyz


@pytest.mark.parametrize("kw", [dict(radius=0.0), dict(radius=-1.0), dict(radius=8.6), dict(radius=float("nan")),
                                dict(radius=17.5, radius_factor=1.0), dict(radius=4.0, radius_factor=0.5),
                                dict(radius=4.0, radius_factor=4.5)])
def test_radius_range_raises_before_any_launch(kw):
    from unified_point_cloud_compression_amd import metrics as M
    from unified_point_cloud_compression_amd.lib import PccError
    for fn in (M.pcqm, M.pcqm_features):
        with pytest.raises(PccError, match="radii"):
            fn(_cloud(), _cloud(), **kw)


def test_radius_bounds_are_inclusive_where_the_issue_says_so():
    from unified_point_cloud_compression_amd import metrics as M
    assert M._pcqm_radii(8.5, None, 2.0) == (8.5, 17.0)
    r, h = M._pcqm_radii(None, 0.004, 2.0, extent=2047)                              # vox11
    assert abs(r - 8.188) < 1e-12 and h == 2.0 * r
    assert M._pcqm_lim(16.38) == 268 and M._pcqm_lim(17.0) == 288 and M._pcqm_lim(4.1) == 16


def test_empty_colourless_and_cpu_inputs_raise():
    from unified_point_cloud_compression_amd import metrics as M
    from unified_point_cloud_compression_amd.lib import PccError
    with pytest.raises(PccError, match="empty"):
        M.pcqm(_cloud(), _cloud()[:0], radius=4.0)
    with pytest.raises(PccError, match="colour"):
        M.pcqm(_cloud(), _cloud(colour=False), radius=4.0)
    with pytest.raises(PccError, match="colour"):
        M.pcqm(_cloud(colour=False), _cloud(), radius=4.0)
    with pytest.raises(PccError, match="GPU tensors"):
        M.pcqm(_cloud(), _cloud(), radius=4.0)
    with pytest.raises(PccError, match="GPU tensors"):
        M.curvature(_cloud(), 4.0)


def test_constants_match_the_restatement():
    from unified_point_cloud_compression_amd import metrics as M
    assert (M.PCQM_K, M.PCQM_C1, M.PCQM_C2, M.PCQM_C3, M.PCQM_C4, M.PCQM_C5) == (P.K, P.C1, P.C2, P.C3, P.C4, P.C5)
    assert [M.PCQM_WEIGHTS.get("f%d" % (k + 1), 0.0) for k in range(8)] == list(P.WEIGHTS)


def test_lab_of_known_colours():
    lab = P.rgb_to_lab(np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))
    assert np.abs(lab[0] - [100.0, 0.0, 0.0]).max() < 2e-3 and np.abs(lab[1]).max() < 1e-12
    assert np.abs(lab[2] - [53.2408, 80.0925, 67.2032]).max() < 2e-3                 # sRGB red, D65
    rgb = torch.tensor([[0.2, 0.5, 0.9], [0.01, 0.02, 0.0]], dtype=torch.float64)
    from unified_point_cloud_compression_amd import metrics as M
    got = M.rgb_to_lab(rgb).numpy()
    assert np.abs(got - P.rgb_to_lab(rgb.numpy())).max() < 1e-12


@pytest.fixture(scope="module")
def shell20():
    src = P.cloud("shell20")
    return src, P.reconstruction(src)


def test_restatement_curvature_of_a_sphere(shell20):
    pts = P.canonical(shell20[0])[0][:, :3].astype(np.int64)
    assert len(pts) == 5034
    rho, info = P.curvature(pts, 4.1)
    assert abs(rho.mean() - 1 / 20) <= 0.05 / 20, rho.mean()
    assert info["comparable"].all() and info["cond"].max() < 1e4
    rev = P.curvature(pts, 4.1, reverse=True)[0]
    assert np.abs(rev - rho).max() < 1e-13


def test_restatement_properties():
    src = P.cloud("sheet48")
    rec, worse = P.reconstruction(src), P.reconstruction(src, sigma=30.0)
    assert len(src) == 2304 and len(rec) == round(0.7 * 2304)
    same = P.pcqm(src, src, 4.1, 8.2)
    assert abs(same["pcqm"]) <= 1e-12 and np.abs(same["features"]).max() <= 1e-12
    a, b = P.pcqm(src, rec, 4.1, 8.2), P.pcqm(src, worse, 4.1, 8.2)
    assert 0 < a["pcqm"] < b["pcqm"]
    assert np.isfinite(a["features"]).all() and (a["features"][:, [0, 1, 2, 3, 4, 6, 7]] >= 0).all()
    again = P.pcqm(src, rec, 4.1, 8.2)
    assert np.array_equal(a["features"], again["features"])
    # rows shuffled, duplicates behind their firsts: the same canonical result, and `rows` leads back to the caller's order
    rng = np.random.default_rng(5)
    rows = np.concatenate([src[rng.permutation(len(src))], src[:50] * [1, 1, 1, 0, 0, 0]], axis=0)
    sh = P.pcqm(rows, rec, 4.1, 8.2)
    assert np.array_equal(sh["features"], a["features"])
    assert np.array_equal(P.canonical(rows)[0][sh["rows"]][:, :3], rows[:, :3])


def test_restatement_on_tiny_clouds():
    for name in ("one", "two"):
        src = P.cloud(name)
        r = P.pcqm(src, src, 4.1, 8.2)
        assert (r["rho_r"] == 0).all() and np.isfinite(r["features"]).all() and abs(r["pcqm"]) <= 1e-12
    d = P.offsets(16.38)
    assert (d * d).sum(axis=1).max() <= 268 and np.abs(d).max() == 16
    assert np.array_equal(d, d[np.lexsort((d[:, 2], d[:, 1], d[:, 0]))])             # dx, then dy, then dz ascending
