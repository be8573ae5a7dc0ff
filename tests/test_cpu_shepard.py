"""CPU suite: the Shepard's-loss ablation (`configs/CVPR_inverse_scaling_shepard.yaml`) is accepted by `Loss`, its window is
`create_window_3D` (`loss.py:192-219`), and the channelwise convolution refuses what it does not implement (no GPU needed)."""
import numpy as np
import pytest

SHEPARD_LOSS_CFG = {   # `configs/CVPR_inverse_scaling_shepard.yaml`, loss block
    "Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
    "ColorLoss": {"type": "ShepardsLoss", "loss": "L2", "window_size": 9, "p": 8},
    "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0},
    "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0},
}


def _window_np(ws, p):
    r = ws // 2
    a = np.arange(ws, dtype=np.int64) - r
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    d = np.sqrt((x ** 2 + y ** 2 + z ** 2).astype(np.float32))
    w = (np.float32(1) / (d ** np.float32(p) + np.float32(1e-5))).astype(np.float32)
    w[d > r] = 0
    return w.reshape(-1, 1)


def test_loss_accepts_shepard_config():
    from unified_point_cloud_compression_amd.loss import Loss, ShepardsLoss
    loss = Loss(SHEPARD_LOSS_CFG)
    s = loss.losses["ColorLoss"]
    assert isinstance(s, ShepardsLoss)
    assert s.identifier == "ColorLoss" and s.p == 8 and s.window_size == 9
    assert tuple(s.conv_sum.kernel.shape) == (729, 1) and not s.conv_sum.kernel.requires_grad


@pytest.mark.parametrize("ws,p", [(9, 8), (7, 2), (5, 1), (3, 8)])
def test_window_matches_create_window_3d(ws, p):
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    s = ShepardsLoss({"id": "c", "loss": "L1", "window_size": ws, "p": p})
    ref = _window_np(ws, p)
    w = s.window.numpy()
    assert w.dtype == np.float32 and w.shape == (ws ** 3, 1)
    np.testing.assert_allclose(w, ref, rtol=1e-6, atol=0)
    assert np.array_equal(w == 0, ref == 0)
    if (ws, p) == (9, 8):
        assert int((w != 0).sum()) == 257
        assert s._taps.ntaps == 257 and s._taps.ncol == 49


def test_shepard_refuses_unsupported_windows():
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    for ws in (8, 11):
        with pytest.raises(L.PccError):
            ShepardsLoss({"id": "c", "loss": "L2", "window_size": ws, "p": 8})


def test_channelwise_conv_refusals():
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import lib as L
    bad = [(dict(kernel_size=3, stride=2), "stride"), (dict(kernel_size=3, dilation=2), "dilation"),
           (dict(kernel_size=3, bias=True), "bias"), (dict(kernel_size=11), "kernel_size 11"), (dict(kernel_size=4), "kernel_size 4")]
    for kw, what in bad:
        m = ME.MinkowskiChannelwiseConvolution(4, dimension=3, **kw)
        with pytest.raises(L.PccError, match=what):
            m(None)        # refused, naming the reason, before the input is looked at
    # the constructor keeps MinkowskiEngine's parameter shape
    assert tuple(ME.MinkowskiChannelwiseConvolution(4, kernel_size=3, dimension=3).kernel.shape) == (27, 4)


def test_channelwise_size_queries():
    from unified_point_cloud_compression_amd import lib
    L = lib.load()
    assert L.pcc_chconv_supported(9, 4) and L.pcc_chconv_supported(1, 1) and L.pcc_chconv_supported(3, 64)
    assert not L.pcc_chconv_supported(11, 4) and not L.pcc_chconv_supported(4, 4) and not L.pcc_chconv_supported(3, 65)
    assert L.pcc_chconv_wgrad_ws_bytes(100, 257, 4) >= 257 * 4 * 4
    assert L.pcc_chconv_wgrad_ws_bytes(10 ** 8, 729, 64) <= 128 * 729 * 64 * 4 + 256


def test_tap_table_columns():
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd import sparse as S
    t = S.channelwise_full_taps(3)
    assert t.ntaps == 27 and t.ncol == 9 and sorted(t.widx) == list(range(27))
    for i in range(t.ncol):
        dx, dy, zm, first = t.table[4 * i:4 * i + 4]
        assert zm == 0b111
        for j in range(3):
            assert t.taps[t.widx[first + j]] == (dx, dy, j - 1)
    n = t.negated()
    assert [n.taps[k] for k in range(27)] == [(-a, -b, -c) for a, b, c in t.taps]
    with pytest.raises(L.PccError):
        S.ChannelwiseTaps([(0, 0, 0), (0, 0, 0)], 3)
    with pytest.raises(L.PccError):
        S.ChannelwiseTaps([(2, 0, 0)], 3)
