"""CPU suite of the multi-rate / rate-targeted encoding: the pure-host parts of `rate.py` and the ABI
entry of the rate sweep (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_choose_picks_largest_prediction_within_budget():
    from unified_point_cloud_compression_amd.rate import choose
    # not monotone on purpose: nothing may rely on an order of the predictions
    pred = [900, 300, 700, 1200, 500]
    assert choose(pred, 800) == (2, True)
    assert choose(pred, 700) == (2, True)            # a prediction equal to the budget fits
    assert choose(pred, 699) == (4, True)
    assert choose(pred, 10 ** 9) == (3, True)
    assert choose(pred, 300) == (1, True)


def test_choose_without_a_fit_returns_smallest_prediction_and_says_so():
    from unified_point_cloud_compression_amd.rate import choose
    pred = [900, 300, 700, 1200, 500]
    assert choose(pred, 299) == (1, False)
    assert choose(pred, 0) == (1, False)
    assert choose([5], 4) == (0, False)


def test_choose_ties_go_to_the_earlier_index():
    from unified_point_cloud_compression_amd.rate import choose
    assert choose([400, 700, 700, 100, 700], 750) == (1, True)
    assert choose([400, 100, 700, 100], 50) == (1, False)
    assert choose([7, 7, 7], 7) == (0, True)         # adaptive_BN false: every candidate the same
    assert choose([7, 7, 7], 6) == (0, False)


def test_choose_exclude():
    from unified_point_cloud_compression_amd.rate import choose
    pred = [900, 300, 700, 1200, 500]
    assert choose(pred, 800, exclude=[2]) == (4, True)
    assert choose(pred, 800, exclude=(2, 4)) == (1, True)
    assert choose(pred, 800, exclude={1, 2, 4}) == (0, False)         # what is left does not fit: its smallest
    assert choose(pred, 299, exclude=[1]) == (4, False)
    assert choose(pred, 800, exclude=range(5)) == (None, False)
    assert choose([400, 700, 700], 750, exclude=[1]) == (2, True)


def test_q_grid_is_the_reference_grid():
    from unified_point_cloud_compression_amd.rate import q_grid
    g = q_grid()
    v = np.arange(11) * 0.1
    want = np.array([[q_g, q_a] for q_g in v for q_a in v]).astype(np.float32)      # q = [q_g, q_a], q_g outer
    assert g.dtype == np.float32 and g.shape == (121, 2)
    assert np.array_equal(g, want)
    assert np.array_equal(q_grid(3), np.array([[a, b] for a in (0, .5, 1) for b in (0, .5, 1)], dtype=np.float32))
    assert np.array_equal(q_grid(1), np.zeros((1, 2), dtype=np.float32))


def test_rate_sweep_symbol_declared_exported_and_bound():
    from unified_point_cloud_compression_amd import lib
    src = open(os.path.join(ROOT, "include", "pcc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pcc_gauss_rate_sweep\s*\(", src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "pcc_gauss_rate_sweep")
    res, args = lib.SIGNATURES["pcc_gauss_rate_sweep"]
    decl = re.search(r"pcc_gauss_rate_sweep\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert res is ctypes.c_int and len(args) == len(decl.split(",")) == 14
    assert lib.load().pcc_gauss_rate_sweep is not None


def _gc():
    from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional
    return GaussianConditional(None)


@pytest.mark.parametrize("n,c", [(24, 64), (1, 8), (3000, 64)])
def test_predicted_bytes_small_matrix_uses_the_size_rule(n, c):
    """Below ADAPTIVE_MIN_SYMBOLS the stream count follows from (n, c) alone: 4 bytes + 12 per stream around the payload."""
    from unified_point_cloud_compression_amd import rate
    gc = _gc()
    assert n * c < gc.ADAPTIVE_MIN_SYMBOLS
    ng, segs = gc.n_streams(n, c)
    for bits256 in (0, 1, 2048, 2049, 123456789):
        assert rate.stream_count(gc, n, c, bits256) == ng * segs
        assert rate.predicted_bytes(gc, n, c, bits256) == (bits256 + 2047) // 2048 + 4 + 12 * ng * segs


def test_predicted_bytes_adaptive_matrix_follows_the_estimate():
    """From ADAPTIVE_MIN_SYMBOLS on the encoder raises the segment count with the payload estimate (`_adaptive_segments`, as
    `StreamsJob.launch_encode` calls it): the prediction carries the framing of THAT plan."""
    from unified_point_cloud_compression_amd import rate
    gc = _gc()
    n, c = 13000, 128
    assert n * c >= gc.ADAPTIVE_MIN_SYMBOLS
    ng, segs = gc.n_streams(n, c)
    counts = set()
    for bits256 in (0, 2048 * 10 ** 4, 2048 * 10 ** 6, 2048 * 10 ** 7):
        want_segs = gc._adaptive_segments(n, c, ng, segs, bits256 / 2048.0)
        assert rate.stream_count(gc, n, c, bits256) == ng * want_segs
        assert rate.predicted_bytes(gc, n, c, bits256) == bits256 // 2048 + 4 + 12 * ng * want_segs
        counts.add(want_segs)
    assert len(counts) > 1 and min(counts) == segs          # the estimate does move the plan, never below the size rule
    # a 1 MB payload at the 2 % framing target: 0.02 * 2^20 / 12 = 1747 streams' worth, 13 segments for each of 128 groups
    assert rate.stream_count(gc, n, c, 2048 * (1 << 20)) == 128 * 13


def test_predicted_bytes_host_stream_has_no_container():
    from unified_point_cloud_compression_amd import rate
    from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional
    gc = GaussianConditional(None, entropy_coder="ans")
    assert rate.predicted_bytes(gc, 24, 64, 4097) == 3
