"""CPU suite of the predicted RAHT colour stream 0xB9 ("Prediction from the parent level"): the numpy
reference `tests/raht_pred_ref.py` against itself (the decoder returns the encoder's closed-loop reconstruction), the kernels'
arithmetic through its host exports against Python integers, the bounds of the rule, the header, and the two conditions the
stream exists for: shorter than 0xB3, and no worse in luma PSNR."""
import ctypes as C
import functools
import json
import math
import os
import struct

import numpy as np
import pytest

from tests import raht_lossless_ref as LL
from tests import raht_pred_ref as P
from tests import raht_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _surface(bits, smooth):
    from unified_point_cloud_compression_amd import synth
    pc = synth.surface_cloud(0, bits)
    return pc, R.levels_of(LL.noise_free_colours(pc, bits) if smooth else pc[:, 3:])


@functools.lru_cache(maxsize=None)
def _coded(bits, smooth, qp):
    """(0xB9 bytes, the encoder's reconstruction, what the reference decoder returns)."""
    pc, lv = _surface(bits, smooth)
    data, rec = P.encode(pc, lv, qp)
    return data, rec, P.decode(data, pc)


@functools.lru_cache(maxsize=None)
def _plain(bits, smooth, qp):
    pc, lv = _surface(bits, smooth)
    data = R.encode(pc, lv, qp)
    return data, R.decode(data, pc)


@pytest.mark.parametrize("qp", (4, 28, 46))
@pytest.mark.parametrize("smooth", (False, True))
@pytest.mark.parametrize("bits", (6, 7))
def test_decoder_returns_the_encoders_reconstruction(bits, smooth, qp):
    data, rec, back = _coded(bits, smooth, qp)
    pc, lv = _surface(bits, smooth)
    assert data[0] == 0xB9 and back.dtype == np.uint8 and back.shape == lv.shape and np.array_equal(back, rec)
    if qp == 4:                                                            # step 1.0: the closed loop loses nothing beyond the plain stream's rounding
        assert R.y_psnr(R.canonical(pc, lv)[1], rec) >= 58.0


def _small_cases():
    rng = np.random.default_rng(11)
    block = np.unique(rng.integers(0, 24, (900, 3)), axis=0)
    return {
        "one_channel": (block, rng.integers(0, 256, (len(block), 1)).astype(np.uint8), False),
        "eight_channels": (block, rng.integers(0, 256, (len(block), 8)).astype(np.uint8), False),
        "two_voxels": (np.array([[5, 9, 2], [5, 9, 3]]), np.array([[9, 200, 31], [250, 3, 77]], dtype=np.uint8), True),
        "lone_child_chain": (np.array([[0, 0, 0], [63, 63, 63]]), np.array([[9, 200, 31], [250, 3, 77]], dtype=np.uint8), True),
    }


@pytest.mark.parametrize("name", sorted(_small_cases()))
def test_round_trip_of_the_small_shapes(name):
    pts, lv, colour = _small_cases()[name]
    for qp in (4, 28, 46):
        data, rec = P.encode(pts, lv, qp, colour=colour, segment_symbols=64)
        assert np.array_equal(P.decode(data, pts), rec) and rec.shape == lv.shape
    if name == "lone_child_chain":
        assert data[5] == 6 and struct.unpack_from("<I", data, 1)[0] == 2   # depth 6: five levels of a lone child below the root's one butterfly


def test_exported_arithmetic_equals_python_integers():
    """`pcc_raht_pred_mean` / `_scale` / `_predict` are the kernels' own functions compiled for the host."""
    from unified_point_cloud_compression_amd import lib
    so = lib.load()
    out = C.c_int64()
    rng = np.random.default_rng(2)
    for w in (1, 2, 3, 1 << 13, (1 << 26) - 2):
        top = math.isqrt(w) * 65280 + 65280                               # the DC bound of DESIGN.md 7f
        dcs = [0, 1, -1, top, -top, top // 2 + 1, -(top // 3)] + [int(v) for v in rng.integers(-top, top + 1, 40)]
        a = math.isqrt(((1 << 32) // w) << 28)
        for dc in dcs:
            assert so.pcc_raht_pred_mean(dc, w, C.byref(out)) == 0
            want = (a * dc + (1 << 29)) >> 30
            assert out.value == want == int(P.mean(np.array([[dc]], dtype=np.int64), np.array([w], dtype=np.int64))[0, 0])
            if w == 1:
                assert want == dc
            assert abs(want) <= 65280 + 65280 // math.isqrt(w) + 1
        s = math.isqrt(w << 32)
        for pred in (0, 1, -1, 65280, -65280, 35190, -35190, 1 << 24, -(1 << 24)) + tuple(int(v) for v in rng.integers(-70000, 70000, 40)):
            assert so.pcc_raht_pred_scale(pred, w, C.byref(out)) == 0
            want = (pred * s + (1 << 15)) >> 16
            assert out.value == want
            if abs(want) <= P.LIMIT:
                assert want == int(P.scale(np.array([[pred]], dtype=np.int64), np.array([w], dtype=np.int64))[0, 0])
    assert so.pcc_raht_pred_mean(0, 0, C.byref(out)) != 0 and so.pcc_raht_pred_mean(0, 1 << 26, C.byref(out)) != 0
    assert so.pcc_raht_pred_mean((1 << 30) + 1, 1, C.byref(out)) != 0 and so.pcc_raht_pred_scale((1 << 24) + 1, 1, C.byref(out)) != 0


def test_prediction_over_all_presence_masks():
    from unified_point_cloud_compression_amd import lib
    so = lib.load()
    rng = np.random.default_rng(4)
    got = C.c_int32()
    wt = [LL.CELL_WEIGHT[bin(b).count("1")] for b in range(8)]
    for mask in range(1, 256):
        for vals in (rng.integers(-35190, 65281, 8), rng.integers(-(1 << 24), (1 << 24) + 1, 8), np.full(8, -(1 << 24)), np.full(8, 1 << 24)):
            have = [(mask >> b) & 1 for b in range(8)]
            den = sum(w * h for w, h in zip(wt, have))
            num = sum(w * h * int(v) for w, h, v in zip(wt, have, vals))
            want = (num + (den >> 1)) // den                               # Python's floor division: Cb and Cr are signed
            assert so.pcc_raht_pred_predict((C.c_int32 * 8)(*[int(v) for v in vals]), mask, C.byref(got)) == 0
            assert got.value == want == int(LL.predict_cell(np.asarray(vals, dtype=np.int64), np.array(have, dtype=np.int64)))
    assert so.pcc_raht_pred_predict((C.c_int32 * 8)(), 0, C.byref(got)) != 0
    assert so.pcc_raht_pred_predict((C.c_int32 * 8)(*([(1 << 24) + 1] * 8)), 255, C.byref(got)) != 0


def test_bounds_of_the_worst_case_chain():
    """All values 255 (Q8 65 280, the largest magnitude any channel takes) and weights doubling up to n = 2^26 - 1, in Python
    integers: a mean stays below 2^17, the 64 weighted means of a prediction sum below 2^23 (int32), a scaled prediction P and
    therefore Hp below 2^29 like the DCs they stand in for, every product below 2^62, and |H - Hp| below the 2^30 clamp."""
    top = 0

    def merge(w1, x1, w2, x2):
        nonlocal top
        w = w1 + w2
        a, b = math.isqrt(((w1 << 32) // w) << 28), math.isqrt(((w2 << 32) // w) << 28)
        top = max(top, abs(a * x1), abs(b * x2), abs(a * x2), abs(b * x1))
        return w, (a * x1 + b * x2 + (1 << 29)) >> 30, (a * x2 - b * x1 + (1 << 29)) >> 30

    def check(w, dc):
        nonlocal top
        a = math.isqrt(((1 << 32) // w) << 28)
        m = (a * dc + (1 << 29)) >> 30
        top = max(top, a * dc)
        assert 65280 - 4 <= m <= 65280 + 64 < (1 << 17)                    # the mean of a constant signal is the constant, up to the stages' roundings
        assert 64 * (m + 1) < (1 << 23)                                    # sum wt <= 64: num + (den >> 1) in int32
        return m

    w, x = 1, 255 << 8
    worst_p = 0
    while w < (1 << 26):
        m = check(w, x)
        for wc in {max(1, w // 8), max(1, w // 2), max(1, w - 1)}:         # a child's weight is below its parent's
            s = math.isqrt(wc << 32)
            p = (m * s + (1 << 15)) >> 16
            top = max(top, m * s)
            worst_p = max(worst_p, p)
            assert p < (1 << 29)
            # the butterfly of two such predictions of opposite sign (signed chroma), the largest |Hp|: below 2^29 like the true
            # |H| of the same values, so |H - Hp| < 2^30 whatever their signs
            if 2 * wc < (1 << 26):
                _, lo, hi = merge(wc, p, wc, -p)
                assert abs(lo) < (1 << 29) and abs(hi) < (1 << 29)
        if 2 * w >= (1 << 26):
            break
        w, x, _ = merge(w, x, w, x)
    w, x, _ = merge(w, x, w - 1, x)
    assert w == (1 << 26) - 1 and x < (1 << 29)
    check(w, x)
    print(f"largest scaled prediction 2^{math.log2(worst_p):.2f}, largest product 2^{math.log2(top):.2f}")
    assert top < (1 << 62)


def test_measured_residual_stays_far_below_the_clamp():
    rep = {}
    pc, lv = _surface(7, False)
    P.encode(pc, lv, 4, report=rep)
    print(f"largest |H - Hp| on surface_cloud(0, 7): {rep['max_abs_residual']}")
    assert rep["max_abs_residual"] < (1 << 22)


def _valid_stream():
    rng = np.random.default_rng(3)
    pts = np.unique(rng.integers(0, 16, (300, 3)), axis=0)
    lv = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    return P.encode(pts, lv, 28, segment_symbols=256)[0], R.encode(pts, lv, 28, segment_symbols=256), len(pts)


def test_parse_header_reads_the_predicted_stream_and_rejects_damage():
    from unified_point_cloud_compression_amd import attributes as A
    from unified_point_cloud_compression_amd.lib import PccError
    good, plain, n = _valid_stream()
    h = A.parse_header(good)
    assert h["predict"] is True and h["inter"] is False
    assert (h["n"], h["depth"], h["channels"], h["colour"], h["qp"], h["chroma_qp_offset"]) == (n, 4, 3, True, 28, -2)
    assert h["streams"] == -(-(n - 1) * 3 // 256) and h["payload"][1] == len(good) and len(h["side"]) == 24
    assert "predict" not in A.parse_header(plain)                          # the key exists for 0xB9 only
    assert A.KINDS[0xB9].name == "predicted attribute stream" and A.KINDS[0xB9].head is A.HEADER and A.KINDS[0xB9].rule is A._dc_rule
    for cut in range(h["payload"][0] + 8 + 1):                             # every cut up to 8 bytes into the container
        with pytest.raises(PccError):
            A.parse_header(good[:cut])
    with pytest.raises(PccError, match="trailing"):
        A.parse_header(good + b"\x00")
    with pytest.raises(PccError, match="magic byte 0xb9"):
        A.parse_lossless_header(good)
    for at, value, word in ((8, 3, "qp 3"), (6, 9, "9 channels"), (7, 2, "flags"), (5, 0, "depth 0")):
        b = bytearray(good)
        b[at] = value
        with pytest.raises(PccError, match=word):
            A.parse_header(bytes(b))
    one = bytearray(R.encode(np.array([[3, 4, 5]]), np.array([[9, 200, 7]], dtype=np.uint8), 28))
    A.parse_header(bytes(one))
    one[0] = 0xB9                                                          # fewer than two voxels travel as 0xB3
    with pytest.raises(PccError, match="predicted attribute stream"):
        A.parse_header(bytes(one))
    with pytest.raises(PccError, match="0xb3, 0xb4 and 0xb8"):             # the wording of the foreign-magic refusal stays
        A.parse_header(b"\xba" + good[1:])


RATE_CASES = [(smooth, qp) for smooth in (False, True) for qp in (22, 28, 34)]


@pytest.mark.parametrize("smooth,qp", RATE_CASES)
def test_predicted_stream_is_strictly_shorter(smooth, qp):
    pred, plain = _coded(7, smooth, qp)[0], _plain(7, smooth, qp)[0]
    print(f"surface7 smooth={smooth} qp {qp}: 0xB3 {len(plain)} B, 0xB9 {len(pred)} B")
    assert len(pred) < len(plain)


def test_luma_psnr_is_not_below_the_plain_streams():
    """Both streams bound every coefficient's error by step / 2, so the luma PSNRs agree apart from rounding.  The allowance is
    the worst shortfall the integer reference measured over these cases (profiles/attribute_pred_rate.json: 0.0 dB, the
    predicted stream is better in every one: +0.09 .. +0.82 dB on the noisy colours, +4.5 .. +5.2 dB on the smooth ones) plus
    0.05 dB, and never more than 0.1 dB."""
    with open(os.path.join(ROOT, "profiles", "attribute_pred_rate.json")) as f:
        measured = json.load(f)["worst_y_psnr_shortfall_db"]
    allow = min(measured + 0.05, 0.1)
    assert 0.0 <= measured and allow <= 0.1
    for smooth, qp in RATE_CASES:
        pc, lv = _surface(7, smooth)
        orig = R.canonical(pc, lv)[1]
        gain = R.y_psnr(orig, _coded(7, smooth, qp)[1]) - R.y_psnr(orig, _plain(7, smooth, qp)[1])
        print(f"surface7 smooth={smooth} qp {qp}: y_psnr(0xB9) - y_psnr(0xB3) = {gain:+.4f} dB (allowed shortfall {allow:.2f})")
        assert gain >= -allow
