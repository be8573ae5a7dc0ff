"""CPU suite of the inter-frame RAHT attribute stream 0xB4 ("Inter frames"): the numpy reference
`tests/raht_inter_ref.py` decodes its own streams to the reconstruction its encoder predicts on every case of the lossless
inter suite at three quantisers, never loses to intra in "auto", its cases exercise what their names say, the host parser
accepts the reference's streams and refuses each damaged header before any GPU work, and on a moved surface the stream is at
most half the intra stream at no loss of Y-PSNR beyond 0.1 dB."""
import struct

import numpy as np
import pytest

from tests import raht_inter_ref as X
from tests import raht_lossless_inter_ref as LI
from tests import raht_ref as R

NAMES = tuple(X.cases())
QPS = X.QPS
AT = X.HEADER.size          # the root residuals begin here


def test_the_cases_and_quantisers_are_the_ones_the_suite_names():
    assert NAMES == tuple(LI.cases()) and QPS == (4, 28, 40)
    for name in ("c_mixed", "d_thinned", "f_two_voxels", "f_full_node", "f_depth3", "f_isolated", "g_negative_origin", "h_reference_empty",
                 "h_reference_outside", "i_one_channel", "i_eight_channels", "j_surface7_segmented", "k_escapes"):
        assert name in NAMES


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_decodes_what_its_encoder_predicts_and_auto_never_loses(name, qp):
    c = X.cases()[name]
    inter, rep = X.coded(name, qp)
    intra = X.intra_coded(name, qp)
    assert inter[0] == X.MAGIC and intra[0] == R.MAGIC
    back = X.decode(inter, c["cur"][0], *c["ref"])
    assert back.dtype == np.uint8 and back.shape == rep["recon"].shape and np.array_equal(back, rep["recon"])
    auto = X.encode(*c["cur"], qp, *c["ref"], mode="auto", colour=c["colour"], segment_symbols=c["segment_symbols"])
    assert len(auto) <= len(intra) and auto == (inter if len(inter) < len(intra) else intra)
    assert X.encode(*c["cur"], qp, *c["ref"], mode="intra", colour=c["colour"], segment_symbols=c["segment_symbols"]) == intra
    assert X.encode(*c["cur"], qp, colour=c["colour"], segment_symbols=c["segment_symbols"]) == intra             # no reference
    assert rep["blocks"] == len(rep["modes"]) and not (rep["modes"] & ~rep["has_match"]).any()


@pytest.mark.parametrize("qp", QPS)
def test_a_root_block_governs_the_dc(qp):
    """depth <= 4: the single block is the root and its mode decides whether the root DC travels as a residual."""
    from unified_point_cloud_compression_amd import attributes as A
    for name in ("f_two_voxels", "f_full_node", "f_depth3", "f_isolated"):
        rep = X.coded(name, qp)[1]
        assert rep["blocks"] == 1 and rep["first"] == 0 and rep["depth"] <= 4
        assert rep["mode1_blocks"] == 1                             # the reference is the cloud itself, moved at the most
        intra_dc = A.parse_header(X.intra_coded(name, qp))["dc"]
        assert max(abs(int(v)) for v in rep["root"]) <= 1 < max(abs(v) for v in intra_dc)
    assert X.coded("f_two_voxels", qp)[1]["depth"] == 1 and X.coded("f_full_node", qp)[1]["n"] == 8 and X.coded("f_depth3", qp)[1]["depth"] == 3
    one = X.cases()["f_two_voxels"]["cur"]
    assert X.encode(one[0][:1], one[1][:1], qp, one[0], one[1], mode="inter")[0] == R.MAGIC                 # n < 2 travels as intra


@pytest.mark.parametrize("qp", QPS)
def test_without_a_match_every_block_is_mode_0_and_the_symbols_are_the_intra_ones(qp):
    from unified_point_cloud_compression_amd import attributes as A
    for name in ("h_reference_empty", "h_reference_outside"):
        rep = X.coded(name, qp)[1]
        assert rep["matched"] == 0 and rep["mode1_blocks"] == 0 and not rep["prediction"].any()
        assert np.array_equal(rep["sym"], rep["intra_sym"]) and not rep["hist"][6 * rep["depth"]:].any()
        assert rep["root"].tolist() == A.parse_header(X.intra_coded(name, qp))["dc"]
        assert X.encode(*X.cases()[name]["cur"], qp, *X.cases()[name]["ref"], mode="auto") == X.intra_coded(name, qp)


def test_thinned_pins_the_floor_divided_block_mean():
    """Unmatched voxels inside mode-1 blocks take floor(sum / count): with chroma sums negative, truncation would differ."""
    c = X.cases()["d_thinned"]
    rep = X.coded("d_thinned", 28)[1]
    assert rep["unmatched_in_mode1"] > 0 and 0 < rep["mode1_blocks"]
    cells, _ = R.canonical(*c["cur"])
    ref_cells, ref_lv = LI.reference_rows(*c["ref"], 3)
    P, has, brow, m = X.prediction(cells, ref_cells, ref_lv, True)
    assert np.array_equal(P, rep["prediction"])
    rv = R.q8_values(ref_lv, True)
    sums = np.zeros((rep["blocks"], 3), dtype=np.int64)
    np.add.at(sums, brow[m >= 0], rv[m[m >= 0]])
    cnt = np.maximum(np.bincount(brow[m >= 0], minlength=rep["blocks"]), 1)[:, None]
    trunc = np.where(sums < 0, -(-sums // cnt), sums // cnt)
    lone = (m < 0) & rep["modes"][brow]
    assert (sums[brow[lone]][:, 1:] < 0).any() and (trunc[brow[lone]] != P[lone]).any()
    assert np.array_equal(P[lone], (sums // cnt)[brow[lone]])


def test_mixed_has_blocks_of_both_modes_and_both_group_sets():
    """The redrawn colours of c_mixed cover less than half of any 16^3 block (the cloud begins at y = 13, they end at y = 20), so
    with the whole block's rows in the sum all 13 blocks choose mode 1 at qp 4 and 28; at qp 40 two of them (11 of 13 mode 1)
    fall back, and rows inside the blocks then sit in both group sets.  The levels above the blocks keep their groups always."""
    for qp in QPS:
        rep = X.coded("c_mixed", qp)[1]
        depth, first = rep["depth"], rep["first"]
        assert first == 2 and 0 < rep["mode1_blocks"] <= rep["blocks"] == 13
        populated = rep["hist"].sum(axis=1) > 0
        assert populated[:6 * first].any() and populated[6 * depth:].any()
    rep = X.coded("c_mixed", 40)[1]
    assert 0 < rep["mode1_blocks"] < rep["blocks"]
    assert (rep["grp"] >= 6 * depth).any() and ((rep["grp"] >= 6 * first) & (rep["grp"] < 6 * depth)).any()


def test_origin_channels_segments_and_escapes():
    for qp in QPS:
        assert X.coded("g_negative_origin", qp)[1]["mode1_blocks"] > 0
        assert len(X.coded("g_negative_origin", qp)[0]) < len(X.intra_coded("g_negative_origin", qp))
        assert X.coded("i_one_channel", qp)[0][6] == 1 and X.coded("i_eight_channels", qp)[0][6] == 8
        assert X.coded("i_one_channel", qp)[0][7] == 0 and X.coded("g_negative_origin", qp)[0][7] == 1
        assert X.coded("j_surface7_segmented", qp)[1]["streams"] >= 3
    assert X.coded("k_escapes", 4)[1]["escapes"] > 0


# ---- the host parser ---------------------------------------------------------------------------------------------------------
def test_parser_reads_the_reference_streams():
    from unified_point_cloud_compression_amd import attributes as A
    for name in NAMES:
        data, rep = X.coded(name, 28)
        hdr = A.parse_header(data)
        assert hdr["inter"] and hdr["n"] == rep["n"] and hdr["depth"] == rep["depth"] and hdr["qp"] == 28
        assert (hdr["block_log2"], hdr["search"], hdr["blocks"]) == (X.BLOCK_LOG2, X.SEARCH, rep["blocks"])
        assert hdr["dc"] == rep["root"].tolist() and hdr["side"] == rep["side"].tolist() and len(hdr["side"]) == (rep["depth"] + 1) * 6
        assert hdr["streams"] == rep["streams"] and hdr["payload"][1] == len(data)
        m0, m1 = hdr["modes"]
        assert data[m0:m1] == np.packbits(rep["modes"], bitorder="little").tobytes()
        assert not A.parse_header(X.intra_coded(name, 28))["inter"]


def test_parser_refuses_each_damaged_header():
    """One refusal per rule of the stream: all on the host, before any GPU work."""
    from unified_point_cloud_compression_amd import attributes as A
    from unified_point_cloud_compression_amd.lib import PccError
    good = X.coded("b_shift_100", 28)[0]          # 13 blocks: three padding bits
    hdr = A.parse_header(good)

    def patched(at, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    bad = {
        "channels": patched(6, "<B", 9),
        "flags": patched(7, "<B", 2),
        "qp": patched(8, "<B", 3),
        "n beyond the limit": patched(1, "<I", 1 << 26),
        "n beyond the depth": patched(5, "<B", 1),
        "block_log2": patched(10, "<B", X.BLOCK_LOG2 - 1),
        "search": patched(11, "<B", X.SEARCH + 1),
        "depth 15": patched(5, "<B", 15),
        "n = 1": patched(1, "<I", 1),
        "blocks above n": patched(12, "<I", hdr["n"] + 1),
        "no blocks": patched(12, "<I", 0),
        "root residual": good[:AT] + b"\xfe\xff\xff\xff\x0f" + good[AT + 1:],
        "side byte": patched(hdr["modes"][0] - 1, "<B", 64),
        "padding bits": patched(hdr["modes"][1] - 1, "<B", good[hdr["modes"][1] - 1] | 0x80),
        "truncated header": good[:AT - 1],
        "truncated root": good[:AT],
        "truncated side bytes": good[:hdr["modes"][0] - 2],
        "truncated mode bytes": good[:hdr["modes"][1] - 1],
        "truncated container": good[:-4],
        "trailing bytes": good + b"\x00",
    }
    for why, data in bad.items():
        with pytest.raises(PccError):
            A.parse_header(data)
            pytest.fail(f"accepted: {why}")
    with pytest.raises(PccError, match="reference"):
        A.parse_header(good, have_reference=False)
    assert A.parse_header(good, have_reference=True)["blocks"] == 13
    assert not A.parse_header(X.intra_coded("b_shift_100", 28), have_reference=False)["inter"]
    with pytest.raises(PccError, match="magic"):
        A.parse_header(b"\xb2" + good[1:])


# ---- rate and quality on a moved surface ---------------------------------------------------------------------------------------
def test_moved_surface_halves_the_stream_at_the_same_quality():
    """surface_cloud(0, 7) moved by one voxel with its colours carried, against its own qp-28 decode: the inter stream is at most
    half the intra stream (framing included) and its Y-PSNR at most 0.1 dB below the intra decode's."""
    p, l, rp, rl = X.moved_surface(7, 28)
    inter, intra = X.encode(p, l, 28, rp, rl, mode="inter"), R.encode(p, l, 28)
    truth = R.canonical(p, l)[1]
    psnr_inter, psnr_intra = R.y_psnr(truth, X.decode(inter, p, rp, rl)), R.y_psnr(truth, R.decode(intra, p))
    print(f"inter {len(inter)} B {psnr_inter:.3f} dB, intra {len(intra)} B {psnr_intra:.3f} dB")
    assert inter[0] == X.MAGIC and 2 * len(inter) <= len(intra)
    assert psnr_inter >= psnr_intra - 0.1
    assert X.encode(p, l, 28, rp, rl, mode="auto") == inter
