"""GPU suite of the lossless attribute coder and the lossless geometry + colour codec: byte equality with
the numpy reference `tests/raht_lossless_ref.py` and exact round trips, on the fixtures of the CPU suite."""
import functools
import struct

import numpy as np
import pytest
import torch

from tests import raht_lossless_ref as Q
from tests import raht_ref as R
from tests.test_cpu_attributes_lossless import NAMES, canonical_levels, cases, coded
from tests.util import dev, t, n

pytestmark = pytest.mark.gpu


def _encode(name, **kw):
    from unified_point_cloud_compression_amd.attributes import encode_attributes_lossless
    pts, lv, colour = cases()[name]
    return encode_attributes_lossless(t(pts), colour=colour, attrs=t(lv), **kw)


@functools.lru_cache(maxsize=None)
def _gpu(name, predict=True):
    return _encode(name, predict=predict)


def _decode(data, name):
    from unified_point_cloud_compression_amd.attributes import decode_attributes_lossless
    got = decode_attributes_lossless(data, t(cases()[name][0]))
    assert got.dtype == torch.uint8 and got.is_cuda
    return n(got)


@pytest.mark.parametrize("predict", (True, False))
@pytest.mark.parametrize("name", NAMES)
def test_stream_equals_the_reference_and_decodes_to_the_input(name, predict):
    """Pins the colour transform, the lifting, the prediction, the row and symbol order, the member choice and the stored
    mode; the forced-coded reference stream also exercises the decoder where the encoder itself would store."""
    want = coded(name, predict)[0]
    data = _gpu(name, predict)
    assert data == want, f"{name}: {len(data)} bytes against the reference's {len(want)}"
    levels = canonical_levels(name)
    assert np.array_equal(_decode(data, name), levels)
    forced = coded(name, predict, stored=False)[0]
    if forced != want:
        assert np.array_equal(_decode(forced, name), levels)


def test_cloud_input_takes_its_colours():
    from unified_point_cloud_compression_amd import synth
    from unified_point_cloud_compression_amd.attributes import encode_attributes_lossless
    assert encode_attributes_lossless(t(synth.surface_cloud(0, 6))) == _gpu("surface6")


def test_several_streams_at_bits6():
    from unified_point_cloud_compression_amd.attributes import parse_lossless_header
    data = _encode("surface6", segment_symbols=2048)
    hdr = parse_lossless_header(data)
    assert hdr["streams"] == struct.unpack_from("<I", data, hdr["payload"][0])[0] == 5
    assert data == coded("surface6", True, 2048)[0] and data != _gpu("surface6")
    assert np.array_equal(_decode(data, "surface6"), canonical_levels("surface6"))


def _as_set(pts):
    from unified_point_cloud_compression_amd import sparse as S
    c4 = torch.cat([torch.zeros((len(pts), 1)), torch.from_numpy(pts[:, :3])], dim=1).to(dev())
    return S.coordset_from_coords(c4, 1)


def test_set_input_and_search_fallback_give_the_same_stream():
    """A pitch-1 CoordSet with attributes in its order is accepted and left alone, and the sorted-search fallback of the child
    and neighbour probes (sets without a grid index) produces the bytes and the levels of the bitmap path."""
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.attributes import encode_attributes_lossless, decode_attributes_lossless
    name = "shifted_surface6"
    pts, lv, _ = cases()[name]
    cs, perm, keep = _as_set(pts)
    assert keep is None
    lv_c = t(lv) if perm is None else t(lv)[perm]
    cs._on_lattice = False
    keys = cs.keys.clone()
    assert encode_attributes_lossless(cs, attrs=lv_c) == _gpu(name)
    assert cs._on_lattice is False and torch.equal(cs.keys, keys)
    assert np.array_equal(n(decode_attributes_lossless(_gpu(name), cs)), canonical_levels(name))
    old = S.USE_GRID
    try:
        S.USE_GRID = False
        data = _encode(name)
        back = _decode(data, name)
    finally:
        S.USE_GRID = old
    assert data == _gpu(name) and np.array_equal(back, canonical_levels(name))


def test_deterministic_and_blind_to_row_order():
    from unified_point_cloud_compression_amd.attributes import encode_attributes_lossless
    rng = np.random.default_rng(5)
    for name in ("surface6", "eight_channels"):
        pts, lv, colour = cases()[name]
        assert _encode(name) == _gpu(name)
        p = rng.permutation(len(pts))
        assert encode_attributes_lossless(t(pts[p]), colour=colour, attrs=t(lv[p])) == _gpu(name)


def test_stored_mode_is_chosen_on_extreme_colours_and_decodes():
    from unified_point_cloud_compression_amd.attributes import parse_lossless_header
    data = _gpu("extreme_block")
    hdr = parse_lossless_header(data)
    assert hdr["stored"] and len(data) == Q.HEADER.size + 3 * hdr["n"] and coded("extreme_block")[1]["stored"]
    assert np.array_equal(_decode(data, "extreme_block"), canonical_levels("extreme_block"))


def test_refusals():
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.attributes import encode_attributes_lossless, decode_attributes_lossless
    from unified_point_cloud_compression_amd.lib import PccError
    pts, lv, _ = cases()["surface6"]
    with pytest.raises(PccError):
        encode_attributes_lossless(t(np.concatenate([pts, pts[:7]])), attrs=t(np.concatenate([lv, lv[:7]])))      # duplicated rows
    with pytest.raises(PccError):
        encode_attributes_lossless(torch.from_numpy(pts), attrs=t(lv))     # CPU tensors
    with pytest.raises(PccError):
        encode_attributes_lossless(t(pts), attrs=torch.from_numpy(lv))
    c4 = torch.tensor([[0, 1, 2, 3], [1, 1, 2, 3], [1, 4, 4, 4]], dtype=torch.int32, device=dev())
    with pytest.raises(PccError):
        encode_attributes_lossless(S.coordset_from_coords(c4, 1)[0], attrs=torch.zeros((3, 3), dtype=torch.uint8, device=dev()))   # batched
    with pytest.raises(PccError):
        encode_attributes_lossless(t(pts), attrs=torch.zeros((len(pts), 9), dtype=torch.uint8, device=dev()))                      # C = 9
    with pytest.raises(PccError):
        encode_attributes_lossless(t(pts), attrs=t(lv[:-1]))
    data = _gpu("surface6")
    with pytest.raises(PccError):
        decode_attributes_lossless(data, t(pts[:-1]))                      # another n
    with pytest.raises(PccError):
        decode_attributes_lossless(data, t(pts * 2))                       # the same n at another depth
    with pytest.raises(PccError):
        decode_attributes_lossless(data, torch.from_numpy(pts))
    one = coded("one_channel", stored=False)[0]
    with pytest.raises(PccError):
        decode_attributes_lossless(one[:7] + bytes([one[7] | 1]) + one[8:], t(cases()["one_channel"][0]))          # colour flag, C = 1


def test_damaged_payload_is_rejected_or_bounded():
    """Asserts rejection or bounded output only.  Safe to run because nothing is sized by the payload: every buffer and launch
    of the decoder is sized by the geometry set, rows are addressed through the geometry's own scan, a symbol is clamped to
    +-1023 and every reconstructed value into its channel's range, and what the payload decoded to (rANS status, clamp flag)
    is read once at the end.  A handful of fixed corruptions, not a search."""
    from unified_point_cloud_compression_amd.attributes import decode_attributes_lossless, parse_lossless_header
    from unified_point_cloud_compression_amd.lib import PccError
    good = _gpu("surface7")
    hdr = parse_lossless_header(good)
    b0, b1 = hdr["payload"]
    words = b0 + 4 * (1 + hdr["streams"])
    geometry = t(cases()["surface7"][0])
    for at, flip in ((words + 1, 0x40), ((words + b1) // 2, 0x10), (b1 - 3, 0xFF), (words + 7, 0x01), (words + 4000, 0x80)):
        b = bytearray(good)
        b[at] ^= flip
        parse_lossless_header(bytes(b))                                    # the header walk cannot see it
        try:
            out = decode_attributes_lossless(bytes(b), geometry)
        except PccError:
            continue
        assert out.dtype == torch.uint8 and tuple(out.shape) == (hdr["n"], 3)


def test_a_stream_that_leaves_the_legal_range_is_refused():
    """A well-formed stream whose root does not belong to its symbols: the header walk accepts it, the reference's decoder
    (which raises where the kernels clamp) refuses it, and so must the device -- through the clamp flag, in its one read."""
    from unified_point_cloud_compression_amd.attributes import decode_attributes_lossless, parse_lossless_header
    from unified_point_cloud_compression_amd.lib import PccError
    good = coded("extreme_block", True, stored=False)[0]
    root = parse_lossless_header(good)["root"]
    rest = good[8 + sum(len(R._zigzag(q)) for q in root):]
    for y in (255, 0):
        bad = good[:8] + R._zigzag(y) + R._zigzag(root[1]) + R._zigzag(root[2]) + rest
        assert parse_lossless_header(bad)["root"] == [y, root[1], root[2]]
        with pytest.raises((ValueError, AssertionError)):
            Q.decode(bad, cases()["extreme_block"][0])
        with pytest.raises(PccError, match="legal range"):
            decode_attributes_lossless(bad, t(cases()["extreme_block"][0]))


# ---- the lossless codec ----------------------------------------------------------------------------------------------------
def test_lossless_round_trip_at_bits7():
    from unified_point_cloud_compression_amd import anchor, synth
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    pc = synth.surface_cloud(0, 7)
    pts, lv, _ = cases()["surface7"]
    data = anchor.compress_lossless(t(pc))
    g, a = anchor.parse_lossless_container(data)
    assert g == encode_geometry(t(pc)) and a == _gpu("surface7") and len(data) == 5 + len(g) + len(a)
    rec = anchor.decompress_lossless(data, dev())
    cells, lv_c = R.canonical(pts, lv)
    rec = n(rec)
    assert rec.dtype == np.float32 and rec.shape == (len(cells), 6) and np.array_equal(rec[:, :3], cells)
    assert np.array_equal(np.rint(rec[:, 3:].astype(np.float64) * 255), lv_c)
    again = anchor.decompress_lossless(anchor.compress_lossless(t(rec)), dev())        # what came out goes through unchanged
    assert np.array_equal(n(again), rec)


def test_lossless_codec_refuses_unvoxelised_input():
    from unified_point_cloud_compression_amd import anchor, synth
    from unified_point_cloud_compression_amd.lib import PccError
    pc = synth.surface_cloud(0, 6)
    moved = pc.copy()
    moved[3, 1] += 0.25
    with pytest.raises(PccError, match="voxelize.voxel_grid"):
        anchor.compress_lossless(t(moved))                                 # non-integer coordinates
    with pytest.raises(PccError, match="voxelize.voxel_grid"):
        anchor.compress_lossless(t(np.concatenate([pc, pc[:5]])))          # repeated voxels
    with pytest.raises(PccError):
        anchor.compress_lossless(torch.from_numpy(pc))
    with pytest.raises(PccError):
        anchor.decompress_lossless(b"\xc1" + anchor.compress_lossless(t(pc))[1:], dev())
