"""GPU suite of the inter-frame RAHT attribute coder ("Inter frames", stream 0xB4): byte equality with
the numpy reference `tests/raht_inter_ref.py` and bit-equal decodes on its cases at three quantisers, with and without the grid
index; input handling, refusals, the unchanged intra path, the anchor codec and its closed-loop sequence, and damaged streams."""
import functools

import numpy as np
import pytest
import torch

from tests import raht_inter_ref as X
from tests import raht_ref as R
from tests.util import dev, t, n

pytestmark = pytest.mark.gpu
NAMES = tuple(X.cases())
QPS = X.QPS


def _encode(name, qp, mode, **kw):
    from unified_point_cloud_compression_amd.attributes import encode_attributes
    c = X.cases()[name]
    return encode_attributes(t(c["cur"][0]), qp, colour=c["colour"], attrs=t(c["cur"][1]), segment_symbols=c["segment_symbols"],
                             reference=t(c["ref"][0]), reference_attrs=t(c["ref"][1]), mode=mode, **kw)


@functools.lru_cache(maxsize=None)
def _gpu(name, qp, mode="inter"):
    return _encode(name, qp, mode)


def _decode(data, name, **kw):
    from unified_point_cloud_compression_amd.attributes import decode_attributes
    c = X.cases()[name]
    ref = {"reference": t(c["ref"][0]), "reference_attrs": t(c["ref"][1])}
    ref.update(kw)
    got = decode_attributes(data, t(c["cur"][0]), **ref)
    assert got.dtype == torch.uint8 and got.is_cuda
    return n(got)


@functools.lru_cache(maxsize=None)
def _reference_levels(name, qp, inter):
    """What the reference decoder returns for the reference's stream (computed once, shared by the parametrised cases)."""
    c = X.cases()[name]
    if not inter:
        return R.decode(X.intra_coded(name, qp), c["cur"][0])
    got = X.decode(X.coded(name, qp)[0], c["cur"][0], *c["ref"])
    assert np.array_equal(got, X.coded(name, qp)[1]["recon"])
    return got


@pytest.mark.parametrize("use_grid", (True, False))
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("name", NAMES)
def test_streams_equal_the_reference_and_decode_to_its_levels(name, qp, use_grid):
    """Pins the prediction fill with its block means, the double forward pass, the block sums and the decision, the levels above
    the blocks, the extra group set, the stream, and the decoder's prediction-only pass and inverse."""
    from unified_point_cloud_compression_amd import sparse as S
    old = S.USE_GRID
    try:
        S.USE_GRID = use_grid
        inter, intra = X.coded(name, qp)[0], X.intra_coded(name, qp)
        for mode, want in (("inter", inter), ("auto", inter if len(inter) < len(intra) else intra)):      # intra on a tie
            data = _encode(name, qp, mode)
            assert data == want, f"{name} qp {qp} {mode}: {len(data)} bytes against the reference's {len(want)}"
            assert np.array_equal(_decode(data, name), _reference_levels(name, qp, want is inter))
    finally:
        S.USE_GRID = old


def _as_set(pts):
    from unified_point_cloud_compression_amd import sparse as S
    c4 = torch.cat([torch.zeros((len(pts), 1)), torch.from_numpy(pts[:, :3])], dim=1).to(dev())
    return S.coordset_from_coords(c4, 1)


def test_deterministic_blind_to_row_order_and_a_set_as_reference():
    from unified_point_cloud_compression_amd.attributes import decode_attributes, encode_attributes
    name, qp = "d_thinned", 28
    c = X.cases()[name]
    (pc, lc), (pr, lr) = c["cur"], c["ref"]
    assert _encode(name, qp, "inter") == _gpu(name, qp) == X.coded(name, qp)[0]
    rng = np.random.default_rng(3)
    p, q = rng.permutation(len(pc)), rng.permutation(len(pr))
    assert encode_attributes(t(pc[p]), qp, attrs=t(lc[p]), reference=t(pr[q]), reference_attrs=t(lr[q]), mode="inter") == _gpu(name, qp)
    rs, perm, keep = _as_set(pr)
    assert keep is None
    lr_s = t(lr) if perm is None else t(lr)[perm].contiguous()
    assert encode_attributes(t(pc), qp, attrs=t(lc), reference=rs, reference_attrs=lr_s, mode="inter") == _gpu(name, qp)
    got = decode_attributes(_gpu(name, qp), t(pc), reference=rs, reference_attrs=lr_s)
    assert np.array_equal(n(got), X.coded(name, qp)[1]["recon"])
    cloud = np.concatenate([pr, lr.astype(np.float32) / np.float32(255)], axis=1)                     # an [M, 6] reference
    assert np.array_equal(R.levels_of(cloud[:, 3:]), lr)
    assert encode_attributes(t(pc), qp, attrs=t(lc), reference=t(cloud), mode="inter") == _gpu(name, qp)


def test_intra_bytes_are_unchanged():
    """mode="intra" and no reference give the bytes of the intra reference coder, and so does `compress_anchor` with its
    default `attributes` whatever the reference."""
    from unified_point_cloud_compression_amd import anchor
    from unified_point_cloud_compression_amd.attributes import encode_attributes
    for name in ("b_shift_100", "i_eight_channels", "f_two_voxels", "j_surface7_segmented"):
        c = X.cases()[name]
        for qp in QPS:
            want = X.intra_coded(name, qp)
            assert _encode(name, qp, "intra") == want
            assert encode_attributes(t(c["cur"][0]), qp, colour=c["colour"], attrs=t(c["cur"][1]), segment_symbols=c["segment_symbols"]) == want
    cur, ref = _frames("b_shift_100")
    _, _, a = anchor.parse_container(anchor.compress_anchor(t(cur), 28, reference=t(ref)))
    assert a == X.intra_coded("b_shift_100", 28)
    assert anchor.compress_anchor(t(cur), 28) == anchor.compress_anchor(t(cur), 28, attributes="intra")


def test_refusals():
    from unified_point_cloud_compression_amd.attributes import decode_attributes, encode_attributes
    from unified_point_cloud_compression_amd.lib import PccError
    c = X.cases()["b_shift_100"]
    (pc, lc), (pr, lr) = c["cur"], c["ref"]
    enc = functools.partial(encode_attributes, t(pc), 28, attrs=t(lc))
    with pytest.raises(PccError, match="repeat a voxel"):
        enc(reference=t(np.concatenate([pr, pr[:5]])), reference_attrs=t(np.concatenate([lr, lr[:5]])))           # duplicated reference voxels
    with pytest.raises(PccError):
        enc(reference=torch.from_numpy(pr), reference_attrs=t(lr))                                              # CPU tensors
    with pytest.raises(PccError, match="channels"):
        enc(reference=t(pr), reference_attrs=t(lr[:, :2].copy()))                                               # a channel mismatch
    with pytest.raises(PccError, match="mode"):
        enc(reference=t(pr), reference_attrs=t(lr), mode="temporal")
    with pytest.raises(PccError):
        enc(reference=t(pr))                                                                                    # coordinates without colours
    deep = np.float32([[0, 0, 0], [20000, 3, 1]])                                                               # depth 15: no inter stream
    l2 = np.uint8([[1, 2, 3], [200, 100, 50]])
    with pytest.raises(PccError, match="depth"):
        encode_attributes(t(deep), 28, attrs=t(l2), reference=t(deep), reference_attrs=t(l2), mode="inter")
    assert encode_attributes(t(deep), 28, attrs=t(l2), reference=t(deep), reference_attrs=t(l2)) == R.encode(deep, l2, 28)
    data = _gpu("b_shift_100", 28)
    with pytest.raises(PccError, match="reference"):
        decode_attributes(data, t(pc))                                                                          # no reference
    with pytest.raises(PccError):
        decode_attributes(data, t(pc), reference=t(pr))                                                         # no reference colours
    with pytest.raises(PccError):
        decode_attributes(data, t(pc[:-1]), reference=t(pr), reference_attrs=t(lr))                             # another n
    bad = bytearray(data)
    bad[12:16] = (12).to_bytes(4, "little")                                                                     # another block count
    with pytest.raises(PccError, match="blocks"):
        decode_attributes(bytes(bad), t(pc), reference=t(pr), reference_attrs=t(lr))


def _frames(name):
    """(current, reference) of a case as [N, 6] float32 clouds whose colours round to the case's levels."""
    c = X.cases()[name]
    out = []
    for pts, lv in (c["cur"], c["ref"]):
        cloud = np.concatenate([pts, lv.astype(np.float32) / np.float32(255)], axis=1).astype(np.float32)
        assert np.array_equal(R.levels_of(cloud[:, 3:]), lv)
        out.append(cloud)
    return out


def test_anchor_with_inter_colour_round_trips():
    from unified_point_cloud_compression_amd import anchor
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    from unified_point_cloud_compression_amd.lib import PccError
    name, qp = "b_shift_100", 28
    cur, ref = _frames(name)
    plain = anchor.compress_anchor(t(cur), qp, reference=t(ref))
    data = anchor.compress_anchor(t(cur), qp, reference=t(ref), attributes="auto")
    assert len(data) < len(plain)
    scale, g, a = anchor.parse_container(data)
    want = X.coded(name, qp)[0]
    assert scale == 1.0 and g == encode_geometry(t(cur), reference=t(ref)) and a == want and a[0] == X.MAGIC
    rec = n(anchor.decompress_anchor(data, dev(), reference=t(ref)))
    cells, _ = R.canonical(*X.cases()[name]["cur"])
    assert rec.shape == (len(cells), 6) and np.array_equal(rec[:, :3], cells)
    assert np.array_equal(R.levels_of(rec[:, 3:]), X.coded(name, qp)[1]["recon"])
    with pytest.raises(PccError):
        anchor.decompress_anchor(data, dev(), reference=t(ref[:, :3].copy()))        # a reference without colours
    with pytest.raises(PccError):
        anchor.compress_anchor(t(cur), qp, reference=t(ref[:, :3].copy()), attributes="auto")
    with pytest.raises(PccError):
        anchor.compress_anchor(t(cur), qp, attributes="inter")


def test_sequence_is_a_closed_loop():
    """Four frames of a surface moving by one voxel: frame 0 intra, every later frame coded against the previous frame AS
    DECODED -- its attribute part equals the numpy reference's stream against the reference decoder's previous output -- and
    shorter than its intra coding; the decoder returns what the encoder's loop held."""
    from unified_point_cloud_compression_amd import anchor
    qp = 28
    ref = _frames("b_shift_100")[1]
    frames = []
    for i in range(4):
        f = ref.copy()
        f[:, 0] += i
        frames.append(f)
    streams = anchor.compress_anchor_sequence([t(f) for f in frames], qp)
    back = anchor.decompress_anchor_sequence(streams, dev())
    prev = None
    for i, (f, s, rec) in enumerate(zip(frames, streams, back)):
        pts, lv = f[:, :3], R.levels_of(f[:, 3:])
        a = anchor.parse_container(s)[2]
        if i == 0:
            assert a == R.encode(pts, lv, qp)
        else:
            assert a[0] == X.MAGIC and a == X.encode(pts, lv, qp, *prev, mode="auto")
            assert len(s) < len(anchor.compress_anchor(t(f), qp))
        dec = X.decode(a, pts, *prev) if i else R.decode(a, pts)
        cells = R.canonical(pts, lv)[0]
        rec = n(rec)
        assert np.array_equal(rec[:, :3], cells) and np.array_equal(R.levels_of(rec[:, 3:]), dec)
        assert np.array_equal(rec, n(anchor.decompress_anchor(s, dev(), reference=None if prev is None else t(
            np.concatenate([prev[0], prev[1].astype(np.float32) / np.float32(255)], axis=1)))))
        prev = (cells.astype(np.float32), dec)


def test_damaged_stream_is_rejected_or_bounded():
    """Asserts rejection or bounded output only.  Safe to run because nothing is sized by the payload: every buffer and launch
    of the decoder is sized by the geometry set and the reference set it was handed, the block count of the header is compared
    with the geometry's before any launch, rows are addressed through the geometry's own scan, a mode outside {0, 1}, a block row
    and a match outside their range count as 0 / unmatched, q * step, Hp + q * step and every butterfly output are clamped to
    +-2^30, and what the payload decoded to (rANS status, flag word) is read once at the end.  Four fixed corruptions, not a
    search: a mode byte, a side byte, a payload word, the block count."""
    from unified_point_cloud_compression_amd.attributes import parse_header
    from unified_point_cloud_compression_amd.lib import PccError
    name, qp = "c_mixed", 40
    good = _gpu(name, qp)
    hdr = parse_header(good)
    shape = (hdr["n"], 3)

    def bounded(data):
        try:
            out = _decode(data, name)
        except PccError:
            return
        assert out.dtype == np.uint8 and out.shape == shape

    flipped = bytearray(good)
    flipped[hdr["modes"][0]] ^= 0x05
    parse_header(bytes(flipped))                                           # the header walk cannot see it
    bounded(bytes(flipped))
    flipped = bytearray(good)
    flipped[hdr["modes"][0] - 1] ^= 0x3F
    parse_header(bytes(flipped))
    bounded(bytes(flipped))
    b0, b1 = hdr["payload"]
    flipped = bytearray(good)
    at = (b0 + 4 * (1 + hdr["streams"]) + b1) // 2 & ~3
    flipped[at:at + 4] = bytes(x ^ 0xA5 for x in flipped[at:at + 4])
    bounded(bytes(flipped))
    flipped = bytearray(good)
    flipped[12:16] = (hdr["blocks"] - 1).to_bytes(4, "little")
    with pytest.raises(PccError):
        _decode(bytes(flipped), name)
