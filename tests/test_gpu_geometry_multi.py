"""GPU suite of the geometry stream with several references, format 0xAB (DESIGN.md section 7e "Several references"): the device
streams against the numpy reference coder of tests/geom_multi_ref.py byte for byte on both lookup paths, round trips, the
kernel `pcc_geom_multi_block_bits` against numpy in both of its forms, the `reference=` list of every caller, the defaults
against the reference coders of the existing formats, and damaged streams."""
import functools

import numpy as np
import pytest
import torch

from tests import geom_inter_ref as I
from tests import geom_multi_ref as MU
from tests import geom_ref as R
from tests import motion_ref as MR
from tests.util import dev, t, n

pytestmark = pytest.mark.gpu

NAMES = ("a_uncovered7", "b_uncovered8", "c_turn8", "d_unrelated_second", "e_one_point", "e_depth3", "e_full_cube8", "e_four_slots",
         "e_faces", "f_wide7")


@pytest.fixture(params=[True, False], ids=["grid", "bsearch"])
def lookup_mode(request):
    """Both lookups of the reference slots (grid index / binary search over the keys)."""
    from unified_point_cloud_compression_amd import sparse as S
    old = S.USE_GRID
    S.USE_GRID = request.param
    yield request.param
    S.USE_GRID = old


def _transform(T):
    from unified_point_cloud_compression_amd.motion import RigidTransform
    return RigidTransform(T[:9], T[9:])


def _device_slots(slots):
    """The `reference=` list of numpy slots: one tensor per distinct cloud (entries that share a cloud share the tensor)."""
    seen, out = {}, []
    for cloud, T in slots:
        if id(cloud) not in seen:
            seen[id(cloud)] = t(cloud) if len(cloud) else torch.zeros((0, 3), device=dev())
        out.append(seen[id(cloud)] if T is None else (seen[id(cloud)], _transform(T)))
    return out


@functools.lru_cache(maxsize=None)
def _ref_stream(name, segment_nodes=MU.SEGMENT_NODES):
    cur, slots, search = MU.cases()[name]
    rep = {}
    return MU.encode_multi(cur, slots, search, segment_nodes, report=rep), rep


def _gpu_stream(name, segment_nodes=MU.SEGMENT_NODES, mode="inter"):
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    cur, slots, search = MU.cases()[name]
    return encode_geometry(t(cur), segment_nodes=segment_nodes, reference=_device_slots(slots), mode=mode, search=search)


# ---- streams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_streams_equal_the_reference_byte_for_byte_and_round_trip(name, lookup_mode):
    """Fails without the feature: `encode_geometry` refuses a list of references and 0xAB does not parse."""
    from unified_point_cloud_compression_amd.geometry import decode_geometry
    cur, slots, _ = MU.cases()[name]
    got = _gpu_stream(name)
    assert got == _ref_stream(name)[0]
    out = decode_geometry(got, dev(), reference=_device_slots(slots))
    assert np.array_equal(n(out), R.unique_cells(cur))


def test_the_selector_container_spans_three_streams(lookup_mode):
    from unified_point_cloud_compression_amd.geometry import decode_geometry, parse_header
    cur, slots, _ = MU.cases()["b_uncovered8"]
    got = _gpu_stream("b_uncovered8", MU.SEGMENTED_NODES)
    assert got == _ref_stream("b_uncovered8", MU.SEGMENTED_NODES)[0]
    hdr = parse_header(got, clouds=2)
    assert hdr["selectors"]["streams"] == 3 and hdr["vectors"]["streams"] == 3
    assert np.array_equal(n(decode_geometry(got, dev(), reference=_device_slots(slots))), R.unique_cells(cur))


# ---- the kernel against numpy -------------------------------------------------------------------------------------------------
def _kernel(name):
    """Both forms of `pcc_geom_multi_block_bits` on a case: (sel, displacements [blocks, 3], counts, encoder pyramids, decoder
    pyramids given that sel and those vectors, the decoder's flag)."""
    from unified_point_cloud_compression_amd import geometry as G
    cur, slots, search = MU.cases()[name]
    cs = G.canonical_rows(t(cur))[0]
    sets = G._slot_sets(G.reference_slots(_device_slots(slots), "test"), "test")[0]
    origin = tuple(cs.bounds.lo)
    depth = max(1, max(cs.bounds.hi[i] - origin[i] for i in range(3)).bit_length())
    blocks, bl, sel, disp, pred, cnt = G.multi_prediction(cs, sets, origin, depth, search=search, counts=True)
    again = torch.full_like(pred, -1)
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    G.multi_block_bits(blocks.keys, blocks.n, bl, sets, origin, disp, search, None, sel, None, again, None, bad.data_ptr())
    d = n(disp).astype(np.int64)
    return n(sel), np.stack([(d & 15) - 8, ((d >> 4) & 15) - 8, ((d >> 8) & 15) - 8], axis=1), n(cnt), n(pred), n(again), int(bad.item())


@pytest.mark.parametrize("name", ["a_uncovered7", "e_one_point", "e_depth3", "e_full_cube8", "e_four_slots", "e_faces"])
def test_selectors_displacements_and_counts_equal_numpy(name, lookup_mode):
    rep = _ref_stream(name)[1]
    sel, disp, cnt, pred, again, bad = _kernel(name)
    assert np.array_equal(cnt, rep["counts"])
    assert np.array_equal(sel, rep["selectors"])
    assert np.array_equal(disp, rep["displacements"])
    assert np.array_equal(again, pred) and bad == 0                 # the decoder form, given that choice, writes the same pyramids


def test_the_decoder_form_flags_a_selector_or_a_vector_out_of_range():
    """A selector K counts as slot 0, a displacement outside the range as zero, and either sets the flag."""
    from unified_point_cloud_compression_amd import geometry as G
    cur, slots, search = MU.cases()["a_uncovered7"]
    cs = G.canonical_rows(t(cur))[0]
    sets = G._slot_sets(G.reference_slots(_device_slots(slots), "test"), "test")[0]
    origin = tuple(cs.bounds.lo)
    depth = max(1, max(cs.bounds.hi[i] - origin[i] for i in range(3)).bit_length())
    blocks, bl, sel, disp, _, _ = G.multi_prediction(cs, sets, origin, depth, search=search)
    zero = torch.full_like(disp, 8 | (8 << 4) | (8 << 8))

    def run(s, v):
        out = torch.full((blocks.n * 75,), -1, dtype=torch.int64, device=dev())
        bad = torch.zeros(1, dtype=torch.int32, device=dev())
        G.multi_block_bits(blocks.keys, blocks.n, bl, sets, origin, v, search, None, s, None, out, None, bad.data_ptr())
        return n(out).reshape(blocks.n, 75), int(bad.item())

    want, flag = run(torch.zeros_like(sel), zero)
    assert flag == 0
    for wrong in (2, 4, -1, 1 << 20):
        s = torch.zeros_like(sel)
        s[3] = wrong
        got, flag = run(s, zero)
        assert flag == 1 and np.array_equal(got, want)
    for wrong in (8 | (8 << 4) | (11 << 8), 1 << 12, -1):           # dz = 3 at search 2; a bit above the 12; all bits
        v = zero.clone()
        v[5] = wrong
        got, flag = run(torch.zeros_like(sel), v)
        assert flag == 1 and np.array_equal(got, want)


# ---- the callers --------------------------------------------------------------------------------------------------------------
def test_list_forms_of_the_reference_argument():
    from unified_point_cloud_compression_amd.geometry import decode_geometry, encode_geometry, stream_search, stream_slots, stream_transform
    from unified_point_cloud_compression_amd.lib import PccError
    cur, slots, _ = MU.cases()["c_turn8"]
    x, (a, (_, T)) = t(cur), _device_slots(slots)
    plain = encode_geometry(x, reference=a)
    wrapped = encode_geometry(x, reference=a, global_motion=T)
    assert encode_geometry(x, reference=[a]) == plain and encode_geometry(x, reference=(a,)) == plain       # a one-entry list is that entry
    assert encode_geometry(x, reference=(a, T)) == wrapped and encode_geometry(x, reference=[(a, T)]) == wrapped
    assert wrapped[0] == 0xA9 and wrapped == MR.encode(cur, slots[0][0], slots[1][1])
    multi = encode_geometry(x, reference=[a, (a, T)])
    assert multi == _ref_stream("c_turn8")[0] and multi == encode_geometry(x, reference=[a, (a, T)], mode="inter")
    assert stream_search(multi) == 2 and stream_transform(multi) is None and stream_transform(wrapped) == T
    assert stream_slots(multi) == [(0, None), (0, T)] and stream_slots(wrapped) is None
    want = R.unique_cells(cur)
    for held in (a, [a], [a, (a, T)], [a, a]):                       # both slots name cloud 0: the cloud alone decodes the stream
        assert np.array_equal(n(decode_geometry(multi, dev(), reference=held)), want)
    assert encode_geometry(x, reference=[a, (a, T)], mode="intra") == R.encode(cur)
    for bad in ([], [a] * 5, [a, None], [a, [a]]):
        with pytest.raises(PccError, match="references"):
            encode_geometry(x, reference=bad)
    for gm in ("auto", "both", T):
        with pytest.raises(PccError, match="global_motion must be None"):
            encode_geometry(x, reference=[a, a], global_motion=gm)
    with pytest.raises(PccError, match="none was given"):
        decode_geometry(multi, dev())


def test_auto_never_costs_bytes_against_the_first_reference_alone():
    """(d): no block takes the unrelated second slot, so "auto" returns the single-reference stream byte for byte; "inter" forces 0xAB."""
    from unified_point_cloud_compression_amd.geometry import decode_geometry, encode_geometry
    cur, slots, _ = MU.cases()["d_unrelated_second"]
    refs = _device_slots(slots)
    single = encode_geometry(t(cur), reference=refs[0])
    assert _gpu_stream("d_unrelated_second", mode="auto") == single == I.encode(cur, slots[0][0], "auto")
    forced = _gpu_stream("d_unrelated_second", mode="inter")
    assert forced[0] == 0xAB and len(forced) > len(single)
    assert np.array_equal(n(decode_geometry(single, dev(), reference=refs)), R.unique_cells(cur))     # a list decodes it too


def test_defaults_keep_every_byte():
    """`encode_geometry(x, reference=r)` and `encode_sequence(frames)` against the reference coders of the existing formats."""
    from unified_point_cloud_compression_amd.geometry import encode_geometry, encode_sequence
    cur, slots, _ = MU.cases()["d_unrelated_second"]
    a, other = slots[0][0], slots[1][0]
    assert encode_geometry(t(cur), reference=t(a)) == I.encode(cur, a, "auto")
    assert encode_geometry(t(cur), reference=t(a), mode="inter") == I.encode(cur, a, "inter")
    assert encode_geometry(t(cur)) == R.encode(cur)
    frames = [a, cur, other]
    want = [R.encode(a), I.encode(cur, a, "auto"), I.encode(other, cur, "auto")]
    assert encode_sequence([t(f) for f in frames]) == want
    assert encode_sequence([t(f) for f in frames], references=1) == want


def test_search_auto_and_the_both_shorthand():
    from unified_point_cloud_compression_amd.geometry import decode_geometry, encode_geometry, stream_search, stream_slots
    cur, slots, _ = MU.cases()["f_wide7"]
    refs = _device_slots(slots)
    got = encode_geometry(t(cur), reference=refs, mode="inter", search="auto")
    assert got == _ref_stream("f_wide7")[0] and stream_search(got) == 7                 # the halves moved by more than 2: the wide stream is shorter
    cur, slots, _ = MU.cases()["c_turn8"]
    a = t(slots[0][0])
    both = encode_geometry(t(cur), reference=a, global_motion="both", mode="inter")
    table = stream_slots(both)
    assert both[0] == 0xAB and [s for s, _ in table] == [0, 0] and table[0][1] is None and table[1][1] is not None
    assert np.array_equal(n(decode_geometry(both, dev(), reference=a)), R.unique_cells(cur))
    assert encode_geometry(t(cur), reference=a, global_motion="both") == both           # far shorter than the plain stream: "auto" keeps it
    assert len(both) < len(encode_geometry(t(cur), reference=a))


def test_a_sequence_with_two_references_recovers_what_only_frame_zero_shows():
    """Frame 1 hides the half x >= 64, frame 2 uncovers it: with references=2 frame 2 is predicted from frames 1 and 0."""
    from unified_point_cloud_compression_amd.geometry import decode_sequence, encode_sequence, stream_slots
    a = MU.surface(0, 7)
    f0, f1 = a, a[a[:, 0] < 64] + np.float32([0, 1, 0])
    f2, f3 = a + np.float32([0, 1, 1]), a + np.float32([1, 1, 1])
    frames = [t(f) for f in (f0, f1, f2, f3)]
    two, one = encode_sequence(frames, references=2), encode_sequence(frames)
    assert two[:2] == one[:2] and two[2][0] == 0xAB and [s for s, _ in stream_slots(two[2])] == [0, 1]
    assert len(two[2]) < 0.75 * len(one[2]) and len(two[3]) <= len(one[3])
    assert two[2] == MU.encode(f2, [(f1, None), (f0, None)], "auto")
    for got, want in zip(decode_sequence(two, dev()), (f0, f1, f2, f3)):
        assert np.array_equal(n(got), R.unique_cells(want))
    for got, want in zip(decode_sequence(one, dev()), (f0, f1, f2, f3)):
        assert np.array_equal(n(got), R.unique_cells(want))


def test_the_lossless_codec_forwards_the_list():
    from unified_point_cloud_compression_amd import anchor as A
    cur, slots, _ = MU.cases()["a_uncovered7"]
    rng = np.random.default_rng(3)

    def coloured(p):
        p = R.unique_cells(p).astype(np.float32)
        return t(np.concatenate([p, rng.integers(0, 256, (len(p), 3)).astype(np.float32) / np.float32(255)], axis=1))

    x, r0, r1 = coloured(cur), coloured(slots[0][0]), coloured(slots[1][0])
    data = A.compress_lossless(x, reference=[r0, r1], attributes="auto")
    geometry = A.parse_lossless_container(data)[0]
    assert geometry == _ref_stream("a_uncovered7")[0]
    assert len(data) < len(A.compress_lossless(x, reference=r0, attributes="auto"))
    assert torch.equal(A.decompress_lossless(data, dev(), reference=[r0, r1]), A.decompress_lossless(A.compress_lossless(x), dev()))
    seq = [r0, x, coloured(cur + np.float32([0, 0, 1]))]
    streams = A.compress_lossless_sequence(seq, references=2)
    assert A.parse_lossless_container(streams[2])[0][0] in (0xA8, 0xAB)
    for got, frame in zip(A.decompress_lossless_sequence(streams, dev()), seq):
        assert torch.equal(got, A.decompress_lossless(A.compress_lossless(frame), dev()))


# ---- damage -------------------------------------------------------------------------------------------------------------------
def test_damaged_streams_are_rejected_or_decode_to_another_cloud():
    """Rejection or a cloud of exactly n rows that differs, never a fault: every buffer and launch is sized by the header walk, a
    selector outside the slots counts as slot 0, and what was decoded is compared with the header in the decode's one read."""
    from unified_point_cloud_compression_amd.geometry import decode_geometry, parse_header
    from unified_point_cloud_compression_amd.lib import PccError

    def differs(data, reference, want):
        try:
            out = decode_geometry(data, dev(), reference=reference)
        except PccError:
            return
        assert tuple(out.shape) == want.shape and not np.array_equal(n(out), want)

    for name in ("a_uncovered7", "b_uncovered8"):
        cur, slots, _ = MU.cases()[name]
        refs, want = _device_slots(slots), R.unique_cells(cur)
        good, rep = _ref_stream(name)
        hdr = parse_header(good, clouds=2)
        at, (b0, b1) = hdr["inner"], hdr["selectors"]["payload"]
        differs(good, refs[::-1], want)                                                # the slots' clouds swapped
        b = bytearray(good)
        if hdr["selectors"]["raw"]:
            b[at + b0 + 7] = 2                                                         # a selector byte set to K: refused on the host
            with pytest.raises(PccError, match="selector outside"):
                decode_geometry(bytes(b), dev(), reference=refs)
            b[at + b0 + 7] = 1 - good[at + b0 + 7]                                     # ... to the other slot
        else:
            b[at + b0 + 4 * (1 + hdr["selectors"]["streams"]) + 5] ^= 0x10             # a selector payload word flipped
        differs(bytes(b), refs, want)
        with pytest.raises(PccError, match="names reference cloud"):                   # a slot source beyond the list
            decode_geometry(good[:4] + bytes([2]) + good[5:], dev(), reference=refs)
        with pytest.raises(PccError, match="names reference cloud"):
            decode_geometry(good, dev(), reference=refs[0])
        for cut in (3, 5):                                                             # a truncated slot table
            with pytest.raises(PccError, match="truncated"):
                decode_geometry(good[:cut], dev(), reference=refs)
        with pytest.raises(PccError):
            decode_geometry(good[:-5], dev(), reference=refs)


def test_a_coded_selector_outside_the_slots_raises_through_the_device_flag():
    """The list of 220 blocks coded with one selector 2 = K (the escape slot of its table row, which the histogram does not
    announce): the host parser cannot see it, `pcc_geom_multi_block_bits` flags it."""
    from unified_point_cloud_compression_amd.geometry import decode_geometry, parse_header
    from unified_point_cloud_compression_amd.lib import PccError
    cur, slots, _ = MU.cases()["b_uncovered8"]
    good, rep = _ref_stream("b_uncovered8")
    hdr = parse_header(good, clouds=2)
    sel = rep["selectors"].copy()
    hist = np.bincount(sel, minlength=2)
    sel[100] = 2
    begin = hdr["inner"] + hdr["levels"][hdr["first"] - 1]["payload"][1]
    bad = good[:begin] + MU.encode_selectors(sel, 2, hist=hist) + good[hdr["inner"] + hdr["selectors"]["payload"][1]:]
    assert parse_header(bad, clouds=2)["selectors"]["hist"] == hist.tolist()
    with pytest.raises(PccError, match="selector list"):
        decode_geometry(bad, dev(), reference=_device_slots(slots))
