"""CPU suite of the geometry stream with several references, format 0xAB (DESIGN.md section 7e "Several references"): the numpy
reference coder of tests/geom_multi_ref.py against itself, the host walk `geometry.parse_header` on its streams and on damaged
ones, and the rate inequalities the format was built for.  No GPU."""
import functools
import struct

import numpy as np
import pytest

from tests import geom_multi_ref as MU
from tests import geom_ref as G
from tests import geom_wide_ref as GW
from tests import motion_ref as MR

SMALL = ("a_uncovered7", "d_unrelated_second", "e_one_point", "e_depth3", "e_full_cube8", "e_four_slots", "e_faces")


@functools.lru_cache(maxsize=None)
def _stream(name, segment_nodes=MU.SEGMENT_NODES):
    cur, slots, search = MU.cases()[name]
    rep = {}
    return MU.encode_multi(cur, slots, search, segment_nodes, report=rep), rep


def _clouds(name):
    return [c for c, _ in MU.cases()[name][1]]


def _parse(data, clouds=2, have_reference=True):
    from unified_point_cloud_compression_amd.geometry import parse_header
    return parse_header(data, have_reference=have_reference, clouds=clouds)


def _refused(data, match, clouds=2, have_reference=True):
    from unified_point_cloud_compression_amd.lib import PccError
    with pytest.raises(PccError, match=match):
        _parse(bytes(data), clouds, have_reference)


# ---- the reference coder against itself --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + ("b_uncovered8", "c_turn8", "f_wide7"))
def test_the_reference_decodes_its_own_streams(name):
    cur = MU.cases()[name][0]
    data, rep = _stream(name)
    assert data[0] == MU.MAGIC_MULTI and data[1] == len(MU.cases()[name][1])
    assert np.array_equal(MU.decode(data, _clouds(name)), G.unique_cells(cur))
    assert rep["selectors"].max() < data[1]


def test_the_segmented_selector_container_decodes():
    cur = MU.cases()["b_uncovered8"][0]
    data, rep = _stream("b_uncovered8", MU.SEGMENTED_NODES)
    assert rep["blocks"] == 220 and -(-rep["blocks"] // MU.SEGMENTED_NODES) == 3
    assert np.array_equal(MU.decode(data, _clouds("b_uncovered8")), G.unique_cells(cur))


def test_blocks_and_list_forms_of_the_cases():
    """(a) has raw lists, (b) coded ones, (f) an 0xAA inner stream; both slots are used where the halves are uncovered."""
    for name, blocks, inner in (("a_uncovered7", 51, 0xA8), ("b_uncovered8", 220, 0xA8), ("f_wide7", None, 0xAA)):
        data, rep = _stream(name)
        if blocks is not None:
            assert rep["blocks"] == blocks
        assert data[MU.parse_slots(data)[1]] == inner
        assert (rep["blocks"] >= MU.RAW_NODES) == (name == "b_uncovered8")
        assert min(np.bincount(rep["selectors"], minlength=2)) > 0


def test_ties_go_to_the_lower_slot_and_to_slot_zero_without_a_match():
    _, rep = _stream("e_four_slots")
    sel, cnt = rep["selectors"], rep["counts"]
    assert np.array_equal(cnt[:, 2], cnt[:, 3]) and not np.any(sel == 3)              # two identical slots: the lower one
    assert not np.any(cnt[:, :2]) and np.all(sel[cnt.max(axis=1) == 0] == 0)          # nothing matches: slot 0 ...
    assert np.all(rep["displacements"][cnt.max(axis=1) == 0] == 0)                    # ... with the zero vector
    assert np.all(sel[cnt.max(axis=1) > 0] == 2)


@pytest.mark.parametrize("name", ["a_uncovered7", "c_turn8"])
def test_a_one_entry_list_is_the_single_reference_stream(name):
    cur, slots, search = MU.cases()[name]
    for slot in slots:
        cloud, T = slot
        want = GW.encode(cur, cloud, "auto", search) if T is None else MR.encode(cur, cloud, T, "auto")
        assert MU.encode(cur, [slot], "auto", search) == want


# ---- the rates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_uncovered7", "b_uncovered8", "c_turn8"])
def test_two_slots_halve_the_best_single_slot(name):
    """The gate of the format: where each reference shows one part of the frame, the stream with both is at most 0.5 x the
    shortest stream any one of them gives."""
    cur, slots, search = MU.cases()[name]
    multi = len(_stream(name)[0])
    singles = [len(MU.encode_single(cur, s, "inter", search)) for s in slots]
    print(name, "multi", multi, "singles", singles, "ratio", multi / min(singles))
    assert multi <= 0.5 * min(singles)
    assert MU.encode(cur, slots, "auto", search) == _stream(name)[0]


def test_auto_returns_the_single_reference_stream_when_the_second_slot_is_useless():
    cur, slots, search = MU.cases()["d_unrelated_second"]
    multi, rep = _stream("d_unrelated_second")
    single = MU.encode_single(cur, slots[0], "auto", search)
    assert not np.any(rep["selectors"]) and len(single) < len(multi)
    assert MU.encode(cur, slots, "auto", search) == single == GW.encode(cur, slots[0][0], "auto", search)


# ---- the host walk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + ("b_uncovered8", "c_turn8", "f_wide7"))
def test_parse_header_walks_the_reference_streams(name):
    data, rep = _stream(name)
    hdr = _parse(data, clouds=len(_clouds(name)))
    table, begin = MU.parse_slots(data)
    assert hdr["inner"] == begin and hdr["n"] == rep["n"] and hdr["inter"]
    assert [(s, None if T is None else tuple(T.ints())) for s, T in hdr["slots"]] == [(s, None if T is None else tuple(T)) for s, T in table]
    assert hdr["selectors"]["raw"] == (rep["blocks"] < MU.RAW_NODES)
    if not hdr["selectors"]["raw"]:
        assert hdr["selectors"]["hist"] == np.bincount(rep["selectors"], minlength=len(table)).tolist()


def _selector_histogram(data):
    """(offset of the histogram's count byte, entries) of a stream whose selector list is coded."""
    hdr = _parse(data)
    m = sum(1 for v in hdr["selectors"]["hist"] if v)
    return hdr["inner"] + hdr["selectors"]["payload"][0] - 4 - 5 * m - 1, m


def test_refusals_of_the_slot_table():
    data, _ = _stream("a_uncovered7")
    for k in (0, 1, 5, 255):
        _refused(data[:1] + bytes([k]) + data[2:], "reference slots")
    _refused(data, "names reference cloud 1", clouds=1)                                # a source outside the list
    _refused(data[:4] + bytes([7]) + data[5:], "names reference cloud 7", clouds=4)
    _refused(data[:3] + bytes([2]) + data[4:], "warped byte 2")
    _refused(data, "none was given", clouds=0, have_reference=False)                   # an 0xAB stream without references
    _refused(data[:6] + bytes([0xA7]) + data[7:], "magic byte 0xa7")                   # inner magic: intra
    _refused(data[:6] + bytes([0xA9]) + data[7:], "magic byte 0xa9")                   # ... a global-motion wrapper
    _refused(data[:6] + bytes([0xAB]) + data[7:], "magic byte 0xab")                   # ... another slot table
    for cut in (1, 2, 3, 5, 6):
        _refused(data[:cut], "truncated")
    _refused(data[:-1], "truncated|gives|expands")
    _refused(data + b"\x00", "trailing bytes")


def test_refusals_of_a_slot_transform():
    data, _ = _stream("c_turn8")
    table, begin = MU.parse_slots(data)
    assert table[1][1] is not None and begin == 2 + 2 + 2 + 48
    bad_m = data[:6] + struct.pack("<i", (1 << 25) + 1) + data[10:]
    _refused(bad_m, "matrix entry")                                                    # what 0xA9 refuses
    bad_t = data[:6 + 36] + struct.pack("<i", 1 << 24) + data[6 + 40:]
    _refused(bad_t, "translation entry")
    _refused(data[:6 + 20], "truncated inside the transform")
    assert _parse(data, clouds=1)["slots"][1][1].ints() == list(table[1][1])


def test_refusals_of_the_selector_histogram():
    data, rep = _stream("b_uncovered8")
    at, m = _selector_histogram(data)
    assert m == 2 and data[at] == 2 and data[at + 1] == 0 and data[at + 6] == 1
    c0, c1 = struct.unpack_from("<I", data, at + 2)[0], struct.unpack_from("<I", data, at + 7)[0]
    assert c0 + c1 == rep["blocks"]

    def with_entries(e0, e1):
        return data[:at + 1] + struct.pack("<BI", *e0) + struct.pack("<BI", *e1) + data[at + 11:]

    _refused(with_entries((1, c1), (0, c0)), "ascending")                              # not ascending
    _refused(with_entries((0, c0), (0, c1)), "ascending")
    _refused(with_entries((0, c0), (2, c1)), "ascending")                              # a slot >= K
    _refused(with_entries((0, c0), (1, c1 + 1)), "counts 221 of 220")                  # does not sum to the block count
    _refused(with_entries((0, c0), (1, 0)), "ascending order, each with a count")
    _refused(data[:at + 3], "truncated")


def test_a_raw_selector_outside_the_slots_is_refused():
    data, rep = _stream("a_uncovered7")
    hdr = _parse(data)
    at = hdr["inner"] + hdr["selectors"]["payload"][0]
    assert hdr["selectors"]["raw"] and data[at:at + rep["blocks"]] == bytes(rep["selectors"].tolist())
    _refused(data[:at] + bytes([2]) + data[at + 1:], "selector outside the 2 reference slots")


def test_single_reference_streams_parse_as_before():
    """The walk of 0xA7 / 0xA8 / 0xA9 / 0xAA streams is untouched by the new arguments."""
    cur, slots, _ = MU.cases()["a_uncovered7"]
    for data in (G.encode(cur), GW.encode(cur, slots[0][0], "inter", 2), GW.encode(cur, slots[0][0], "inter", 7)):
        hdr = _parse(data, clouds=None)
        assert "slots" not in hdr and "selectors" not in hdr and hdr["n"] == len(G.unique_cells(cur))
