"""GPU suite of the lossless geometry coder and the lossless-geometry mode of the model."""
import functools
import struct

import numpy as np
import pytest
import torch

from oracle import codec
from tests import geom_ref as R
from tests.util import dev, t, n, load_params

pytestmark = pytest.mark.gpu

NAMES = ("one_point", "corners_depth10", "full_cube8", "random_block", "surface7", "surface8", "shifted_block",
         "shuffled_duplicated_block", "threshold")


@functools.lru_cache(maxsize=None)
def _clouds():
    return R.clouds()


@functools.lru_cache(maxsize=None)
def _ref_stream(name, segment_nodes=R.SEGMENT_NODES):
    return R.encode(_clouds()[name], segment_nodes=segment_nodes)


@functools.lru_cache(maxsize=None)
def _gpu_stream(name, segment_nodes=R.SEGMENT_NODES):
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    return encode_geometry(t(_clouds()[name]), segment_nodes=segment_nodes)


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_as_tensor_and_as_set(name):
    from unified_point_cloud_compression_amd.geometry import decode_geometry
    want = R.unique_cells(_clouds()[name])
    data = _gpu_stream(name)
    got = decode_geometry(data, dev())
    assert got.dtype == torch.int32 and np.array_equal(n(got), want)
    cs = decode_geometry(data, dev(), as_set=True)
    assert cs.ts == 1 and cs.n == len(want) and np.array_equal(n(cs.coords())[:, 1:], want)
    assert cs.bounds.lo == tuple(want.min(axis=0)) and cs.bounds.hi == tuple(want.max(axis=0))
    k = n(cs.keys)[:cs.n]
    assert np.all(k[1:] > k[:-1])                                # canonical: no caller re-sorts


@pytest.mark.parametrize("name", NAMES[:6])
def test_stream_equals_the_reference_byte_for_byte(name):
    """Pins the node order, the bit order of the bytes, the contexts and the integer table rule."""
    assert _gpu_stream(name) == _ref_stream(name)


def test_stream_equality_across_three_segments_at_bits7():
    from unified_point_cloud_compression_amd.geometry import decode_geometry, parse_header
    data = _gpu_stream("surface7", 1024)
    assert parse_header(data)["levels"][-1]["streams"] >= 3
    assert data == _ref_stream("surface7", 1024)
    assert np.array_equal(n(decode_geometry(data, dev())), R.unique_cells(_clouds()["surface7"]))


def test_device_tables_equal_the_host_rule():
    """The decoder derives its tables on the device (`pcc_geom_tables`): same CDF rows as `derive_tables` / the reference,
    and the decoder table blob `pcc_rans_build_dec_table` builds from them, also past the 2^20 rescale of the counts."""
    import ctypes as C
    from unified_point_cloud_compression_amd import geometry as G, lib as L
    lib = L.load()
    rng = np.random.default_rng(0)
    cases = [(np.zeros((64, 256), np.int64), [0, 0, 0, 128, 0, 0, 0, 0]),
             (rng.integers(0, 5000, (64, 256)), [5, 0, 100, 2000, 300, 0, 1, 0]),
             (rng.integers(0, 3, (64, 256)) * (rng.random((64, 256)) < 0.02), [1, 1, 1, 1, 1, 1, 1, 1]),
             (rng.integers(0, 1 << 26, (64, 256)), [(1 << 30) - 5, 3, 0, 0, 0, 0, 0, 1]),
             (rng.integers(0, 40, (64, 256)), [1, 0, 0, 0, 0, 0, 0, (1 << 31) - 2])]
    for counts, pop in cases:
        counts = np.asarray(counts, dtype=np.int64)
        counts[:, 0] = 0
        want = G.derive_tables(counts, pop)
        assert np.array_equal(want, R.tables(counts, pop))
        blob = np.zeros(lib.pcc_rans_dec_table_bytes(64, G.TABLE_SIZES.ctypes.data_as(C.c_void_p)), dtype=np.uint8)
        assert lib.pcc_rans_build_dec_table(want.ctypes.data_as(C.c_void_p), 64, 257, G.TABLE_SIZES.ctypes.data_as(C.c_void_p),
                                            blob.ctypes.data_as(C.c_void_p)) == 0
        assert len(blob) == lib.pcc_geom_dec_table_bytes()
        d_cdf = torch.empty((64, 257), dtype=torch.int32, device=dev())
        d_tab = torch.zeros(len(blob), dtype=torch.uint8, device=dev())
        L.call("pcc_geom_tables", L.ptr(t(counts.reshape(-1))), (C.c_uint32 * 8)(*pop), L.ptr(d_cdf), L.ptr(d_tab), L.stream())
        assert np.array_equal(n(d_cdf), want)
        assert np.array_equal(n(d_tab), blob)


def test_set_input_leaves_the_callers_set_alone():
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    pc = _clouds()["random_block"]
    c4 = torch.cat([torch.zeros((len(pc), 1)), torch.from_numpy(pc[:, :3])], dim=1).to(dev())
    cs = S.coordset_from_coords(c4, 1)[0]
    cs._on_lattice = False
    assert encode_geometry(cs) == _gpu_stream("random_block") and cs._on_lattice is False


def test_set_input_and_search_fallback_give_the_same_stream():
    """A pitch-1 CoordSet is accepted as it is, and the sorted-search fallback of the symbol kernel (sets without a grid
    index) produces the bytes of the bitmap path."""
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.geometry import encode_geometry, decode_geometry
    pc = _clouds()["shifted_block"]
    c4 = torch.cat([torch.zeros((len(pc), 1)), torch.from_numpy(pc[:, :3])], dim=1).to(dev())
    cs = S.coordset_from_coords(c4, 1)[0]
    assert encode_geometry(cs) == _gpu_stream("shifted_block")
    old = S.USE_GRID
    try:
        S.USE_GRID = False
        data = encode_geometry(t(pc))
        back = n(decode_geometry(data, dev()))
    finally:
        S.USE_GRID = old
    assert data == _gpu_stream("shifted_block") and np.array_equal(back, R.unique_cells(pc))


def test_deterministic_and_blind_to_order_and_duplicates():
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    for name in ("random_block", "surface7"):
        assert encode_geometry(t(_clouds()[name])) == _gpu_stream(name)
    assert _gpu_stream("shuffled_duplicated_block") == _gpu_stream("random_block")


def test_batched_and_cpu_input_is_refused():
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.geometry import encode_geometry
    from unified_point_cloud_compression_amd.lib import PccError
    c4 = torch.tensor([[0, 1, 2, 3], [1, 1, 2, 3], [1, 4, 4, 4]], dtype=torch.int32, device=dev())
    with pytest.raises(PccError):
        encode_geometry(S.coordset_from_coords(c4, 1)[0])
    with pytest.raises(PccError):
        encode_geometry(torch.zeros((4, 3)))
    with pytest.raises(PccError):
        encode_geometry(S.coordset_from_coords(c4[:1] * 2, 2)[0])


def test_malformed_streams_are_rejected_or_bounded():
    """Asserts rejection or bounded output only.  Safe to run because nothing is sized by the payload: every buffer and
    launch of the decoder is sized by the child counts the header walk derived on the host (<= n), the expansion drops writes
    past its capacity, keys stay inside the level's cube by construction, and what the payload decoded to is compared with
    the header in the decode's one read at the end."""
    from unified_point_cloud_compression_amd.geometry import decode_geometry, parse_header
    from unified_point_cloud_compression_amd.lib import PccError
    good = _gpu_stream("surface7")
    hdr = parse_header(good)
    for bad in (good[:-5], good[:len(good) // 2]):
        with pytest.raises(PccError):
            parse_header(bad)                                   # refused on the host
        with pytest.raises(PccError):
            decode_geometry(bad, dev())
    for delta in (-1, 1):
        b = bytearray(good)
        struct.pack_into("<I", b, 1, hdr["n"] + delta)
        with pytest.raises(PccError):
            parse_header(bytes(b))                              # refused on the host
        with pytest.raises(PccError):
            decode_geometry(bytes(b), dev())
    b0, b1 = hdr["levels"][-1]["payload"]
    b = bytearray(good)
    b[(b0 + b1) // 2] ^= 0x10                                    # one flipped byte inside the last level's rANS words
    parse_header(bytes(b))                                       # the header walk cannot see it
    try:
        out = decode_geometry(bytes(b), dev())
    except PccError:
        return
    assert tuple(out.shape) == (hdr["n"], 3)


# ---- the model's lossless-geometry mode ----------------------------------------------------------------------------------
def _model(cfg, P, coder="symbols"):
    import copy
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = copy.deepcopy(cfg)
    cfg["entropy_model"]["entropy_coder"] = coder
    m = load_params(UnifiedModel(cfg), P).to(dev()).eval()
    m.update()
    return m


@pytest.mark.parametrize("which", ["small", "r2"])
def test_model_one_block_matches_the_probe_forced_path(which):
    """`decompress_lossless_geometry` returns exactly the input's voxels, derives y's coordinate set from them, and colours
    them as the existing decoder does when every level's mask is forced to the true geometry (`bench.true_geometry_ms`).
    Bound: the project's cross-path bound of test_fused_up_predict_matches_layerwise (levels differ by at most 1 in fewer
    than 5e-3 of the entries); the kept rows go through the same kernels wherever the probe path fuses a level, so the
    count printed here is expected to be 0 there (DESIGN.md section 7e names the dispatch that differs otherwise)."""
    from unified_point_cloud_compression_amd import lib as L, synth
    from unified_point_cloud_compression_amd.geometry import decode_geometry
    if which == "small":
        cfg, pc, gain = codec.small_config(), synth.random_block(4, 40, 0.08), 4.0
    else:
        cfg, pc, gain = codec.R2_CONFIG, synth.surface_cloud(0, 7), 3.0
    model = _model(cfg, codec.random_params(cfg, 3, gain=gain))
    q = np.array([[0.5, 0.5]], dtype=np.float32)
    cells = R.unique_cells(pc)
    strings, shapes, geometry, qs = model.compress_lossless_geometry(t(pc), t(q), block_size=1024)
    assert len(strings) == len(shapes) == len(geometry) == len(qs) == 1 and isinstance(geometry[0], bytes)
    rec = n(model.decompress_lossless_geometry(strings, shapes, geometry, qs))
    assert rec.shape == (len(cells), 6) and np.array_equal(rec[:, :3], cells)

    streams, shapes2, ks, coords, qs2 = model.compress(t(pc), t(q), block_size=1024)
    s1 = decode_geometry(geometry[0], dev(), as_set=True)
    y = s1.stride(2).stride(4).stride(8)
    assert y.n == coords[0].shape[0] and np.array_equal(n(y.coords()), n(coords[0]))
    gt = [s1.stride(2).stride(4), s1.stride(2), s1]

    def probe(stage, lvl, cset, logit, mask, feats):
        if stage != "select":
            return None
        rows = torch.empty(max(cset.n, 1), dtype=torch.int32, device=dev())
        L.call("pcc_lookup_rows", L.ptr(gt[lvl].keys), gt[lvl].n, L.ptr(cset.keys), cset.n, L.ptr(rows), L.stream())
        return rows[:cset.n] >= 0

    rec_p = n(model.decompress(coordinates=coords, strings=streams, shape=shapes2, k=ks, q_vals=qs2, probe=probe))
    assert rec_p.shape == rec.shape and np.array_equal(rec_p[:, :3], rec[:, :3])
    lv, lv_p = np.rint(rec[:, 3:] * 255).astype(int), np.rint(rec_p[:, 3:] * 255).astype(int)
    print(f"{which}: {int((lv != lv_p).sum())} of {lv.size} colour levels differ from the probe-forced path, max {np.abs(lv - lv_p).max()}")
    assert np.abs(lv - lv_p).max() <= 1 and (lv != lv_p).mean() < 5e-3


def test_model_multi_block():
    from unified_point_cloud_compression_amd import synth
    from unified_point_cloud_compression_amd.geometry import parse_header
    cfg = codec.small_config()
    model = _model(cfg, codec.random_params(cfg, 2, gain=4.0), coder="pcc_streams")
    pc = synth.random_block(3, 48, 0.05)
    q = np.array([[0.5, 0.5]], dtype=np.float32)
    strings, shapes, geometry, qs = model.compress_lossless_geometry(t(pc), t(q), block_size=32)
    assert len(geometry) == len(strings) == 8                    # one geometry stream per block
    assert sum(parse_header(g)["n"] for g in geometry) == len(pc)
    rec = n(model.decompress_lossless_geometry(strings, shapes, geometry, qs))
    assert rec.shape == (len(pc), 6)
    order = np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))
    assert np.array_equal(rec[order, :3], R.unique_cells(pc))
    assert rec[:, 3:].min() >= 0 and rec[:, 3:].max() <= 1
