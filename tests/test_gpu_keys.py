"""a1 / a2-i / a3-i / a11: coordinate keys on the GPU against the oracle -- bit exact."""
import numpy as np
import pytest
import torch

from oracle import coords as co
from tests.util import dev, t, n, cloud_keys

pytestmark = pytest.mark.gpu


def _S():
    from unified_point_cloud_compression_amd import sparse as S, lib as L
    return S, L


def test_pack_unpack_roundtrip_and_negatives():
    S, L = _S()
    rng = np.random.default_rng(0)
    C = rng.integers(-300, 2048, size=(5000, 4)).astype(np.int32)
    C[:, 0] = rng.integers(0, 3, size=5000)
    keys = S.pack_keys(t(C))
    assert np.array_equal(n(keys)[:5000], co.pack_keys(C))
    Cf = C.astype(np.float32) + rng.random((5000, 4)).astype(np.float32) * 0.99
    Cf[:, 0] = C[:, 0]
    assert np.array_equal(n(S.pack_keys(t(Cf)))[:5000], co.pack_keys(C))      # floor, also for negatives
    out = torch.empty((5000, 4), dtype=torch.int32, device=dev())
    L.call("pcc_keys_unpack", L.ptr(keys), 5000, L.ptr(out), L.stream())
    assert np.array_equal(n(out), C)


@pytest.mark.parametrize("nkeys", [1, 63, 2048, 2049, 100_000, 1_000_003])
def test_sort_matches_numpy_stable(nkeys):
    S, L = _S()
    rng = np.random.default_rng(nkeys)
    C = np.concatenate([rng.integers(0, 2, (nkeys, 1)), rng.integers(-5, 700, (nkeys, 3))], axis=1)
    keys = co.pack_keys(C)
    b = S.Bounds(1, (-5, -5, -5), (699, 699, 699))
    k_in = t(keys)
    k_out = torch.empty_like(k_in)
    perm = torch.empty(nkeys, dtype=torch.int32, device=dev())
    ws = L.workspace(L.load().pcc_sort_ws_bytes(nkeys), dev())
    L.call("pcc_sort_keys", L.ptr(k_in), nkeys, b.bit_mask(), L.ptr(k_out), L.ptr(perm), L.ptr(ws), ws.numel(), L.stream())
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(n(k_out), keys[order])
    assert np.array_equal(n(perm), order.astype(np.int32))


@pytest.mark.parametrize("by_grid", [True, False], ids=["bitmap", "sort"])
def test_sparse_tensor_dedup_first_wins_and_user_order(by_grid, monkeypatch):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    S, _ = _S()
    monkeypatch.setattr(S, "CANON_BY_GRID", by_grid)
    C = np.array([[0, 5, 5, 5], [0, 1, 2, 3], [0, 5, 5, 5], [0, -1, 0, 7], [0, 1, 2, 3]], dtype=np.int32)
    F = np.arange(5, dtype=np.float32)[:, None]
    x = ME.SparseTensor(coordinates=t(C), features=t(F))
    assert n(x.C).tolist() == [[0, 5, 5, 5], [0, 1, 2, 3], [0, -1, 0, 7]]       # original order, first kept (A.1)
    assert n(x.F)[:, 0].tolist() == [0.0, 1.0, 3.0]
    keys = n(x._cset.keys)[:x._cset.n]
    assert np.array_equal(keys, np.unique(co.pack_keys(C)))
    assert n(x._canonical_features())[:, 0].tolist() == [3.0, 1.0, 0.0]           # canonical = (b,x,y,z) ascending
    cq, fq = ME.utils.sparse_quantize(coordinates=t(C), features=t(F), quantization_size=1.0)
    oc, of = co.sparse_quantize(C, F)
    assert np.array_equal(n(cq), oc) and np.array_equal(n(fq), of)
    # O(1) re-wrap of an existing coordinate tensor keeps the coordinate set
    y = ME.SparseTensor(coordinates=x.C, features=x.F * 2, tensor_stride=x.tensor_stride, device=x.device)
    assert y._cset is x._cset
    # a large shuffled cloud with duplicates, two batches, stride-4 lattice with negative coordinates
    rng = np.random.default_rng(3)
    Cb = rng.integers(-20, 90, size=(20000, 4)).astype(np.int32) * 4
    Cb[:, 0] = rng.integers(0, 2, size=20000)
    Fb = rng.standard_normal((20000, 3)).astype(np.float32)
    xb = ME.SparseTensor(coordinates=t(Cb), features=t(Fb), tensor_stride=4)
    oc, of = co.sparse_quantize(Cb, Fb)
    assert np.array_equal(n(xb.C), oc) and np.array_equal(n(xb.F), of)            # user order, first duplicate kept
    kb = np.unique(co.pack_keys(Cb))
    assert np.array_equal(n(xb._cset.keys)[:xb._cset.n], kb)
    order = np.argsort(co.pack_keys(oc), kind="stable")
    assert np.array_equal(n(xb._canonical_features()), of[order])
    if by_grid:
        bits, rank, h = xb._cset.grid()
        fresh = S.CoordSet(xb._cset.keys[:xb._cset.n].clone(), xb._cset.n, 4, xb._cset.bounds).grid()
        assert torch.equal(bits, fresh[0]) and torch.equal(rank, fresh[1])
    # coordinates that are not multiples of the tensor stride: the bitmap path must step aside, not alias cells
    Co = Cb.copy()
    Co[7, 1] += 1
    xo = ME.SparseTensor(coordinates=t(Co), features=t(Fb), tensor_stride=4)
    assert np.array_equal(n(xo._cset.keys)[:xo._cset.n], np.unique(co.pack_keys(Co)))


def test_empty_inputs():
    S, L = _S()
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    x = ME.SparseTensor(coordinates=torch.zeros((0, 4), dtype=torch.int32, device=dev()),
                        features=torch.zeros((0, 4), device=dev()))
    assert x._cset.n == 0 and x.C.shape == (0, 4)
    assert x._cset.stride(2).n == 0
    assert x._cset.expand(2, 1).n == 0


@pytest.mark.parametrize("by_grid", [True, False], ids=["bitmap", "sort"])
@pytest.mark.parametrize("seed,size,p,ts", [(0, 40, 0.1, 1), (1, 24, 0.3, 2), (2, 64, 0.02, 4)])
def test_stride_matches_oracle(seed, size, p, ts, by_grid, monkeypatch):
    S, L = _S()
    monkeypatch.setattr(S, "STRIDE_BY_GRID", by_grid)
    keys = cloud_keys(seed, size, p, ts, batch=2)
    C = co.unpack_keys(keys)
    C[:, 1:] -= 3 * ts                                 # some negative coordinates
    keys = np.unique(co.pack_keys(C))
    C = co.unpack_keys(keys)
    cs = S.CoordSet(t(keys), len(keys), ts, S.Bounds(1, C[:, 1:].min(0), C[:, 1:].max(0)))
    for m in (2 * ts, 4 * ts):
        got = cs.stride(m)
        want = co.stride_keys(keys, m)
        assert got.n == len(want)
        assert np.array_equal(n(got.keys)[:got.n], want)
        cs2 = got.stride(2 * m)                         # chained (down_conv twice, model/model.py:228-229)
        assert np.array_equal(n(cs2.keys)[:cs2.n], co.stride_keys(want, 2 * m))
        if by_grid:                                     # the grid index that came with the set == one built from its keys
            bits, rank, h = got.grid()
            fresh = S.CoordSet(got.keys[:got.n].clone(), got.n, m, got.bounds).grid()
            assert torch.equal(bits, fresh[0]) and torch.equal(rank, fresh[1]) and list(h) == list(fresh[2])


@pytest.mark.parametrize("mode", ["bitmap", "sort32", "sort64"])
@pytest.mark.parametrize("ks,ts_in", [(5, 2), (2, 2), (2, 32), (5, 8), (3, 2)])
def test_expand_matches_oracle(ks, ts_in, mode, monkeypatch):
    """The three expansion paths (bitmap marking + grid probing / 32-bit cell sort with pair ids / 64-bit key sort)."""
    S, L = _S()
    use_csr = mode != "sort64"
    monkeypatch.setattr(S, "USE_CSR", use_csr)
    monkeypatch.setattr(S, "EXPAND_BY_GRID", mode == "bitmap")
    keys = cloud_keys(7, 20, 0.08, ts_in, batch=2)       # includes coordinates at 0 -> negative outputs for k5
    C = co.unpack_keys(keys)
    cs = S.CoordSet(t(keys), len(keys), ts_in, S.Bounds(1, C[:, 1:].min(0), C[:, 1:].max(0)))
    got = cs.expand(ks, ts_in // 2)
    want = co.expand_keys(keys, ks, ts_in // 2)
    assert got.n == len(want)
    assert np.array_equal(n(got.keys)[:got.n], want)
    assert got.ts == ts_in // 2
    csr = cs.csr_map(ks, ts_in // 2)
    assert (csr is not None) == use_csr
    if csr is not None:      # CSR lists == the oracle's transposed map: pair id = in_row * K + k, ascending per output
        first, pair_ids = n(csr[0]), n(csr[1])
        nbr = co.kernel_map(keys, want, ks, ts_in // 2, transposed=True)          # [K, n_out]
        K = ks ** 3
        assert first[0] == 0 and first[-1] == len(keys) * K and len(first) == len(want) + 1
        for o in list(range(0, len(want), max(len(want) // 200, 1))) + [len(want) - 1]:
            lst = pair_ids[first[o]:first[o + 1]]
            ks_valid = np.nonzero(nbr[:, o] >= 0)[0]
            want_ids = np.sort(nbr[ks_valid, o].astype(np.int64) * K + ks_valid)
            assert np.array_equal(lst, want_ids), o
    if mode == "bitmap":     # the grid index that came with the output set == one built from its keys
        bits, rank, h = got.grid()
        fresh = S.CoordSet(got.keys[:got.n].clone(), got.n, got.ts, got.bounds).grid()
        assert torch.equal(bits, fresh[0]) and torch.equal(rank, fresh[1]) and list(h) == list(fresh[2])


@pytest.mark.parametrize("rows,canonical", [(2, True), (777, False), (100_003, False), (100_003, True)])
def test_frame_intake_matches_the_torch_chain(rows, canonical):
    """`pcc_frame_intake` (keys, [1, r, g, b] features, bounds, order flag of a frame in one kernel) against the element-wise
    chain it replaces (`model/model.py:141-161`): floor of negative / fractional coordinates, rows in and out of canonical
    order, duplicates."""
    S, L = _S()
    rng = np.random.default_rng(rows)
    xyz = rng.integers(-40, 900, size=(rows, 3)).astype(np.float32) + rng.random((rows, 3)).astype(np.float32) * 0.9
    pc = np.concatenate([xyz, rng.random((rows, 3)).astype(np.float32) * 255], axis=1).astype(np.float32)
    if canonical:
        C = np.concatenate([np.zeros((rows, 1)), np.floor(xyz)], axis=1).astype(np.int64)
        order = np.argsort(co.pack_keys(C), kind="stable")
        pc = pc[order]
        keep = np.concatenate([[True], np.diff(co.pack_keys(C)[order]) > 0])
        pc = pc[keep]
    keys, feats, b, flag = S.frame_intake(t(pc))
    C = np.concatenate([np.zeros((len(pc), 1)), np.floor(pc[:, :3])], axis=1).astype(np.int64)
    want = co.pack_keys(C)
    assert np.array_equal(n(keys), want)
    assert np.array_equal(n(feats), np.concatenate([np.ones((len(pc), 1), np.float32), pc[:, 3:6]], axis=1))
    assert b.lo == tuple(C[:, 1:].min(0)) and b.hi == tuple(C[:, 1:].max(0)) and b.bmax == 0
    assert flag == bool(np.all(np.diff(want) > 0)) == canonical


def test_decode_finish_matches_the_torch_chain():
    """`pcc_decode_finish` against `cat([C[:, 1:4].float(), clamp(round(255 F), 0, 255) / 255])` (`model/model.py:240-250`),
    bit for bit: halves (round half to even), values outside [0, 1], NaN."""
    S, L = _S()
    keys = cloud_keys(3, 24, 0.3, 1)
    m = len(keys)
    rng = np.random.default_rng(5)
    f = (rng.random((m, 3)).astype(np.float32) * 1.4 - 0.2).astype(np.float32)
    f[:64] = (np.arange(64 * 3, dtype=np.float32).reshape(64, 3) + 0.5) / 255      # exact halves after the multiplication
    f[64] = [np.nan, -3.0, 7.0]
    out = torch.empty((m, 6), dtype=torch.float32, device=dev())
    kt, ft = t(keys), t(f)                                      # (held: a temporary's memory is recycled by the next allocation)
    L.call("pcc_decode_finish", L.ptr(kt), L.ptr(ft), m, L.ptr(out), L.stream())
    C = t(co.unpack_keys(keys).astype(np.int32))
    want = torch.cat([C[:, 1:4].to(torch.float32), torch.clamp(torch.round(ft * 255), 0.0, 255.0) / 255], dim=1)
    assert np.array_equal(n(out), n(want), equal_nan=True)


@pytest.mark.parametrize("batch", [3, 8])
def test_batch_ranges_from_the_bounds_kernel_equal_searchsorted(batch):
    """`pcc_batch_bounds` (per-batch row ranges read together with a set's size; top-k runs per batch, reference
    `model/transforms.py:228-254`): for a set whose size the host knows and for a generative expansion whose size is still on
    the device, against torch.searchsorted over the keys.  A batch of 8 is the reference's training batch size."""
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.model.transforms import batch_segments_begin
    keys = cloud_keys(batch, 10, 0.25, 2, batch=batch)
    x = ME.SparseTensor(coordinates=t(co.unpack_keys(keys)), features=t(np.ones((len(keys), 1), np.float32)), tensor_stride=2)
    cs = x._cset

    def ref(c):
        q = torch.arange(0, c.bounds.bmax + 2, device=c.device, dtype=torch.int64) << 48
        return torch.searchsorted(c.keys[:c.n], q).tolist()
    S.resolve(batch_segments_begin(cs))
    assert cs._derived["segments"] == ref(cs)
    ex = cs.expand(5, 1)                                   # size read together with its ranges
    assert ex._derived.get("segments") == ref(ex)
    assert ex._derived["segments"][-1] == ex.n


def test_stride_chain_equals_stride_link_by_link():
    """`stride_chain_begin` (every link queued before the one read, row counts kept on the device between the links) from the
    set's own keys and from a shuffled copy of the rows with duplicates: every link's keys, row count and grid index equal
    what `stride()` gives link by link on a fresh set, and the links sit in the `_derived` caches the modules look them up in."""
    S, L = _S()
    strides = (2, 4, 8, 32)
    C = co.unpack_keys(cloud_keys(11, 40, 0.03, 1, batch=2))
    C[:, 1:] -= 13                                      # some negative coordinates
    keys = np.unique(co.pack_keys(C))
    assert 2000 < len(keys) < 10000
    b = S.Bounds(1, C[:, 1:].min(0), C[:, 1:].max(0))
    want, cur = [], S.CoordSet(t(keys), len(keys), 1, b)
    for m in strides:
        cur = cur.stride(m)
        want.append(cur)
    assert [w.n for w in want] == [len(np.unique(co.stride_keys(keys, m))) for m in strides]
    rng = np.random.default_rng(5)
    rows = rng.permutation(np.concatenate([keys, keys[rng.integers(0, len(keys), 700)]]))
    own = S.CoordSet(t(keys), len(keys), 1, b)
    user = S.CoordSet(t(keys), len(keys), 1, b)
    rows_t = t(rows)
    last_own, last_user = S.resolve(own.stride_chain_begin(strides),
                                    user.stride_chain_begin(strides, keys=rows_t, n_keys=len(rows)))
    for root, last in ((own, last_own), (user, last_user)):
        cur = root
        for m, w in zip(strides, want):
            assert ("stride", m) in cur._derived
            cur = cur._derived[("stride", m)]
            assert cur.ts == m and cur.n == w.n and cur._on_lattice
            assert torch.equal(cur.keys[:cur.n], w.keys[:w.n])
            assert (cur.bounds.bmax, cur.bounds.lo, cur.bounds.hi) == (w.bounds.bmax, w.bounds.lo, w.bounds.hi)
            bits, rank, h = cur.grid()
            fresh = w.grid()
            assert torch.equal(bits, fresh[0]) and torch.equal(rank, fresh[1]) and list(h) == list(fresh[2])
        assert cur is last
        assert root.stride(2) is root._derived[("stride", 2)]          # stride() finds the chain's sets: nothing is rebuilt


# ---- the kernels that take a PccLattice by value, at the smallest lattice where a swapped field shows ------------------------
def _np_keys(C):
    """b << 48 | (x + 2^15) << 32 | (y + 2^15) << 16 | (z + 2^15), from the definition"""
    C = np.asarray(C, dtype=np.int64)
    return (C[:, 0] << 48) | ((C[:, 1] + 32768) << 32) | ((C[:, 2] + 32768) << 16) | (C[:, 3] + 32768)


def _np_grid(C, lo, dims, pitch, batches):
    """bits (uint64, an even number of words) and rank (exclusive prefix popcount per word) of the coordinates C in the lattice"""
    cell = ((C[:, 0] * dims[0] + (C[:, 1] - lo[0]) // pitch) * dims[1] + (C[:, 2] - lo[1]) // pitch) * dims[2] + (C[:, 3] - lo[2]) // pitch
    words = ((batches * dims[0] * dims[1] * dims[2] + 63) // 64 + 1) // 2 * 2
    occ = np.zeros(words * 64, dtype=np.uint64)
    occ[cell] = 1
    per_word = occ.reshape(words, 64)
    bits = (per_word << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    count = per_word.sum(axis=1).astype(np.int64)
    return bits, (np.cumsum(count) - count).astype(np.int32)


def _np_expand(C, ks, ts_out):
    """sorted unique output coordinates of the generative expansion and, per output, its ascending pair ids i * K + k
    (i: canonical input row, k = ix + ks * iy + ks^2 * iz, offsets centred for odd ks and 0 .. ks - 1 for even ks)"""
    o0 = -(ks - 1) // 2 if ks % 2 else 0
    lists = {}
    for i, (b, x, y, z) in enumerate(C.tolist()):
        for k in range(ks ** 3):
            off = (k % ks + o0, k // ks % ks + o0, k // (ks * ks) + o0)
            lists.setdefault((b, x + off[0] * ts_out, y + off[1] * ts_out, z + off[2] * ts_out), []).append(i * ks ** 3 + k)
    out = sorted(lists)
    return np.array(out, dtype=np.int64), [sorted(lists[c]) for c in out]


def test_small_lattice_with_distinct_dims_through_every_lattice_kernel(monkeypatch):
    """lo = (-8, -16, 8), dims (3, 5, 7), pitch 4, two batches: 105 cells per batch, so bitmap word 1 straddles the batch
    boundary and the read-out carries z into y, x and the batch.  About 60 occupied cells as shuffled user rows with duplicates
    go through canonicalisation on the bitmap (keys, first-wins perm and keep), the grid index, stride(8), and expand(3, 4) /
    expand(2, 2) on the bitmap and the 32-bit sort, CSR lists included.  Everything is compared exactly with numpy computed
    here from the definitions; pairwise distinct dims make any mix-up of the lattice fields change a result."""
    S, L = _S()
    monkeypatch.setattr(S, "USE_GRID", True)
    monkeypatch.setattr(S, "CANON_BY_GRID", True)
    monkeypatch.setattr(S, "STRIDE_BY_GRID", True)
    monkeypatch.setattr(S, "USE_CSR", True)
    lo, dims, pitch, batches = np.array([-8, -16, 8]), (3, 5, 7), 4, 2
    rng = np.random.default_rng(17)
    pinned = np.array([0, 63, 64, 100, 104, 105, 106, 127, 128, 209])       # both corners of both batches, around word ends
    cells = np.unique(np.concatenate([pinned, rng.choice(210, 52, replace=False)]))
    assert 55 <= len(cells) <= 62
    cz, cy, cx, cb = cells % 7, cells // 7 % 5, cells // 35 % 3, cells // 105
    Cu = np.stack([cb, lo[0] + pitch * cx, lo[1] + pitch * cy, lo[2] + pitch * cz], axis=1).astype(np.int64)    # canonical order
    rows = rng.permutation(np.concatenate([np.arange(len(Cu)), rng.integers(0, len(Cu), 25)]))
    user = Cu[rows]
    assert np.array_equal(np.sort(_np_keys(Cu)), _np_keys(Cu))                  # ascending cell == ascending key
    # canonicalisation through the bitmap
    cs, perm, keep = S.coordset_from_coords(t(user.astype(np.int32)), pitch)
    assert cs._on_lattice and cs.n == len(Cu)
    assert np.array_equal(n(cs.keys)[:cs.n], _np_keys(Cu))
    first_user = np.array([np.nonzero(rows == c)[0].min() for c in range(len(Cu))])
    want_keep = np.sort(first_user)
    assert np.array_equal(n(keep), want_keep) and np.array_equal(n(perm), np.searchsorted(want_keep, first_user))
    # the grid index that came with it, and one built from the canonical keys (pcc_grid_build)
    want_bits, want_rank = _np_grid(Cu, lo, dims, pitch, batches)
    assert len(want_bits) == 4
    for g in (cs.grid(), S.CoordSet(cs.keys[:cs.n].clone(), cs.n, pitch, cs.bounds).grid()):
        assert list(g.h) == [-8, -16, 8, 3, 5, 7, 4, 2]
        assert np.array_equal(n(g.bits).view(np.uint64), want_bits) and np.array_equal(n(g.rank), want_rank)
    # stride(8): floor to multiples of 8 -> lo (-8, -16, 8), dims (2, 3, 4)
    C8 = Cu.copy()
    C8[:, 1:] = C8[:, 1:] // 8 * 8
    C8 = np.unique(C8, axis=0)
    s8 = cs.stride(8)
    assert s8.n == len(C8) and np.array_equal(n(s8.keys)[:s8.n], _np_keys(C8))
    g8 = s8.grid()
    b8, r8 = _np_grid(C8, lo, (2, 3, 4), 8, batches)
    assert list(g8.h) == [-8, -16, 8, 2, 3, 4, 8, 2]
    assert np.array_equal(n(g8.bits).view(np.uint64), b8) and np.array_equal(n(g8.rank), r8)
    # generative expansions, bitmap marking + grid probing and the 32-bit cell sort
    for ks, ts_out, want_h in ((3, 4, [-12, -20, 4, 5, 7, 9, 4, 2]), (2, 2, [-8, -16, 8, 6, 10, 14, 2, 2])):
        Co, lists = _np_expand(Cu, ks, ts_out)
        for mode in ("bitmap", "sort32"):
            monkeypatch.setattr(S, "EXPAND_BY_GRID", mode == "bitmap")
            src = S.CoordSet(cs.keys[:cs.n].clone(), cs.n, pitch, cs.bounds)
            got = src.expand(ks, ts_out)
            assert got.n == len(Co) and np.array_equal(n(got.keys)[:got.n], _np_keys(Co)), (ks, mode)
            first, pair_ids = (n(x) for x in src.csr_map(ks, ts_out))
            assert len(first) == len(Co) + 1 and first[0] == 0 and first[-1] == len(Cu) * ks ** 3, (ks, mode)
            assert np.array_equal(first, np.cumsum([0] + [len(v) for v in lists])), (ks, mode)
            assert np.array_equal(pair_ids[:first[-1]], np.concatenate(lists)), (ks, mode)
            go = got.grid()
            bo, ro = _np_grid(Co, want_h[0:3], want_h[3:6], ts_out, batches)
            assert list(go.h) == want_h, (ks, mode)
            assert np.array_equal(n(go.bits).view(np.uint64), bo) and np.array_equal(n(go.rank), ro), (ks, mode)
