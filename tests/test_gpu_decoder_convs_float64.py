"""The convolutions of a decoder level (`SparseSynthesisTransform._up_predict_fused`) against float64, stage by stage:

  1. `pcc_convt_fwd_csr_grid` -- the composite 7x7x7 up+head convolution h = relu(c0(genT(x))) on every candidate row: the composite
     kernel `_fused_weights` builds, its z-fastest numbering against `csr_for(zk=True)`, the [27, ch] neighbour-existence
     constants, the subset-sum tables of `k_presence_tables` and the bitmap windows of `k_convt_gather_csr` (lattice faces, the last
     dword of the bitmap, 2 / 4 / 8 / 16 / 32 lanes per row, the VEC = 1 instantiation);
  2. `pcc_conv_thin_grid_fwd` -- the head's second convolution (the logits top-k ranks), in both plane forms;
  3. `pcc_convt_fwd_rows` -- the up-sampled features of the kept rows: the bucketing passes (`k_csr_khist`, `k_csr_kstarts`,
     `k_csr_kscatter`), the pair GEMM over the buckets and `k_csr_reduce`;
and one run of `_up_predict_fused` itself, whose logits and kept features must be the bits of the stage-by-stage calls.

Every kernel sees identical fp32 inputs on both sides: stage 2 reads the GPU's own output of stage 1.  The regime a product took is
READ from the library (`pcc_prof_sequence`, `pcc_prof_sequence_tiles`); the last test checks that every regime of EXPECT was reached.

Metric (that of test_gpu_conv_forward_regimes.py): |got - ref| / S2 per output entry, S2 = the root of the sum of squares of the
terms the kernel actually adds (bias, presence constants, x[p][ci] * W[...][ci][co]); max and rms over all entries (`util.ratios`:
an entry with S2 = 0 must be exactly 0, a non-finite output counts as infinite).

Reference, independent of the library's maps and of `_fused_weights`: float64 through torch over the ORACLE's pairs, LAYER-WISE --
u = gen.bias + sum_k index_add(x[i_k] @ W5[k]) on all candidates, h = relu(c0.bias + sum_j index_add(u[i_j] @ V3[j])).  S2 of the
composite needs the composite's own terms: M[d] = sum over (k, j) with off5[k] - off3[j] = d of W5[k] @ V3[j], built here in a
dictionary keyed by the displacement, and cb[j] = gen.bias @ V3[j] once per existing neighbour j; one test without a GPU checks
that the composite evaluated this way equals the layer-wise evaluation to 1e-12 S2.

Coordinate sets: two batch entries, negative coordinates (`util.two_batch_keys`, seed 9, shift -3) at input pitch 2 and 4, plus one
parent at the minimum corner of the bounds in batch 0 and one at the maximum corner in the last batch: the candidate set has a row
in the first and in the last cell of its bitmap.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import codec, coords as co
from tests.util import dev, t, n, bits, conv_sums64, coord_set, ratios, shape_rows, two_batch_keys

gpu = pytest.mark.gpu

FORM_GEMM_H2, FORM_GEMM_BF2, FORM_PAIR_H2, FORM_PAIR_BF, FORM_CONV_BF, FORM_CONV_F32 = 1, 2, 3, 4, 5, 6    # include/pcc_hip.h PCC_FORM_*
FORM_GATHER_CSR = 8
DISTS = ("relu", "spread")
TAGS = ("h3", "bf6", "f32")

# One absolute bound on |got - ref| / S2 for the three kernels of this file: 3x the worst measured on MI355X over every case,
# distribution and form (profiles/decoder_convs_float64.txt) -- max 3.539e-6 (kept rows 128 -> 64, every fifth row, spread rows,
# the fp32-input kernel), rms 2.521e-7 (kept rows 128 -> 128, the one-row set, spread rows, the fp32-input kernel); composite
# level alone: max 2.727e-6, rms 1.496e-7 (128 -> 64 at 925 parents); logits: max 7.5e-7, rms 1.44e-7.  Both lie below the bounds
# of test_gpu_conv_forward_regimes.py (5e-5 / 2.5e-6: same metric, reductions no deeper here -- at most 37 parents x 128 channels
# against 27 x 256 there), which is their ceiling.
MAX_RATIO = 1.06e-5
RMS_RATIO = 7.6e-7


# ---------------------------------------------------------------------------------------------------------------------------------
# coordinate sets (canonical keys, numpy) and the oracle's pairs
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (per-batch (size, p), input pitch, parent cells by which the maximum corner lies beyond the clouds' own bounds in z).
# 416a / 416b differ by one cell of extent: the window of the candidate set's last row lies inside (a), respectively beyond (b), the
# last full dword pair of its bitmap (`last_dw` of k_convt_gather_csr) -- asserted in test_lattice_variants_...
SETS = {
    "416a": (((10, 0.3), (8, 0.25)), 2, 4),
    "416b": (((10, 0.3), (8, 0.25)), 2, 5),
    "925": (((14, 0.25), (11, 0.2)), 4, 0),
    "3719": (((21, 0.3), (17, 0.2)), 2, 0),
}


class _Geom:
    """Parents, candidates and the oracle's pairs of one set (numpy; nothing of the library)."""

    def __init__(self, name):
        sizes, ts, extra = SETS[name]
        C = co.unpack_keys(two_batch_keys(9, ts, -3, sizes)).astype(np.int64)
        lo, hi = C[:, 1:].min(0), C[:, 1:].max(0)
        hi[2] += extra * ts
        corners = np.array([[0, *lo], [C[:, 0].max(), *hi]], np.int64)
        self.keys = np.unique(co.pack_keys(np.concatenate([C, corners])))
        self.ts_in, self.ts_out = ts, ts // 2
        self.out_keys = co.expand_keys(self.keys, 5, self.ts_out)
        self.n_in, self.n_out = len(self.keys), len(self.out_keys)
        self.pairs5 = codec.kernel_map_pairs(self.keys, self.out_keys, 5, self.ts_out, transposed=True)
        self.pairs3 = codec.kernel_map_pairs(self.out_keys, self.out_keys, 3, self.ts_out)

    @functools.cached_property
    def pairs7(self):
        """parent p -> candidate p + off7[d] * ts_out for the 343 displacements of the composite (x fastest, the oracle's order)"""
        return codec.kernel_map_pairs(self.keys, self.out_keys, 7, self.ts_out, transposed=True)

    @functools.cached_property
    def parents_per_row(self):
        return np.bincount(np.concatenate([o for _, o in self.pairs5]), minlength=self.n_out)


@functools.lru_cache(maxsize=None)
def _geom(name):
    return _Geom(name)


@functools.lru_cache(maxsize=None)
def _cset(name):
    """The library's CoordSet of the parents (its grid index, candidate set and pair lists are cached on it)."""
    g = _geom(name)
    return coord_set(g.keys, g.ts_in)


def _candidates(name):
    """The library's candidate set of `name`, checked row for row against the oracle's: the reference's rows are the kernel's rows."""
    g, cs = _geom(name), _cset(name)
    out_set = cs.expand(5, g.ts_out, want_csr=False)
    assert out_set.n == g.n_out and np.array_equal(n(out_set.keys[:out_set.n]), g.out_keys)
    assert out_set.grid() is not None
    return out_set


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference (torch, on the device of its inputs: the GPU in the tests, the CPU in the test of the reference itself)
# ---------------------------------------------------------------------------------------------------------------------------------
def _composite64(W5, V3):
    """M [343, cin, ch] float64, M[d] = sum over (k, j) with off5[k] - off3[j] == off7[d] of W5[k] @ V3[j], collected in a
    dictionary keyed by the displacement vector."""
    off5, off3, off7 = co.kernel_offsets(5), co.kernel_offsets(3), co.kernel_offsets(7)
    M = {}
    for j in range(27):
        P = W5 @ V3[j]                                   # [125, cin, ch]
        for k in range(125):
            d = tuple(int(v) for v in off5[k] - off3[j])
            M[d] = P[k] if d not in M else M[d] + P[k]
    assert len(M) == 343
    return torch.stack([M[tuple(int(v) for v in d)] for d in off7])


def _layerwise64(g, x64, W5, gb, V3, c0b):
    """(u, v) float64: u = gen.bias + genT(x) on all candidates, v = c0.bias + conv3(u) (before the ReLU), over the oracle's pairs."""
    u, _ = conv_sums64(x64, W5, gb, g.pairs5, g.n_out)
    v, _ = conv_sums64(u, V3, c0b, g.pairs3, g.n_out)
    return u, v


def _composite_sums64(g, x64, W5, gb, V3, c0b):
    """(sum, sum of squares) of the composite's own terms per entry: c0.bias, cb[j] = gen.bias @ V3[j] for every existing
    neighbour j, and x[p][ci] * M[d][ci][co] for every parent p at displacement d."""
    s, sq = conv_sums64(x64, _composite64(W5, V3), c0b, g.pairs7, g.n_out)
    cb = torch.einsum("m,jmc->jc", gb, V3)
    for j, (_, o) in enumerate(g.pairs3):
        oo = torch.from_numpy(o.astype(np.int64)).to(x64.device)
        s.index_add_(0, oo, cb[j].expand(len(o), -1))
        sq.index_add_(0, oo, (cb[j] * cb[j]).expand(len(o), -1))
    return s, sq


def _weights(rng, K, cin, cout):
    """(kernel [K, cin, cout], bias [cout]) float32: standard_normal / sqrt(fan_in * 4), a non-zero bias"""
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(cin * 4)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.5).astype(np.float32)
    b[b == 0] = 0.25
    return W, b


def test_composite_reference_equals_the_layerwise_reference():
    """No GPU: on the 416-parent set (8 -> 6 -> 5 channels), the composite's terms summed in float64 -- M from the displacement
    dictionary, the presence constants over the oracle's 3x3x3 pairs -- equal the layer-wise float64 evaluation to 1e-12 S2
    (measured 3e-15): the reference of this file and its S2 describe the same function.  Also the sets themselves: a candidate
    row in the first and in the last cell of the lattice, rows with one parent and with many."""
    g = _geom("416a")
    rng = np.random.default_rng(5)
    x = shape_rows(rng.standard_normal((g.n_in, 8)).astype(np.float32), "spread", rng)
    (W5, gb), (V3, c0b) = _weights(rng, 125, 8, 6), _weights(rng, 27, 6, 5)
    x64, W5, gb, V3, c0b = (torch.from_numpy(a).double() for a in (x, W5, gb, V3, c0b))
    _, v = _layerwise64(g, x64, W5, gb, V3, c0b)
    s, sq = _composite_sums64(g, x64, W5, gb, V3, c0b)
    s2 = sq.sqrt()
    assert bool((s2 > 0).all())
    worst = float(((s - v).abs() / s2).max())
    print(f"composite vs layer-wise float64: max |diff| / S2 = {worst:.2e}")
    assert worst <= 1e-12
    C = co.unpack_keys(g.out_keys)
    assert tuple(C[0]) == (0, *C[:, 1:].min(0)) and tuple(C[-1]) == (C[:, 0].max(), *C[:, 1:].max(0))
    assert sum(len(i) for i, _ in g.pairs7) > sum(len(i) for i, _ in g.pairs5) == 125 * g.n_in
    assert g.parents_per_row.min() == 1 and g.parents_per_row.max() >= 8


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU side: what _up_predict_fused calls
# ---------------------------------------------------------------------------------------------------------------------------------
def _recorded(call):
    """call() with the per-launch record on: (its result, [(form, BM, BN, ksplit)] in launch order)."""
    from unified_point_cloud_compression_amd import lib as L
    lib = L.load()
    L.call("pcc_prof_enable", 1)
    try:
        out = call()
        forms = (ctypes.c_int32 * 16)()
        tiles = (ctypes.c_int32 * 48)()
        cnt = int(lib.pcc_prof_sequence(forms, 16))
        assert int(lib.pcc_prof_sequence_tiles(tiles, 16)) == cnt <= 16
        rec = [(forms[j], tiles[3 * j], tiles[3 * j + 1], tiles[3 * j + 2]) for j in range(cnt)]
    finally:
        L.call("pcc_prof_enable", 0)
    return out, rec


def _forms():
    from unified_point_cloud_compression_amd import lib as L
    return dict(zip(TAGS, (L.ARITH_H3, L.ARITH_BF6, L.ARITH_F32)))


def _clear_guard():
    """Rows spread over e^+-6 may trip the range guard of the three-term form (a flag for the codec to repeat the call in the
    six-term form; the call itself is not changed by it): left clean for the tests that follow."""
    from unified_point_cloud_compression_amd import lib as L
    L.h_guard(dev()).zero_()


class _Level:
    """The modules of one decoder level with seeded weights: gen (5x5x5 stride-2 generative transposed, cin -> cm), c0 (3x3x3,
    cm -> ch), c2 (3x3x3, ch -> 1), and the SparseSynthesisTransform whose `_fused_weights` / `_up_predict_fused` are under test."""

    def __init__(self, cin, cm, ch, seed):
        import unified_point_cloud_compression_amd.MinkowskiEngine as ME
        from unified_point_cloud_compression_amd.model.transforms import SparseSynthesisTransform
        rng = np.random.default_rng(seed)
        self.cin, self.cm, self.ch = cin, cm, ch
        self.gen = ME.MinkowskiGenerativeConvolutionTranspose(cin, cm, kernel_size=5, stride=2, bias=True, dimension=3).to(dev())
        self.c0 = ME.MinkowskiConvolution(cm, ch, kernel_size=3, stride=1, bias=True, dimension=3).to(dev())
        self.c2 = ME.MinkowskiConvolution(ch, 1, kernel_size=3, stride=1, bias=True, dimension=3).to(dev())
        with torch.no_grad():
            for m, K, ci, c_out in ((self.gen, 125, cin, cm), (self.c0, 27, cm, ch), (self.c2, 27, ch, 1)):
                W, b = _weights(rng, K, ci, c_out)
                m.kernel.copy_(t(W))
                m.bias.copy_(t(b).reshape(1, -1))
        self.gs = SparseSynthesisTransform(dict(C_out=3, N1=16, N2=16, N3=16, N4=16))

    def f64(self, m):
        return m.kernel.detach().double(), m.bias.detach().double().reshape(-1)


def _composite_gpu(lv, name, x, form, slots=True):
    """Stage 1 as the decoder runs it: (h [n_out, ch], the launches recorded)."""
    from unified_point_cloud_compression_amd import lib as L, sparse as S
    g, cs, out_set = _geom(name), _cset(name), _candidates(name)
    with torch.no_grad():
        packedM, cb = lv.gs._fused_weights(lv.gen, lv.c0)
        csr7 = cs.csr_for(out_set.keys, out_set.n, 7, g.ts_out, zk=True, slots=slots)
        assert len(csr7) == (3 if slots else 2)

        def call():
            with L.arith_scope(form):
                return S.convt_forward_csr_grid(x, packedM, lv.c0.bias, 343, lv.cin, lv.ch, csr7, out_set, L.ACT_RELU, cb)
        return _recorded(call)


def _logits_gpu(lv, name, h):
    """Stage 2 as the decoder runs it."""
    from unified_point_cloud_compression_amd import sparse as S
    with torch.no_grad():
        w2 = lv.c2._packed.get(lv.c2.kernel, state_dict_order=True)
        return S.conv_thin_grid_forward(h, w2, lv.c2.bias, lv.ch, 1, _candidates(name))


def _kept_lists(name, kept_keys):
    """The 5-wide pair lists of the given candidate rows, as the decoder builds them: (csr5, the device counter's value)."""
    from unified_point_cloud_compression_amd import lib as L
    total = L.counter()
    csr5 = _cset(name).csr_for(kept_keys, kept_keys.shape[0], 5, _geom(name).ts_out, total=total)
    return csr5, int(L.read(total)[0])


def _rows_gpu(gen, x, csr5, n_kept, pairs_bound, form=None):
    """Stage 3 as the decoder runs it: (features of the kept rows, the launches recorded)."""
    from unified_point_cloud_compression_amd import lib as L, sparse as S
    with torch.no_grad():
        if "_packed_conv" not in gen.__dict__:
            gen.__dict__["_packed_conv"] = S.PackedConv(transposed=False)
        packed = gen._packed_conv.get(gen.kernel, state_dict_order=True)

        def call():
            with L.arith_scope(L.arith() if form is None else form):
                return S.convt_forward_rows(x, packed, gen.bias, 125, gen.in_channels, gen.out_channels, csr5, n_kept,
                                            pairs_bound=pairs_bound)
        return _recorded(call)


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 1: the composite level
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (cin, cm, ch, set): cin -> ch is the composite's shape, cm the width between the two layers it is made of
CASES = {
    "32x16_416a": (32, 32, 16, "416a"),        # 4 lanes per row, 3 bitmap columns per lane, JB = 4; last window inside the bitmap
    "32x16_416b": (32, 32, 16, "416b"),        #   ... last window clamped to the last dword pair
    "32x16_925": (32, 32, 16, "925"),          # another row tile of the dense product; input pitch 4
    "32x16_3719": (32, 32, 16, "3719"),        # the stripped GEMMs
    "128x32_925": (128, 64, 32, "925"),        # 8 lanes per row
    "128x64_925": (128, 128, 64, "925"),       # 16 lanes, one column per lane; T is 81 MB
    "16x8_925": (16, 16, 8, "925"),            # 2 lanes: the loop form of the probe
    "32x24_416a": (32, 48, 24, "416a"),        # 6 vectors on 8 lanes: idle lanes
    "32x6_416a": (32, 12, 6, "416a"),          # VEC = 1 (not a shape _can_fuse picks: the entry point is called directly anyway)
    "128x128_416a": (128, 128, 128, "416a"),   # 32 lanes per row
}

# (form, row tile, column tile, split) the dense product of a 16-channel composite (5488 columns: 43 column blocks, row tiles in
# groups of 8) records at the commit that added this file, and the forms of the kept-row pair GEMM.  NOT asserted per case from
# here: the last test checks that each is reached by some case and names the case meant to reach it.
EXPECT = {
    ("32x16_416a", "h3"): (FORM_CONV_BF, 32, 128, 1), ("32x16_925", "h3"): (FORM_CONV_BF, 64, 128, 1),
    ("32x16_3719", "h3"): (FORM_GEMM_H2, 128, 128, 1), ("32x16_3719", "bf6"): (FORM_GEMM_BF2, 128, 128, 1),
    ("32x16_416a", "f32"): (FORM_CONV_F32, 32, 128, 1), ("32x16_925", "f32"): (FORM_CONV_F32, 64, 128, 1),
    ("32x16_416b", "h3"): (FORM_GATHER_CSR, 0, 0, 1),
    ("rows_128x128", "h3"): (FORM_PAIR_H2, 128, 128, 1), ("rows_128x128", "bf6"): (FORM_PAIR_BF, 128, 128, 1),
    ("rows_128x128", "f32"): (FORM_CONV_F32, 128, 128, 1),
    ("rows_128x64", "bf6"): (FORM_PAIR_BF, 128, 64, 1), ("rows_128x32", "bf6"): (FORM_PAIR_BF, 128, 32, 1),
}
_seen = {}          # (case, arithmetic tag) -> {(form, BM, BN, ksplit)} recorded by the tests of this file


@functools.lru_cache(maxsize=None)
def _level(name):
    cin, cm, ch, _ = CASES[name]
    return _Level(cin, cm, ch, sum(name.encode()))


def _rows_of(name, set_name, cin, dist):
    g = _geom(set_name)
    rng = np.random.default_rng(sum(name.encode()) * 31 + DISTS.index(dist))
    return t(np.ascontiguousarray(shape_rows(rng.standard_normal((g.n_in, cin)).astype(np.float32), dist, rng)))


def _check(res, what):
    """The two rules on {tag: (max, rms)} of one data set: the absolute bounds for every form, rms(H3), rms(BF6) <= 3 rms(F32)."""
    for tag, (mx, rms) in res.items():
        assert mx <= MAX_RATIO and rms <= RMS_RATIO, (what, tag, mx, rms)
    for tag in ("h3", "bf6"):
        assert res[tag][1] <= 3.0 * res["f32"][1], (what, tag, res)


@gpu
def test_lattice_variants_put_the_last_window_inside_and_beyond_the_last_dword_pair():
    """416a / 416b: the candidate lattices differ by one parent cell of extent; (cells - 2) % 64 -- the cell of the last row's own
    z window -- is below 32 in one (the window starts in the low dword of the last pair) and at least 32 in the other (it starts
    in the last dword: `dw > last_dw`, the clamped branch of k_convt_gather_csr).  Both sets have their first row in cell 0 and
    their last row in the last cell."""
    from unified_point_cloud_compression_amd import sparse as S
    cells = {}
    for name in ("416a", "416b"):
        out_set = _candidates(name)
        lat = S.Lattice.of(out_set.bounds, out_set.ts)
        cells[name] = lat.cells
        C = co.unpack_keys(_geom(name).out_keys)
        assert tuple(C[0, 1:]) == tuple(out_set.bounds.lo) and C[0, 0] == 0
        assert tuple(C[-1, 1:]) == tuple(out_set.bounds.hi) and C[-1, 0] == out_set.bounds.bmax == 1
    assert (cells["416a"] - 2) % 64 < 32 <= (cells["416b"] - 2) % 64, cells


@gpu
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", list(CASES))
def test_composite_level_matches_layerwise_float64(name, dist):
    """h = relu(c0(genT(x))) of `pcc_convt_fwd_csr_grid` with `_fused_weights`' kernel and constants over
    `csr_for(zk=True, slots=True)`, every entry against the layer-wise float64 reference, under H3, BF6 and F32 on the same data:
    the absolute bounds for each, rms(H3) and rms(BF6) <= 3 rms(F32).  Two records per call: the dense product, then the
    gather-sum.  Under H3 a second call and a call over the prefix-form lists (slots=False) give the same bits.

    Measured on MI355X, rms(H3) / rms(F32) over the cases 0.76 - 1.11, rms(BF6) / rms(F32) 0.81 - 1.08.
    Sensitivity, measured once on scratch builds of the library (nothing of them committed; both change arithmetic only):
    (i) `k_gemm_h2` without its h * l' MFMA term: the ten runs whose product takes that kernel fail, e.g. 32x16_3719 relu rms(H3)
    1.170e-4 against rms(F32) 7.186e-8 (1628x; intact 7.968e-8, 1.11x), max 8.0e-4; the others 1.06e-4 - 1.43e-4 (> 900x).
    (ii) `k_convt_gather_csr` without the fourth table row of the presence constants (neighbours 21 - 26): all twenty runs fail
    outright under every form, max 0.85 - 1.53, rms 0.049 - 0.28 of S2."""
    from unified_point_cloud_compression_amd import lib as L
    cin, cm, ch, set_name = CASES[name]
    g, lv = _geom(set_name), _level(name)
    x = _rows_of(name, set_name, cin, dist)
    (W5, gb), (V3, c0b) = lv.f64(lv.gen), lv.f64(lv.c0)
    _, v = _layerwise64(g, x.double(), W5, gb, V3, c0b)
    _, sq = _composite_sums64(g, x.double(), W5, gb, V3, c0b)
    ref, s2 = torch.clamp_min(v, 0), sq.sqrt()
    res = {}
    try:
        for tag, form in _forms().items():
            h, rec = _composite_gpu(lv, set_name, x, form)
            assert h.shape == (g.n_out, ch)
            assert len(rec) == 2 and rec[1][0] == FORM_GATHER_CSR, (name, tag, rec)
            _seen.setdefault((name, tag), set()).update(rec)
            res[tag] = ratios(h, ref, s2)
            print(f"DECCONV composite {name:13s} {dist:6s} {tag:3s} form {L.FORM_NAMES[rec[0][0]]:14s} tile {rec[0][1]:3d} x {rec[0][2]:3d} "
                  f"max {res[tag][0]:.3e} rms {res[tag][1]:.3e}")
            if tag == "h3":
                again, rec2 = _composite_gpu(lv, set_name, x, form)
                assert rec2 == rec and np.array_equal(bits(h), bits(again)), f"{name}: two calls differ"
                prefix, _ = _composite_gpu(lv, set_name, x, form, slots=False)
                assert np.array_equal(bits(h), bits(prefix)), f"{name}: slotted and prefix-form lists give different bits"
    finally:
        _clear_guard()
    _check(res, (name, dist))


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 2: the logits
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,z_folded", [("32x16_925", False), ("32x16_925", True), ("128x32_925", False), ("128x64_925", False)])
def test_head_logits_match_float64_on_the_gpus_own_hidden_features(name, z_folded):
    """`pcc_conv_thin_grid_fwd` on h = the GPU's own stage-1 output (ch = 16, 32, 64; for 16 both plane forms) against float64
    b2 + sum_j index_add(h[i_j] @ V2[j]) over the oracle's 3x3x3 pairs of the candidate set; same bits on a second call."""
    from unified_point_cloud_compression_amd import lib as L
    cin, cm, ch, set_name = CASES[name]
    g, lv = _geom(set_name), _level(name)
    try:
        h, _ = _composite_gpu(lv, set_name, _rows_of(name, set_name, cin, "relu"), L.ARITH_H3)
    finally:
        _clear_guard()
    assert float(h.abs().max()) > 0 and bool((h == 0).any())          # (a ReLU output: both signs of the pre-activation occur)
    V2, b2 = lv.f64(lv.c2)
    ref, sq = conv_sums64(h.double(), V2, b2, g.pairs3, g.n_out)
    try:
        if z_folded:
            L.call("pcc_set_thin_z_min_rows", 0)
        logit = _logits_gpu(lv, set_name, h)
        again = _logits_gpu(lv, set_name, h)
    finally:
        L.call("pcc_set_thin_z_min_rows", 1 << 20)
    assert logit.shape == (g.n_out, 1)
    mx, rms = ratios(logit, ref, sq.sqrt())
    print(f"DECCONV logits    {name:13s} relu   {'z-folded planes' if z_folded else '27 planes':15s} max {mx:.3e} rms {rms:.3e}")
    assert np.array_equal(bits(logit), bits(again))
    assert mx <= MAX_RATIO and rms <= RMS_RATIO, (name, z_folded, mx, rms)


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 3: the kept rows
# ---------------------------------------------------------------------------------------------------------------------------------
ROW_SHAPES = ((128, 128), (128, 64), (128, 32))          # cin -> cout of the generative convolution; 128 -> 32: the model's last level
KEPT = ("fifth", "one", "2048", "2049", "all416")


def _thinned(cnt, target, seed):
    """Rows in a seeded random order, each taken while the pair total stays within `target`, until it is met exactly."""
    total, sel = 0, []
    for o in np.random.default_rng(seed).permutation(len(cnt)):
        if total + cnt[o] <= target:
            sel.append(o)
            total += cnt[o]
            if total == target:
                break
    assert total == target
    return np.sort(np.asarray(sel, np.int64))


@functools.lru_cache(maxsize=None)
def _kept(kind):
    """(set, candidate rows kept (ascending), the oracle's pairs restricted to them, its (first, pair_ids) of the kept rows)."""
    set_name = "416a" if kind == "all416" else "3719"
    g = _geom(set_name)
    if kind == "fifth":              # ~26 k rows, ~93 k pairs: 46 blocks of the bucketing passes
        sel = np.unique(np.concatenate([np.arange(0, g.n_out, 5), [0, g.n_out - 1]]))
    elif kind == "one":              # nearly all of the 125 offset buckets empty
        sel = np.array([g.n_out // 3], np.int64)
    elif kind == "all416":
        sel = np.arange(g.n_out)
    else:                            # exactly one block of CK_B = 2048 pairs / one block and one pair more
        sel = _thinned(g.parents_per_row, int(kind), 11)
    new = np.full(g.n_out, -1, np.int64)
    new[sel] = np.arange(len(sel))
    pairs = []
    for i, o in g.pairs5:
        o2 = new[o]
        pairs.append((i[o2 >= 0], o2[o2 >= 0]))
    rows = np.concatenate([o for _, o in pairs])
    src = np.concatenate([i for i, _ in pairs]).astype(np.int64)
    off = np.concatenate([np.full(len(i), k, np.int64) for k, (i, _) in enumerate(pairs)])
    order = np.lexsort((src, rows))                      # by kept row, inside a row by ascending input row
    first = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(sel)))])
    return set_name, sel, pairs, (first, (src * 125 + off)[order])


@gpu
@pytest.mark.parametrize("kind", KEPT)
def test_kept_row_pair_lists_hold_the_oracles_parents(kind):
    """`csr_for(kept keys, 5, total=counter)`: the device counter equals the oracle's pair total, and `first` / `pair_ids` hold for
    EVERY kept row the oracle's parents in ascending input row, each with the oracle's offset (pair id = input row * 125 + k)."""
    set_name, sel, pairs, (first, pids) = _kept(kind)
    g = _geom(set_name)
    total = sum(len(i) for i, _ in pairs)
    if kind in ("2048", "2049"):
        assert total == int(kind)
    elif kind == "fifth":
        assert total > 40 * 2048 and g.parents_per_row[sel].max() > 16
    csr5, counted = _kept_lists(set_name, t(g.out_keys[sel]))
    assert counted == total == int(first[-1])
    assert np.array_equal(n(csr5[0])[:len(sel) + 1], first)
    assert np.array_equal(n(csr5[1])[:total], pids)


@gpu
@pytest.mark.parametrize("kind", KEPT)
@pytest.mark.parametrize("cin,cout", ROW_SHAPES)
def test_kept_row_features_match_float64(cin, cout, kind):
    """`pcc_convt_fwd_rows` on the kept rows against the rows of float64 u = gen.bias + sum_k index_add(x[i_k] @ W5[k]) at the kept
    indices (the oracle's pairs restricted to them), under H3, BF6 and F32, rows of both distributions: the absolute bounds for
    each, rms(H3) and rms(BF6) <= 3 rms(F32).  Every call is repeated and gives the same bits; for the every-fifth-row set a
    pair bound of pairs + 129 and of 2 pairs (larger T, workspace and grids; same buckets) gives the bits of the exact count.
    Measured on MI355X, rms(H3) / rms(F32) and rms(BF6) / rms(F32) over the cases: 0.65 - 1.48 (both ends on the one-row set, 32 entries)."""
    from unified_point_cloud_compression_amd import lib as L
    assert L.load().pcc_conv_pairs_supported(125, cin, cout)
    set_name, sel, pairs, _ = _kept(kind)
    g = _geom(set_name)
    name = f"rows_{cin}x{cout}"
    lv = _rows_level(cin, cout)
    W5, gb = lv.f64(lv.gen)
    csr5, total = _kept_lists(set_name, t(g.out_keys[sel]))
    assert total == sum(len(i) for i, _ in pairs)
    try:
        for dist in DISTS:
            x = _rows_of(f"{name}_{kind}", set_name, cin, dist)
            ref, sq = conv_sums64(x.double(), W5, gb, pairs, len(sel))
            s2 = sq.sqrt()
            res = {}
            for tag, form in _forms().items():
                xk, rec = _rows_gpu(lv.gen, x, csr5, len(sel), total, form)
                assert xk.shape == (len(sel), cout) and len(rec) == 1, (name, kind, tag, rec)
                _seen.setdefault((name, tag), set()).update(rec)
                res[tag] = ratios(xk, ref, s2)
                print(f"DECCONV rows      {name:13s} {kind:6s} {dist:6s} {tag:3s} form {L.FORM_NAMES[rec[0][0]]:14s} tile {rec[0][1]:3d} x {rec[0][2]:3d} "
                      f"max {res[tag][0]:.3e} rms {res[tag][1]:.3e}")
                again, rec2 = _rows_gpu(lv.gen, x, csr5, len(sel), total, form)
                assert rec2 == rec and np.array_equal(bits(xk), bits(again)), f"{name} {kind} {tag}: two calls differ"
                if kind == "fifth":
                    for bound in (total + 129, 2 * total):
                        other, _ = _rows_gpu(lv.gen, x, csr5, len(sel), bound, form)
                        assert np.array_equal(bits(xk), bits(other)), f"{name} {tag}: pairs_bound {bound} changes the result"
            _check(res, (name, kind, dist))
    finally:
        _clear_guard()


@functools.lru_cache(maxsize=None)
def _rows_level(cin, cout):
    return _Level(cin, cout, 16, cin * 1000 + cout)


# ---------------------------------------------------------------------------------------------------------------------------------
# the decoder's own call sequence
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_up_predict_fused_runs_these_kernels_on_these_inputs():
    """`_up_predict_fused` on the 32 -> 16 level (925 parents) with a probe that records the logits at "select", returns a fixed
    pseudo-random mask and records the kept features at "kept": both records are bit-identical to the stage-by-stage calls of
    this file on the same inputs -- the kernels tested above are the ones a decoder level runs, in its call sequence."""
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd.MinkowskiEngine.sparse_tensor import SparseTensor
    name, set_name = "32x16_925", "925"
    g, lv, cs = _geom(set_name), _level(name), _cset(set_name)
    x = _rows_of(name, set_name, lv.cin, "relu")
    keep = np.random.default_rng(17).random(g.n_out) < 0.1
    keep[[0, -1]] = True
    seen = {}

    def probe(stage, lvl, cset, logit, mask, feats):
        if stage == "select":
            assert cset.n == g.n_out and mask.shape == (g.n_out,)
            seen["logit"] = logit.detach().clone()
            return t(keep)
        seen["kept_keys"], seen["kept"] = n(cset.keys[:cset.n]), feats.detach().clone()

    up = torch.nn.Sequential(lv.gen)
    head = torch.nn.Sequential(lv.c0, ME.MinkowskiReLU(inplace=False), lv.c2)
    try:
        with torch.no_grad():
            assert lv.gs._can_fuse(up, head, SparseTensor._from_canonical(cs, x))      # (the decoder would take this path)
            out, pred, mask = lv.gs._up_predict_fused(up, head, SparseTensor._from_canonical(cs, x), [5, 5], probe=probe)
        h, _ = _composite_gpu(lv, set_name, x, L.arith())
        logit = _logits_gpu(lv, set_name, h)
        kept_keys = g.out_keys[keep]
        csr5, total = _kept_lists(set_name, t(kept_keys))
        xk, _ = _rows_gpu(lv.gen, x, csr5, len(kept_keys), total)
    finally:
        _clear_guard()
    assert L.load().pcc_conv_pairs_supported(125, lv.cin, lv.cm)        # (the level takes the kept-row form, not the slot map)
    assert np.array_equal(bits(seen["logit"]), bits(logit)) and np.array_equal(bits(pred.F), bits(logit))
    assert np.array_equal(seen["kept_keys"], kept_keys) and np.array_equal(n(mask), keep)
    assert np.array_equal(bits(seen["kept"]), bits(xk)) and np.array_equal(bits(out.F), bits(xk))


@gpu
def test_every_listed_regime_was_reached():
    """The union of the records of this file's runs covers every regime of EXPECT.  A case that did not run in this process (the
    test selected alone) is run here, without a reference.  When a later change of the dispatch moves a threshold, the message
    names the regime that lost its case, the case meant to reach it and what that case records now."""
    forms = _forms()
    try:
        for name, tag in EXPECT:
            if (name, tag) in _seen:
                continue
            if name.startswith("rows_"):
                cin, cout = (int(v) for v in name[5:].split("x"))
                set_name, sel, _, _ = _kept("fifth")
                csr5, total = _kept_lists(set_name, t(_geom(set_name).out_keys[sel]))
                _, rec = _rows_gpu(_rows_level(cin, cout).gen, _rows_of(name, set_name, cin, "relu"), csr5, len(sel), total, forms[tag])
            else:
                cin, _, _, set_name = CASES[name]
                _, rec = _composite_gpu(_level(name), set_name, _rows_of(name, set_name, cin, "relu"), forms[tag])
            _seen.setdefault((name, tag), set()).update(rec)
    finally:
        _clear_guard()
    reached = set().union(*_seen.values())
    lost = {}
    for key, regime in EXPECT.items():
        if regime not in reached:
            lost.setdefault(regime, []).append((key, sorted(_seen[key])))
    assert not lost, f"regimes no case reaches any more (form, BM, BN, ksplit) -> [((case, arithmetic) meant to, what it records now)]: {lost}"
