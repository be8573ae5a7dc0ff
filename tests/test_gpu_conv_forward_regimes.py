"""Forward convolutions (`pcc_conv_fwd`, K = 27 / 125 maps and the K = 1 products) against float64 in every regime of the MFMA
dispatch: the 128-, 64- and 32-row tiles of `k_conv_mfma_bf` / `k_conv_mfma` on 128-, 64- and 32-column outputs, the split
reduction (`ksplit`, `k_splitk_reduce`) on each row tile, the row-group sweep of wide dense products, `k_conv_in4_bf` at its own
row threshold, and the persistent loops of `k_conv_wave16z` / `k_conv_wave16` below, at and above the row count where their
grid wraps.  Every case runs under `ARITH_BF6` (six bf16 terms) and under `ARITH_F32` (fp32-input MFMAs, same tile templates).

The regime a call reached is READ from the library (`pcc_prof_sequence`, `pcc_prof_sequence_tiles`), never computed from a copy
of the dispatch rules; the last test of the file checks that the regimes listed in EXPECT were all reached.

Metric (that of test_gpu_weight_gradients.py).  For every entry out[o][co] = bias + sum over the pairs (i, o) of every offset k
of x[i] . W[k][:, co], the error |got - ref| is divided by S2 = sqrt(bias^2 + sum of the squared terms), the size of random
rounding in a sum of those terms; max and rms over all entries.  An entry with S2 = 0 must be exactly 0, a non-finite output
counts as infinite.  The float64 reference runs on the GPU through torch over the ORACLE's pairs (never the library's map); one
test checks it against numpy float64 on the CPU.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import codec, coords as co
from tests.util import dev, t, n, bits as _bits, conv_sums64, coord_set, flat_keys, ratios, shape_rows, surface_keys

pytestmark = pytest.mark.gpu

FORM_CONV_BF, FORM_CONV_F32, FORM_WAVE16 = 5, 6, 7      # include/pcc_hip.h PCC_FORM_*
DISTS = ("relu", "spread")
EPILOGUES = ((False, 0), (True, 1), (True, 2))      # (bias, activation): none / bias + ReLU / bias + leaky(0.2), in rotation
FIXED_EPILOGUE = {"128x128_k1_65409": (True, 1), "128x1152_k1_7301": (True, 0)}
SLOPE = 0.2


# ---------------------------------------------------------------------------------------------------------------------------------
# coordinate sets (canonical keys, numpy)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _keys(name):
    """'surf:N' -- the first N keys of the 209 853-row surface (an x-slab of it: again a canonical set); 'surf' -- all of it;
    'surf/2' -- its stride-2 set; 'isolated' -- a 30^3 lattice of pitch 3 (27 000 rows, only the centre offset of a 3x3x3 kernel
    has pairs); 'flat' -- one z plane (9 of the 27 offsets have pairs)."""
    if name == "surf":
        return surface_keys(0.515)
    if name.startswith("surf:"):
        return surface_keys(0.515)[:int(name[5:])]
    if name == "surf/2":
        return co.stride_keys(surface_keys(0.515), 2)
    if name == "isolated":
        g = np.arange(30, dtype=np.int64) * 3
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        C = np.stack([np.zeros(27000, np.int64), x.ravel(), y.ravel(), z.ravel()], axis=1)
        return co.canonicalize(C)[0]
    if name == "flat":
        return flat_keys()
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _cset(name):
    if name == "surf/2":
        return _cset("surf").stride(2)
    return coord_set(_keys(name), 1)


@functools.lru_cache(maxsize=None)
def _pairs(src, dst, ks):
    """The oracle's pairs per offset: [(in_rows, out_rows)] (numpy, independent of the library's map)."""
    return codec.kernel_map_pairs(_keys(src), _keys(dst), ks, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (cin, cout, ks, in set, out set (None: K = 1, no map), morton, kind)
#   kind: "mfma" -- k_conv_mfma_bf under BF6, k_conv_mfma under F32;  "in4lo" -- 4 input channels below the row threshold of the
#   flattened form: k_conv_mfma under both;  "in4" -- k_conv_in4_bf under BF6, k_conv_mfma under F32;  "wave16" -- both alike
def _surf(cin, cout, rows, morton=False, kind="mfma", ks=3):
    s = "surf" if rows is None else f"surf:{rows}"
    return (cin, cout, ks, s, s, morton, kind)


CASES = {
    "128x128_16320": _surf(128, 128, 16320), "128x128_16321": _surf(128, 128, 16321),
    "128x128_32640": _surf(128, 128, 32640), "128x128_32641": _surf(128, 128, 32641),
    "128x128_32704": _surf(128, 128, 32704), "128x128_32705": _surf(128, 128, 32705),
    "128x128_65408": _surf(128, 128, 65408), "128x128_65409": _surf(128, 128, 65409),     # 511 full 128-row tiles + one row
    "128x128_65409_morton": _surf(128, 128, 65409, morton=True),                          # row-list map: outputs scattered
    "128x128_stride2": (128, 128, 3, "surf", "surf/2", False, "mfma"),                    # n_in != n_out
    "256x128_13057": _surf(256, 128, 13057),                                              # deep reduction: 5-way split
    "192x256_8065": _surf(192, 256, 8065),                                                # two column blocks, 4-way split
    "192x192_32641": _surf(192, 192, 32641),                                              # second column block half empty
    "128x64_32640": _surf(128, 64, 32640), "128x64_65409": _surf(128, 64, 65409),
    "32x64_65408": _surf(32, 64, 65408),
    "128x32_32640": _surf(128, 32, 32640), "128x32_65409": _surf(128, 32, 65409),
    "128x128_isolated": (128, 128, 3, "isolated", "isolated", False, "mfma"),
    "128x128_flat": (128, 128, 3, "flat", "flat", False, "mfma"),
    "128x128_k1_65409": (128, 128, 1, "surf:65409", None, False, "mfma"),                 # identity tile
    "128x1152_k1_7301": (128, 1152, 1, "surf:7301", None, False, "mfma"),                 # 9 column blocks: row tiles in groups of 8
    "4x128_k125_65535": _surf(4, 128, 65535, kind="in4lo", ks=5),
    "4x128_k125_65536": _surf(4, 128, 65536, kind="in4", ks=5),                           # the flattened form's own threshold
    "4x128_k27_209853": _surf(4, 128, None, kind="in4"),
    "32x16_209853_morton": _surf(32, 16, None, morton=True, kind="wave16"),               # generic k_conv_wave16
}
for _cin, _cout in ((32, 16), (16, 16), (32, 8)):         # k_conv_wave16z: 512 workgroups x 8 tiles x 32 rows = 131 072 rows a pass
    for _rows in (131072, 131073, None):                  # no wrap / first wrap / several passes
        CASES[f"{_cin}x{_cout}_{_rows or 209853}"] = _surf(_cin, _cout, _rows, kind="wave16")

# (form, row tile, column tile, reduction split) the dispatch at the commit that added this file gives under BF6.  NOT asserted per
# case from here: the last test of the file checks that every regime listed is reached by some case, and names the cases meant to.
EXPECT = {
    "128x128_16320": (FORM_CONV_BF, 32, 128, 2), "128x128_16321": (FORM_CONV_BF, 64, 128, 2),
    "128x128_32640": (FORM_CONV_BF, 64, 128, 2), "128x128_32641": (FORM_CONV_BF, 32, 128, 1),
    "128x128_32704": (FORM_CONV_BF, 32, 128, 1), "128x128_32705": (FORM_CONV_BF, 64, 128, 1),
    "128x128_65408": (FORM_CONV_BF, 64, 128, 1), "128x128_65409": (FORM_CONV_BF, 128, 128, 1),
    "128x128_65409_morton": (FORM_CONV_BF, 128, 128, 1),
    "256x128_13057": (FORM_CONV_BF, 128, 128, 5), "192x256_8065": (FORM_CONV_BF, 128, 128, 4),
    "192x192_32641": (FORM_CONV_BF, 128, 128, 1),
    "128x64_32640": (FORM_CONV_BF, 64, 64, 2), "128x64_65409": (FORM_CONV_BF, 128, 64, 1), "32x64_65408": (FORM_CONV_BF, 64, 64, 1),
    "128x32_32640": (FORM_CONV_BF, 128, 32, 2), "128x32_65409": (FORM_CONV_BF, 128, 32, 1),
    "128x128_isolated": (FORM_CONV_BF, 64, 128, 2),
    "128x128_k1_65409": (FORM_CONV_BF, 128, 128, 1), "128x1152_k1_7301": (FORM_CONV_BF, 128, 128, 1),
    "4x128_k125_65535": (FORM_CONV_F32, 128, 128, 1), "4x128_k125_65536": (FORM_CONV_BF, 128, 128, 1),
    "4x128_k27_209853": (FORM_CONV_BF, 128, 128, 1),
    "32x16_209853_morton": (FORM_WAVE16, 32, 16, 1),
}
EXPECT.update({name: (FORM_WAVE16, 32, 16, 1) for name, c in CASES.items() if c[6] == "wave16"})

_seen = {}          # case -> {(form, BM, BN, ksplit)} recorded under BF6 by the tests of this file


def _case_seed(name, dist):
    return sum(name.encode()) * 31 + DISTS.index(dist)


def _epilogue(name):
    return FIXED_EPILOGUE.get(name) or EPILOGUES[list(CASES).index(name) % 3]


def _case_inputs(name, dist):
    """(x [n_in, cin], W [K, cin, cout], bias [cout] or None, act) float32: weights standard_normal / sqrt(cin * 8)."""
    cin, cout, ks, src, dst, _, _ = CASES[name]
    rng = np.random.default_rng(_case_seed(name, dist))
    x = shape_rows(rng.standard_normal((len(_keys(src)), cin)).astype(np.float32), dist, rng)
    W = (rng.standard_normal((ks ** 3 if dst is not None else 1, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32)
    has_bias, act = _epilogue(name)
    b = rng.standard_normal(cout).astype(np.float32) if has_bias else None
    return np.ascontiguousarray(x, np.float32), W, b, act


def _act64(v, act):
    if act == 1:
        return torch.clamp_min(v, 0)
    if act == 2:
        return torch.where(v > 0, v, v * SLOPE)
    return v


def _ref64(x, W, b, act, pairs, n_out):
    """(ref, S2) [n_out, cout] float64 on the GPU: ref = act(bias + sum_k index_add(x[i_k] @ W[k])),
    S2 = sqrt(bias^2 + sum_k index_add(x[i_k]^2 @ W[k]^2)) over the oracle's pairs (pairs None: the identity, K = 1)."""
    ref, sq = conv_sums64(t(x).double(), t(W).double(), t(b).double() if b is not None else None, pairs, n_out)
    return _act64(ref, act), sq.sqrt()


def _run(name, xt, Wt, bt, act, form):
    """One `sparse.conv_forward` of the case under arithmetic form `form` with the per-launch record on: (out, recorded
    [(form, BM, BN, ksplit)] of the call in launch order)."""
    from unified_point_cloud_compression_amd import lib as L, sparse as S
    cin, cout, ks, src, dst, morton, _ = CASES[name]
    kmap = _cset(src).kernel_map(_cset(dst), ks, morton=morton) if dst is not None else None
    n_out = _cset(dst).n if dst is not None else xt.shape[0]
    pk = S.PackedConv().get(torch.nn.Parameter(Wt if dst is not None else Wt[0]))
    lib = L.load()
    L.call("pcc_prof_enable", 1)
    try:
        with L.arith_scope(form):
            out = S.conv_forward(xt, pk, bt, Wt.shape[0], cin, cout, kmap, n_out, act=act, slope=SLOPE)
        forms = (ctypes.c_int32 * 16)()
        tiles = (ctypes.c_int32 * 48)()
        cnt = int(lib.pcc_prof_sequence(forms, 16))
        assert int(lib.pcc_prof_sequence_tiles(tiles, 16)) == cnt
        rec = [(forms[j], tiles[3 * j], tiles[3 * j + 1], tiles[3 * j + 2]) for j in range(min(cnt, 16))]
    finally:
        L.call("pcc_prof_enable", 0)
    assert cnt == 1, (name, rec)                # one event-timed launch per pcc_conv_fwd
    return out, rec[0]


def _expected_form(kind, form):
    from unified_point_cloud_compression_amd import lib as L
    if kind == "wave16":
        return FORM_WAVE16
    if kind == "in4lo" or form == L.ARITH_F32:
        return FORM_CONV_F32
    return FORM_CONV_BF


# One absolute bound on |got - ref| / S2 for every forward kernel of this file.  Measured on MI355X over every case, both operand
# distributions and both forms (profiles/conv_forward_regimes.txt): max 1.68e-5 (128 -> 128 at 32 641 rows, spread rows, the
# fp32-input kernel; the six-term kernel's worst is 9.2e-6), rms 8.6e-7 (192 -> 192 at 32 641 rows, spread rows, the fp32-input
# kernel; six-term 7.1e-7).  Bounds: 3.0x / 2.9x above.
MAX_RATIO = 5e-5
RMS_RATIO = 2.5e-6


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_convolution_matches_float64_in_its_regime(name, dist):
    """Every entry of the output against float64 over the oracle's pairs, under BF6 and under F32 on the same data: max and rms
    of |got - ref| / S2 below the file's absolute bounds for both, and rms(BF6) <= 3 rms(F32) (the rule of
    `test_split_path_accuracy`: fp32-level error, not that of a product with a term missing).  The recorded form must be the
    kernel the case is about; a case whose record shows a split reduction is run twice and must give the same bits (the
    partial sums are reduced in fixed order).

    Measured on MI355X, rms(BF6) / rms(F32) over the cases: 0.36 - 1.34 (the largest: 4 -> 128, K = 125, at 65 536 rows).
    Sensitivity, measured once with a library built without the m * m term of `bf6_terms` (pcc_mfma.h), case 128x128_65409: rms
    of the six-term kernel 1.56e-6 against 2.85e-7 of the fp32-input kernel on relu rows (5.5x; intact 3.28e-7, 1.15x) and
    1.98e-6 against 5.06e-7 on spread rows (3.9x; intact 3.44e-7, 0.68x): the 3x rule fails on both, while the absolute bounds
    alone (max 1.5e-5, rms 2.0e-6) would not notice."""
    from unified_point_cloud_compression_amd import lib as L
    cin, cout, ks, src, dst, morton, kind = CASES[name]
    x, W, b, act = _case_inputs(name, dist)
    xt, Wt, bt = t(x), t(W), (t(b) if b is not None else None)
    n_out = len(_keys(dst)) if dst is not None else len(x)
    ref, s2 = _ref64(x, W, b, act, _pairs(src, dst, ks) if dst is not None else None, n_out)
    res, outs = {}, {}
    for tag, form in (("bf6", L.ARITH_BF6), ("f32", L.ARITH_F32)):
        out, rec = _run(name, xt, Wt, bt, act, form)
        assert out.shape == (n_out, cout)
        assert rec[0] == _expected_form(kind, form), (name, tag, rec)
        if rec[3] > 1:
            again, rec2 = _run(name, xt, Wt, bt, act, form)
            assert rec2 == rec and np.array_equal(_bits(out), _bits(again)), f"{name} {tag}: two calls of a split reduction differ"
        mx, rms = ratios(out, ref, s2)
        res[tag], outs[tag] = (mx, rms, rec), out
        print(f"CONVFWD {name:22s} {dist:6s} {tag} form {L.FORM_NAMES[rec[0]]:14s} tile {rec[1]:3d} x {rec[2]:3d} ksplit {rec[3]} "
              f"max {mx:.3e} rms {rms:.3e}")
    _seen.setdefault(name, set()).add(res["bf6"][2])
    for tag in ("bf6", "f32"):
        assert res[tag][0] <= MAX_RATIO and res[tag][1] <= RMS_RATIO, (name, dist, tag, res[tag])
    assert res["bf6"][1] <= 3.0 * res["f32"][1], (name, dist, res)
    if name == "128x128_isolated":                    # only the centre offset has pairs: out = act(bias + x W[13]), directly
        assert [len(i) for i, _ in _pairs(src, dst, ks)] == [0] * 13 + [len(x)] + [0] * 13
        ref1, s21 = _ref64(x, W[13:14], b, act, None, n_out)
        mx1, rms1 = ratios(outs["bf6"], ref1, s21)
        assert mx1 <= MAX_RATIO and rms1 <= RMS_RATIO, (mx1, rms1)
    if name == "128x128_flat":
        dz = co.kernel_offsets(3)[:, 2]
        assert [len(i) > 0 for i, _ in _pairs(src, dst, ks)] == (dz == 0).tolist()        # 9 of 27 offsets live


def test_float64_reference_on_the_gpu_equals_numpy_float64():
    """The GPU float64 reference (torch fp64 GEMMs + index_add) against numpy float64 on the CPU: 32 -> 128, K = 27, bias and
    leaky ReLU, on the first 65 409 rows of the surface (821 879 pairs)."""
    rows = 65409
    src = f"surf:{rows}"
    rng = np.random.default_rng(77)
    x = shape_rows(rng.standard_normal((rows, 32)).astype(np.float32), "spread", rng)
    W = (rng.standard_normal((27, 32, 128)) / np.sqrt(32 * 8)).astype(np.float32)
    b = rng.standard_normal(128).astype(np.float32)
    pairs = _pairs(src, src, 3)
    assert sum(len(i) for i, _ in pairs) == 821879
    ref, s2 = _ref64(x, W, b, 2, pairs, rows)
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    want = np.zeros((rows, 128)) + b.astype(np.float64)
    sq = np.zeros((rows, 128)) + b.astype(np.float64) ** 2
    for k, (i, o) in enumerate(pairs):               # (an output row has at most one pair per offset: o has no repeats)
        if len(i):
            want[o] += x64[i] @ W64[k]
            sq[o] += (x64[i] ** 2) @ (W64[k] ** 2)
    want = np.where(want > 0, want, want * SLOPE)
    s = np.sqrt(sq)
    assert np.all(np.abs(n(s2) - s) <= 1e-12 * s)
    err = np.abs(n(ref) - want)
    assert np.all(err <= 1e-12 * s), float((err / s).max())


def test_results_do_not_depend_on_what_the_library_scratch_held():
    """The split reduction keeps its bf16 planes and its partial sums in the library's scratch: the 256 -> 128 case (5-way
    split: 20 MB of planes, then 33 MB of partial sums), then a call whose features are all NaN (128 -> 128 at 65 409 rows:
    50 MB of NaN planes from the start of the same scratch, over the first call's planes and four and a half of its five
    partial slabs), then the first case again -- bit-identical and finite."""
    from unified_point_cloud_compression_amd import lib as L
    name, big = "256x128_13057", "128x128_65409"
    x, W, b, act = _case_inputs(name, "relu")
    xt, Wt, bt = t(x), t(W), (t(b) if b is not None else None)
    first, rec = _run(name, xt, Wt, bt, act, L.ARITH_BF6)
    assert rec[3] > 1, rec                              # (the record: this case does split its reduction)
    xb, Wb, _, _ = _case_inputs(big, "relu")
    assert x.size * 6 + (rec[3] - 1) * first.numel() * 4 <= xb.size * 6     # the NaN planes reach into the last partial slab
    poison, _ = _run(big, torch.full(xb.shape, float("nan"), dtype=torch.float32, device=dev()), t(Wb), None, 0, L.ARITH_BF6)
    assert bool(torch.isnan(poison).all())              # (no bias, no activation: every row has its own NaN row as a neighbour)
    second, rec2 = _run(name, xt, Wt, bt, act, L.ARITH_BF6)
    assert rec2 == rec
    assert bool(torch.isfinite(first).all())
    assert np.array_equal(_bits(first), _bits(second)), "the scratch's earlier contents changed the result"


def test_every_listed_regime_was_reached():
    """The union of the (form, row tile, column tile, reduction split) records of this file's BF6 runs covers every regime of
    EXPECT.  A case that did not run in this process (the test selected alone) is run here, without a reference.  When a later
    change of the dispatch moves a threshold, the message names the regime that lost its case and what its cases reach now."""
    from unified_point_cloud_compression_amd import lib as L
    for name in EXPECT:
        if name not in _seen:
            x, W, b, act = _case_inputs(name, "relu")
            _seen.setdefault(name, set()).add(_run(name, t(x), t(W), t(b) if b is not None else None, act, L.ARITH_BF6)[1])
    reached = set().union(*_seen.values())
    lost = {}
    for name, regime in EXPECT.items():
        if regime not in reached:
            lost.setdefault(regime, []).append((name, sorted(_seen[name])))
    assert not lost, f"regimes no case reaches any more (form, BM, BN, ksplit) -> [(case meant to, what it records now)]: {lost}"
