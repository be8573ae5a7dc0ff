"""Weight gradients of the sparse convolutions (`pcc_conv_wgrad`, `pcc_conv_wgrad_self`) against float64 at the shapes, row counts
and kernel geometries of the R2-width training step (`profiles/r04_train_step_by_layer.txt`), plus the structural edges where a
reduction kernel goes wrong without a loose tolerance noticing: empty offsets, empty inputs, a poisoned workspace, slice and
sub-block boundaries, and the empty trailing blocks of the input-stationary forms at a million rows.

Metric.  For every entry dW[k][ci][co] = sum over the pairs (i, o) of offset k of x[i][ci] g[o][co], the error |got - ref| is
divided by S2 = sqrt(sum over the same pairs of (x[i][ci] g[o][co])^2), the size of random rounding in a sum of those terms.
(sum |x g| is not used: over 1e5 pairs it is ~300x larger than S2 and hides even a bf16-only product.)  The float64 reference
runs on the GPU through torch (fp64 GEMMs of the oracle's pairs: a different code path from the library); one test checks it
against numpy float64 on the CPU.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import codec, coords as co
from tests.util import dev, t, n, coord_set, shape_rows
from tests.util import surface_keys as _surface_keys, flat_keys as _flat_keys, ratios as _ratios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# coordinate sets (canonical keys, numpy) and their kernel maps
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_keys(ts):
    """Keys of the training batch (4 cubes of 128^3, 78 288 points) at tensor stride ts: 21 870 rows at 2, 5 731 at 4."""
    if ts == 1:
        from tests.golden import make_train_fixture as mk
        return co.canonicalize(mk.batch()[0].astype(np.int64))[0]
    return co.stride_keys(_train_keys(ts // 2), ts)


_SETS = {"surf205k": lambda: _surface_keys(0.515), "surf1M": lambda: _surface_keys(1.17), "flat": _flat_keys,
         "train1": lambda: _train_keys(1), "train2": lambda: _train_keys(2), "train4": lambda: _train_keys(4)}
_TS = {"surf205k": 1, "surf1M": 1, "flat": 1, "train1": 1, "train2": 2, "train4": 4}


@functools.lru_cache(maxsize=None)
def _cset(name):
    return coord_set(_SETS[name](), _TS[name])


def _kmap(src, dst, ks):
    """The library's map from set `src` to set `dst` (step = the input's tensor stride, as MinkowskiConvolution builds it)."""
    return _cset(src).kernel_map(_cset(dst), ks)


@functools.lru_cache(maxsize=None)
def _pairs(src, dst, ks):
    """The oracle's pairs per offset: [(in_rows, out_rows)] (numpy, independent of the library's map)."""
    return codec.kernel_map_pairs(_SETS[src](), _SETS[dst](), ks, _TS[src])


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, reference, metric
# ---------------------------------------------------------------------------------------------------------------------------------
DISTS = ("relu", "spread", "zero_rows")


def _operands(n_in, n_out, cin, cout, dist, seed):
    """(x [n_in, cin], g [n_out, cout]) float32:
    relu      -- non-negative ReLU-like features (about half exact zeros), Gaussian gradients;
    spread    -- rows whose magnitudes spread over e^+-6, gradients at the 1e-7 scale of a mean loss (also spread per row);
    zero_rows -- Gaussian features, gradients with 40 % all-zero rows (outputs the loss does not reach)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    if dist == "relu":
        x = shape_rows(x, dist, rng)
    elif dist == "spread":
        x = shape_rows(x, dist, rng)
        g = g * (1e-7 * np.exp(rng.uniform(-2, 2, (n_out, 1)))).astype(np.float32)
    elif dist == "zero_rows":
        g[rng.random(n_out) < 0.4] = 0.0
    else:
        raise ValueError(dist)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(g, np.float32)


def _ref64(x, g, pairs, K):
    """(ref, S2) [K, cin, cout] float64 on the GPU: ref = sum x[i]^T g[o], S2 = sqrt(sum (x[i] g[o])^2) over the pairs of each
    offset (pairs None: the identity map, K = 1)."""
    x64, g64 = t(x).double(), t(g).double()
    ref = torch.zeros((K, x.shape[1], g.shape[1]), dtype=torch.float64, device=dev())
    s2 = torch.zeros_like(ref)
    for k in range(K):
        if pairs is None:
            xi, go = x64, g64
        else:
            i, o = pairs[k]
            if len(i) == 0:
                continue
            xi, go = x64[torch.from_numpy(i.astype(np.int64)).to(dev())], g64[torch.from_numpy(o.astype(np.int64)).to(dev())]
        ref[k] = xi.T @ go
        s2[k] = (xi * xi).T @ (go * go)
    return ref, s2.sqrt()


# ---------------------------------------------------------------------------------------------------------------------------------
# section 1: pcc_conv_wgrad at the training shapes
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (cin, cout, ks, in set, out set (None: identity), kernel, what it reaches)
CASES = {
    "128x64_k27_self205k": (128, 64, 3, "surf205k", "surf205k", "bf"),       # half column tile, 52 slices of 4 sub-blocks
    "4x128_k125_s2_78k": (4, 128, 5, "train1", "train2", "bf"),              # 4-row M tile (thin_m wave layout)
    "192x256_k27_self5.7k": (192, 256, 3, "train4", "train4", "bf"),         # ragged 64-row second M tile, two N tiles
    "128x128_k125_s2_22k": (128, 128, 5, "train2", "train4", "bf"),
    "128x16000_k1_5.7k": (128, 16000, 1, "train4", None, "bf"),              # 125 column tiles (flattened transposed conv)
    "128x4000_k1_22k": (128, 4000, 1, "train2", None, "bf"),                 # ragged last column tile: 4000 = 31 * 128 + 32
    "128x128_k1_22k": (128, 128, 1, "train2", None, "bf"),                   # GDN gamma: 64 slices, k_wgrad_reduce_wide
    "32x3_k1_78k": (32, 3, 1, "train1", None, "narrow"),                     # scalar loads (cout % 4 != 0)
    "64x1_k27_self205k": (64, 1, 3, "surf205k", "surf205k", "fp32"),         # k_wgrad<false> through the pair-list form
    "32x16_k27_self205k": (32, 16, 3, "surf205k", "surf205k", "narrow"),     # k_wgrad<true> through the pair-list form
}


def _case_seed(name, dist):
    return sum(name.encode()) * 31 + DISTS.index(dist)


def _case_inputs(name, dist):
    cin, cout, ks, src, dst, _ = CASES[name]
    n_in = len(_SETS[src]())
    n_out = len(_SETS[dst]()) if dst is not None else n_in
    return _operands(n_in, n_out, cin, cout, dist, _case_seed(name, dist))


def _case_run(name, dist):
    """dW of the case through `sparse.conv_wgrad` (the entry point autograd uses for the pair-list form)."""
    from unified_point_cloud_compression_amd import sparse as S
    cin, cout, ks, src, dst, _ = CASES[name]
    x, g = _case_inputs(name, dist)
    kmap = _kmap(src, dst, ks) if dst is not None else None
    return S.conv_wgrad(t(x), t(g), ks ** 3, cin, cout, kmap)


def _child_main(out_path):
    """Child process (PCC_WGRAD_BF=0, a load-time switch): the fp32-input MFMA kernel on every case that otherwise runs
    `k_wgrad_bf`, results saved for the parent."""
    assert os.environ.get("PCC_WGRAD_BF") == "0"
    res = {}
    for name, case in CASES.items():
        if case[5] == "bf":
            for dist in DISTS:
                res[f"{name}|{dist}"] = n(_case_run(name, dist))
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def fp32_input_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wgrad_fp32") / "fp32.npz")
    r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_weight_gradients import _child_main; _child_main({out!r})"],
                       cwd=ROOT, env=dict(os.environ, PCC_WGRAD_BF="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return dict(np.load(out))


# One absolute bound on |got - ref| / S2 for every weight-gradient kernel in sections 1-3.  Measured on MI355X over every case,
# operand distribution and kernel of this file (k_wgrad_bf, k_wgrad<false> with and without PCC_WGRAD_BF=0, k_wgrad<true>,
# k_wgrad_thin, k_wgrad_self16): max 5.8e-6, rms 1.8e-6 (both at 64 x 4097 positions, the longest accumulation chains here).
# Bounds: 3.4x / 2.8x above that.
MAX_RATIO = 2e-5
RMS_RATIO = 5e-6


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_matches_float64_at_training_shapes(name, dist, fp32_input_results):
    """Every entry of dW against float64 over the oracle's pairs.  Bounds: max and rms of |got - ref| / S2 below one absolute
    bound for every kernel, and, where the default is the six-term bf16 kernel (`k_wgrad_bf`), an rms within 3x of the
    fp32-input kernel's (`k_wgrad<false>`, run in a child with PCC_WGRAD_BF=0) on the same data.

    Measured on MI355X (max / rms of the ratio, worst distribution): k_wgrad_bf 1.2e-6 - 4.8e-6 / 2.8e-7 - 9.3e-7, the fp32-input
    kernel on the same data up to 5.8e-6 / 7.8e-7; k_wgrad<true> (32 -> 3, 32 -> 16) <= 2.2e-6 / 4.0e-7; k_wgrad<false>
    (64 -> 1) 3.0e-6 / 7.8e-7.  rms(six-term) / rms(fp32-input) is 1.0 - 1.6 (128 -> 64 over 205 k rows the largest): bound 3x.
    (A six-term product without its m*m term adds ~2^-18 S2 per entry, ~4e-6 rms: 5-10x the fp32-input kernel's.)"""
    cin, cout, ks, src, dst, kind = CASES[name]
    K = ks ** 3
    x, g = _case_inputs(name, dist)
    got = _case_run(name, dist)
    assert got.shape == (K, cin, cout)
    ref, s2 = _ref64(x, g, _pairs(src, dst, ks) if dst is not None else None, K)
    mx, rms = _ratios(got, ref, s2)
    line = f"WGRAD {name:22s} {dist:9s} {kind:6s} max {mx:.3e} rms {rms:.3e}"
    if kind == "bf":
        mx32, rms32 = _ratios(fp32_input_results[f"{name}|{dist}"], ref, s2)
        line += f" | fp32-input max {mx32:.3e} rms {rms32:.3e}"
    print(line)
    assert mx <= MAX_RATIO and rms <= RMS_RATIO, line
    if kind == "bf":
        assert mx32 <= MAX_RATIO and rms32 <= RMS_RATIO, line
        assert rms <= 3.0 * rms32, line


def test_float64_reference_on_the_gpu_equals_numpy_float64():
    """The GPU float64 reference (torch fp64 GEMMs) against numpy float64 on the CPU for one layer (192 -> 256, K = 27)."""
    name, dist = "192x256_k27_self5.7k", "spread"
    cin, cout, ks, src, dst, _ = CASES[name]
    x, g = _case_inputs(name, dist)
    pairs = _pairs(src, dst, ks)
    ref, s2 = _ref64(x, g, pairs, 27)
    want = np.zeros((27, cin, cout))
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    for k, (i, o) in enumerate(pairs):
        if len(i):
            want[k] = x64[i].T @ g64[o]
    err = np.abs(n(ref) - want)
    s = n(s2)
    assert np.all(err <= 1e-12 * s + 1e-300), float((err / np.maximum(s, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# section 2: structural edges
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_raw(x, g, K, cin, cout, kmap, dW, ws):
    from unified_point_cloud_compression_amd import lib as L
    L.call("pcc_conv_wgrad", L.ptr(x), x.shape[0], cin, L.ptr(g), g.shape[0], cout, K,
           L.ptr(kmap.hdr) if kmap is not None else None, L.ptr(kmap.nbr) if kmap is not None else None,
           L.ptr(kmap.rows) if kmap is not None else None, L.ptr(dW), L.ptr(ws) if ws is not None else None,
           ws.numel() if ws is not None else 0, L.stream())


def _ws_bytes(fn, *args):
    from unified_point_cloud_compression_amd import lib as L
    return int(getattr(L.load(), fn)(*args))


def _poisoned_and_zero(nbytes):
    ws_nan = torch.full((nbytes // 4 + 1,), float("nan"), dtype=torch.float32, device=dev()).view(torch.uint8)
    ws_zero = torch.zeros(nbytes + 4, dtype=torch.uint8, device=dev())
    return ws_nan, ws_zero


def _bits(a):
    return n(a.contiguous().view(torch.int32))


@pytest.mark.parametrize("cin,cout", [(128, 64), (32, 16), (64, 1), (16, 1)])
def test_empty_offsets_give_exact_zeros(cin, cout):
    """On a set flat in z, the 18 offsets of a 3x3x3 kernel with dz != 0 have no pair: their dW[k] must be exactly 0 (NaN
    pre-fill of the workspace, so a partial that is never written shows); the other nine against float64."""
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd import sparse as S
    keys = _flat_keys()
    x, g = _operands(len(keys), len(keys), cin, cout, "relu", 11)
    kmap = _kmap("flat", "flat", 3)
    ws_nan, _ = _poisoned_and_zero(_ws_bytes("pcc_conv_wgrad_ws_bytes", len(keys), 27, cin, cout))
    dW = torch.full((27, cin, cout), float("nan"), dtype=torch.float32, device=dev())
    _wgrad_raw(t(x), t(g), 27, cin, cout, kmap, dW, ws_nan)
    dz = co.kernel_offsets(3)[:, 2]
    got = n(dW)
    assert np.all(got[dz != 0] == 0.0)
    pairs = _pairs("flat", "flat", 3)
    assert all(len(pairs[k][0]) == 0 for k in np.nonzero(dz != 0)[0]) and all(len(pairs[k][0]) > 0 for k in np.nonzero(dz == 0)[0])
    ref, s2 = _ref64(x, g, pairs, 27)
    mx, rms = _ratios(dW, ref, s2)
    assert mx <= MAX_RATIO and rms <= RMS_RATIO, (mx, rms)
    if L.load().pcc_conv_wgrad_self_supported(27, cin, cout):
        a = S.conv_wgrad_self(t(x), t(g), 27, cin, kmap, cout)
        assert np.all(n(a)[dz != 0] == 0.0)
        assert _ratios(a, ref, s2)[0] <= MAX_RATIO


@pytest.mark.parametrize("cin,cout,K", [(128, 64, 27), (32, 16, 27), (64, 1, 27), (128, 4000, 1), (32, 3, 1)])
def test_empty_inputs_give_zero_gradients(cin, cout, K):
    """n_out = 0 or n_in = 0: dW is all zeros, every entry written (dW pre-filled with NaN)."""
    from unified_point_cloud_compression_amd import lib as L
    for n_in, n_out in ((0, 0), (100, 0), (0, 100)):
        x = torch.ones((max(n_in, 1), cin), dtype=torch.float32, device=dev())[:n_in]
        g = torch.ones((max(n_out, 1), cout), dtype=torch.float32, device=dev())[:n_out]
        dW = torch.full((K, cin, cout), float("nan"), dtype=torch.float32, device=dev())
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
        L.call("pcc_conv_wgrad", L.ptr(x) if n_in else None, n_in, cin, L.ptr(g) if n_out else None, n_out, cout, K, None, None,
               None, L.ptr(dW), L.ptr(ws), ws.numel(), L.stream())
        assert torch.all(dW == 0), (n_in, n_out)
    if L.load().pcc_conv_wgrad_self_supported(K, cin, cout):
        dW = torch.full((K, cin, cout), float("nan"), dtype=torch.float32, device=dev())
        L.call("pcc_conv_wgrad_self", None, 0, cin, None, cout, K, None, None, L.ptr(dW), None, 0, L.stream())
        assert torch.all(dW == 0)


@pytest.mark.parametrize("name", ["128x64_k27_self205k", "4x128_k125_s2_78k", "128x4000_k1_22k", "128x128_k1_22k", "32x3_k1_78k",
                                  "64x1_k27_self205k", "32x16_k27_self205k"])
def test_poisoned_workspace_and_reproducibility_of_conv_wgrad(name):
    """`pcc_conv_wgrad` with a workspace full of NaN must give the same bits as with a zeroed one (every partial slab element
    the reduction reads is written first), and two calls the same bits."""
    cin, cout, ks, src, dst, _ = CASES[name]
    K = ks ** 3
    x, g = _case_inputs(name, "relu")
    x, g = t(x), t(g)
    kmap = _kmap(src, dst, ks) if dst is not None else None
    ws_nan, ws_zero = _poisoned_and_zero(_ws_bytes("pcc_conv_wgrad_ws_bytes", g.shape[0], K, cin, cout))
    outs = []
    for ws in (ws_zero, ws_nan, ws_nan):
        dW = torch.full((K, cin, cout), float("nan"), dtype=torch.float32, device=dev())
        _wgrad_raw(x, g, K, cin, cout, kmap, dW, ws)
        outs.append(_bits(dW))
    assert np.isfinite(outs[0].view(np.float32)).all()
    assert np.array_equal(outs[0], outs[1]), "poisoned workspace changed the result"
    assert np.array_equal(outs[1], outs[2]), "two calls differ"


def test_poisoned_workspace_of_channelwise_wgrad():
    """`pcc_chconv_wgrad` (partial slabs + a fixed-order reduce) with a NaN workspace: bit-identical to a zeroed one."""
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd import sparse as S
    cs = _cset("train1")
    taps = S.channelwise_full_taps(3)
    x, g = _operands(cs.n, cs.n, 3, 3, "relu", 5)
    x, g = t(x), t(g)
    for wc in (3, 1):
        ws_nan, ws_zero = _poisoned_and_zero(_ws_bytes("pcc_chconv_wgrad_ws_bytes", cs.n, taps.ntaps, 3))
        outs = []
        for ws in (ws_zero, ws_nan, ws_nan):
            dW = torch.full((taps.ntaps, wc), float("nan"), dtype=torch.float32, device=dev())
            L.call("pcc_chconv_wgrad", *S._chconv_common(cs, x, taps), L.ptr(cs.keys), cs.n, L.ptr(g), L.ptr(dW), wc, L.ptr(ws),
                   ws.numel(), L.stream())
            outs.append(_bits(dW))
        assert np.isfinite(outs[0].view(np.float32)).all()
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2]), wc


SLICE_ROWS = [64 * 1024 - 1, 64 * 1024, 64 * 1024 + 1, 64 * 4096 + 33, 64 * (1024 + 31)]


@pytest.mark.parametrize("rows", SLICE_ROWS)
def test_identity_gradient_slice_geometry(rows):
    """K = 1 identity, 128 -> 128 (64 slices, `k_wgrad_bf` + `k_wgrad_reduce_wide`): per-slice position counts just below, at
    and above multiples of WG_SUB (1024, the compaction block) and of WG_PAIRS (32, one step) -- the carried `pending`
    remainder and the tail step of each slice.  Against float64 with the shared bounds, and a poisoned workspace."""
    x, g = _operands(rows, rows, 128, 128, "zero_rows", rows)
    ref, s2 = _ref64(x, g, None, 1)
    nbytes = _ws_bytes("pcc_conv_wgrad_ws_bytes", rows, 1, 128, 128)
    assert nbytes - 256 == 64 * 128 * 128 * 4                    # 64 slices
    ws_nan, ws_zero = _poisoned_and_zero(nbytes)
    outs = []
    for ws in (ws_zero, ws_nan):
        dW = torch.full((1, 128, 128), float("nan"), dtype=torch.float32, device=dev())
        _wgrad_raw(t(x), t(g), 1, 128, 128, None, dW, ws)
        outs.append(dW)
    mx, rms = _ratios(outs[0], ref, s2)
    print(f"WGRAD slices rows={rows} max {mx:.3e} rms {rms:.3e}")
    assert mx <= MAX_RATIO and rms <= RMS_RATIO, (mx, rms)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# section 3: input-stationary forms at full size
# ---------------------------------------------------------------------------------------------------------------------------------
SELF_CASES = {   # (cin, cout, set): kernel
    "16x1_1M": (16, 1, "surf1M"),          # k_wgrad_thin<4>
    "32x1_1M": (32, 1, "surf1M"),          # k_wgrad_thin<8>
    "16x16_1M": (16, 16, "surf1M"),        # k_wgrad_self16<16>
    "32x16_1M": (32, 16, "surf1M"),        # k_wgrad_self16<32>
    "64x1_205k": (64, 1, "surf205k"),      # k_wgrad_thin<16>
}


@pytest.mark.parametrize("name", list(SELF_CASES))
def test_input_stationary_weight_gradient_at_full_size(name):
    """`pcc_conv_wgrad_self` at the training step's row counts: 1 024 workgroups (the cap), per-block rows rounded up to 256
    (thin) / 64 (self16) so that the trailing blocks are EMPTY and must still write zero partials.  Against float64 (same
    metric and bounds as the pair-list kernels), bit-identical with a NaN-poisoned workspace, reproducible, and in agreement
    with the pair-list form on the same map.  Measured on MI355X: max 5.9e-7 - 1.5e-6, rms 1.5e-7 - 3.4e-7 (the pair-list
    form on the same data: <= 3.2e-6 / 5.8e-7; |self - pair-list| / S2 <= 2.9e-6)."""
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd import sparse as S
    cin, cout, src = SELF_CASES[name]
    rows = len(_SETS[src]())
    x, g = _operands(rows, rows, cin, cout, "relu", cin * 100 + cout)
    xt, gt = t(x), t(g)
    kmap = _kmap(src, src, 3)
    assert L.load().pcc_conv_wgrad_self_supported(27, cin, cout)
    nbytes = _ws_bytes("pcc_conv_wgrad_self_ws_bytes", rows, 27, cin, cout)
    blocks = (nbytes - 256) // (27 * cin * cout * 4)
    if src == "surf1M":
        per = -(-rows // 1024)
        per = -(-per // (256 if cout == 1 else 64)) * (256 if cout == 1 else 64)
        assert blocks == 1024 and per * 1023 >= rows, (blocks, per, rows)      # empty trailing blocks
    ws_nan, ws_zero = _poisoned_and_zero(nbytes)
    outs = []
    for ws in (ws_zero, ws_nan, ws_nan):
        dW = torch.full((27, cin, cout), float("nan"), dtype=torch.float32, device=dev())
        L.call("pcc_conv_wgrad_self", L.ptr(xt), rows, cin, L.ptr(gt), cout, 27, L.ptr(kmap.hdr), L.ptr(kmap.nbr), L.ptr(dW),
               L.ptr(ws), ws.numel(), L.stream())
        outs.append(dW)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "poisoned workspace changed the result"
    assert np.array_equal(_bits(outs[1]), _bits(outs[2])), "two calls differ"
    ref, s2 = _ref64(x, g, _pairs(src, src, 3), 27)
    mx, rms = _ratios(outs[0], ref, s2)
    pl = S.conv_wgrad(xt, gt, 27, cin, cout, kmap)
    mx_pl, rms_pl = _ratios(pl, ref, s2)
    agree = float(((outs[0].double() - pl.double()).abs() / s2.clamp_min(1e-300)).max())
    print(f"WGRAD self {name:10s} rows={rows} max {mx:.3e} rms {rms:.3e} | pair-list max {mx_pl:.3e} rms {rms_pl:.3e} | "
          f"|self - pair-list| / S2 max {agree:.3e}")
    assert mx <= MAX_RATIO and rms <= RMS_RATIO, (mx, rms)
    assert mx_pl <= MAX_RATIO and rms_pl <= RMS_RATIO, (mx_pl, rms_pl)
    assert agree <= 2 * MAX_RATIO


# ---------------------------------------------------------------------------------------------------------------------------------
# section 5: weight packing of the data gradient, scatter of the transposed conv's gradient rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _step_conv_shapes():
    """(K, cin, cout) of every non-transposed convolution of the R2-width training model (a set, sorted)."""
    import copy
    from unified_point_cloud_compression_amd.model import UnifiedModel
    from tests.golden import make_train_fixture as mk
    torch.manual_seed(0)
    model = UnifiedModel(copy.deepcopy(mk.train_config()))
    shapes = set()
    for m in model.modules():
        if hasattr(m, "kernel_volume") and hasattr(m, "TRANSPOSED") and not m.TRANSPOSED:
            shapes.add((m.kernel_volume, m.in_channels, m.out_channels))
    return sorted(shapes)


def test_transposed_and_reversed_weight_pack_equals_packing_the_explicit_tensor():
    """`pcc_conv_pack_weights_ex(transpose, flip)` -- the data gradient's kernel W'[k] = W[K-1-k]^T packed straight from the
    parameter -- bit-identical to `pcc_conv_pack_weights` of the explicitly flipped and transposed tensor, for every
    (K, cin, cout) of the training step and every (transpose, flip) the pack accepts for it."""
    from unified_point_cloud_compression_amd import lib as L
    lib = L.load()
    shapes = _step_conv_shapes()
    assert len(shapes) >= 8, shapes
    checked = 0
    rng = np.random.default_rng(9)
    for K, a, b in shapes:
        src = t(rng.standard_normal((K, a, b)).astype(np.float32) * np.exp(rng.uniform(-4, 4, (K, a, b))).astype(np.float32))
        for transpose in (0, 1):
            for flip in ((0, 1) if K > 1 else (0,)):
                cin, cout = (b, a) if transpose else (a, b)
                plain = not transpose and not flip
                if not plain and not (cin % 32 == 0 and cout > 16):      # (what autograd._conv_view hands to the _ex pack)
                    continue
                ne = lib.pcc_conv_packed_elems(K, cin, cout)
                if ne <= 0:
                    continue
                w = torch.flip(src, dims=[0]) if flip else src
                w = (w.permute(0, 2, 1) if transpose else w).contiguous()
                want = torch.zeros(ne, dtype=torch.float32, device=dev())
                got = torch.zeros(ne, dtype=torch.float32, device=dev())
                L.call("pcc_conv_pack_weights", L.ptr(w), K, cin, cout, L.ptr(want), ne, L.stream())
                L.call("pcc_conv_pack_weights_ex", L.ptr(src), K, cin, cout, transpose, flip, L.ptr(got), ne, L.stream())
                assert np.array_equal(_bits(got), _bits(want)), (K, a, b, transpose, flip)
                checked += 1
    assert checked >= len(shapes) + 4, checked


@pytest.mark.parametrize("cout", [32, 3])
def test_transposed_conv_gradient_scatter_is_exact(cout):
    """`pcc_convt_scatter_rows` (dT[pair] = g[output row of the pair]) at ~1 M pairs: float4 rows (cout = 32) and scalar rows
    (cout = 3); pair ids a random permutation, 0-3 pairs per output row; every pair written once (NaN pre-fill), bit-exact."""
    from unified_point_cloud_compression_amd import lib as L
    rng = np.random.default_rng(cout)
    n_out = 700_001
    cnt = rng.integers(0, 4, n_out)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    n_pairs = int(first[-1])
    assert n_pairs > 1_000_000
    pair_ids = rng.permutation(n_pairs).astype(np.int32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    want = np.empty((n_pairs, cout), np.float32)
    want[pair_ids] = g[np.repeat(np.arange(n_out), cnt)]
    g_d, first_d, ids_d = t(g), t(first), t(pair_ids)        # (named: a temporary's memory could be reused before the launch)
    dT = torch.full((n_pairs, cout), float("nan"), dtype=torch.float32, device=dev())
    L.call("pcc_convt_scatter_rows", L.ptr(g_d), L.ptr(first_d), L.ptr(ids_d), n_out, cout, L.ptr(dT), L.stream())
    got = n(dT)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), (int(bad.sum()), int(np.isnan(got).sum()), np.argwhere(bad)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# section 4: every convolution of one real training step, every entry
# ---------------------------------------------------------------------------------------------------------------------------------
def _record_r2_step(force=None):
    """One forward + backward of the R2-width training step of `test_gpu_train_step.py::
    test_train_step_at_r2_width_matches_the_oracle_fixture` (its batch, config, noise and seed), with
    `autograd.SparseConvFn.backward` wrapped to record, per call: features, kernel, incoming g, saved output, the map (dense
    table, CSR pair lists or identity), the returned g_feats / g_kernel, the dispatch class and the arithmetic form the call
    saw.  force: `lib.ARITH_FORCE` for the step (None: the default form)."""
    import copy
    import threading
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import autograd as A, lib as L, sparse as S
    from unified_point_cloud_compression_amd.model import UnifiedModel
    from unified_point_cloud_compression_amd.loss import Loss
    from tests.golden import make_train_fixture as mk
    recs = []
    orig = A.SparseConvFn.backward
    main_thread = threading.get_ident()

    def wrapped(ctx, g):
        feats, kernel, out = ctx.saved_tensors
        module, in_set, out_set, kmap, act, slope, _ = ctx.meta
        K, cin, cout = module.kernel_volume, module.in_channels, module.out_channels
        res = orig(ctx, g)
        if isinstance(kmap, tuple):
            m = ("csr", kmap[0][:out_set.n + 1].clone(), kmap[1].clone())
        elif kmap is None:
            m = ("identity",)
        else:
            m = ("dense", kmap.dense())
        if module.TRANSPOSED:
            cls = "flattened transposed"
        elif (A.WGRAD_SELF and in_set is out_set and kmap is not None and kmap.rows is None and module.stride == 1
              and g.shape[0] == feats.shape[0] and L.load().pcc_conv_wgrad_self_supported(K, cin, cout)):
            cls = "self thin" if cout == 1 else "self16"
        elif cin <= 32 and cout <= 32:
            cls = "narrow"
        elif (cin | cout) % 4 == 0:
            cls = "wide bf16"
        else:
            cls = "fp32-input"
        pair_dgrad = False
        if not module.TRANSPOSED and K > 1 and res[0] is not None and cout % 32 == 0 and cin > 16 and S.wants_pairs(K, cout, cin):
            pair_dgrad = out_set.kernel_map(in_set, module.kernel_size, step=in_set.ts).pair_plan() is not None
        recs.append(dict(
            K=K, cin=cin, cout=cout, transposed=module.TRANSPOSED, act=act, slope=slope, n_in=feats.shape[0], n_out=g.shape[0],
            feats=feats.detach().clone(), kernel=kernel.detach().reshape(K, cin, cout).clone(), g=g.detach().clone(),
            out=out.detach().clone() if out is not None else None, map=m, cls=cls, pair_dgrad=pair_dgrad,
            g_feats=res[0].detach().clone() if res[0] is not None else None,
            g_kernel=res[1].detach().reshape(K, cin, cout).clone() if res[1] is not None else None,
            arith=L.arith(), on_main_thread=threading.get_ident() == main_thread,
            scope_seen=getattr(L._tls, "scope", None)))
        return res

    fx_cfg = mk.train_config()
    C, rgb = mk.batch()
    nb = int(C[:, 0].max()) + 1
    ny, nz = mk.noise(fx_cfg, C)
    prev_force = L.ARITH_FORCE
    A.SparseConvFn.backward = staticmethod(wrapped)
    L.ARITH_FORCE = force
    try:
        torch.manual_seed(0)
        model = UnifiedModel(copy.deepcopy(fx_cfg)).to(dev()).train()
        model.entropy_model.noise_fn = lambda tag, like: t(ny if tag.startswith("y") else nz)
        x = ME.SparseTensor(coordinates=t(C), features=t(rgb))
        q = torch.tensor([[0.4, 0.7]] * nb, device=dev())
        Lam = torch.tensor([[5.0, 400.0]] * nb, device=dev())
        out = model(x, q, Lam)
        total, _ = Loss(copy.deepcopy(mk.LOSS_CFG))(x, out)
        with L.arith_scope(L.arith()):            # a scope on the calling thread (the form it names is the run's own)
            total.backward()
        torch.cuda.synchronize()
    finally:
        A.SparseConvFn.backward = orig
        L.ARITH_FORCE = prev_force
    return recs


def _rec_pairs(r):
    """(i, o, k) int64 index tensors of every pair of a recorded call."""
    m = r["map"]
    d = dev()
    if m[0] == "identity":
        a = torch.arange(r["n_in"], device=d)
        return a, a, torch.zeros_like(a)
    if m[0] == "dense":
        nbr = m[1].long()
        k, o = torch.nonzero(nbr >= 0, as_tuple=True)
        return nbr[k, o], o, k
    first, pair_ids = m[1].long(), m[2].long()
    total = int(first[-1])
    o = torch.repeat_interleave(torch.arange(r["n_out"], device=d), first[1:] - first[:-1])
    p = pair_ids[:total]
    return p // r["K"], o, p % r["K"]


def _rec_reference(r):
    """float64 (dW, S2_w, g_feats, S2_f) of a recorded call: the activation derivative from the saved output, then
    dW[k] = sum x[i]^T g[o] and g_feats[i] = sum g[o] W[k]^T over the pairs of offset k."""
    g = r["g"].double()
    if r["act"] == 1:
        g = g * (r["out"] > 0)
    elif r["act"] == 2:
        g = torch.where(r["out"] > 0, g, g * r["slope"])
    x, W = r["feats"].double(), r["kernel"].double()
    i, o, k = _rec_pairs(r)
    order = torch.argsort(k, stable=True)
    i, o, k = i[order], o[order], k[order]
    counts = torch.bincount(k, minlength=r["K"]).tolist()
    K, cin, cout = r["K"], r["cin"], r["cout"]
    dW = torch.zeros((K, cin, cout), dtype=torch.float64, device=dev())
    sw = torch.zeros_like(dW)
    gf = torch.zeros((r["n_in"], cin), dtype=torch.float64, device=dev())
    sf = torch.zeros_like(gf)
    at = 0
    for kk, c in enumerate(counts):
        if c:
            ii, oo = i[at:at + c], o[at:at + c]
            xi, go = x[ii], g[oo]
            dW[kk] = xi.T @ go
            sw[kk] = (xi * xi).T @ (go * go)
            gf.index_add_(0, ii, go @ W[kk].T)
            sf.index_add_(0, ii, (go * go) @ (W[kk] * W[kk]).T)
        at += c
    return dW, sw.sqrt(), gf, sf.sqrt()


def _step_ratios(recs):
    rows = []
    for j, r in enumerate(recs):
        dW, sw, gf, sf = _rec_reference(r)
        w = _ratios(r["g_kernel"], dW, sw) if r["g_kernel"] is not None else (0.0, 0.0)
        f = _ratios(r["g_feats"], gf, sf) if r["g_feats"] is not None else None
        rows.append((j, r, w, f))
    return rows


# Weight gradients of the step, |got - ref| / S2: the step's sums are largely COHERENT (ReLU features, gradients of one sign
# over long runs of rows), where fp32 accumulation errs by a multiple of 2^-24 sum |x g| -- up to ~sqrt(pairs) times S2.
# Measured on MI355X: max 2.3e-4, rms 5.0e-5 (the 992 k-row heads, self16 / self thin); 7e-7 - 7e-6 on the layers below 6 k
# rows.  Bounds 4.4x / 4x above.  (A wrong offset slot, tile edge or slice boundary errs by the entry itself: ratio >= 1.)
STEP_W_MAX = 1e-3
STEP_W_RMS = 2e-4
# Data gradients run the forward kernels (scaled fp16 pairs by default) on the inverse map: bounds of their own, against a run
# of the same step with every product forced to fp32-input MFMAs.
# Measured on MI355X (|got - ref| / S2 over the 19 data gradients of the step): default max 7.1e-6, rms at most 1.23x the
# fp32 run's; fp32 run max 2.7e-5 (its flattened transposed layers).  Bounds: 3.5x, 2.4x and 3.7x above.
DATA_MAX_RATIO = 2.5e-5
DATA_RMS_FACTOR = 3.0
DATA_F32_MAX_RATIO = 1e-4


def test_every_convolution_gradient_of_a_training_step_against_float64():
    """Every entry of every weight gradient and every data gradient that `SparseConvFn.backward` returns during one R2-width
    training step (21 calls), against float64 over the recorded maps (dense table, CSR pair lists or identity), with the
    activation derivative taken from the saved output.  Weight gradients: STEP_W_*.  Data gradients: the default run (scaled
    fp16-pair products, whose range guard nothing reads during training) against a run with `lib.ARITH_FORCE = ARITH_F32`.
    `arith_scope` is thread-local, and autograd runs the backward of GPU tensors on a device thread of its own: measured on
    MI355X, every recorded call ran off the main thread and saw no scope, although `.backward()` was called inside one -- so
    the fp32 run needs ARITH_FORCE.  No data gradient of the default run exceeded the fp32 run's error by more than 1.23x
    (rms), so the unguarded fp16-pair form loses nothing measurable here.  The recorded calls must include every dispatch
    class, so that a change of dispatch cannot quietly shrink what is covered."""
    from unified_point_cloud_compression_amd import lib as L
    recs = _record_r2_step()
    print(f"backward on main thread: {sorted({r['on_main_thread'] for r in recs})}; scope seen there: "
          f"{sorted({str(r['scope_seen']) for r in recs})}; forms: {sorted({r['arith'] for r in recs})}")
    classes = {r["cls"] for r in recs} | ({"pair-list data gradient"} if any(r["pair_dgrad"] for r in recs) else set())
    rows = _step_ratios(recs)
    del recs
    recs32 = _record_r2_step(force=L.ARITH_F32)
    assert all(r["arith"] == L.ARITH_F32 for r in recs32)
    rows32 = _step_ratios(recs32)
    del recs32
    assert len(rows32) == len(rows)
    print(f"{'#':>3} {'class':22s} {'K':>4} {'cin':>4} {'cout':>6} {'rows in':>8} {'rows out':>8}  dW max / rms       "
          f"dX max / rms (default)   dX max / rms (fp32)")
    bad = []
    for (j, r, w, f), (_, r32, w32, f32) in zip(rows, rows32):
        assert (r["K"], r["cin"], r["cout"]) == (r32["K"], r32["cin"], r32["cout"])
        fs = f"{f[0]:.2e} / {f[1]:.2e}" if f is not None else "-"
        fs32 = f"{f32[0]:.2e} / {f32[1]:.2e}" if f32 is not None else "-"
        print(f"{j:3d} {r['cls']:22s} {r['K']:4d} {r['cin']:4d} {r['cout']:6d} {r['n_in']:8d} {r['n_out']:8d}  "
              f"{w[0]:.2e} / {w[1]:.2e}   {fs:22s}   {fs32}")
        if not (w[0] <= STEP_W_MAX and w[1] <= STEP_W_RMS and w32[0] <= STEP_W_MAX and w32[1] <= STEP_W_RMS):
            bad.append(("dW", j, r["cls"], r["K"], r["cin"], r["cout"], w, w32))
        if f is not None and not (f[0] <= DATA_MAX_RATIO and f[1] <= DATA_RMS_FACTOR * f32[1] + 1e-9 and f32[0] <= DATA_F32_MAX_RATIO):
            bad.append(("dX", j, r["cls"], r["K"], r["cin"], r["cout"], f, f32))
    assert not bad, bad
    want = {"wide bf16", "narrow", "self thin", "self16", "flattened transposed", "pair-list data gradient"}
    assert want <= classes, sorted(classes)
