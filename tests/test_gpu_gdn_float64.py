"""GDN / IGDN forward (`pcc_gdn_fwd`) and backward (`GdnFn`) against float64 in every regime of the GDN dispatch: the fp32-input
kernel (c = 8, 16, and every c under `PCC_ARITH_F32`), the 32-, 64- and 128-row tiles of `k_conv_mfma_bf` in GDN mode on 128-,
64- and 32-column tiles with one, two and half-empty column blocks, `k_gdn_bf<1>` / `k_gdn_bf<2>` from 32 768 rows, and the
general kernel as the fallback for an `x` that is not 16-byte aligned.

The regime a call reached is READ from the library (`pcc_gdn_last_launch`), never computed from a copy of the dispatch rules;
the last test of the file checks that the regimes listed in EXPECT were all reached.

Forward reference and metric.  From the RAW parameters in float64: eff = max(raw, sqrt(minimum + 2^-36))^2 - 2^-36 (minimum =
beta_min for beta, 0 for gamma), n64 = beta_eff + |x| gamma_eff^T, y64 = x / n64 (GDN) or x * n64 (IGDN), through torch on the
GPU; one test checks it against numpy float64 on the CPU.  Every term of the norm is non-negative (no cancellation), so the
metric is the plain relative error |got - y64| / |y64|, max and rms over the entries with x != 0; an entry with x == 0 must come
back as exactly +-0; a non-finite output counts as infinite error.

Forward bounds.  The claim is fp32 accuracy, so the yardstick is a plain fp32 evaluation of the same formula outside the library
(numpy float32 on the CPU: np.abs(x) @ gamma_eff32.T + beta_eff32, then the divide or multiply), fed the same data and measured
with the same metric.  For every case and form: rms(kernel) <= 3 rms(plain fp32) (the rule of test_gpu_conv_forward_regimes.py:
equally accurate kernels measured 0.36 - 1.34 of each other there, a product without its m * m term 3.9 - 5.5), max(kernel) <=
4 max(plain fp32) (a little more room for an extreme value), and, independent of any measurement, max(kernel) <= (c + 8) 2^-24:
the worst case of c fp32 additions of non-negative terms plus the dropped m*l, l*m, l*l terms of the split plus the divide.

Measured on MI355X (profiles/gdn_float64.txt): see the docstring of `test_gdn_forward_matches_float64_in_its_regime`.

Backward reference and metric.  torch float64 autograd on the GPU over the GDN1 formula from the raw parameters through the two
LowerBound-and-square reparametrisations, same x and same upstream g.  Per output entry |got - ref| / S2, S2 the root of the
sum of the squared terms of that entry (the metric of test_gpu_weight_gradients.py); yardstick: fp32 torch autograd of the same
formula on the CPU, same metric, same 3x / 4x factors per output tensor.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import dev, t, n, bits as _bits, ratios, shape_rows

pytestmark = pytest.mark.gpu

PED = 2.0 ** -36                 # CompressAI's pedestal (reparam_offset^2)
BETA_MIN = 1e-6
K_NONE, K_F32, K_BF, K_FUSED = 0, 1, 2, 3            # include/pcc_hip.h PCC_GDN_KERNEL_*
KERNEL_NAMES = ("none", "k_conv_mfma", "k_conv_mfma_bf", "k_gdn_bf")
DISTS = ("gauss", "spread", "sparse")
CHILD_MAX_ROWS = 33000           # the child run with PCC_MFMA_BUF=0 takes the cases up to this many rows

# c -> row counts: they straddle every threshold of the dispatch at the commit that added this file
ROWS = {
    128: (1, 33, 777, 32704, 32705, 32767, 32768, 32769, 65409, 130944, 130945),
    192: (16320, 16321, 32641, 32768, 65408, 65409),
    256: (16321, 65409),
    160: (777, 33000),
    96: (777, 32641),
    64: (777, 65408, 65409),
    32: (1, 127, 128, 129, 40000),
    16: (1, 129, 40000),
    8: (1, 129, 40000),
}
CASES = {f"c{c}_r{r}": (c, r) for c, rows in ROWS.items() for r in rows}

# (kernel, row tile, column tile) the dispatch at the commit that added this file gives, under BF6 and (where listed) under F32.
# NOT asserted per case from here: the last test of the file checks that every regime listed is reached by some case, and names
# the cases meant to.  c = 160, 96, 16 and 8 are not listed: their record is printed (and c = 16, 8 must show the fp32-input kernel).
EXPECT = {
    "bf6": {
        "c128_r1": (K_BF, 32, 128), "c128_r33": (K_BF, 32, 128), "c128_r777": (K_BF, 32, 128), "c128_r32704": (K_BF, 32, 128),
        "c128_r32705": (K_BF, 64, 128), "c128_r32767": (K_BF, 64, 128),
        "c128_r32768": (K_FUSED, 64, 128), "c128_r32769": (K_FUSED, 64, 128), "c128_r130944": (K_FUSED, 64, 128),
        "c128_r130945": (K_FUSED, 128, 128),                 # 1 024 tiles, the last with one row
        "c192_r16320": (K_BF, 32, 128), "c192_r16321": (K_BF, 64, 128), "c192_r32641": (K_BF, 128, 128),
        "c192_r32768": (K_FUSED, 64, 128), "c192_r65408": (K_FUSED, 64, 128), "c192_r65409": (K_FUSED, 128, 128),
        "c256_r16321": (K_BF, 64, 128), "c256_r65409": (K_FUSED, 128, 128),
        "c64_r777": (K_BF, 64, 64), "c64_r65408": (K_BF, 64, 64), "c64_r65409": (K_BF, 128, 64),
        "c32_r1": (K_BF, 128, 32), "c32_r127": (K_BF, 128, 32), "c32_r128": (K_BF, 128, 32), "c32_r129": (K_BF, 128, 32),
        "c32_r40000": (K_BF, 128, 32),
        "unaligned_c128_r65409": (K_BF, 128, 128),           # reached only through the alignment fallback
    },
    "f32": {"c128_r65409": (K_F32, 128, 128), "c128_r32704": (K_F32, 32, 128)},
}

_seen = {"bf6": {}, "f32": {}}   # form tag -> case -> {(kernel, BM, BN)} recorded by the tests of this file


# ---------------------------------------------------------------------------------------------------------------------------------
# parameters, inputs, references
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_params(c):
    """(beta_raw [c], gamma_raw [c, c]) float32: gamma entries below the bound (some negative), four beta entries below it."""
    rng = np.random.default_rng(1000 + c)
    gamma = (np.sqrt(0.1 * np.eye(c) + PED) + rng.uniform(-0.01, 0.05, (c, c))).astype(np.float32)
    beta = (np.sqrt(1 + PED) + rng.uniform(0, 0.3, c)).astype(np.float32)
    low = rng.choice(c, 4, replace=False)
    beta[low[:2]] = 0.0
    beta[low[2:]] = -0.25
    assert (gamma < 2.0 ** -18).any() and (gamma < 0).any()
    return beta, gamma


def _low_beta(c):
    beta, _ = _raw_params(c)
    return np.nonzero(beta < np.sqrt(BETA_MIN + PED))[0]


def _eff64(raw, minimum):
    return np.maximum(raw.astype(np.float64), np.sqrt(minimum + PED)) ** 2 - PED


def _eff32(raw, minimum):
    r = np.maximum(raw, np.float32(np.sqrt(minimum + PED)))
    return r * r - np.float32(PED)


def _rows(c, rows, dist, seed=0):
    """x [rows, c] float32.  gauss: signed standard normal x 3; spread: rows over e^+-6; sparse: Gaussian with half the entries
    exactly zero (a fifth of those -0.0) and 5 % of the rows all zero."""
    rng = np.random.default_rng([c, rows, DISTS.index(dist), seed])
    x = rng.standard_normal((rows, c), dtype=np.float32)
    if dist == "gauss":
        return x * np.float32(3)
    if dist == "spread":
        return shape_rows(x, "spread", rng)
    if dist == "sparse":
        u = rng.random((rows, c), dtype=np.float32)
        x[u < 0.4] = 0.0
        x[(u >= 0.4) & (u < 0.5)] = -0.0
        x[rng.random(rows) < 0.05] = 0.0
        return x
    raise ValueError(dist)


@functools.lru_cache(maxsize=None)
def _packed(c):
    """(packed, beta_eff) of `pcc_gdn_pack` for the raw parameters of c, on the GPU."""
    from unified_point_cloud_compression_amd import lib as L
    beta, gamma = _raw_params(c)
    cap = int(L.load().pcc_gdn_packed_elems(c))
    assert cap > 0
    packed = torch.empty(cap, dtype=torch.float32, device=dev())
    beta_eff = torch.empty(c, dtype=torch.float32, device=dev())
    bt, gt = t(beta), t(gamma)                  # (named: a temporary would be freed, and its block reused, before the call)
    L.call("pcc_gdn_pack", L.ptr(bt), L.ptr(gt), c, BETA_MIN, L.ptr(packed), cap, L.ptr(beta_eff), L.stream())
    torch.cuda.synchronize()
    return packed, beta_eff


def _last_launch():
    from unified_point_cloud_compression_amd import lib as L
    rec = (ctypes.c_int32 * 4)()
    L.call("pcc_gdn_last_launch", rec)
    return tuple(rec)


def _fwd(xt, c, inverse, form, out=None, rows=None):
    """One raw `pcc_gdn_fwd` over the first `rows` rows of xt (all of them by default) under arithmetic form `form`:
    (out, (kernel, row tile, column tile, inverse) as the library recorded it)."""
    from unified_point_cloud_compression_amd import lib as L
    packed, beta_eff = _packed(c)
    rows = xt.shape[0] if rows is None else rows
    if out is None:
        out = torch.empty((rows, c), dtype=torch.float32, device=dev())
    with L.arith_scope(form):
        L.call("pcc_gdn_fwd", L.ptr(xt), rows, c, L.ptr(packed), L.ptr(beta_eff), 1 if inverse else 0, L.ptr(out), L.arith(),
               L.stream())
    rec = _last_launch()
    assert rows == 0 or rec[3] == (1 if inverse else 0), rec
    return out, rec


def _ref64(xt, c, inverse):
    """y64 [rows, c] float64 on the GPU, from the raw parameters."""
    beta, gamma = _raw_params(c)
    x64 = xt.double()
    n64 = x64.abs() @ t(_eff64(gamma, 0.0)).t() + t(_eff64(beta, BETA_MIN))
    return x64 * n64 if inverse else x64 / n64


def _rel(got, y64, nz):
    """(max, rms) of |got - y64| / |y64| over the entries nz; a non-finite output counts as infinite."""
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    if not bool(nz.any()):
        return 0.0, 0.0
    r = ((got.double() - y64).abs() / y64.abs())[nz]
    return float(r.max()), float(torch.sqrt((r * r).mean()))


_plain = {}          # (c, rows, dist, inverse) -> (max, rms) of the plain fp32 evaluation


def _plain_fp32(c, rows, dist, inverse, x, y64, nz):
    key = (c, rows, dist, inverse)
    if key not in _plain:
        beta, gamma = _raw_params(c)
        n32 = np.abs(x) @ _eff32(gamma, 0.0).T + _eff32(beta, BETA_MIN)
        assert n32.dtype == np.float32
        _plain[key] = _rel(t(x * n32 if inverse else x / n32), y64, nz)
    return _plain[key]


def _forms(c):
    from unified_point_cloud_compression_amd import lib as L
    forms = [("bf6", L.ARITH_BF6), ("f32", L.ARITH_F32)]
    if c in (128, 192):
        forms.append(("h3", L.ARITH_H3))
    return forms


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
_FWD_PARAMS = [(name, dist) for name in CASES for dist in DISTS]


def _fwd_id(name, dist):
    return f"{name}-{dist}"


@pytest.mark.parametrize("name,dist", _FWD_PARAMS, ids=[_fwd_id(*p) for p in _FWD_PARAMS])
def test_gdn_forward_matches_float64_in_its_regime(name, dist):
    """Every entry of GDN and IGDN against float64 under BF6 and F32 (c = 128, 192: also the default H3, which must give the bits
    of BF6): rms(kernel) <= 3 rms(plain fp32), max(kernel) <= 4 max(plain fp32), max(kernel) <= (c + 8) 2^-24, entries with
    x == 0 exactly +-0.  Under F32, and for c = 8, 16 under every form, the record must show the fp32-input kernel.

    Measured on MI355X (profiles/gdn_float64.txt; 37 cases x 3 row distributions x GDN / IGDN).  rms(kernel) / rms(plain fp32):
    0.72 - 1.98 under BF6, 0.72 - 2.37 under F32 (both largest at c = 128 with ONE spread row: 128 entries); max / max: 0.60 -
    3.32 under BF6 (the same one-row case), 0.60 - 3.07 under F32 (c = 32, one row).  max(kernel) against (c + 8) 2^-24: at
    most 0.36 (c = 8, 40 000 spread rows).  Largest figures: max 1.14e-6 (BF6, c = 256, 65 409 rows) and 1.50e-6 (F32, c =
    192, 32 768 spread rows); the fp32-input kernel often gives the very max of the plain evaluation.  No intact build
    exceeded a factor.
    Sensitivity, measured once with a library built without the m * m MFMA of `k_gdn_bf` and of `bf6_terms` (pcc_mfma.h), c =
    128, GDN, gauss / spread / sparse rows.  32 768 rows (`k_gdn_bf<1>`): rms 4.90e-7 / 7.35e-7 / 3.28e-7 against 6.59e-8 /
    9.22e-8 / 4.73e-8 of plain fp32 (7.4x / 8.0x / 6.9x; intact 0.90x / 0.88x / 1.02x), max 6.2e-6 / 1.13e-5 / 6.9e-6 against
    9.1e-7 / 1.00e-6 / 6.6e-7 (6.8x - 11x).  130 945 rows (`k_gdn_bf<2>`): rms 4.91e-7 / 7.42e-7 / 3.29e-7 against 6.59e-8 /
    9.28e-8 / 4.74e-8 (7.4x / 8.0x / 6.9x; intact 0.90x / 0.88x / 1.02x), max 6.7e-6 / 1.18e-5 / 7.0e-6.  The 3x rule and the
    4x rule fail on all six (and on the general kernel at 777 rows: 7.4x / 7.9x / 7.1x); the measurement-free bound (c + 8)
    2^-24 = 8.1e-6 alone would notice only the spread rows."""
    c, rows = CASES[name]
    x = _rows(c, rows, dist)
    xt = t(x)
    nz = xt != 0
    for inverse in (False, True):
        y64 = _ref64(xt, c, inverse)
        pmax, prms = _plain_fp32(c, rows, dist, inverse, x, y64, nz)
        res = {}
        for tag, form in _forms(c):
            got, rec = _fwd(xt, c, inverse, form)
            mx, rms = _rel(got, y64, nz)
            res[tag] = (got, rec, mx, rms)
            print(f"GDNFWD {name:13s} {dist:6s} {'igdn' if inverse else 'gdn ':4s} {tag:3s} kernel {KERNEL_NAMES[rec[0]]:14s} "
                  f"tile {rec[1]:3d} x {rec[2]:3d} max {mx:.3e} rms {rms:.3e} | plain fp32 max {pmax:.3e} rms {prms:.3e}")
            if tag in _seen:
                _seen[tag].setdefault(name, set()).add(rec[:3])
        for tag, (got, rec, mx, rms) in res.items():
            what = (name, dist, inverse, tag, rec, mx, rms, pmax, prms)
            assert bool((got[~nz] == 0).all()), ("x == 0 did not give +-0", what)
            if tag == "f32" or c < 32:
                assert rec[0] == K_F32, what
            assert rms <= 3.0 * prms, what
            assert mx <= 4.0 * pmax, what
            assert mx <= (c + 8) * 2.0 ** -24, what
        if "h3" in res:
            assert res["h3"][1] == res["bf6"][1], (name, res["h3"][1], res["bf6"][1])
            assert np.array_equal(_bits(res["h3"][0]), _bits(res["bf6"][0])), f"{name} {dist}: H3 and BF6 differ in bits"


def test_float64_reference_on_the_gpu_equals_numpy_float64():
    """The GPU float64 reference against numpy float64 on the CPU: c = 192, 777 spread rows, GDN and IGDN, to 1e-12 relative."""
    c, rows = 192, 777
    x = _rows(c, rows, "spread")
    beta, gamma = _raw_params(c)
    b = np.maximum(beta.astype(np.float64), np.sqrt(BETA_MIN + PED)) ** 2 - PED
    g = np.maximum(gamma.astype(np.float64), np.sqrt(PED)) ** 2 - PED
    low = _low_beta(c)
    assert len(low) == 4 and np.all(np.abs(b[low] - BETA_MIN) <= 1e-15)      # below the bound: beta_eff = beta_min
    assert np.all(g[gamma < 2.0 ** -18] == 0.0)
    n64 = np.abs(x.astype(np.float64)) @ g.T + b
    for inverse in (False, True):
        want = x * n64 if inverse else x / n64
        got = n(_ref64(t(x), c, inverse))
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# structure: guard rows, one result per row, alignment fallback, empty call, load-time fallback
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 0x7FC0BEEF              # a quiet NaN with a marked payload


@pytest.mark.parametrize("c,rows", [(128, 32769), (128, 130945), (192, 65409), (32, 129)])
def test_rows_past_n_are_left_alone(c, rows):
    """`out` has 128 rows more than the call covers and is pre-filled with a marked NaN: afterwards every entry of the rows
    below n is finite and the guard rows carry the marked bits (the tail tile of `k_gdn_bf` re-reads its last row for the
    rows past n; none of them may be stored).  `out` is [n][c] without padding, so a store to one of the channels between c
    and the padded column count (c = 192: 256) of the last row would land in the first guard row; in any other row it lands in
    the next row's entries, which the float64 comparison of every entry covers."""
    from unified_point_cloud_compression_amd import lib as L
    xt = t(_rows(c, rows, "gauss"))
    for form in (L.ARITH_BF6, L.ARITH_F32):
        for inverse in (False, True):
            buf = torch.full(((rows + 128) * c,), POISON, dtype=torch.int32, device=dev()).view(torch.float32).view(rows + 128, c)
            _, rec = _fwd(xt, c, inverse, form, out=buf)
            assert bool(torch.isfinite(buf[:rows]).all()), (c, rows, form, inverse, rec)
            assert bool((buf[rows:].view(torch.int32) == POISON).all()), (c, rows, form, inverse, rec)


def test_one_result_per_row_whatever_the_call():
    """c = 128 under BF6: rows 0 - 999 carry the same bits in the 1 000-, 32 705-, 32 768- and 130 945-row calls (general kernel
    with 32- and 64-row tiles, `k_gdn_bf<1>`, `k_gdn_bf<2>`), the last 1 000 rows of each carry the bits of a call of their
    own, and two identical calls give identical bits."""
    from unified_point_cloud_compression_amd import lib as L
    c = 128
    xt = t(_rows(c, 130945, "spread"))
    recs = set()
    for inverse in (False, True):
        first = None
        for rows in (1000, 32705, 32768, 130945):
            got, rec = _fwd(xt, c, inverse, L.ARITH_BF6, rows=rows)
            again, rec2 = _fwd(xt, c, inverse, L.ARITH_BF6, rows=rows)
            recs.add(rec[:3])
            assert rec2 == rec and np.array_equal(_bits(got), _bits(again)), f"{rows} rows: two identical calls differ"
            if first is None:
                first = _bits(got)
            assert np.array_equal(_bits(got[:1000]), first), f"rows 0 - 999 of the {rows}-row call differ from the 1 000-row call {rec}"
            tail, _ = _fwd(xt[rows - 1000:rows].contiguous(), c, inverse, L.ARITH_BF6)
            assert np.array_equal(_bits(got[rows - 1000:]), _bits(tail)), f"the last 1 000 rows of the {rows}-row call {rec}"
    assert len(recs) == 4, recs              # (the record: four different regimes were compared)


def _unaligned_call(inverse):
    """c = 128, 65 409 rows with x 8 bytes past a fresh allocation (`k_feat_split`'s float2 loads stay aligned):
    (out, record, out of the aligned call, its record)."""
    from unified_point_cloud_compression_amd import lib as L
    c, rows = 128, 65409
    xt = t(_rows(c, rows, "gauss"))
    buf = torch.empty(rows * c + 4, dtype=torch.float32, device=dev())
    xu = buf[2:2 + rows * c].view(rows, c)
    xu.copy_(xt)
    assert buf.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 8 and xu.is_contiguous()
    got, rec = _fwd(xu, c, inverse, L.ARITH_BF6)
    _seen["bf6"].setdefault("unaligned_c128_r65409", set()).add(rec[:3])
    want, rec_al = _fwd(xt, c, inverse, L.ARITH_BF6)
    return got, rec, want, rec_al


def test_unaligned_input_falls_back_to_the_general_kernel():
    """An `x` that is not 16-byte aligned cannot take `k_gdn_bf` (float4 loads): the record must show the general BF kernel with
    its 128-row tile -- a combination no aligned call reaches with one column block -- and the output must carry the bits of the
    aligned call, which records `k_gdn_bf<1>`."""
    for inverse in (False, True):
        got, rec, want, rec_al = _unaligned_call(inverse)
        assert rec[:3] == (K_BF, 128, 128), rec
        assert rec_al[:3] == (K_FUSED, 64, 128), rec_al
        assert np.array_equal(_bits(got), _bits(want))


def test_empty_call_writes_nothing():
    """n = 0 returns PCC_OK, stores nothing and leaves the launch record."""
    from unified_point_cloud_compression_amd import lib as L
    c = 128
    xt = t(_rows(c, 33, "gauss"))
    _fwd(xt, c, False, L.ARITH_BF6)
    before = _last_launch()
    out = torch.full((33 * c,), POISON, dtype=torch.int32, device=dev()).view(torch.float32).view(33, c)
    _, rec = _fwd(xt, c, True, L.ARITH_BF6, out=out, rows=0)
    torch.cuda.synchronize()
    assert rec == before and rec[0] != K_NONE
    assert bool((out.view(torch.int32) == POISON).all())


def test_load_time_fallback_in_subprocess():
    """`PCC_MFMA_BUF=0` (pointer-addressed gathers, no split path: every GDN call takes the fp32-input kernel without buffer
    loads) is a load-time switch: the forward cases of this file up to 33 000 rows once more in a child process."""
    if os.environ.get("PCC_TEST_CHILD"):
        pytest.skip("already the child")
    env = dict(os.environ, PCC_TEST_CHILD="1", PCC_MFMA_BUF="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ids = [f"tests/test_gpu_gdn_float64.py::test_gdn_forward_matches_float64_in_its_regime[{_fwd_id(name, dist)}]"
           for name, dist in _FWD_PARAMS if CASES[name][1] <= CHILD_MAX_ROWS]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q"] + ids, cwd=root, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert f"{len(ids)} passed" in r.stdout, r.stdout[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
class _LowerBound(torch.autograd.Function):
    """max(x, bound) with CompressAI's gradient rule: the gradient passes where x >= bound or where it is negative."""

    @staticmethod
    def forward(ctx, x, bound):
        b = torch.full_like(x, bound)
        ctx.save_for_backward(x, b)
        return torch.max(x, b)

    @staticmethod
    def backward(ctx, g):
        x, b = ctx.saved_tensors
        return ((x >= b) | (g < 0)).to(g.dtype) * g, None


def _formula_grads(x, g, beta_raw, gamma_raw, inverse, dtype, device):
    """(y, dx, d beta_raw, d gamma_raw) of the GDN1 formula by torch autograd in `dtype` on `device` (numpy float32 inputs)."""
    xr = torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(True)
    br = torch.from_numpy(beta_raw).to(device=device, dtype=dtype).requires_grad_(True)
    gr = torch.from_numpy(gamma_raw).to(device=device, dtype=dtype).requires_grad_(True)
    beta = _LowerBound.apply(br, float(np.sqrt(BETA_MIN + PED))) ** 2 - PED
    gamma = _LowerBound.apply(gr, float(np.sqrt(PED))) ** 2 - PED
    nrm = beta + xr.abs() @ gamma.t()
    y = xr * nrm if inverse else xr / nrm
    y.backward(torch.from_numpy(g).to(device=device, dtype=dtype))
    return y.detach(), xr.grad, br.grad, gr.grad


def _terms64(x, g, beta_raw, gamma_raw, inverse):
    """S2 of every entry of dx, d beta_raw, d gamma_raw and the LowerBound classes of the raw parameters, float64 on the GPU.
    Returns (s2_dx, s2_beta, s2_gamma, d_beta_eff, d_gamma_eff, s2_beta_eff, s2_gamma_eff)."""
    x64, g64 = t(x).double(), t(g).double()
    beta, gamma = t(_eff64(beta_raw, BETA_MIN)), t(_eff64(gamma_raw, 0.0))
    n64 = beta + x64.abs() @ gamma.t()
    if inverse:
        u, dx0 = g64 * x64, g64 * n64
    else:
        u, dx0 = -g64 * x64 / (n64 * n64), g64 / n64
    s2_dx = torch.sqrt(dx0 * dx0 + (x64 != 0).double() * ((u * u) @ (gamma * gamma)))
    d_gamma = u.t() @ x64.abs()                                   # [co][ci] = sum over rows of u_co |x|_ci
    s2_gamma = torch.sqrt((u * u).t() @ (x64 * x64))
    d_beta = u.sum(0)
    s2_beta = torch.sqrt((u * u).sum(0))
    fb = 2.0 * torch.clamp_min(t(beta_raw).double(), float(np.sqrt(BETA_MIN + PED)))       # the exact factor 2 max(raw, bound)
    fg = 2.0 * torch.clamp_min(t(gamma_raw).double(), float(np.sqrt(PED)))
    return s2_dx, fb * s2_beta, fg * s2_gamma, d_beta, d_gamma, s2_beta, s2_gamma


BAND = 1e-5      # |d eff| below BAND * S2: the sign of an fp32 sum may differ from float64's, either LowerBound outcome is accepted


def _lower_bound_classes(raw, bound, d_eff, s2_eff):
    """(zeroed, passed, unsure) masks of the BELOW-bound entries by the float64 gradient of the effective parameter."""
    low = t(raw).double() < bound
    unsure = low & (d_eff.abs() <= BAND * s2_eff) & (d_eff != 0)
    return low & (d_eff >= 0) & ~unsure, low & (d_eff < 0) & ~unsure, unsure


def _upstream(c, rows, dist, inverse, x):
    """Gaussian upstream gradient (the sums over rows are not coherent).  d beta_eff[co] = sum over rows of u[:, co] is linear in
    column co of g, so negating that column negates it: the columns of the four channels whose beta is below its bound get the
    sign that makes d beta_eff positive in two of them and negative in the other two (a negated Gaussian column is a Gaussian
    column) -- both outcomes of the LowerBound rule then occur among them, unless x is zero there."""
    rng = np.random.default_rng([c, rows, DISTS.index(dist), int(inverse), 7])
    g = rng.standard_normal((rows, c), dtype=np.float32)
    beta_raw, gamma_raw = _raw_params(c)
    low = _low_beta(c)
    x64 = x.astype(np.float64)
    n_low = _eff64(beta_raw, BETA_MIN)[low] + np.abs(x64) @ _eff64(gamma_raw, 0.0)[low].T          # [rows, 4]
    u_low = g[:, low] * x64[:, low] if inverse else -g[:, low] * x64[:, low] / (n_low * n_low)      # GDN u = -g x / n^2, IGDN u = g x
    want = np.array([1.0, -1.0, 1.0, -1.0])
    g[:, low] *= np.where(np.sign(u_low.sum(0)) * want < 0, -1.0, 1.0).astype(np.float32)
    return g


def _backward_case(c, rows, dist, inverse):
    import unified_point_cloud_compression_amd.autograd as AG
    from unified_point_cloud_compression_amd.model.blocks import MinkowskiGDN
    beta_raw, gamma_raw = _raw_params(c)
    x = _rows(c, rows, dist, seed=1)
    g = _upstream(c, rows, dist, inverse, x)
    m = MinkowskiGDN(c, inverse=inverse, beta_min=BETA_MIN).to(dev())
    with torch.no_grad():
        m.beta.copy_(t(beta_raw))
        m.gamma.copy_(t(gamma_raw))
        y_eval = m.forward_rows(t(x))
    runs = {}
    for tag, fused in (("fused", True), ("torch", False)) if c % 32 == 0 else (("torch", True),):
        AG.GDN_FUSED_BWD = fused
        try:
            for p in m.parameters():
                p.grad = None
            xg = t(x).requires_grad_(True)
            y = m.forward_rows(xg)
            assert y.grad_fn is not None
            y.backward(t(g))
            runs[tag] = (y.detach(), xg.grad, m.beta.grad.clone(), m.gamma.grad.clone())
        finally:
            AG.GDN_FUSED_BWD = True
        assert np.array_equal(_bits(runs[tag][0]), _bits(y_eval)), "GdnFn.forward and forward_rows under no_grad differ in bits"
    ref = _formula_grads(x, g, beta_raw, gamma_raw, inverse, torch.float64, dev())
    yard = _formula_grads(x, g, beta_raw, gamma_raw, inverse, torch.float32, torch.device("cpu"))
    s2_dx, s2_b, s2_g, d_b, d_g, s2_be, s2_ge = _terms64(x, g, beta_raw, gamma_raw, inverse)
    cls_b = _lower_bound_classes(beta_raw, float(np.sqrt(BETA_MIN + PED)), d_b, s2_be)
    cls_g = _lower_bound_classes(gamma_raw, float(np.sqrt(PED)), d_g, s2_ge)
    assert bool(cls_g[0].any()) and bool(cls_g[1].any()), "gamma: both LowerBound outcomes must occur below the bound"
    if rows > 1 or dist == "gauss":                 # (one sparse row: x may be zero in all four channels)
        assert bool(cls_b[0].any()) and bool(cls_b[1].any()), "beta: both LowerBound outcomes must occur below the bound"
    # the float64 reference itself follows the rule
    assert bool((ref[2][cls_b[0]] == 0).all()) and bool((ref[3][cls_g[0]] == 0).all())
    s2 = {"dx": s2_dx, "d beta": torch.where(cls_b[0] | cls_b[2], torch.zeros_like(s2_b), s2_b),
          "d gamma": torch.where(cls_g[0] | cls_g[2], torch.zeros_like(s2_g), s2_g)}
    keep = {"dx": None, "d beta": ~cls_b[2], "d gamma": ~cls_g[2]}
    cls = {"d beta": cls_b, "d gamma": cls_g}
    fig = {}
    for tag, out in list(runs.items()) + [("yard", yard)]:
        for i, what in enumerate(("dx", "d beta", "d gamma")):
            got, want = out[i + 1].to(dev()), ref[i + 1]
            if what in cls:
                zeroed, passed, _ = cls[what]
                assert bool((got[zeroed] == 0).all()), (tag, what, "an entry the LowerBound rule zeroes is not exactly 0")
                assert bool((got[passed] != 0).all()), (tag, what, "an entry the LowerBound rule passes below the bound is 0")
                got, want = got * keep[what], want * keep[what]
            fig[tag, what] = ratios(got, want, s2[what])
    return fig


_BWD_CASES = [(128, 1), (128, 3001), (192, 3001), (64, 3001), (32, 3001), (128, 40003), (16, 3001), (8, 3001)]


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("dist", ["gauss", "sparse"])
@pytest.mark.parametrize("c,rows", _BWD_CASES, ids=[f"c{c}_r{r}" for c, r in _BWD_CASES])
def test_gdn_gradients_match_float64_autograd(c, rows, dist, inverse):
    """`GdnFn.backward` -- fused (`pcc_gdn_bwd_pre/post`, `pcc_gdn_gamma_eff`, `pcc_gdn_reparam_bwd`, the library's products) for
    c a multiple of 32, `_backward_torch` for c = 8, 16 -- against float64 autograd: per output tensor rms <= 3 rms(fp32 CPU
    autograd) and max <= 4 max(fp32 CPU autograd) of |got - ref| / S2; the fused result also within the same factors of the
    `GDN_FUSED_BWD = False` run.  Entries of d beta_raw / d gamma_raw that the LowerBound rule zeroes are exactly 0, those it
    passes below the bound are not; both kinds occur.  `GdnFn.forward` gives the bits of `forward_rows` under no_grad.

    Measured on MI355X (profiles/gdn_float64.txt), rms / rms and max / max against fp32 CPU autograd over the 32 cases: dx 0.84
    - 1.96 and 0.59 - 1.82 (largest at c = 128 with one row), d beta 0.62 - 1.32 and 0.52 - 1.55, d gamma 0.14 - 1.37 and 0.13
    - 2.10; the fused backward measures 0.97 - 1.10 (rms) and 0.86 - 1.15 (max) of the torch-operator backward.  Largest figures: dx max 2.0e-6
    rms 1.6e-7, d beta max 8.0e-7 rms 2.3e-7, d gamma max 2.0e-6 rms 5.0e-7.  (A first version of this test added a coherent
    part to g in the four below-bound beta channels; the sums of those channels then carried an fp32 error far above S2's
    random-rounding model, and two equally accurate backward paths measured 3x apart on d beta.  g is purely Gaussian now.)"""
    fig = _backward_case(c, rows, dist, inverse)
    main = "fused" if c % 32 == 0 else "torch"
    for what in ("dx", "d beta", "d gamma"):
        for tag in [k[0] for k in fig if k[1] == what and k[0] != "yard"]:
            print(f"GDNBWD c{c}_r{rows:<6d} {dist:6s} {'igdn' if inverse else 'gdn ':4s} {what:7s} {tag:5s} max {fig[tag, what][0]:.3e} "
                  f"rms {fig[tag, what][1]:.3e} | fp32 autograd max {fig['yard', what][0]:.3e} rms {fig['yard', what][1]:.3e}")
    for what in ("dx", "d beta", "d gamma"):
        (mx, rms), (ymx, yrms) = fig[main, what], fig["yard", what]
        assert rms <= 3.0 * yrms and mx <= 4.0 * ymx, (what, main, fig[main, what], "fp32 autograd", fig["yard", what])
        if main == "fused":
            tmx, trms = fig["torch", what]
            assert rms <= 3.0 * trms and mx <= 4.0 * tmx, (what, "fused", fig[main, what], "GDN_FUSED_BWD = False", fig["torch", what])


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage of the regimes, from the library's own record
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_listed_regime_was_reached():
    """The union of the (kernel, row tile, column tile) records of this file's runs covers every regime of EXPECT, per form.  A
    case that did not run in this process (the test selected alone) is run here, without a reference.  When a later change of
    the dispatch moves a threshold, the message names the regime that lost its case and what its cases reach now."""
    from unified_point_cloud_compression_amd import lib as L
    for tag, form in (("bf6", L.ARITH_BF6), ("f32", L.ARITH_F32)):
        for name in EXPECT[tag]:
            if name in _seen[tag]:
                continue
            if name.startswith("unaligned"):
                _unaligned_call(False)
                continue
            c, rows = CASES[name]
            _seen[tag].setdefault(name, set()).add(_fwd(t(_rows(c, rows, "gauss")), c, False, form)[1][:3])
        reached = set().union(*_seen[tag].values())
        lost = {}
        for name, regime in EXPECT[tag].items():
            if regime not in reached:
                lost.setdefault(regime, []).append((name, sorted(_seen[tag][name])))
        assert not lost, f"{tag}: regimes no case reaches any more (kernel, BM, BN) -> [(case meant to, what it records now)]: {lost}"
