"""The element-wise training kernels of `csrc/pcc_entropy.hip` against float64, likelihood errors in BITS: `pcc_gauss_lik_fwd/bwd`,
`pcc_eb_lik_fwd/bwd`, `pcc_quant_mlp_fwd/bwd` with its two-stage reduction, `pcc_focal_rows`, and the `lik` outputs of
`pcc_gauss_encode` / `pcc_eb_encode`.  They produce the rate term and the occupancy loss of every training step and the
likelihoods the encoder reports.

Reference.  tests/rate_loss_ref.py: the formulas restated with torch operators, evaluated in float64 on the GPU (the convention
of test_gpu_weight_gradients.py), gradients by float64 autograd with CompressAI's LowerBound rule; the bounds are the kernels'
float32 constants widened to double.  tests/test_cpu_rate_loss_ref.py checks it against `math.erfc` / `tanh` / `exp`.

Yardstick.  The float32 torch operator chain each kernel replaced, on the same inputs, measured against the same float64
reference with the same metric: the Gaussian and factorised-prior chains as `likelihood_rows` falls back to them, `quant_nn` as
torch layers, the operator sequence `loss.Multiscale_FocalLoss` runs with `FUSED_FOCAL = False` (restated on plain tensors in
`rate_loss_ref.focal_rows`: the loss itself takes sparse tensors and a ground-truth set).  Every accuracy bound is
        kernel error <= max(MARGIN x yardstick error, floor),   MARGIN = 4,   for the max and for the rms.
MARGIN covers device transcendentals (`erfcf`, `expf`, `tanhf`, `powf`) that differ from torch's by a few ulps; a structural
error is of the order of the quantity itself.  The floor is what float32 cannot avoid when the yardstick happens to be exact
(one element; every element on the likelihood floor): FLOOR_ULPS = 4 float32 ulps (2^-23) of the normalising magnitude -- every
result here is the end of a chain of eight or more roundings of half an ulp each -- for the ratio metrics 4 x 2^-23 outright, for
a likelihood in bits the move of 4 x 2^-23 x (up + lo) in the likelihood (up, lo: the two
cumulative terms whose difference the likelihood is), taken off the kernel's error element by element.

Metrics (rate_loss_ref.py): likelihoods |log2 got - log2 ref| in bits with the 1e-9 floor on both sides; total bits as a
relative error; element-wise gradients |got - ref| over the float64 sum of the magnitudes of the terms whose difference forms
them; reduced parameter gradients (`d_packed` [c, 58], `d_params` [151]) |got - ref| / S2, S2 = sqrt(sum of the squared
per-element contributions), with random-sign and with all-positive upstream gradients.  Kinks (a likelihood within 1e-4 of
1e-9, a ReLU pre-activation within 1e-5 of its terms, a focal v within 1e-6 of 1e-2) are taken out of the gradient comparisons
(zero upstream gradient for the reduced sums); every test asserts they are at most 0.2 % of its input.  Decisions on exact
float32 inputs (scale >= 0.11f, v == mean, the sign of g) are never excluded.

Every case prints one line with the kernel's and the yardstick's error (run with -s); the MI355X output is
profiles/rate_loss_float64.txt, and the ranges it shows are quoted in the docstrings of the tests.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import rate_loss_ref as R
from tests.util import dev, t, bits as _bits, ratios

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR_ULPS = 4
FLOOR = FLOOR_ULPS * R.ULP
TAIL = 256                                   # guard elements behind every output
PCC_EWS = -3                                 # include/pcc_hip.h
NAN_BITS = np.array([np.nan], np.float32).view(np.int32)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def _L():
    from unified_point_cloud_compression_amd import lib as L
    return L


def _out(nelem):
    """A NaN-filled float32 buffer of nelem outputs plus the guard tail."""
    return torch.full((nelem + TAIL,), float("nan"), dtype=torch.float32, device=dev())


def _take(buf, nelem, what):
    """The nelem outputs of a buffer of `_out`: every one written (no NaN left), the guard tail untouched."""
    assert bool(torch.isnan(buf[nelem:]).all()), f"{what}: written past the end"
    assert not bool(torch.isnan(buf[:nelem]).any()), f"{what}: not every element written"
    return buf[:nelem]


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _bounded(what, k, y, floor=(FLOOR, FLOOR)):
    print(f"{what}: kernel max {k[0]:.3e} rms {k[1]:.3e} | float32 torch chain max {y[0]:.3e} rms {y[1]:.3e}"
          f" | floor {floor[0]:.2e} {floor[1]:.2e}")
    assert k[0] <= max(MARGIN * y[0], floor[0]), f"{what}: max {k[0]:.3e} against {y[0]:.3e} of the float32 torch chain"
    assert k[1] <= max(MARGIN * y[1], floor[1]), f"{what}: rms {k[1]:.3e} against {y[1]:.3e} of the float32 torch chain"


def _share(what, kink):
    share = float(kink.double().mean())
    print(f"{what}: excluded share {share:.4%}")
    assert share <= R.MAX_KINK_SHARE
    return ~kink


def _bits_floor(up, lo, raw):
    """Per element, in bits: what FLOOR_ULPS ulps of the two cumulative terms do to the floored likelihood."""
    moved = (raw + FLOOR * (up + lo)).clamp_min(R.LIK_BOUND)
    return torch.log2(moved) - torch.log2(raw.clamp_min(R.LIK_BOUND))


def _check_bits(what, got, yard, ref, floor):
    """Per-element bits, then the total.  The floor is taken off the kernel's error element by element (one element with a
    large floor does not make room for the others), and what is left is held against the yardstick.  The total is one number,
    and the yardstick's own total can be small by luck (errors of both signs cancel in it), so it is also allowed what
    independent errors of the yardstick's rms size (or of the floor's) sum to over n elements: rms x sqrt(n)."""
    ek, ey = R.bits_err(got, ref), R.bits_err(yard, ref)
    over = R.max_rms((ek - floor).clamp_min(0))
    ek, ey, fl = R.max_rms(ek), R.max_rms(ey), R.max_rms(floor)
    print(f"{what} [bits]: kernel max {ek[0]:.3e} rms {ek[1]:.3e} | float32 torch chain max {ey[0]:.3e} rms {ey[1]:.3e}"
          f" | kernel beyond the floor max {over[0]:.3e} rms {over[1]:.3e}")
    assert over[0] <= MARGIN * ey[0], f"{what}: max {ek[0]:.3e} bits against {ey[0]:.3e} of the float32 torch chain"
    assert over[1] <= MARGIN * ey[1], f"{what}: rms {ek[1]:.3e} bits against {ey[1]:.3e} of the float32 torch chain"
    tb, walk = R.total_bits(ref), math.sqrt(ref.numel())
    k, y = abs(R.total_bits(got) - tb) / tb, abs(R.total_bits(yard) - tb) / tb
    print(f"{what} [total bits, relative]: kernel {k:.3e} | float32 torch chain {y:.3e} | rms x sqrt(n) {ey[1] * walk / tb:.3e}"
          f" | total {tb:.6e}")
    assert k <= max(MARGIN * y, MARGIN * ey[1] * walk / tb, fl[1] * walk / tb)


# ---------------------------------------------------------------------------------------------------------------------------------
# Gaussian likelihood
# ---------------------------------------------------------------------------------------------------------------------------------
GAUSS_SIZES = (1, 255, 256, 257, 200003)


@functools.lru_cache(maxsize=None)
def _gc():
    from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional, get_scale_table
    gc = GaussianConditional(None).to(dev())
    gc.update_scale_table(get_scale_table(), force=True)
    return gc


def _gauss_chain(v, s, m):
    """The float32 torch chain `GaussianConditional.likelihood_rows` falls back to."""
    gc = _gc()
    sb = gc.lower_bound_scale(s)
    a = torch.abs(v - m)
    return gc.likelihood_lower_bound(gc._standardized_cumulative((0.5 - a) / sb) - gc._standardized_cumulative((-0.5 - a) / sb))


@functools.lru_cache(maxsize=None)
def _gauss_case(n):
    v, s, m, g = (t(a) for a in R.gauss_inputs(n))
    ref = R.gauss_grads(v.double(), s.double(), m.double(), g.double())
    tm = R.gauss_terms(v.double(), s.double(), m.double())
    lv, ls, lm = (x.clone().requires_grad_(True) for x in (v, s, m))
    lik = _gauss_chain(lv, ls, lm)
    (lik * g).sum().backward()
    return dict(v=v, s=s, m=m, g=g, ref=ref, tm=tm, yard=(lik.detach(), lv.grad, ls.grad, lm.grad))


def _gauss_bwd(c, n, want=(True, True, True)):
    L = _L()
    outs = [_out(n) if w else None for w in want]
    L.call("pcc_gauss_lik_bwd", L.ptr(c["v"]), L.ptr(c["s"]), L.ptr(c["m"]), L.ptr(c["g"]), n,
           *(o.data_ptr() if o is not None else None for o in outs), L.stream())
    return [_take(o, n, "gauss bwd") if o is not None else None for o in outs]


@pytest.mark.parametrize("n", GAUSS_SIZES)
def test_gaussian_likelihood_forward_in_bits(n):
    """`pcc_gauss_lik_fwd`, with `mean` given and with `mean == NULL`, around the 256-thread block and at 200 003 elements.
    Measured on MI355X (bits): kernel max 1.3e-7 - 2.5e-4, rms 1.3e-7 - 1.3e-5 over the sizes, and the float32 torch chain the
    same figures to every digit printed (it runs the same device erfc); the largest errors sit at scales near 300, 4 to 5 sigma
    out, where the two cumulative terms differ by 1.5 %.  Total bits: 1.6e-8 - 1.9e-7 relative."""
    L = _L()
    c = _gauss_case(n)
    floor = _bits_floor(c["tm"]["up"], c["tm"]["lo"], c["tm"]["raw"])
    buf = _out(n)
    L.call("pcc_gauss_lik_fwd", L.ptr(c["v"]), L.ptr(c["s"]), L.ptr(c["m"]), n, buf.data_ptr(), L.stream())
    _check_bits(f"gauss fwd n={n}", _take(buf, n, "gauss fwd"), c["yard"][0], c["ref"][0], floor)
    if n >= 255:
        on_floor = float((c["ref"][0] == R.LIK_BOUND).double().mean())
        print(f"gauss fwd n={n}: floor share {on_floor:.2%}")
        assert on_floor >= 0.05
    # mean == NULL: the same distances as values of their own
    d = (c["v"] - c["m"]).contiguous()
    buf = _out(n)
    L.call("pcc_gauss_lik_fwd", L.ptr(d), L.ptr(c["s"]), None, n, buf.data_ptr(), L.stream())
    ref0 = R.gauss_lik(d.double(), c["s"].double())
    tm0 = R.gauss_terms(d.double(), c["s"].double())
    _check_bits(f"gauss fwd n={n} mean=NULL", _take(buf, n, "gauss fwd"), _gauss_chain(d, c["s"], torch.zeros_like(d)), ref0,
                _bits_floor(tm0["up"], tm0["lo"], tm0["raw"]))


@pytest.mark.parametrize("n", GAUSS_SIZES)
def test_gaussian_likelihood_gradients(n):
    """`pcc_gauss_lik_bwd`: dv, dscale, dmean over the magnitude sums |g| (p1 + p2) / s and |g| (|u1| p1 + |u2| p2) / s, and
    the values the kernel decides exactly.  Measured on MI355X, of the magnitude sum: dv and dmean kernel max 1.1e-7 - 4.7e-6, rms
    1.1e-7 - 4.8e-7 (float32 torch chain max up to 7.4e-6, rms up to 6.5e-7); dscale kernel max 0 - 9.1e-4, rms up to 2.5e-6
    (chain 9.0e-4, 2.5e-6).  The 9e-4 is shared: |v - mean| within 1e-3 of 0.5 at a small scale makes u1 = (0.5 - |v - mean|) / s a
    difference of nearly equal float32 numbers, and u1 p1 is the whole gradient there."""
    c = _gauss_case(n)
    tm, g64 = c["tm"], c["g"].double()
    keep = _share(f"gauss bwd n={n}", R.gauss_kinks(tm["raw"]))
    dv, ds, dm = _gauss_bwd(c, n)
    d_a = g64.abs() * (tm["p1"] + tm["p2"]) / tm["s"]
    d_s = g64.abs() * (tm["u1"].abs() * tm["p1"] + tm["u2"].abs() * tm["p2"]) / tm["s"]
    for name, got, k, den in (("dv", dv, 1, d_a), ("dscale", ds, 2, d_s), ("dmean", dm, 3, d_a)):
        _bounded(f"gauss bwd n={n} {name}", R.ratio(got, c["ref"][k], den, keep), R.ratio(c["yard"][k], c["ref"][k], den, keep))
    assert _same(dm, -dv)
    at_mean = c["v"] == c["m"]
    assert bool((dv[at_mean] == 0).all()) and bool((dm[at_mean] == 0).all())
    # below the scale bound the gradient passes only when it would raise the scale (g * dl_ds < 0).  The sign of dl_ds is a
    # difference of two products: where they cancel to 1e-5 of their magnitudes float32 may see the other sign
    low = c["s"].double() < R.SCALE_BOUND
    blocked = low & (g64 * tm["dl_ds"] >= 0)
    den = (tm["u1"].abs() * tm["p1"] + tm["u2"].abs() * tm["p2"]) / tm["s"]
    sure = blocked & ((g64 == 0) | (den == 0) | (tm["dl_ds"].abs() > 1e-5 * den))
    print(f"gauss bwd n={n}: {int(low.sum())} below the scale bound, {int(blocked.sum())} blocked, {int(sure.sum())} of them decided")
    assert int(blocked.sum()) - int(sure.sum()) <= 1 + n // 10000
    assert bool((ds[sure] == 0).all())
    if n >= 255:
        assert bool((low & ~blocked & (ds != 0)).any()) and bool(sure.any())
    on_floor = (tm["raw"] < R.LIK_BOUND) & keep & (g64 >= 0)
    for got in (dv, ds, dm):
        assert bool((got[on_floor] == 0).all())
    if n >= 255:
        passing = (tm["raw"] < R.LIK_BOUND) & keep & (g64 < 0) & (tm["p2"] > 1e-20) & (c["v"] != c["m"])
        assert bool(on_floor.any()) and bool(passing.any()) and bool((dv[passing] != 0).all())
    for drop in range(3):
        outs = _gauss_bwd(c, n, tuple(i != drop for i in range(3)))
        for i, (a, b) in enumerate(zip(outs, (dv, ds, dm))):
            assert (a is None) == (i == drop) and (a is None or _same(a, b))


def test_gaussian_likelihood_through_autograd_equals_the_direct_calls():
    """`GaussianConditional.likelihood_rows` -> `GaussLikFn`: the bits of the direct calls, for a [n, 1] shape and with `mean`
    not requiring a gradient."""
    n = 200003
    c = _gauss_case(n)
    L = _L()
    buf = _out(n)
    L.call("pcc_gauss_lik_fwd", L.ptr(c["v"]), L.ptr(c["s"]), L.ptr(c["m"]), n, buf.data_ptr(), L.stream())
    dv, ds, dm = _gauss_bwd(c, n)
    for mean_grad in (True, False):
        lv, ls = (c[k].clone().reshape(n, 1).requires_grad_(True) for k in ("v", "s"))
        lm = c["m"].clone().reshape(n, 1).requires_grad_(mean_grad)
        lik = _gc().likelihood_rows(lv, ls, lm)
        assert lik.shape == (n, 1) and _same(lik.reshape(-1), buf[:n])
        lik.backward(c["g"].reshape(n, 1))
        assert _same(lv.grad.reshape(-1), dv) and _same(ls.grad.reshape(-1), ds)
        assert (lm.grad is None) if not mean_grad else _same(lm.grad.reshape(-1), dm)


@pytest.mark.parametrize("adaptive", [False, True])
def test_gaussian_encoder_likelihood_in_bits(adaptive):
    """`lik` of `pcc_gauss_encode` on the integer symbols the kernel itself produced, with and without adaptive gain rows, scales
    across the whole table and the floor reached.  Measured on MI355X (bits): kernel max 2.7e-4 / 3.2e-4 (without / with gain rows), rms
    1.3e-5, and the float32 torch chain the same figures; total bits 2e-8 relative."""
    rows, c, nb = 1500, 128, 2
    rng = np.random.default_rng(21)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(300.0), (rows, c))).astype(np.float32)
    means = rng.standard_normal((rows, c)).astype(np.float32)
    y = (means + rng.uniform(-7.5, 7.5, (rows, c)) * np.maximum(scales, 0.11)).astype(np.float32)
    keys = np.sort(rng.choice(10 ** 6, rows, replace=False)).astype(np.int64)
    keys[rows // 2:] += 1 << R.KEY_B_SHIFT
    gain = (0.5 + rng.random((nb, c))).astype(np.float32)
    params = t(np.concatenate([scales, means], axis=1))
    sym, _, lik = _gc().encode_rows(t(y), params, t(keys), t(gain) if adaptive else None)
    g_rows = t(gain)[t(keys) >> R.KEY_B_SHIFT] if adaptive else torch.ones((rows, c), device=dev())
    s32 = t(scales) * g_rows                                  # one float32 product: the same bits as the kernel's
    q = sym.to(torch.float32)
    zero = torch.zeros_like(q)
    ref = R.gauss_lik(q.double(), s32.double())
    tm = R.gauss_terms(q.double(), s32.double())
    assert float((tm["raw"] < R.LIK_BOUND).double().mean()) >= 0.05 and int(sym.abs().max()) > 100 and bool((sym == 0).any())
    _check_bits(f"gauss encode adaptive={adaptive}", lik, _gauss_chain(q, s32, zero), ref, _bits_floor(tm["up"], tm["lo"], tm["raw"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# factorised prior
# ---------------------------------------------------------------------------------------------------------------------------------
EB_SHAPES = ((1, 1), (255, 3), (257, 24), (1000, 24), (900, 192))


@functools.lru_cache(maxsize=None)
def _eb(c):
    from unified_point_cloud_compression_amd.compressai.entropy_models import EntropyBottleneck
    eb = EntropyBottleneck(c).to(dev())
    with torch.no_grad():
        for k, a in R.eb_params(c).items():
            getattr(eb, k).copy_(t(a))
    return eb


def _eb_chain(eb, v):
    """The float32 torch chain `EntropyBottleneck.likelihood_rows` falls back to."""
    x = v.t().unsqueeze(1)
    lo, up = eb._logits_cumulative(x - 0.5), eb._logits_cumulative(x + 0.5)
    sg = -torch.sign(lo + up).detach()
    return eb.likelihood_lower_bound(torch.abs(torch.sigmoid(sg * up) - torch.sigmoid(sg * lo))[:, 0, :].t())


@functools.lru_cache(maxsize=None)
def _eb_case(n, c):
    eb = _eb(c)
    P = eb._packed_with_grad().detach().contiguous()          # float32 [c, 58]: what the kernels are handed
    v, g = (t(a) for a in R.eb_inputs(n, c))
    raw, d_v = R.eb_terms(P.double(), v.double())
    kink = R.gauss_kinks(raw)
    g = torch.where(kink, torch.zeros_like(g), g)             # kinks: no upstream gradient (they feed the reduced sums)
    return dict(eb=eb, P=P, v=v, g=g, raw=raw, d_v=d_v, kink=kink)


def _eb_bwd(c, g, want_dv=True, fill=float("nan")):
    L = _L()
    n, ch = c["v"].shape
    dv = _out(n * ch) if want_dv else None
    dp = _out(ch * 58)
    dp[:ch * 58] = fill
    L.call("pcc_eb_lik_bwd", L.ptr(c["v"]), L.ptr(g), n, ch, L.ptr(c["P"]), dv.data_ptr() if want_dv else None, dp.data_ptr(), L.stream())
    return (_take(dv, n * ch, "eb dv").reshape(n, ch) if want_dv else None), _take(dp, ch * 58, "eb d_packed").reshape(ch, 58)


@pytest.mark.parametrize("n,c", EB_SHAPES)
def test_factorised_prior_likelihood_and_gradients(n, c):
    """`pcc_eb_lik_fwd/bwd`: likelihood in bits, dv over |s_u (1 - s_u) up'| + |s_l (1 - s_l) lo'|, `d_packed` over S2 with
    random-sign and with all-positive upstream gradients; one channel odd (floor with all gradients 0), one with saturated
    tanh factors, one with softplus(matrices) about 1e-4; 1000 rows = four strided passes, the last ragged.  Measured on MI355X:
    likelihood kernel max 1.4e-6 - 9.0e-5, rms 1.4e-6 - 3.4e-6 bits (float32 torch chain max 1.4e-6 - 8.9e-5, rms up to
    3.5e-6); dv kernel max 8.5e-8 - 8.7e-6, rms up to 2.8e-7 (chain the same to two digits); d_packed kernel max 2.8e-7 - 6.1e-7,
    rms 0.9e-7 - 1.4e-7 of S2 (chain max 1.9e-7 - 4.6e-6, rms up to 7.2e-7); the flat channel on its own 5.6e-2 of S2 in kernel
    and chain alike with random-sign g, 0 with all-positive g."""
    L = _L()
    cs = _eb_case(n, c)
    eb, P, v = cs["eb"], cs["P"], cs["v"]
    _share(f"eb n={n} c={c}", cs["kink"])
    buf = _out(n * c)
    L.call("pcc_eb_lik_fwd", L.ptr(v), n, c, L.ptr(P), buf.data_ptr(), L.stream())
    lik = _take(buf, n * c, "eb fwd").reshape(n, c)
    with torch.no_grad():
        ref = R.eb_lik(P.double(), v.double())
        lo, up = R.eb_logits(P.double(), v.double() - 0.5), R.eb_logits(P.double(), v.double() + 0.5)
        sg = -torch.sign(lo + up)
        floor = _bits_floor(torch.sigmoid(sg * up) * sg.abs(), torch.sigmoid(sg * lo) * sg.abs(), cs["raw"])   # sg == 0: exact
        yard = _eb_chain(eb, v)
    _check_bits(f"eb fwd n={n} c={c}", lik, yard, ref, floor)
    on_floor = cs["raw"] < R.LIK_BOUND
    print(f"eb fwd n={n} c={c}: floor share {float(on_floor.double().mean()):.2%}")
    odd = torch.zeros_like(on_floor)
    odd[R.EB_ODD_ROWS, 0] = True
    assert bool((cs["raw"][odd] == 0).all()) and bool((lik[odd] == np.float32(1e-9)).all())
    if n >= 255:
        assert float(on_floor.double().mean()) >= 0.03 and bool(odd.any())
    for tag, g in (("random-sign", cs["g"]), ("all-positive", cs["g"].abs())):
        what = f"eb bwd n={n} c={c} {tag} g"
        _, dv64, dp64, s2 = R.eb_grads(P.double(), v.double(), g.double())
        dv, dp = _eb_bwd(cs, g)
        lv = v.clone().requires_grad_(True)
        _eb_chain(eb, lv).backward(g)                                          # yardstick of dv: the module's chain
        lp = P.clone().requires_grad_(True)
        R.eb_lik(lp, v).backward(g)                                            # yardstick of d_packed: the same formulas in float32
        den = g.double().abs() * cs["d_v"]
        _bounded(f"{what} dv", R.ratio(dv, dv64, den), R.ratio(lv.grad, dv64, den))
        # the channel with softplus(matrices) ~ 1e-4 is measured on its own: its logits barely move over the unit bin, float32
        # gives su - sl == 0 exactly where float64 gives ~1e-17, and the gradient that passes the floor for g < 0 is lost whole --
        # in the kernel and in the torch chain alike; kept apart, it does not set the scale for the other channels
        rest = torch.ones(c, dtype=torch.bool, device=dev())
        rest[R.EB_FLAT_CHANNEL:R.EB_FLAT_CHANNEL + 1] = False
        _bounded(f"{what} d_packed", ratios(dp[rest], dp64[rest], s2[rest]), ratios(lp.grad[rest], dp64[rest], s2[rest]))
        if c >= 3:
            f = R.EB_FLAT_CHANNEL
            _bounded(f"{what} d_packed, flat channel", ratios(dp[f], dp64[f], s2[f]), ratios(lp.grad[f], dp64[f], s2[f]))
        blocked = on_floor & (g >= 0)
        assert bool((dv[blocked] == 0).all()) and bool((dv[odd] == 0).all())
        dv2, dp2 = _eb_bwd(cs, g, fill=0.0)
        assert _same(dv, dv2) and _same(dp, dp2)                               # deterministic, and every entry of d_packed written
        none, dp3 = _eb_bwd(cs, g, want_dv=False)
        assert none is None and _same(dp, dp3)
    # no rows: d_packed is all zeros
    dp = _out(c * 58)
    L.call("pcc_eb_lik_bwd", None, None, 0, c, L.ptr(P), None, dp.data_ptr(), L.stream())
    assert bool((_take(dp, c * 58, "eb d_packed, n == 0") == 0).all())


def test_factorised_prior_raw_parameter_gradients_match_the_float64_module():
    """All 14 raw-parameter gradients through `likelihood_rows(...).backward` (kernel + torch's softplus / tanh derivatives)
    against the float64 restatement from the raw parameters; error relative to each tensor's largest entry.  Measured on MI355X:
    kernel 5.9e-7 - 2.7e-6, float32 torch chain 8.0e-7 - 4.2e-6."""
    n, c = 1000, 24
    cs = _eb_case(n, c)
    eb, v, g = cs["eb"], cs["v"], cs["g"]
    raw64 = {k: p.detach().double().requires_grad_(True) for k, p in eb.named_parameters() if k != "quantiles"}
    R.eb_lik(R.eb_pack(raw64), v.double()).backward(g.double())
    res = {}
    for tag, fn in (("kernel", eb.likelihood_rows), ("chain", lambda x: _eb_chain(eb, x))):
        eb.zero_grad(set_to_none=True)
        fn(v.clone().requires_grad_(True)).backward(g)
        res[tag] = {k: p.grad.clone() for k, p in eb.named_parameters() if p.grad is not None}
    assert set(res["kernel"]) == set(res["chain"]) == set(raw64) and len(raw64) == 14
    for k, p64 in raw64.items():
        top = float(p64.grad.abs().max())
        assert top > 0
        err = [float((res[tag][k].double() - p64.grad).abs().max()) / top for tag in ("kernel", "chain")]
        print(f"eb raw gradient {k}: kernel {err[0]:.3e} | float32 torch chain {err[1]:.3e}")
        assert err[0] <= max(MARGIN * err[1], FLOOR)


def test_factorised_prior_encoder_likelihood_in_bits():
    """`lik` of `pcc_eb_encode` at c = 192 on the quantised values the kernel itself produced.  Measured on MI355X (bits): kernel
    max 7.9e-5, rms 3.3e-6; float32 torch chain max 6.6e-5, rms 3.4e-6; total bits 1.5e-9 relative."""
    n, c = 900, 192
    cs = _eb_case(n, c)
    eb = cs["eb"]
    with torch.no_grad():
        eb.quantiles[:, 0, 1] = t(np.random.default_rng(22).normal(0, 2, c).astype(np.float32))
        sym, zh, lik = eb.encode_rows(cs["v"])
        P = eb.packed()
        assert _same(P, cs["P"])
        z64 = zh.double()
        ref = R.eb_lik(P.double(), z64)
        lo, up = R.eb_logits(P.double(), z64 - 0.5), R.eb_logits(P.double(), z64 + 0.5)
        sg = -torch.sign(lo + up)
        floor = _bits_floor(torch.sigmoid(sg * up) * sg.abs(), torch.sigmoid(sg * lo) * sg.abs(), R.eb_raw(P.double(), z64))
        assert float((ref == R.LIK_BOUND).double().mean()) >= 0.03
        _check_bits("eb encode c=192", lik, _eb_chain(eb, zh), ref, floor)


# ---------------------------------------------------------------------------------------------------------------------------------
# quantisation-offset network
# ---------------------------------------------------------------------------------------------------------------------------------
QM_SIZES = (1, 255, 256, 257, 1023, 1025, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1025)


@functools.lru_cache(maxsize=None)
def _qm_net():
    """(params float32 [151] on the GPU, the same network as float32 torch layers)."""
    p = t(R.qm_params())
    net = torch.nn.Sequential(torch.nn.Linear(2, 10), torch.nn.ReLU(), torch.nn.Linear(10, 10), torch.nn.ReLU(),
                              torch.nn.Linear(10, 1)).to(dev())
    with torch.no_grad():
        at = 0
        for q in net.parameters():
            q.copy_(p[at:at + q.numel()].view(q.shape))
            at += q.numel()
    return p, net


def _qm_ws_blocks(n):
    return (int(_L().load().pcc_quant_mlp_ws_bytes(n)) - 256) // (151 * 4)


def _qm_bwd(p, s, d, g, want=(True, True), ws_fill=0xFF, short=0):
    """-> (rc, d_scale, d_stddev, d_params); the workspace is exactly ws_bytes (minus `short`) plus a guard tail, filled with
    `ws_fill` (0xFF: every float of it a NaN)."""
    L = _L()
    n = s.shape[0]
    nbytes = int(L.load().pcc_quant_mlp_ws_bytes(n)) - short
    ws = torch.full((nbytes + TAIL,), ws_fill, dtype=torch.uint8, device=dev())
    ws[nbytes:] = 0xA5
    outs = [_out(n) if w else None for w in want]
    dp = _out(151)
    rc = L.load().pcc_quant_mlp_bwd(L.ptr(s), L.ptr(d), L.ptr(g), n, L.ptr(p), *(o.data_ptr() if o is not None else None for o in outs),
                                    dp.data_ptr(), ws.data_ptr(), nbytes, L.stream())
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace written past the end"
    if rc != 0:
        return rc, None, None, dp
    return rc, *(_take(o, n, "quant d_in") if o is not None else None for o in outs), _take(dp, 151, "quant d_params")


@pytest.mark.parametrize("n", QM_SIZES)
def test_quant_offset_network_against_float64(n):
    """`pcc_quant_mlp_fwd/bwd` around the 256-thread block, around one and two workgroups of 1024 elements, and around the cap of
    1024 workgroups (1024 * 1024 + 1025 elements: some threads take five elements and some four): offsets and input derivatives
    over the magnitude sums of their terms, the 151 parameter sums over S2 with random-sign and all-positive upstream gradients,
    and the structure of the two-stage reduction.  Measured on MI355X: offsets kernel max 2.4e-8 - 2.4e-7, rms up to 5.4e-8
    (float32 torch layers max 0.8e-8 - 2.9e-7, rms up to 5.9e-8); d_scale / d_stddev kernel max 0.6e-8 - 2.0e-7, rms up to 3.7e-8
    (layers the same to two digits); d_params of S2: random-sign kernel max 5.3e-7 - 1.3e-5, rms up to 2.4e-6 (layers max
    2.2e-7 - 1.3e-5), all-positive kernel max 1.1e-6 - 6.7e-4, rms up to 1.7e-4 (layers max 1.9e-6 - 3.3e-3, rms up to 3.9e-4)."""
    L = _L()
    p, net = _qm_net()
    s, d, g = (t(a) for a in R.qm_inputs(n))
    kink, d_out, d_s, d_d, off1, off2 = R.qm_terms(p.double(), s.double(), d.double())
    keep = _share(f"quant network n={n}", kink)
    print(f"quant network n={n}: hidden units off {off1:.1%} / {off2:.1%}")
    if n >= 255:
        assert 0.1 <= off1 <= 0.9 and 0.1 <= off2 <= 0.9
    g = torch.where(kink, torch.zeros_like(g), g)
    out64, ds64, dd64, sums = R.qm_grads(p.double(), s.double(), d.double(), [g.double(), g.double().abs()])
    assert _qm_ws_blocks(n) == min(-(-n // 1024), 1024)
    buf = _out(n)
    L.call("pcc_quant_mlp_fwd", L.ptr(s), L.ptr(d), n, L.ptr(p), buf.data_ptr(), L.stream())
    ls, ld = s.clone().requires_grad_(True), d.clone().requires_grad_(True)
    yard = net(torch.stack([ls, ld], dim=-1)).squeeze(-1)
    _bounded(f"quant network n={n} offsets", R.ratio(_take(buf, n, "quant fwd"), out64, d_out), R.ratio(yard.detach(), out64, d_out))
    for tag, gg, (dp64, s2) in zip(("random-sign", "all-positive"), (g, g.abs()), sums):
        what = f"quant network n={n} {tag} g"
        rc, ds, dd, dp = _qm_bwd(p, s, d, gg)
        assert rc == 0
        net.zero_grad(set_to_none=True)
        ls.grad = ld.grad = None
        yard.backward(gg, retain_graph=True)
        yp = torch.cat([q.grad.reshape(-1) for q in net.parameters()])
        g64 = gg.double()
        _bounded(f"{what} d_scale", R.ratio(ds, ds64 * g64, d_s * g64.abs(), keep), R.ratio(ls.grad, ds64 * g64, d_s * g64.abs(), keep))
        _bounded(f"{what} d_stddev", R.ratio(dd, dd64 * g64, d_d * g64.abs(), keep), R.ratio(ld.grad, dd64 * g64, d_d * g64.abs(), keep))
        _bounded(f"{what} d_params", ratios(dp, dp64, s2), ratios(yp, dp64, s2))
        # a workspace of NaNs, a second call, and either input derivative left out: the same bits
        for kw in (dict(ws_fill=0x00), dict(), dict(want=(False, True)), dict(want=(True, False))):
            rc2, ds2, dd2, dp2 = _qm_bwd(p, s, d, gg, **kw)
            assert rc2 == 0 and _same(dp, dp2) and (ds2 is None or _same(ds, ds2)) and (dd2 is None or _same(dd, dd2))
            assert (ds2 is None) == (not kw.get("want", (True, True))[0]) and (dd2 is None) == (not kw.get("want", (True, True))[1])
    rc, _, _, dp = _qm_bwd(p, s, d, g, short=1)
    assert rc == PCC_EWS and bool((_bits(dp) == NAN_BITS).all())                # refused, and nothing written


def test_quant_offset_network_without_elements_and_through_autograd():
    """n == 0 gives zero `d_params`; `QuantMlpFn` with `scale` an expanded [n, 1] -> [n, 128] view, as `get_offsets` passes it: the
    gradient of the unexpanded tensor against float64.  Measured on MI355X: kernel max 1.3e-8, rms 4.0e-9 of the magnitude sum;
    float32 torch layers max 1.6e-8, rms 3.8e-9."""
    from unified_point_cloud_compression_amd.autograd import QuantMlpFn
    L = _L()
    p, net = _qm_net()
    dp = _out(151)
    L.call("pcc_quant_mlp_bwd", None, None, None, 0, L.ptr(p), None, None, dp.data_ptr(), None, 0, L.stream())
    assert bool((_take(dp, 151, "quant d_params, n == 0") == 0).all())
    L.call("pcc_quant_mlp_fwd", None, None, 0, L.ptr(p), None, L.stream())
    rows, c = 301, 128
    rng = np.random.default_rng(23)
    s0 = t(rng.uniform(0.2, 3.0, (rows, 1)).astype(np.float32))
    d0 = t(rng.uniform(0.1, 9.0, (rows, c)).astype(np.float32))
    g = t(rng.standard_normal((rows, c)).astype(np.float32))
    se = s0.expand(rows, c).reshape(-1)
    kink, _, d_s, _, _, _ = R.qm_terms(p.double(), se.double(), d0.reshape(-1).double())
    g = torch.where(kink.reshape(rows, c), torch.zeros_like(g), g)
    _share("quant network autograd", kink)
    _, ds64, _, _ = R.qm_grads(p.double(), se.double(), d0.reshape(-1).double(), [])
    ref = (ds64.reshape(rows, c) * g.double()).sum(1, keepdim=True)
    den = (d_s.reshape(rows, c) * g.double().abs()).sum(1, keepdim=True)
    res = []
    for fused in (True, False):
        ls, ld = s0.clone().requires_grad_(True), d0.clone().requires_grad_(True)
        if fused:
            out = QuantMlpFn.apply(ls.expand_as(ld), ld, *(q for q in net.parameters()))
        else:
            out = net(torch.stack([ls.expand_as(ld), ld], dim=-1)).squeeze(-1)
        out.backward(g)
        assert ls.grad.shape == (rows, 1)
        res.append(R.ratio(ls.grad, ref, den))
    _bounded("quant network autograd d_scale [n,1]", res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# focal rows
# ---------------------------------------------------------------------------------------------------------------------------------
ALPHA = 0.7


@functools.lru_cache(maxsize=None)
def _focal_case(n, strided):
    x, occ_row, keys, q_map = R.focal_inputs(n)
    if strided:
        wide = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev())
        wide[:, 1] = t(x)
        logits = wide[:, 1]
    else:
        logits = t(x)
    occ_row, keys, q_map = t(occ_row), t(keys), t(q_map)
    occ = occ_row >= 0
    w = q_map[:, 0][keys >> R.KEY_B_SHIFT]
    v, kink = R.focal_terms(logits.double(), occ)
    aw = torch.where(occ, torch.full_like(v, ALPHA), torch.full_like(v, 1 - ALPHA)) * w.double()
    return dict(logits=logits, occ_row=occ_row, keys=keys, q_map=q_map, occ=occ, w=w, v=v, kink=kink, aw=aw)


@pytest.mark.parametrize("gamma", [1.0, 1.5, 2.0, 3.0])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_focal_rows_against_float64(n, strided, gamma):
    """`pcc_focal_rows`: f and df over (occupied ? alpha : 1 - alpha) * w, contiguous logits and column 1 of a NaN-filled [n, 3]
    tensor, three batches with a q_map pitch of 2 (the other column NaN), logits out to +-90.  Floor: 4 ulps of the case's
    largest normalised value.  Measured on MI355X: f kernel max 1.1e-8 - 8.8e-6, rms up to 5.7e-7 (float32 torch chain max
    the same, rms up to 6.1e-7; the 8.8e-6 is 1 - p at p near 1, shared); df kernel max 0 - 5.9e-7, rms up to 6.8e-8 (chain max
    0 - 5.9e-7, rms up to 6.3e-8)."""
    L = _L()
    c = _focal_case(n, strided)
    keep = _share(f"focal n={n}", c["kink"])
    f64, df64 = R.focal_grads(c["logits"].double(), c["occ"], c["w"].double(), ALPHA, gamma)
    fy, dfy = R.focal_grads(c["logits"].contiguous(), c["occ"], c["w"], ALPHA, gamma)
    f, df = _out(n), _out(n)
    L.call("pcc_focal_rows", c["logits"].data_ptr(), c["logits"].stride(0), L.ptr(c["occ_row"]), L.ptr(c["keys"]), n,
           L.ptr(c["q_map"]), c["q_map"].stride(0), ALPHA, gamma, f.data_ptr(), df.data_ptr(), L.stream())
    f, df = _take(f, n, "focal f"), _take(df, n, "focal df")
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(df).all())
    what = f"focal n={n} {'stride 3' if strided else 'contiguous'} gamma={gamma}"
    for name, got, yard, ref, kp in (("f", f, fy, f64, None), ("df", df, dfy, df64, keep)):
        top = FLOOR * max(1.0, float((ref.abs() / c["aw"]).max()))
        _bounded(f"{what} {name}", R.ratio(got, ref, c["aw"], kp), R.ratio(yard, ref, c["aw"], kp), (top, top))
    clipped = c["v"] < R.FOCAL_CLIP - 1e-6
    assert bool((df[clipped] == 0).all())
    x = c["logits"]
    one = ((x == 90) & c["occ"]) | ((x == -90) & ~c["occ"])          # p exactly 1 (0): pt == 1, om == 0
    assert bool((f[one] == 0).all()) and bool((df[one] == 0).all())
    if n >= 257:
        assert bool(clipped.any()) and bool(((x == 90) & c["occ"]).any()) and bool(((x == -90) & ~c["occ"]).any())


@pytest.mark.parametrize("strided", [False, True])
def test_focal_level_mean_through_autograd(strided):
    """`FocalRowsFn / n` (one level of `Multiscale_FocalLoss`) and its gradient against the float64 mean; yardstick: the mean of
    the float32 torch chain.  Floor of the mean: 4 ulps of the mean -- both sides are tree sums of 1e5 non-negative float32
    terms, a few ulps either way.  Measured on MI355X: mean kernel 5.2e-8 relative, float32 torch chain 5.2e-8; gradient kernel max 4.8e-7, rms 5.8e-8,
    chain max 4.4e-7, rms 5.3e-8.
    n == 0 is accepted."""
    from unified_point_cloud_compression_amd.autograd import FocalRowsFn
    L = _L()
    n, gamma = 100003, 2.0
    c = _focal_case(n, strided)
    keep = ~c["kink"]
    f64, df64 = R.focal_grads(c["logits"].double(), c["occ"], c["w"].double(), ALPHA, gamma)
    mean64 = float(f64.mean())
    res = []
    for fused in (True, False):
        if strided:
            wide = torch.zeros((n, 3), device=dev())
            wide[:, 1] = c["logits"]
            wide.requires_grad_(True)
            logit = wide[:, 1]
        else:
            wide = logit = c["logits"].clone().requires_grad_(True)
        if fused:
            out = FocalRowsFn.apply(logit, c["occ_row"], c["keys"], c["q_map"], ALPHA, gamma) / n
        else:
            out = R.focal_rows(logit, c["occ"], c["w"], ALPHA, gamma).mean()
        out.backward()
        grad = wide.grad[:, 1] if strided else wide.grad
        res.append((abs(float(out.detach()) - mean64) / mean64, R.ratio(grad * n, df64, c["aw"], keep)))
    print(f"focal level mean stride {3 if strided else 1} [relative]: kernel {res[0][0]:.3e} | float32 torch chain {res[1][0]:.3e}")
    assert res[0][0] <= max(MARGIN * res[1][0], FLOOR)
    _bounded(f"focal level mean stride {3 if strided else 1} gradient", res[0][1], res[1][1])
    L.call("pcc_focal_rows", None, 1, None, None, 0, None, 2, ALPHA, gamma, None, None, L.stream())
