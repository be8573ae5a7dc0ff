"""The float64 references and input generators of tests/rate_loss_ref.py, checked without a GPU: every restated formula against
`math.erfc` / `math.tanh` / `math.exp` evaluated element by element (1e-13 relative, about 2 000 samples per formula), the
LowerBound rule on both signs of the upstream gradient, and the share conditions the GPU tests rely on (elements on the
likelihood floor, hidden units that are off, elements excluded as kinks).  Each generator's floor share and excluded share is
printed (run with -s)."""
import math

import numpy as np
import torch

from tests import rate_loss_ref as R

N_SAMPLES = 2000
REL = 1e-13


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _sigmoid(x):
    if x >= 0:
        return 1.0 / (1.0 + math.exp(-x))
    e = math.exp(x)
    return e / (1.0 + e)


def _phi(x):
    return 0.5 * math.erfc(-math.sqrt(0.5) * x)


def test_gaussian_reference_equals_math_erfc_element_by_element():
    v, s, m, _ = R.gauss_inputs(N_SAMPLES, seed=1)
    got = R.gauss_lik(_d(v), _d(s), _d(m)).numpy()
    want = []
    for vi, si, mi in zip(v.astype(np.float64), s.astype(np.float64), m.astype(np.float64)):
        sb, a = max(si, R.SCALE_BOUND), abs(vi - mi)
        want.append(max(_phi((0.5 - a) / sb) - _phi((-0.5 - a) / sb), R.LIK_BOUND))
    assert _rel(got, want) <= REL
    assert R.SCALE_BOUND == float(np.float32(0.11)) and R.LIK_BOUND == float(np.float32(1e-9)) and R.SCALE_BOUND != 0.11


def test_gaussian_gradients_follow_the_lower_bound_rule_on_both_signs():
    v, s, m, g = R.gauss_inputs(N_SAMPLES, seed=2)
    v, s, m, g = _d(v), _d(s), _d(m), _d(g)
    lik, dv, ds, dm = R.gauss_grads(v, s, m, g)
    tm = R.gauss_terms(v, s, m)
    passes = (tm["raw"] >= R.LIK_BOUND) | (g < 0)
    gl = torch.where(passes, g, torch.zeros_like(g))
    want_dv = gl * (tm["p2"] - tm["p1"]) / tm["s"] * torch.sign(v - m)
    gs = gl * tm["dl_ds"]
    want_ds = torch.where((s >= R.SCALE_BOUND) | (gs < 0), gs, torch.zeros_like(gs))
    scale = float(dv.abs().max())
    assert float((dv - want_dv).abs().max()) <= 1e-12 * scale and torch.equal(dm, -dv)
    assert float((ds - want_ds).abs().max()) <= 1e-12 * float(ds.abs().max())
    floor = tm["raw"] < R.LIK_BOUND
    assert bool((floor & (g < 0) & (dv != 0)).any()) and bool((dv[floor & (g >= 0)] == 0).all())       # both branches on the floor
    low = s < R.SCALE_BOUND
    assert bool((low & (ds != 0)).any()) and bool((low & (ds == 0) & (g != 0)).any())                  # both branches below 0.11


def test_gaussian_generator_meets_its_share_conditions():
    for n in (1, 255, 256, 257, 200003):
        v, s, m, g = R.gauss_inputs(n)
        assert v.dtype == s.dtype == m.dtype == g.dtype == np.float32 and len(v) == n
        tm = R.gauss_terms(_d(v), _d(s), _d(m))
        floor = float((tm["raw"] < R.LIK_BOUND).double().mean())
        kinks = float(R.gauss_kinks(tm["raw"]).double().mean())
        print(f"gauss n={n}: floor share {floor:.4%}, excluded share {kinks:.4%}")
        assert kinks <= R.MAX_KINK_SHARE
        if n < 255:
            continue
        assert floor >= 0.05
        b = np.float32(0.11)
        for val in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1)), np.float32(0), np.float32(-0.3)):
            assert (s == val).any()
        assert (v == m).any() and (np.abs(v - m) == np.float32(0.5)).any() and (g == 0).any() and (g > 0).any() and (g < 0).any()
        assert float(s.min()) < 0.011 and float(s.max()) > 250 and float((tm["a"] / tm["s"]).max()) >= 59
        assert bool(((tm["raw"] < R.LIK_BOUND) & _d(g).lt(0)).any()) and bool(((tm["raw"] < R.LIK_BOUND) & _d(g).gt(0)).any())


def _eb_math(P, x):
    m0, Ms, m4, b, f = P[0:3], P[3:30], P[30:33], P[33:46], P[46:58]
    h = [m0[i] * x + b[i] for i in range(3)]
    h = [h[i] + f[i] * math.tanh(h[i]) for i in range(3)]
    for l in range(1, 4):
        M = Ms[9 * (l - 1):9 * l]
        a = [M[o * 3] * h[0] + M[o * 3 + 1] * h[1] + M[o * 3 + 2] * h[2] + b[3 * l + o] for o in range(3)]
        h = [a[o] + f[3 * l + o] * math.tanh(a[o]) for o in range(3)]
    return m4[0] * h[0] + m4[1] * h[1] + m4[2] * h[2] + b[12]


def test_factorised_prior_reference_equals_math_tanh_and_exp_element_by_element():
    n, c = 84, 24
    P = R.eb_pack({k: _d(a) for k, a in R.eb_params(c).items()})
    v, _ = R.eb_inputs(n, c)
    got_lo = R.eb_logits(P, _d(v) - 0.5).numpy()
    got = R.eb_lik(P, _d(v)).numpy()
    Pn = P.numpy()
    want, want_lo = np.zeros((n, c)), np.zeros((n, c))
    for r in range(n):
        for ch in range(c):
            x = float(v[r, ch])
            lo, up = _eb_math(Pn[ch], x - 0.5), _eb_math(Pn[ch], x + 0.5)
            sg = -float(np.sign(lo + up))
            want_lo[r, ch] = lo
            want[r, ch] = max(abs(_sigmoid(sg * up) - _sigmoid(sg * lo)), R.LIK_BOUND)
    assert n * c >= N_SAMPLES
    assert _rel(got_lo, want_lo) <= REL
    assert _rel(got, want) <= REL


def test_factorised_prior_generator_meets_its_share_conditions():
    for n, c in ((1, 1), (255, 3), (257, 24), (1000, 24), (900, 192)):
        params = {k: _d(a) for k, a in R.eb_params(c).items()}
        P32 = R.eb_pack({k: a.float() for k, a in params.items()}).double()     # what the kernel is handed
        v, g = R.eb_inputs(n, c)
        raw = R.eb_raw(P32, _d(v))
        floor = float((raw < R.LIK_BOUND).double().mean())
        kinks = float(R.gauss_kinks(raw).double().mean())
        print(f"eb n={n} c={c}: floor share {floor:.4%}, excluded share {kinks:.4%}")
        assert kinks <= R.MAX_KINK_SHARE
        odd = raw[R.EB_ODD_ROWS, 0]
        assert bool((odd == 0).all())                                            # lo == -up: sg == 0, raw likelihood exactly 0
        raw32 = R.eb_raw(P32.float(), torch.from_numpy(v))
        assert bool((raw32[R.EB_ODD_ROWS, 0] == 0).all())                                 # ... in float32 as well
        if n >= 255:
            assert floor >= 0.03
        if c >= 3:
            assert float(P32[1, 46:58].abs().min()) > 0.9999 and float(P32[2, 0:33].max()) < 1e-3
            assert bool((P32[0, 33:46] == 0).all())


def test_quant_network_reference_equals_plain_arithmetic_and_its_generator_keeps_units_on_both_sides():
    p = _d(R.qm_params())
    assert p.numel() == 151
    s, d, g = R.qm_inputs(N_SAMPLES)
    got = R.qm_forward(p, _d(s), _d(d)).numpy()
    q = p.numpy()
    want = []
    for si, di in zip(s.astype(np.float64), d.astype(np.float64)):
        h1 = [max(q[2 * j] * si + q[2 * j + 1] * di + q[20 + j], 0.0) for j in range(10)]
        h2 = [max(sum(q[30 + 10 * j + i] * h1[i] for i in range(10)) + q[130 + j], 0.0) for j in range(10)]
        want.append(sum(q[140 + j] * h2[j] for j in range(10)) + q[150])
    assert float(np.max(np.abs(got - np.array(want)))) <= REL * float(np.max(np.abs(want)))
    # per-element parameter copies give the same gradients as one shared copy
    out, ds, dd, ((dp, s2), (dp_pos, s2_pos)) = R.qm_grads(p, _d(s), _d(d), [_d(g), _d(g).abs()], chunk=700)
    pl = p.clone().requires_grad_(True)
    sl, dl = _d(s).requires_grad_(True), _d(d).requires_grad_(True)
    (R.qm_forward(pl, sl, dl) * _d(g)).sum().backward()
    assert float((dp - pl.grad).abs().max()) <= 1e-12 * float(pl.grad.abs().max()) and torch.equal(s2, s2_pos)
    assert float((ds * _d(g) - sl.grad).abs().max()) <= 1e-12 and float((dd * _d(g) - dl.grad).abs().max()) <= 1e-12
    assert bool((dp_pos.abs() <= s2 * math.sqrt(N_SAMPLES) * (1 + 1e-12)).all())
    for n in (257, 1024 * 1024 + 1025):
        s, d, _ = R.qm_inputs(n)
        kink, _, _, _, off1, off2 = R.qm_terms(p, _d(s), _d(d))
        share = float(kink.double().mean())
        print(f"quant network n={n}: units off {off1:.1%} / {off2:.1%}, excluded share {share:.4%}")
        assert 0.1 <= off1 <= 0.9 and 0.1 <= off2 <= 0.9 and share <= R.MAX_KINK_SHARE


def test_focal_reference_equals_math_and_its_generator_reaches_every_planted_edge():
    x, occ_row, keys, q_map = R.focal_inputs(N_SAMPLES)
    occ = torch.from_numpy(occ_row >= 0)
    w = _d(q_map[:, 0])[torch.from_numpy(keys >> R.KEY_B_SHIFT)]
    al = float(np.float32(0.7))
    for gamma in (1.0, 1.5, 2.0, 3.0):
        got = R.focal_rows(_d(x), occ, w, 0.7, gamma).numpy()
        want = []
        for xi, oi, wi in zip(x.astype(np.float64), occ.numpy(), w.numpy()):
            p = _sigmoid(xi)
            pt = min(max(p if oi else 1.0 - p, R.FOCAL_CLIP), 1.0)
            want.append(-(al if oi else 1 - al) * (1.0 - pt) ** gamma * math.log(pt) * wi)
        assert float(np.max(np.abs(got - np.array(want)))) <= REL * float(np.max(np.abs(want)))
        f, df = R.focal_grads(_d(x), occ, w, 0.7, gamma)
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(df).all())
    for n in (1, 257, 100003):
        x, occ_row, keys, q_map = R.focal_inputs(n)
        occ = torch.from_numpy(occ_row >= 0)
        v, kink = R.focal_terms(_d(x), occ)
        share = float(kink.double().mean())
        print(f"focal n={n}: clipped share {float((v < R.FOCAL_CLIP).double().mean()):.4%}, excluded share {share:.4%}")
        assert set(np.unique(keys >> R.KEY_B_SHIFT)) <= {0, 1, 2} and np.isnan(q_map[:, 1]).all()
        if n < 257:
            continue
        assert share <= R.MAX_KINK_SHARE and (n < 1000 or bool(kink.any()))                  # the planted +-ln 99 rows are the kinks
        assert set(np.unique(keys >> R.KEY_B_SHIFT)) == {0, 1, 2}
        assert bool(((v == 1) & occ).any()) and bool(((v == 1) & ~occ).any())      # pt == 1 (om == 0) on both kinds of row
        assert bool(((v < R.FOCAL_CLIP - 1e-6) & occ).any()) and bool(((v < R.FOCAL_CLIP - 1e-6) & ~occ).any())
        assert (np.abs(x) == 90).any() and (np.abs(x) == 20).any()
