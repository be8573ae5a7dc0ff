"""Float64 references, input generators and metrics of the rate and loss training kernels (`csrc/pcc_entropy.hip`):
the Gaussian likelihood, the factorised prior, the quantisation-offset network and the focal loss rows.  Used by
tests/test_gpu_rate_loss_float64.py (on the GPU) and checked by tests/test_cpu_rate_loss_ref.py (here: no GPU is needed to
import or run anything in this module).

References.  Every formula is restated below with torch operators and evaluated in float64 on whatever device its inputs live
on; nothing calls the library.  The two bounds are the float32 constants of the kernels widened to double (SCALE_BOUND,
LIK_BOUND: `0.11f`, `1e-9f`), and the focal clip is `1e-2f` widened, so that a decision on an exact float32 input (scale >=
0.11f) is the same decision in both precisions.  Gradients are float64 autograd over the restatement with CompressAI's
LowerBound rule (`lower_bound`: the gradient passes when the value is inside the bound or when g < 0).  The functions are
dtype-generic: the same text evaluated on float32 tensors is a plain float32 chain.

Metrics.
  bits_err        |log2 max(got, 1e-9f) - log2 max(ref, 1e-9f)|: the rate is -log2(lik), so this is the error of the rate in bits
                  per symbol.  The floor is continuous: nothing is excluded.
  total_bits      sum(-log2 lik) in float64.
  ratio           |got - ref| / D per element, D the float64 sum of the MAGNITUDES of the terms whose signed sum is the result
                  (cancellation is then judged against what float32 can deliver, not against the near-zero result); an entry with
                  D == 0 must be exactly 0.  D > 0 is taken as D + 2^-103: float32 has no normal numbers below 2^-126, and a result
                  of that size flushed to zero then counts as one ulp, not as a total loss.  Returns (max, rms).
  reduced sums    |got - ref| / S2, S2 = sqrt(sum over the elements of contribution^2) (tests.util.ratios); the per-element
                  contributions come from autograd over PER-ELEMENT copies of the parameters (`eb_grads`, `qm_grads`).

Kinks.  A gradient may jump where float32 can land on the other side of a decision the inputs do not fix exactly: a likelihood
within 1e-4 relative of 1e-9, a ReLU pre-activation within 1e-5 of the sum of its terms' magnitudes, a focal v within 1e-6 of
1e-2.  `*_kinks` return those elements; the tests take them out of the gradient comparisons (for the reduced sums: give them a
zero upstream gradient) and assert that they are at most MAX_KINK_SHARE of the input.
"""
import math

import numpy as np
import torch

SCALE_BOUND = float(np.float32(0.11))
LIK_BOUND = float(np.float32(1e-9))
FOCAL_CLIP = float(np.float32(1e-2))
MAX_KINK_SHARE = 2e-3
ULP = 2.0 ** -23                       # one float32 ulp of 1: the unit of the floors the tests state
UNDERFLOW = 2.0 ** -126 / ULP          # see `ratio`
KEY_B_SHIFT = 48                       # batch field of a packed key (include/pcc_hip.h)
EB_FLAT_CHANNEL = 2                    # the channel of eb_params with softplus(matrices) about 1e-4
EB_ODD_ROWS = slice(5, None, 11)       # rows of eb_inputs with v == 0 in channel 0
QM_SIZES = (20, 10, 100, 10, 10, 1)    # W1 [10][2] | b1 | W2 [10][10] | b2 | W3 [10] | b3 = 151


# ---------------------------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------------------------
class _LowerBoundFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return x.clamp_min(bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.where((x >= ctx.bound) | (g < 0), g, torch.zeros_like(g)), None


def lower_bound(x, bound):
    """max(x, bound) with CompressAI's gradient rule."""
    return _LowerBoundFn.apply(x, bound)


def bits_err(got, ref):
    return (torch.log2(got.double().clamp_min(LIK_BOUND)) - torch.log2(ref.double().clamp_min(LIK_BOUND))).abs()


def total_bits(lik):
    return float(-torch.log2(lik.double()).sum())


def max_rms(err):
    if err.numel() == 0:
        return 0.0, 0.0
    if not bool(torch.isfinite(err).all()):
        return float("inf"), float("inf")
    return float(err.max()), float(torch.sqrt((err * err).mean()))


def ratio(got, ref, denom, keep=None):
    """(max, rms) of |got - ref| / denom over the kept entries; an entry with denom == 0 must be exactly 0 (else: inf)."""
    got, ref, denom = got.double().reshape(-1), ref.double().reshape(-1), denom.double().reshape(-1)
    if keep is not None:
        keep = keep.reshape(-1)
        got, ref, denom = got[keep], ref[keep], denom[keep]
    err = (got - ref).abs()
    on = denom > 0
    if bool(torch.any(~on & (err != 0))) or not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    return max_rms(err[on] / (denom[on] + UNDERFLOW))


def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrays)


# ---------------------------------------------------------------------------------------------------------------------------------
# Gaussian likelihood:  s = max(scale, 0.11), a = |v - mean|, lik = max(Phi((.5 - a)/s) - Phi((-.5 - a)/s), 1e-9)
# ---------------------------------------------------------------------------------------------------------------------------------
def std_cum(x):
    return 0.5 * torch.erfc(-math.sqrt(0.5) * x)


def gauss_raw(v, scale, mean=None):
    s = lower_bound(scale, SCALE_BOUND)
    a = (v if mean is None else v - mean).abs()
    return std_cum((0.5 - a) / s) - std_cum((-0.5 - a) / s)


def gauss_lik(v, scale, mean=None):
    return lower_bound(gauss_raw(v, scale, mean), LIK_BOUND)


def gauss_terms(v, scale, mean=None):
    """The pieces the metrics and the exact-value assertions need, without gradients: s, a, u1, u2, the densities p1, p2, the
    raw likelihood and its two cumulative terms, and dl_ds = (u2 p2 - u1 p1) / s."""
    with torch.no_grad():
        s = scale.clamp_min(SCALE_BOUND)
        a = (v if mean is None else v - mean).abs()
        u1, u2 = (0.5 - a) / s, (-0.5 - a) / s
        c = 1.0 / math.sqrt(2.0 * math.pi)
        p1, p2 = c * torch.exp(-0.5 * u1 * u1), c * torch.exp(-0.5 * u2 * u2)
        up, lo = std_cum(u1), std_cum(u2)
        return dict(s=s, a=a, u1=u1, u2=u2, p1=p1, p2=p2, up=up, lo=lo, raw=up - lo, dl_ds=(u2 * p2 - u1 * p1) / s)


def gauss_grads(v, scale, mean, g):
    """(lik, dv, dscale, dmean) of sum(g * lik) by autograd, in the dtype of the inputs."""
    v, scale, mean = (x.detach().clone().requires_grad_(True) for x in (v, scale, mean))
    lik = gauss_lik(v, scale, mean)
    (lik * g).sum().backward()
    return lik.detach(), v.grad, scale.grad, mean.grad


def gauss_kinks(raw):
    return (raw - LIK_BOUND).abs() <= 1e-4 * LIK_BOUND


def gauss_inputs(n, seed=0):
    """(v, scale, mean, g) float32 [n].  Scales log-uniform in [0.01, 300]; distance a / max(s, 0.11) uniform in [0, 7.5]; every
    64th element plants, in turn: scale == 0.11f, its float32 neighbour below, above, scale == 0, scale < 0, v == mean,
    |v - mean| == 0.5 exactly, a 60-sigma tail.  Upstream gradients of both signs, every 5th exactly 0."""
    rng = np.random.default_rng([n, seed, 11])
    scale = np.exp(rng.uniform(np.log(0.01), np.log(300.0), n)).astype(np.float32)
    mean = rng.standard_normal(n).astype(np.float32)
    dist = rng.uniform(0.0, 7.5, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n).astype(np.float32)
    g[np.arange(n) % 5 == 3] = 0.0
    b = np.float32(0.11)
    slot = (np.arange(n) + (5 if n < 64 else 0)) % 64           # (a single element is an ordinary one)
    plant = {0: b, 1: np.nextafter(b, np.float32(0)), 2: np.nextafter(b, np.float32(1)), 3: np.float32(0), 4: np.float32(-0.3)}
    for k, val in plant.items():
        scale[slot == k] = val
    a = dist * np.maximum(scale, b)
    a[slot == 40] = 0.0
    a[slot == 48] = 60.0 * np.maximum(scale[slot == 48], b)
    half = slot == 56
    mean[half] = np.round(mean[half] * 8) / 8                    # v - mean == +-0.5 exactly in float32
    a[half] = 0.5
    v = (mean.astype(np.float64) + sign * a).astype(np.float32)
    v[slot == 40] = mean[slot == 40]
    return _f32(v, scale, mean, g)


# ---------------------------------------------------------------------------------------------------------------------------------
# factorised prior, filters (3,3,3,3).  packed [c, 58] = softplus(matrices) 3|9|9|9|3, biases 3|3|3|3|1, tanh(factors) 3|3|3|3
# ---------------------------------------------------------------------------------------------------------------------------------
def eb_pack(params):
    """[c, 58] from the 14 raw tensors of a parameter dict (`_matrix{i}` [c, out, in], `_bias{i}`, `_factor{i}` [c, out, 1])."""
    c = params["_matrix0"].shape[0]
    parts = [torch.nn.functional.softplus(params[f"_matrix{i}"]).reshape(c, -1) for i in range(5)]
    parts += [params[f"_bias{i}"].reshape(c, -1) for i in range(5)]
    parts += [torch.tanh(params[f"_factor{i}"]).reshape(c, -1) for i in range(4)]
    return torch.cat(parts, dim=1)


def eb_logits(P, x):
    """Logits of the cumulative at x [n, c]; P [c, 58], or [n, c, 58] for per-element parameter copies."""
    h = x.unsqueeze(-1) * P[..., 0:3] + P[..., 33:36]
    h = h + P[..., 46:49] * torch.tanh(h)
    for l in range(1, 4):
        M = P[..., 3 + 9 * (l - 1):3 + 9 * l].reshape(*P.shape[:-1], 3, 3)                     # [.., out, in]
        a = (M * h.unsqueeze(-2)).sum(-1) + P[..., 33 + 3 * l:36 + 3 * l]
        h = a + P[..., 46 + 3 * l:49 + 3 * l] * torch.tanh(a)
    return (h * P[..., 30:33]).sum(-1) + P[..., 45]


def eb_raw(P, v, P_up=None):
    """P_up: a second copy of the parameters for the upper evaluation (`eb_grads` separates the two terms with it)."""
    lo, up = eb_logits(P, v - 0.5), eb_logits(P if P_up is None else P_up, v + 0.5)
    sg = -torch.sign(lo + up).detach()
    return (torch.sigmoid(sg * up) - torch.sigmoid(sg * lo)).abs()


def eb_lik(P, v, P_up=None):
    return lower_bound(eb_raw(P, v, P_up), LIK_BOUND)


def eb_terms(P, v):
    """(raw, D): raw likelihood and the magnitude sum of the two terms of d lik / d v, |s_u (1 - s_u) up'| + |s_l (1 - s_l) lo'|
    (without the upstream gradient)."""
    xl, xu = (v - 0.5).detach().requires_grad_(True), (v + 0.5).detach().requires_grad_(True)
    lo, up = eb_logits(P.detach(), xl), eb_logits(P.detach(), xu)
    dlo, = torch.autograd.grad(lo.sum(), xl)
    dup, = torch.autograd.grad(up.sum(), xu)
    with torch.no_grad():
        sg = -torch.sign(lo + up)
        su, sl = torch.sigmoid(sg * up), torch.sigmoid(sg * lo)
        return (su - sl).abs(), (su * (1 - su) * dup).abs() + (sl * (1 - sl) * dlo).abs()


def eb_grads(P, v, g):
    """(lik, dv, d_packed [c, 58], S2 [c, 58]) of sum(g * lik): autograd over copies of the packed parameters per element AND
    per evaluation point.  Every element adds two terms to an entry of d_packed, one through the logits at v + 0.5 and one
    through those at v - 0.5, of opposite signs (for the biases of a nearly odd channel they cancel to 1e-3 of their size): the
    kernel and the torch chain both add them one after the other, so S2 runs over the terms, not over their per-element sums."""
    v = v.detach().clone().requires_grad_(True)
    Pl, Pu = (P.detach().unsqueeze(0).expand(v.shape[0], *P.shape).clone().requires_grad_(True) for _ in range(2))
    lik = eb_lik(Pl, v, Pu)
    (lik * g).sum().backward()
    cl, cu = (x.grad if x.grad is not None else torch.zeros_like(x) for x in (Pl, Pu))
    return lik.detach(), v.grad, (cl + cu).sum(0), (cl * cl + cu * cu).sum(0).sqrt()


def eb_params(c, seed=0):
    """Raw parameter dict (numpy float32) of `oracle.entropy.eb_init` plus N(0, 0.3) on every matrix, bias and factor.
    Channel 0: all biases exactly 0 (the logits are an odd function: v == 0 gives lo == -up, sg == 0, likelihood on the floor).
    With c >= 3, channel 1: factors pushed to tanh saturation (+-6); channel 2: raw matrices at -9 (softplus about 1e-4)."""
    from oracle import entropy as en
    rng = np.random.default_rng([c, seed, 12])
    p = en.eb_init(c, seed=seed)
    for i in range(5):
        for name in (f"_matrix{i}", f"_bias{i}") + ((f"_factor{i}",) if i < 4 else ()):
            p[name] = (p[name] + rng.normal(0, 0.3, p[name].shape)).astype(np.float32)
        p[f"_bias{i}"][0] = 0.0
        if c >= 3:
            if i < 4:
                p[f"_factor{i}"][1] = np.where(rng.random(p[f"_factor{i}"][1].shape) < 0.5, -6.0, 6.0)
            p[f"_matrix{i}"][2] = -9.0 + rng.normal(0, 0.3, p[f"_matrix{i}"][2].shape)
    p.pop("quantiles")
    return {k: np.ascontiguousarray(a, np.float32) for k, a in p.items()}


def eb_inputs(n, c, seed=0):
    """(v, g) float32 [n, c]: v = N(0, 6), every 7th row x 40 (far tails: the floor), every 11th row (EB_ODD_ROWS) exactly 0 in
    channel 0."""
    rng = np.random.default_rng([n, c, seed, 13])
    v = rng.standard_normal((n, c)) * 6.0
    v[3::7] *= 40.0
    v[EB_ODD_ROWS, 0] = 0.0
    g = rng.standard_normal((n, c))
    g[rng.random((n, c)) < 0.1] = 0.0
    return _f32(v, g)


# ---------------------------------------------------------------------------------------------------------------------------------
# quantisation-offset network: 2 -> 10 -> 10 -> 1, ReLU.  params [151] (or [n, 151]: one copy per element) in the layout above
# ---------------------------------------------------------------------------------------------------------------------------------
def _qm_split(p):
    parts, at = [], 0
    for k in QM_SIZES:
        parts.append(p[..., at:at + k])
        at += k
    W1, b1, W2, b2, W3, b3 = parts
    return W1.reshape(*p.shape[:-1], 10, 2), b1, W2.reshape(*p.shape[:-1], 10, 10), b2, W3, b3[..., 0]


def qm_forward(p, s, d, terms=False):
    """Offsets [n] of (scale, stddev) pairs [n].  terms=True: also the pre-activations and the magnitude sums of their terms."""
    W1, b1, W2, b2, W3, b3 = _qm_split(p)
    t1s, t1d = W1[..., 0] * s.unsqueeze(-1), W1[..., 1] * d.unsqueeze(-1)
    a1 = t1s + t1d + b1
    h1 = torch.relu(a1)
    t2 = W2 * h1.unsqueeze(-2)
    a2 = t2.sum(-1) + b2
    h2 = torch.relu(a2)
    t3 = W3 * h2
    out = t3.sum(-1) + b3
    if not terms:
        return out
    m1 = t1s.abs() + t1d.abs() + b1.abs()
    m2 = t2.abs().sum(-1) + b2.abs()
    return out, dict(a1=a1, a2=a2, m1=m1, m2=m2, m_out=t3.abs().sum(-1) + b3.abs())


def qm_terms(p, s, d):
    """(kink [n], D_out [n], D_scale [n], D_stddev [n], off1, off2): kink -- some ReLU pre-activation within 1e-5 of the sum of
    its terms' magnitudes; D_* the magnitude sums of the forward result and of the two input derivatives (per unit upstream
    gradient); off1 / off2 the share of hidden units that are off in each layer."""
    with torch.no_grad():
        W1, _, W2, _, W3, _ = _qm_split(p)
        _, tm = qm_forward(p, s, d, terms=True)
        kink = ((tm["a1"].abs() <= 1e-5 * tm["m1"]).any(-1)) | ((tm["a2"].abs() <= 1e-5 * tm["m2"]).any(-1))
        on1, on2 = (tm["a1"] > 0).to(p.dtype), (tm["a2"] > 0).to(p.dtype)
        back = (on2 * W3.abs()) @ W2.abs() * on1                                             # [n, 10]: sum_j |w3_j| |W2_ji|
        return (kink, tm["m_out"], back @ W1[:, 0].abs(), back @ W1[:, 1].abs(),
                float(1 - on1.mean()), float(1 - on2.mean()))


def qm_grads(p, s, d, gs, chunk=1 << 17):
    """(out, d_scale, d_stddev, [(d_params [151], S2 [151]) for g in gs]): autograd of sum(out) over one copy of the 151
    parameters per element, `chunk` elements at a time.  The network is linear in its upstream gradient, so d_scale and
    d_stddev are per UNIT gradient (times g for the real ones), and every g of `gs` weighs the same per-element contributions."""
    n = s.shape[0]
    out, ds, dd = (torch.empty_like(s) for _ in range(3))
    sums = [(torch.zeros_like(p), torch.zeros_like(p)) for _ in gs]
    for at in range(0, n, chunk):
        sl = slice(at, min(at + chunk, n))
        sc, dc = s[sl].detach().clone().requires_grad_(True), d[sl].detach().clone().requires_grad_(True)
        pe = p.detach().unsqueeze(0).expand(sc.shape[0], -1).clone().requires_grad_(True)
        o = qm_forward(pe, sc, dc)
        o.sum().backward()
        out[sl], ds[sl], dd[sl] = o.detach(), sc.grad, dc.grad
        for g, (dp, sq) in zip(gs, sums):
            c = pe.grad * g[sl].unsqueeze(-1)
            dp += c.sum(0)
            sq += (c * c).sum(0)
    return out, ds, dd, [(dp, sq.sqrt()) for dp, sq in sums]


def qm_params(seed=3):
    """[151] float32: torch.nn.Linear initial values of the three layers (uniform +-1/sqrt(fan_in)) x 2, as the existing test of
    the network scales them."""
    rng = np.random.default_rng([seed, 14])
    fan = (2, 2, 10, 10, 10, 10)
    return np.concatenate([2.0 * rng.uniform(-1, 1, k) / math.sqrt(f) for k, f in zip(QM_SIZES, fan)]).astype(np.float32)


def qm_inputs(n, seed=0):
    """(scale in [0.2, 3], stddev in [0.1, 9], g ~ N(0, 1) with every 9th exactly 0) float32 [n]."""
    rng = np.random.default_rng([n, seed, 15])
    g = rng.standard_normal(n)
    g[np.arange(n) % 9 == 4] = 0.0
    return _f32(rng.uniform(0.2, 3.0, n), rng.uniform(0.1, 9.0, n), g)


# ---------------------------------------------------------------------------------------------------------------------------------
# focal rows:  p = sigmoid(x), v = occ ? p : 1 - p, pt = clip(v, 1e-2, 1), f = -(occ ? alpha : 1 - alpha) (1 - pt)^gamma log(pt) w
# ---------------------------------------------------------------------------------------------------------------------------------
def focal_rows(x, occ, w, alpha, gamma):
    """f [n] (the operator sequence of the torch chain in `loss.Multiscale_FocalLoss`, in the dtype of x)."""
    p = torch.sigmoid(x)
    pt = torch.clip(torch.where(occ, p, 1 - p), FOCAL_CLIP, 1)
    alpha = float(np.float32(alpha))                             # the kernel's argument is a float
    a = torch.where(occ, torch.full_like(x, alpha), torch.full_like(x, 1 - alpha))
    return -a * (1 - pt) ** gamma * torch.log(pt) * w


def focal_grads(x, occ, w, alpha, gamma):
    """(f, df / dx) by autograd."""
    x = x.detach().clone().requires_grad_(True)
    f = focal_rows(x, occ, w, alpha, gamma)
    f.sum().backward()
    return f.detach(), x.grad


def focal_terms(x, occ):
    """(v, kink): v in float64 and the rows within 1e-6 of the clip."""
    with torch.no_grad():
        p = torch.sigmoid(x)
        v = torch.where(occ, p, 1 - p)
        return v, (v - FOCAL_CLIP).abs() <= 1e-6


def focal_inputs(n, seed=0):
    """(logits float32 [n], occ_row int32 [n] (>= 0: occupied), keys int64 [n] with three batches in the batch field, q_map
    float32 [3, 2] with NaN in the column the kernel must not read).  Logits N(0, 4); every 16th row plants, in turn, +-20 and +-90 (p exactly 0
    or 1); n // 1000 rows (at most 96) plant +-ln 99 (the clip) and its float32 neighbours on both sides -- float32 may land on
    either side of the clip on each of them, so they count as kinks and their number is kept under the share the tests allow."""
    rng = np.random.default_rng([n, seed, 16])
    x = (rng.standard_normal(n) * 4.0).astype(np.float32)
    ln99 = np.float32(math.log(99.0))
    occ = rng.random(n) < 0.4
    slot = (np.arange(n) + (13 if n < 16 else 0)) % 16
    far = np.nonzero(slot == 0)[0]                               # +-20, +-90, each on occupied and on empty rows
    x[far] = np.array([20, 90, -20, -90], np.float32)[np.arange(len(far)) % 4]
    occ[far] = (np.arange(len(far)) // 4) % 2 == 0
    clip = [ln99, np.nextafter(ln99, np.float32(0)), np.nextafter(ln99, np.float32(9))]
    clip = np.array(clip + [-u for u in clip], np.float32)
    at = np.nonzero(slot == 8)[0][:min(n // 1000, 96)]           # every one of them is a kink: at most 0.1 % of the rows
    x[at] = clip[np.arange(len(at)) % 6]
    occ[at] = (np.arange(len(at)) // 6) % 2 == 0
    occ_row = np.where(occ, rng.integers(0, 1 << 20, n), -1).astype(np.int32)
    keys = (np.sort(rng.integers(0, 3, n)).astype(np.int64) << KEY_B_SHIFT) | rng.integers(0, 1 << 40, n).astype(np.int64)
    q_map = np.array([[0.3, np.nan], [2.0, np.nan], [0.7, np.nan]], dtype=np.float32)
    return x, occ_row, keys, q_map
