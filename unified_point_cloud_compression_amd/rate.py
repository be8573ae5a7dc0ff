"""Rate of the latents for many quality points at once.

The codec is variable-rate: one set of weights, a quality pair q = (q_g, q_a) chosen at encode time, and q reaches the
encoder through one gain row only (`MeanScaleHyperprior._gains`).  `sweep_bits` is the host side of `pcc_gauss_rate_sweep`:
the exact integer payload estimate of y (`pcc_rans_estimate_bits`, 1/256 bit) for K gain rows from one pass over y and its
parameter rows.  `predicted_bytes` turns estimates into string sizes with the stream container's framing, `choose` picks the
candidate for a byte budget.  `UnifiedModel.compress_multirate / rate_map / compress_to_size` are built on these.
"""
import numpy as np
import torch

from . import lib as L

MAX_CANDIDATES = 256      # pcc_gauss_rate_sweep takes up to this many gain rows per launch


def q_grid(steps=11):
    """The [steps^2, 2] float32 quality pairs of the reference's evaluation grid (`evaluate.py:76-77`): q_g and q_a each run
    over i / (steps - 1), i = 0 .. steps - 1 (0.0, 0.1, .., 1.0 for 11 steps), q_g major."""
    steps = int(steps)
    if steps < 1:
        raise L.PccError("q_grid: at least one step")
    v = np.arange(steps) * (1.0 / (steps - 1) if steps > 1 else 0.0)      # (11 steps: np.arange(11) * 0.1)
    g, a = np.meshgrid(v, v, indexing="ij")
    return np.stack([g.reshape(-1), a.reshape(-1)], axis=1).astype(np.float32)


def sweep_bits(gaussian_conditional, y_rows, params, gains, cset=None):
    """int64 [K] device tensor: the payload estimate of y [n, c] with parameter rows params [n, 2c] = (scales | means) under
    each gain row of gains [K, c] -- for every k exactly what `encode_rows(y, params, keys, gains[k:k+1])` followed by
    `rans.estimate` on its symbols and table rows gives.  One launch, nothing read back.  Every gain row is applied to ALL
    rows of y, as `compress` does with its one q: a coordinate set `cset` with rows outside batch 0 is refused."""
    if cset is not None and cset.bounds.bmax > 0:
        raise L.PccError("sweep_bits: the rows span more than one batch id; a gain row applies to one batch (batch 0), as in compress")
    y_rows, params, gains = y_rows.contiguous(), params.contiguous(), gains.to(torch.float32).contiguous()
    n, c = params.shape[0], params.shape[1] // 2
    if gains.dim() != 2 or gains.shape[1] != c or tuple(y_rows.shape) != (n, c) or params.shape[1] != 2 * c:
        raise L.PccError(f"sweep_bits: y {tuple(y_rows.shape)}, params {tuple(params.shape)}, gains {tuple(gains.shape)} do not fit")
    K = gains.shape[0]
    dev = params.device
    tabs = gaussian_conditional.tables(dev)
    tab = gaussian_conditional._table(dev)
    if tabs.sizes.numel() < tab.numel():
        raise L.PccError("sweep_bits: fewer rANS table rows than scale-table entries")
    out = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
    L.call("pcc_gauss_rate_sweep", L.ptr(y_rows), L.ptr(params), n, c, L.ptr(gains), K, L.ptr(tab), tab.numel(), L.ptr(tabs.cdf),
           tabs.cdf.shape[1], L.ptr(tabs.sizes), L.ptr(tabs.offsets), L.ptr(out), L.stream())
    return out[:K]


def stream_count(em, n, c, bits256):
    """Streams of the container `StreamsJob` writes for an [n, c] symbol matrix whose payload estimate is bits256."""
    ng, segs = em.n_streams(n, c)
    if em.FRAMING_TARGET > 0 and n * c >= em.ADAPTIVE_MIN_SYMBOLS:
        segs = em._adaptive_segments(n, c, ng, segs, int(bits256) / 2048.0)
    return ng * segs


def predicted_bytes(em, n, c, bits256):
    """Predicted length of the string of an [n, c] symbol matrix from its payload estimate: ceil(bits256 / 2048) bytes of
    payload plus the framing of the stream plan that estimate implies, 4 bytes + 12 per stream (entropy coder "pcc_streams";
    the single host stream of "ans" has no container: payload alone)."""
    payload = -(-int(bits256) // 2048)
    if em.entropy_coder != "pcc_streams":
        return payload
    return payload + 4 + 12 * stream_count(em, n, c, bits256)


def choose(predicted, max_bytes, exclude=()):
    """(index, fits): the candidate with the largest prediction not above max_bytes (fits = True), ties to the earlier
    index; when none is, the one with the smallest prediction, ties to the earlier index, and fits = False.  Indices in
    `exclude` are not considered; (None, False) when nothing is left.  Pure host; nothing is assumed about how the
    predictions are ordered."""
    skip = set(int(i) for i in exclude)
    best, small = None, None
    for i, p in enumerate(predicted):
        if i in skip:
            continue
        if p <= max_bytes and (best is None or p > predicted[best]):
            best = i
        if small is None or p < predicted[small]:
            small = i
    if best is not None:
        return best, True
    return small, False
