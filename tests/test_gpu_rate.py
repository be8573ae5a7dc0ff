"""GPU suite of the multi-rate / rate-targeted encoding.

Kernel: `pcc_gauss_rate_sweep` against the two-step route it replaces, `pcc_gauss_encode` with one gain row followed by
`pcc_rans_estimate_bits` on its symbols and table rows -- int64 results, exact equality.  Codec: `compress_multirate`,
`rate_map` and `compress_to_size` against `compress` called once per quality point -- byte equality, integer equality, and
real sizes by brute force.  Nothing here assumes that rate is monotone in q (with random weights it is not)."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import codec
from tests.util import dev, t, n as to_np, load_params, coord_set, cloud_keys

pytestmark = pytest.mark.gpu

C_SMALL = codec.small_config()["entropy_model"]["C_bottleneck"]
SHAPES = [(3, 8), (31, 8), (32, 8), (33, 8), (257, C_SMALL)]      # below a wave; around 256 elements; several passes of a workgroup
ROW_TINY, ROW_ONE, ROW_LARGE, ROW_TIE = 0, 1, 2, 3
TIE_GAIN = np.float32(1.2345678)                                  # 0x3f9e0651: a full mantissa


@functools.lru_cache(maxsize=None)
def _gc():
    from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional, get_scale_table
    gc = GaussianConditional(None).to(dev())
    gc.update_scale_table(get_scale_table())
    return gc


def _gain_rows(c, K=256):
    """[K, c] float32: row 0 tiny (every scale clamps to 0.11: table row 0), row 1 ones, row 2 large (symbols leave the support
    of their rows), row 3 one full-mantissa value (the tie row), the rest log-uniform with full mantissas per channel."""
    rng = np.random.default_rng(7)
    g = np.exp(rng.uniform(-3.0, 5.0, (K, c))).astype(np.float32)
    g[ROW_TINY], g[ROW_ONE], g[ROW_LARGE], g[ROW_TIE] = 1e-6, 1.0, 300.0, TIE_GAIN
    return g


def _inputs(n, c, seed=0):
    """y [n, c] and params [n, 2c] = (scales | means): scales from far below the bound to above the table, |y - mean| often far
    above 6 scales (escapes)."""
    rng = np.random.default_rng(seed + 100 * n + c)
    scales = np.exp(rng.uniform(np.log(0.005), np.log(400.0), (n, c)))
    means = rng.normal(0, 2.0, (n, c))
    y = means + rng.normal(0, 1.0, (n, c)) * np.where(rng.random((n, c)) < 0.3, 3.0, scales)
    return y.astype(np.float32), np.concatenate([scales, means], axis=1).astype(np.float32)


def _tie_inputs(n, c):
    """y and means with y*g - mean*g next to a half-integer for g = TIE_GAIN: small magnitudes, so that one rounding of y
    (<= 2^-23 relative) leaves the difference within ~2^-22 of the tie."""
    rng = np.random.default_rng(11)
    g = np.float64(TIE_GAIN)
    means = rng.uniform(-1, 1, (n, c)).astype(np.float32)
    half = rng.integers(-3, 3, (n, c)) + 0.5
    mg = (means * TIE_GAIN).astype(np.float32).astype(np.float64)           # mean*g as the kernels round it
    y = ((half + mg) / g).astype(np.float32)
    scales = np.exp(rng.uniform(np.log(0.05), np.log(20.0), (n, c))).astype(np.float32)
    return y, np.concatenate([scales, means], axis=1).astype(np.float32)


def _two_step(y, params, gains):
    """The route the sweep replaces, one gain row at a time -> (int64 [K] numpy, symbols and table rows per k on request)."""
    from unified_point_cloud_compression_amd import rans as R
    gc = _gc()
    tabs = gc.tables(dev())
    keys = torch.zeros(max(y.shape[0], 1), dtype=torch.int64, device=dev())          # batch 0
    out = torch.zeros(gains.shape[0], dtype=torch.int64, device=dev())
    kept = {}
    for k in range(gains.shape[0]):
        sym, idx, _ = gc.encode_rows(y, params, keys, gains[k:k + 1], want_likelihood=False)
        R.estimate(tabs, sym, idx, out.data_ptr() + 8 * k)
        if k < 4:
            kept[k] = (to_np(sym), to_np(idx))
    return to_np(out), kept


@functools.lru_cache(maxsize=None)
def _case(n, c, tie=False):
    """(y, params, gains [256, c], reference bits [256], kept symbols) -- computed once per shape, shared, never changed."""
    y, params = _tie_inputs(n, c) if tie else _inputs(n, c)
    y, params, gains = t(y), t(params), t(_gain_rows(c))
    ref, kept = _two_step(y, params, gains)
    return y, params, gains, ref, kept


def _sweep(y, params, gains, cset=None):
    from unified_point_cloud_compression_amd import rate
    return to_np(rate.sweep_bits(_gc(), y, params, gains, cset))


@pytest.mark.parametrize("K", [1, 2, 17, 121, 256])
@pytest.mark.parametrize("n,c", SHAPES)
def test_sweep_equals_two_step_route(n, c, K):
    y, params, gains, ref, _ = _case(n, c)
    got = _sweep(y, params, gains[:K].contiguous())
    assert got.dtype == np.int64 and got.shape == (K,)
    assert np.array_equal(got, ref[:K]), (got[:8], ref[:8])
    assert (ref[1:K] > 0).all()          # (row 0, the tiny gain: every symbol is 0 at a frequency near 2^16, next to no bits)


def test_gain_regimes_are_exercised():
    """On the reference route's own symbols: the tiny gain clamps every scale to table row 0; the large gain sends many symbols
    outside the support of their rows (the escape / bypass-digit term), and so does gain one."""
    gc = _gc()
    sizes, offsets = to_np(gc._cdf_length), to_np(gc._offset)
    _, _, _, ref, kept = _case(257, C_SMALL)
    sym, idx = kept[ROW_TINY]
    assert idx.max() <= 1 and len(np.unique(idx)) == 1        # s = 0.11 for every element: the bottom of the table (its first
    #                                                           entry is exp(log 0.11), a rounding away from 0.11 either way)
    for row in (ROW_ONE, ROW_LARGE):
        sym, idx = kept[row]
        v = sym - offsets[idx]
        esc = (v < 0) | (v >= sizes[idx] - 2)
        assert esc.sum() > 500, (row, int(esc.sum()))
        assert len(np.unique(idx)) > 8
    sym, _ = kept[ROW_LARGE]
    assert np.abs(sym).max() > 256                               # more than one bypass digit pair


def test_ties_at_half_integers():
    """y*g - mean*g within 2^-20 of a half-integer for thousands of elements: a sweep that contracted the expression another
    way than k_gauss (two rounded products and a subtraction, say) rounds many of them to the other neighbour."""
    n, c = 257, C_SMALL
    y, params, gains, ref, kept = _case(n, c, True)
    d = to_np(y).astype(np.float64) * np.float64(TIE_GAIN) - to_np(params)[:, c:].astype(np.float64) * np.float64(TIE_GAIN)
    near = np.abs(np.abs(d - np.floor(d)) - 0.5) < 2.0 ** -20
    assert near.sum() >= 100, int(near.sum())
    # the case is not vacuous: the separately rounded form would give other symbols on this data
    yg = (to_np(y) * TIE_GAIN).astype(np.float32)
    mg = (to_np(params)[:, c:] * TIE_GAIN).astype(np.float32)
    assert (np.rint(yg - mg).astype(np.int32) != kept[ROW_TIE][0]).sum() >= 100
    got = _sweep(y, params, gains[:17].contiguous())
    assert np.array_equal(got, ref[:17]), (got[:8], ref[:8])


def test_two_calls_give_equal_bits():
    y, params, gains, ref, _ = _case(257, C_SMALL)
    a, b = _sweep(y, params, gains), _sweep(y, params, gains)
    assert np.array_equal(a, b) and np.array_equal(a, ref)


def test_no_rows_zeroes_the_outputs():
    from unified_point_cloud_compression_amd import lib as L
    gc = _gc()
    tabs, tab = gc.tables(dev()), gc._table(dev())
    gains = t(_gain_rows(8)[:5])
    out = torch.full((6,), 77, dtype=torch.int64, device=dev())
    L.call("pcc_gauss_rate_sweep", None, None, 0, 8, L.ptr(gains), 5, L.ptr(tab), tab.numel(), L.ptr(tabs.cdf), tabs.cdf.shape[1],
           L.ptr(tabs.sizes), L.ptr(tabs.offsets), L.ptr(out), L.stream())
    assert out.tolist() == [0, 0, 0, 0, 0, 77]
    empty = _sweep(torch.empty((0, 8), device=dev()), torch.empty((0, 16), device=dev()), gains)
    assert empty.tolist() == [0] * 5


def test_refusals():
    from unified_point_cloud_compression_amd import lib as L
    y, params, gains, _, _ = _case(33, 8)
    with pytest.raises(L.PccError, match="candidates"):
        _sweep(y, params, gains[:0].contiguous())
    with pytest.raises(L.PccError, match="candidates"):
        _sweep(y, params, torch.cat([gains, gains[:1]]))
    keys = cloud_keys(1, 8, 0.3, ts=8, batch=2)                  # rows of batches 0 and 1
    cs = coord_set(keys, 8)
    yb, pb = torch.zeros((cs.n, 8), device=dev()), torch.ones((cs.n, 16), device=dev())
    with pytest.raises(L.PccError, match="batch"):
        _sweep(yb, pb, gains[:2].contiguous(), cs)
    with pytest.raises(L.PccError, match="do not fit"):
        _sweep(y, params, torch.ones((2, 9), device=dev()))


# ---- codec ---------------------------------------------------------------------------------------------------------------
SEED = 2
PAIR = [0.3 + 0.2 * SEED, 0.6]                                   # the pair test_gpu_codec.py codes this configuration with


@functools.lru_cache(maxsize=None)
def _model(coder, adaptive=True):
    from tests.golden import make_golden
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = codec.small_config(adaptive=adaptive, offsets=adaptive)
    P = codec.random_params(cfg, SEED, gain=make_golden.GAIN[SEED])
    cfg = copy.deepcopy(cfg)
    cfg["entropy_model"]["entropy_coder"] = coder
    m = load_params(UnifiedModel(cfg), P).to(dev()).eval()
    m.update()
    return m


@functools.lru_cache(maxsize=None)
def _cloud():
    from unified_point_cloud_compression_amd import synth
    return t(synth.random_block(SEED, 32, 0.08))


@functools.lru_cache(maxsize=None)
def _qs():
    from unified_point_cloud_compression_amd.rate import q_grid
    return t(np.concatenate([q_grid(3), np.array([PAIR], dtype=np.float32)]))


@functools.lru_cache(maxsize=None)
def _singles(coder):
    """`compress` once per quality point: the oracle of everything below."""
    m, pc, qs = _model(coder), _cloud(), _qs()
    return [m.compress(pc, qs[i:i + 1]) for i in range(qs.shape[0])]


def _assert_same_result(got, want, coder):
    streams, shapes, ks, coords, q_vals = got
    w_streams, w_shapes, w_ks, w_coords, w_q = want
    assert len(streams) == len(w_streams) and shapes == w_shapes and ks == w_ks
    for b in range(len(streams)):
        assert torch.equal(coords[b], w_coords[b]) and torch.equal(q_vals[b], w_q[b])
        if coder == "symbols":
            assert torch.equal(streams[b][0], w_streams[b][0]) and torch.equal(streams[b][1], w_streams[b][1])
            continue
        (ys,), (zs,) = streams[b]
        (w_ys,), (w_zs,) = w_streams[b]
        assert bytes(ys) == bytes(w_ys) and bytes(zs) == bytes(w_zs)
        assert getattr(ys, "groups", 0) == getattr(w_ys, "groups", 0) and getattr(zs, "groups", 0) == getattr(w_zs, "groups", 0)


@pytest.mark.parametrize("coder", ["pcc_streams", "symbols", "ans"])
def test_multirate_equals_one_compress_per_q(coder):
    m, pc, qs = _model(coder), _cloud(), _qs()
    calls = []
    hook = m.g_a.register_forward_hook(lambda *a: calls.append(1))
    try:
        multi = m.compress_multirate(pc, qs)
    finally:
        hook.remove()
    assert len(calls) == 1                                       # one analysis for the whole list (one block)
    assert len(multi) == qs.shape[0]
    for got, want in zip(multi, _singles(coder)):
        _assert_same_result(got, want, coder)
    if coder != "symbols":
        assert len({len(r[0][0][0][0]) for r in multi}) > 1      # the quality points do differ


def test_multirate_decodes_like_the_single_encodes():
    m, pc, qs = _model("pcc_streams"), _cloud(), _qs()
    multi = m.compress_multirate(pc, qs)
    for i in (0, 4, qs.shape[0] - 1):
        s, sh, k, c, q = multi[i]
        w = _singles("pcc_streams")[i]
        rec = m.decompress(coordinates=c, strings=s, shape=sh, k=k, q_vals=q)
        rec_w = m.decompress(coordinates=w[3], strings=w[0], shape=w[1], k=w[2], q_vals=w[4])
        assert rec.shape[0] > 0 and torch.equal(rec, rec_w)


def test_multirate_multi_block():
    from unified_point_cloud_compression_amd import synth
    m = _model("pcc_streams")
    pc = t(synth.random_block(3, 48, 0.05))
    qs = _qs()[[1, 9, 6]].contiguous()
    calls = []
    hook = m.g_a.register_forward_hook(lambda *a: calls.append(1))
    try:
        multi = m.compress_multirate(pc, qs, block_size=32)     # 2 x 2 x 2 blocks
    finally:
        hook.remove()
    assert len(calls) == 8                                       # one analysis per block, not per (block, q)
    for i, got in enumerate(multi):
        want = m.compress(pc, qs[i:i + 1], block_size=32)
        assert len(got[0]) == 8
        _assert_same_result(got, want, "pcc_streams")
    s, sh, k, c, q = multi[1]
    assert m.decompress(coordinates=c, strings=s, shape=sh, k=k, q_vals=q).shape == (pc.shape[0], 6)


def _estimate_of_compress(pc, q, block_size):
    """Per block, `pcc_rans_estimate_bits` on the symbols `compress` (coder "symbols") returns for q, with the
    table rows from `index_rows`."""
    from unified_point_cloud_compression_amd import rans as R
    m = _model("symbols")
    em, gc = m.entropy_model, m.entropy_model.gaussian_conditional
    tabs = gc.tables(dev())
    streams = m.compress(pc, q, block_size=block_size)[0]
    blocks = m.blocks_of(pc, block_size)
    out = torch.zeros(len(blocks), dtype=torch.int64, device=dev())
    for b, x_block in enumerate(blocks):
        y, _ = m.g_a(m.block_input(x_block))
        a = em.analyse(y)
        idx = gc.index_rows(a.params, a.y_cset.keys, em._gains(q, a.y_cset, a.y_rows.shape[1])[0])
        assert streams[b][0].shape == idx.shape
        R.estimate(tabs, streams[b][0], idx, out.data_ptr() + 8 * b)
    return out.tolist()


@pytest.mark.parametrize("blocks", [1, 8])
def test_rate_map_equals_the_estimate_of_the_coded_symbols(blocks):
    from unified_point_cloud_compression_amd import synth
    m, qs = _model("pcc_streams"), _qs()
    pc, bs = (_cloud(), 1024) if blocks == 1 else (t(synth.random_block(3, 48, 0.05)), 32)
    if blocks == 8:
        qs = qs[[0, 9]].contiguous()
    with torch.no_grad():
        want_blocks = [_estimate_of_compress(pc, qs[i:i + 1], bs) for i in range(qs.shape[0])]
    rm = m.rate_map(pc, qs, block_size=bs)
    assert rm["y_bits256"].dtype == torch.int64 and rm["y_bits256"].tolist() == [sum(w) for w in want_blocks]
    singles = [m.compress(pc, qs[i:i + 1], block_size=bs) for i in range(qs.shape[0])] if blocks == 8 else _singles("pcc_streams")
    assert rm["fixed_bytes"] == sum(len(s[1][0]) for s in singles[0][0])
    assert len(rm["predicted_bytes"]) == qs.shape[0]
    # predicted_bytes by its definition, written out: the fixed bytes, and per block ceil(estimate / 2048) + 4 + 12 per stream of
    # the plan (these blocks are far below the adaptive size: the plan follows from (n, c)).  How close this is to the real
    # size is measured by tools/multirate_timing.py, not asserted (DESIGN.md section 7h says what separates the two).
    gc = m.entropy_model.gaussian_conditional
    n_rows = [yc.shape[0] for yc in singles[0][3]]
    for i in range(qs.shape[0]):
        expect = rm["fixed_bytes"]
        for nb, e in zip(n_rows, want_blocks[i]):
            ng, segs = gc.n_streams(nb, C_SMALL)
            expect += (e + 2047) // 2048 + 4 + 12 * ng * segs
        real = sum(len(s[0][0]) + len(s[1][0]) for s in singles[i][0])
        print(f"q {i}: predicted {rm['predicted_bytes'][i]} real {real}")
        assert rm["predicted_bytes"][i] == expect


def test_compress_to_size():
    from unified_point_cloud_compression_amd.metrics import count_bits
    m, pc, qs = _model("pcc_streams"), _cloud(), _qs()
    K = qs.shape[0]
    real = [count_bits(s[0]) // 8 for s in _singles("pcc_streams")]              # brute force
    pred = m.rate_map(pc, qs)["predicted_bytes"]
    assert min(real) < max(real)
    for budget in ((min(real) + max(real)) // 2, max(real), min(real)):
        result, info = m.compress_to_size(pc, budget, qs=qs)
        i = info["index"]
        assert info["met"] and info["bytes"] <= budget and 1 <= info["tries"] <= K
        assert info["bytes"] == real[i] == count_bits(result[0]) // 8
        assert info["predicted_bytes"] == pred[i] and torch.equal(info["q"], qs[i:i + 1])
        _assert_same_result(result, _singles("pcc_streams")[i], "pcc_streams")
        # the order of trial: predictions within the budget from the largest down, then the others from the smallest up (ties
        # to the earlier index); the first whose REAL size fits is the answer
        order = sorted((j for j in range(K) if pred[j] <= budget), key=lambda j: (-pred[j], j)) + \
            sorted((j for j in range(K) if pred[j] > budget), key=lambda j: (pred[j], j))
        first = next(p for p, j in enumerate(order) if real[j] <= budget)
        assert i == order[first] and info["tries"] == first + 1
        if pred[i] <= budget:       # no candidate that fits has a larger prediction within the budget than the chosen one
            assert all(pred[j] <= pred[i] for j in range(K) if real[j] <= budget and pred[j] <= budget)
        s, sh, k, c, q = result
        rec = m.decompress(coordinates=c, strings=s, shape=sh, k=k, q_vals=q)
        assert rec.shape == (pc.shape[0], 6)
    # below the smallest real size nothing fits: the smallest prediction comes back, flagged
    small = min(range(K), key=lambda j: (pred[j], j))
    result, info = m.compress_to_size(pc, min(min(real), min(pred)) // 2, qs=qs)
    assert not info["met"] and info["index"] == small and info["bytes"] == real[small] and info["tries"] == K
    _assert_same_result(result, _singles("pcc_streams")[small], "pcc_streams")


def test_compress_to_size_default_grid_and_refusals():
    from unified_point_cloud_compression_amd import lib as L
    from unified_point_cloud_compression_amd.metrics import count_bits
    m, pc = _model("pcc_streams"), _cloud()
    real = [count_bits(s[0]) // 8 for s in _singles("pcc_streams")]
    budget = (min(real) + max(real)) // 2
    result, info = m.compress_to_size(pc, budget)                # the 121-point grid
    assert info["met"] and info["bytes"] <= budget and 0 <= info["index"] < 121 and info["tries"] <= 121
    assert count_bits(result[0]) // 8 == info["bytes"]
    with pytest.raises(L.PccError, match="byte strings"):
        _model("symbols").compress_to_size(pc, budget)
    with pytest.raises(L.PccError):
        m.rate_map(pc, t(np.zeros((257, 2), dtype=np.float32)))


def test_without_adaptive_gains_every_candidate_is_the_same():
    m, pc, qs = _model("pcc_streams", adaptive=False), _cloud(), _qs()[:3].contiguous()
    rm = m.rate_map(pc, qs)
    assert len(set(rm["y_bits256"].tolist())) == 1 and len(set(rm["predicted_bytes"])) == 1
    multi = m.compress_multirate(pc, qs)
    for i in range(3):
        _assert_same_result(multi[i], m.compress(pc, qs[i:i + 1]), "pcc_streams")
    real = len(multi[0][0][0][0][0]) + len(multi[0][0][0][1][0])
    result, info = m.compress_to_size(pc, real, qs=qs)
    assert info["met"] and info["index"] == 0 and info["tries"] == 1 and info["bytes"] == real
    result, info = m.compress_to_size(pc, real - 1, qs=qs)
    assert not info["met"] and info["index"] == 0 and info["bytes"] == real
