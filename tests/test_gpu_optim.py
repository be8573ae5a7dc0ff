"""`optim.FusedOptimizer` / `csrc/pcc_optim.hip` (clip + Adam / SGD-momentum for all tensors in two launches) against float64.

Reference.  tests/optim_ref.py (numpy float64; tests/test_cpu_optim_ref.py holds it against CPU float64 torch to 1e-12),
fed the same float32 parameters and gradients.

Yardstick.  torch's float32 foreach `optim.Adam` / `optim.SGD(momentum=0.9)` after `clip_grad_norm_` on the same inputs,
measured against the same reference with the same metric.  Every bound is
        kernel error <= max(MARGIN x yardstick error, FLOOR),   MARGIN = 4,   for the max and for the rms
(the convention of tests/test_gpu_rate_loss_float64.py).  The metric is |got - ref| over the largest magnitude of the quantity
in the parameter list (parameters, first state, second state: one figure each; the reported norm: relative), and FLOOR is
4 float32 ulps (4 x 2^-23) of that magnitude: the update is the end of a chain of about eight roundings.  MARGIN covers the
differences that are not errors: torch forms exp_avg with `lerp` and the norm from float32 per-tensor norms, the kernel with
b1 m + (1 - b1) g (contracted to one FMA) and an fp64 sum.
"""
import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.util import dev, n, bits

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR = 4 * 2.0 ** -23
TAIL = 64
PCC_EWS = -3


def _O():
    from unified_point_cloud_compression_amd import optim
    return optim


def _chunk():
    from unified_point_cloud_compression_amd import lib as L
    return int(L.load().pcc_optim_chunk_elems())


def _edge_sizes():
    c = _chunk()
    return [1, 3, 255, 256, 257, c - 1, c, c + 1, 3 * c + 5, 0]


def _params(sizes, seed, unaligned=()):
    """float32 parameters ~ 0.05 N(0,1) (numpy) and their device leaves; the tensors listed in `unaligned` start 4 bytes off
    a 16-byte boundary (a contiguous slice of a larger buffer), which takes the kernels' scalar path."""
    rng = np.random.default_rng(seed)
    host = [(0.05 * rng.standard_normal(s)).astype(np.float32) for s in sizes]
    leaves = []
    for i, h in enumerate(host):
        if i in unaligned:
            base = torch.zeros(h.size + 8, dtype=torch.float32, device=dev())
            p = base[1:1 + h.size]
            p.copy_(torch.from_numpy(h))
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            leaves.append(p.requires_grad_())
        else:
            leaves.append(torch.from_numpy(h).to(dev()).requires_grad_())
    return host, leaves


def _grads(sizes, rng, scale, none_at=()):
    return [None if i in none_at else (scale * rng.standard_normal(s)).astype(np.float32) for i, s in enumerate(sizes)]


def _set_grads(leaves, grads, unaligned=()):
    for i, (p, g) in enumerate(zip(leaves, grads)):
        if g is None:
            p.grad = None
        elif i in unaligned:
            base = torch.zeros(g.size + 8, dtype=torch.float32, device=dev())
            base[1:1 + g.size].copy_(torch.from_numpy(g))
            p.grad = base[1:1 + g.size]
        else:
            p.grad = torch.from_numpy(g).to(dev())


def _torch_opt(leaves, mode, lr):
    return (torch.optim.Adam(leaves, lr=lr, foreach=True) if mode == "adam"
            else torch.optim.SGD(leaves, lr=lr, momentum=0.9, foreach=True))


def _err(got, ref):
    """(max, rms) of |got - ref| / max|ref| over the concatenation of the lists' tensors (None entries: skipped in both)."""
    g = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a, r in zip(got, ref) if r is not None] + [np.zeros(0)])
    r = np.concatenate([np.asarray(r, np.float64).reshape(-1) for r in ref if r is not None] + [np.zeros(0)])
    assert g.shape == r.shape
    if r.size == 0:
        return 0.0, 0.0
    assert np.isfinite(g).all()
    e = np.abs(g - r) / max(np.abs(r).max(), 1e-30)
    return float(e.max()), float(np.sqrt((e * e).mean()))


def _bounded(what, k, y):
    print(f"{what}: kernel max {k[0]:.3e} rms {k[1]:.3e} | float32 torch max {y[0]:.3e} rms {y[1]:.3e} | floor {FLOOR:.2e}")
    assert k[0] <= max(MARGIN * y[0], FLOOR), f"{what}: max {k[0]:.3e} against {y[0]:.3e} of float32 torch"
    assert k[1] <= max(MARGIN * y[1], FLOOR), f"{what}: rms {k[1]:.3e} against {y[1]:.3e} of float32 torch"


def _state_of(opt, leaves, name):
    return [n(opt.state[p][name]) if p in opt.state and opt.state[p] else None for p in leaves]


def _compare(what, mode, fused, f_leaves, yard, y_leaves, params64, state64):
    _bounded(f"{what} parameters", _err([n(p) for p in f_leaves], params64), _err([n(p) for p in y_leaves], params64))
    s1 = "exp_avg" if mode == "adam" else "momentum_buffer"
    for name, ref in ((s1, state64.s1),) + ((("exp_avg_sq", state64.s2),) if mode == "adam" else ()):
        k_s, y_s = _state_of(fused, f_leaves, name), _state_of(yard, y_leaves, name)
        for i, r in enumerate(ref):                      # a tensor has state in all three or in none
            assert (r is None) == (k_s[i] is None) == (y_s[i] is None), (name, i)
        _bounded(f"{what} {name}", _err(k_s, ref), _err(y_s, ref))
    if mode == "adam":
        for i, p in enumerate(f_leaves):
            if state64.s1[i] is not None:
                assert int(fused.state[p]["step"]) == state64.step[i] == int(yard.state[y_leaves[i]]["step"])


def _run(mode, sizes, steps, max_norm, scale, seed=0, none_at=None, unaligned=(), sched=None, lr=1e-2):
    """`steps` steps of the kernel, of float32 torch and of the float64 reference on the same gradients.  none_at(step) ->
    indices without a gradient at that step; sched: (step_size, gamma) of a StepLR stepped after every optimiser step."""
    O = _O()
    host, f_leaves = _params(sizes, seed, unaligned)
    _, y_leaves = _params(sizes, seed)
    fused = O.FusedOptimizer(f_leaves, lr=lr, mode=mode, max_norm=max_norm)
    yard = _torch_opt(y_leaves, mode, lr)
    scheds = [torch.optim.lr_scheduler.StepLR(o, *sched) for o in (fused, yard)] if sched else []
    params64, state64 = [h.astype(np.float64) for h in host], R.State(len(sizes))
    rng = np.random.default_rng(seed + 100)
    norms = []
    for s in range(steps):
        skip = none_at(s) if none_at else ()
        grads = _grads(sizes, rng, scale, skip)
        _set_grads(f_leaves, grads, unaligned)
        _set_grads(y_leaves, grads)
        kept = [None if p.grad is None else p.grad.clone() for p in f_leaves]
        versions = [p._version for p in f_leaves]
        frozen = {i: (n(f_leaves[i]).copy(), {k: n(v).copy() for k, v in fused.state.get(f_leaves[i], {}).items()}) for i in skip}
        assert fused.param_groups[0]["lr"] == yard.param_groups[0]["lr"]
        lr_now = fused.param_groups[0]["lr"]
        fused.step()
        norm_y = torch.nn.utils.clip_grad_norm_(y_leaves, max_norm, foreach=True) if max_norm is not None else None
        yard.step()
        for sc in scheds:
            sc.step()
        norm64 = R.step(params64, grads, state64, lr_now, mode=mode, max_norm=max_norm)
        if max_norm is not None:
            norms.append((float(fused.last_norm), float(norm_y), norm64))
        for i, p in enumerate(f_leaves):
            if i in skip:                                # no gradient: parameter, state and step untouched, as in torch
                assert p._version == versions[i]
                assert np.array_equal(n(p), frozen[i][0])
                for k, v in frozen[i][1].items():
                    assert np.array_equal(n(fused.state[p][k]), v), (i, k)
            else:
                assert p._version > versions[i], f"_version of stepped parameter {i} did not increase"
                assert torch.equal(p.grad, kept[i]), "the stored gradient must keep its unclipped value"
    return fused, f_leaves, yard, y_leaves, params64, state64, norms


def _check_norms(what, norms):
    k = max(abs(a - r) / max(r, 1e-30) for a, _, r in norms)
    y = max(abs(b - r) / max(r, 1e-30) for _, b, r in norms)
    print(f"{what} norm (relative): kernel {k:.3e} | float32 torch {y:.3e} | floor {FLOOR:.2e}")
    assert k <= max(MARGIN * y, FLOOR)


# ---------------------------------------------------------------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["adam", "sgd"])
@pytest.mark.parametrize("clip", ["active", "inactive", "none"])
def test_ten_steps_over_the_edge_sizes(mode, clip):
    """Sizes 1, 3, 255, 256, 257, chunk - 1, chunk, chunk + 1, 3 chunk + 5 and 0 in one list (tensor 2 and 7 on the scalar path), 10
    steps with StepLR(3, 0.5) changing lr between them, tensor 4 without a gradient on steps 2..4 and tensor 8 on step 0 (its
    bias correction then runs one step behind the others')."""
    sizes = _edge_sizes()
    max_norm, scale = {"active": (1.0, 1.0), "inactive": (1.0, 1e-4), "none": (None, 1.0)}[clip]
    none_at = lambda s: ((4,) if 2 <= s <= 4 else ()) + ((8,) if s == 0 else ())
    out = _run(mode, sizes, 10, max_norm, scale, none_at=none_at, unaligned=(2, 7), sched=(3, 0.5))
    fused, f_leaves, yard, y_leaves, params64, state64, norms = out
    _compare(f"{mode}/{clip}", mode, fused, f_leaves, yard, y_leaves, params64, state64)
    if max_norm is not None:
        _check_norms(f"{mode}/{clip}", norms)
        active = [r > max_norm for _, _, r in norms]
        assert all(active) if clip == "active" else not any(active)
    assert abs(fused.param_groups[0]["lr"] - 1e-2 * 0.5 ** 3) < 1e-15
    assert state64.step[4] == 7 and state64.step[8] == 9 and state64.step[0] == 10


@pytest.mark.parametrize("mode", ["adam", "sgd"])
def test_three_hundred_tiny_tensors_with_gaps(mode):
    """300 tensors of 1..7 elements: more than any kernel-argument block would hold, and odd sizes, so that the 16-byte aligned
    offsets leave gaps in the flat state buffers -- which must stay zero."""
    sizes = [1 + (i * 5) % 7 for i in range(300)]
    fused, f_leaves, yard, y_leaves, params64, state64, norms = _run(mode, sizes, 3, 1.0, 1.0, seed=3)
    _compare(f"{mode}/tiny", mode, fused, f_leaves, yard, y_leaves, params64, state64)
    _check_norms(f"{mode}/tiny", norms)
    used = np.zeros(fused._flat1.numel(), dtype=bool)
    for i, s in enumerate(sizes):
        a = int(fused._offsets[i])
        assert a % 4 == 0 and fused.state[f_leaves[i]]["exp_avg" if mode == "adam" else "momentum_buffer"].data_ptr() % 16 == 0
        used[a:a + s] = True
    assert (~used).sum() > 300
    for flat in (fused._flat1, fused._flat2):
        if flat is not None:
            assert not n(flat)[~used].any() and n(flat)[used].all()


def test_non_finite_norm_propagates_as_in_torch():
    """An infinite gradient: norm inf, coefficient 0, so finite gradients become 0 and the infinite one NaN; a NaN gradient: every
    updated element NaN.  The NaN patterns of parameters and state equal torch's."""
    sizes = [5, 300, 7]
    for bad in (np.inf, np.nan):
        _, f_leaves = _params(sizes, 1)
        _, y_leaves = _params(sizes, 1)
        grads = _grads(sizes, np.random.default_rng(2), 1.0)
        grads[1][17] = bad
        _set_grads(f_leaves, grads), _set_grads(y_leaves, grads)
        fused = _O().FusedOptimizer(f_leaves, lr=1e-2, max_norm=1.0)
        yard = _torch_opt(y_leaves, "adam", 1e-2)
        fused.step()
        torch.nn.utils.clip_grad_norm_(y_leaves, 1.0, foreach=True)
        yard.step()
        assert np.isnan(float(fused.last_norm)) if np.isnan(bad) else np.isinf(float(fused.last_norm))
        for p, q in zip(f_leaves, y_leaves):
            assert np.array_equal(np.isnan(n(p)), np.isnan(n(q)))
            for name in ("exp_avg", "exp_avg_sq"):
                assert np.array_equal(np.isnan(n(fused.state[p][name])), np.isnan(n(yard.state[q][name])))
            ok = ~np.isnan(n(q))
            assert np.allclose(n(p)[ok], n(q)[ok], rtol=0, atol=1e-6)
        assert np.isnan(n(f_leaves[1])[17])


@pytest.mark.parametrize("mode", ["adam", "sgd"])
def test_two_runs_from_equal_inputs_give_equal_bits(mode):
    sizes = _edge_sizes()
    a = _run(mode, sizes, 3, 1.0, 1.0, seed=5, unaligned=(2,))
    b = _run(mode, sizes, 3, 1.0, 1.0, seed=5, unaligned=(2,))
    for p, q in zip(a[1], b[1]):
        assert np.array_equal(bits(p), bits(q))
    assert np.array_equal(bits(a[0]._flat1), bits(b[0]._flat1))
    assert [x[0] for x in a[6]] == [x[0] for x in b[6]]
    # the summation order is a function of the sizes alone: an unaligned base (scalar loads) gives the same bits too
    c = _run(mode, sizes, 3, 1.0, 1.0, seed=5, unaligned=(5, 8))
    for p, q in zip(a[1], c[1]):
        assert np.array_equal(bits(p), bits(q))


# ---------------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_guard_tails_behind_every_buffer_stay_intact(mode):
    """The C entry points on buffers with NaN tails: partials, parameters, both states and the norm word."""
    from unified_point_cloud_compression_amd import lib as L
    lib, c = L.load(), _chunk()
    sizes = np.array([1, 257, c + 1, 3 * c + 5, 0, 6], dtype=np.int64)
    nchunks = int(lib.pcc_optim_build_chunks(L.nptr(sizes), len(sizes), None, 0))
    assert nchunks == 1 + 1 + 2 + 4 + 0 + 1
    chunks = np.zeros((nchunks, 2), dtype=np.int32)
    assert lib.pcc_optim_build_chunks(L.nptr(sizes), len(sizes), L.nptr(chunks), nchunks) == nchunks
    d_chunks = torch.from_numpy(chunks).to(dev())
    nan = float("nan")
    bufs = {k: [torch.full((int(s) + TAIL,), nan, dtype=torch.float32, device=dev()) for s in sizes] for k in "pgab"}
    rng = np.random.default_rng(0)
    for k in "pgab":
        for b, s in zip(bufs[k], sizes):
            b[:int(s)] = torch.from_numpy(np.abs(rng.standard_normal(int(s))).astype(np.float32)).to(dev())
    seg = np.zeros((len(sizes), 6), dtype=np.int64)
    for i in range(len(sizes)):
        seg[i] = [bufs["p"][i].data_ptr(), bufs["g"][i].data_ptr(), bufs["a"][i].data_ptr(), bufs["b"][i].data_ptr(), sizes[i], 2]
    d_seg = torch.from_numpy(seg).to(dev())
    ws_bytes = int(lib.pcc_optim_ws_bytes(nchunks))
    assert ws_bytes >= nchunks * 8
    partials = torch.full((ws_bytes // 8 + TAIL,), nan, dtype=torch.float64, device=dev())
    norm = torch.full((1 + TAIL,), nan, dtype=torch.float32, device=dev())
    before = {k: [b.clone() for b in bufs[k]] for k in "pgab"}
    L.call("pcc_optim_sqnorm", d_seg.data_ptr(), len(sizes), d_chunks.data_ptr(), nchunks, partials.data_ptr(), ws_bytes, L.stream())
    assert not bool(torch.isnan(partials[:nchunks]).any()) and bool(torch.isnan(partials[nchunks:]).all())
    want = sum(float((b[:int(s)].double() ** 2).sum()) for b, s in zip(bufs["g"], sizes))
    assert abs(float(partials[:nchunks].sum()) - want) <= 1e-10 * want
    L.call("pcc_optim_step", d_seg.data_ptr(), len(sizes), d_chunks.data_ptr(), nchunks, partials.data_ptr(), ws_bytes, mode,
           1e-2, 0.9, 0.999, 1e-8, 1.0, norm.data_ptr(), L.stream())
    assert abs(float(norm[0]) - want ** 0.5) <= 1e-6 * want ** 0.5 and bool(torch.isnan(norm[1:]).all())
    assert bool(torch.isnan(partials[nchunks:]).all())
    for k in "pgab":
        for i, (b, s) in enumerate(zip(bufs[k], sizes)):
            s = int(s)
            assert bool(torch.isnan(b[s:]).all()), f"{k}[{i}]: written past the end"
            assert not bool(torch.isnan(b[:s]).any())
            changed = not torch.equal(b[:s], before[k][i][:s])
            assert changed == (s > 0 and (k in "pa" or (k == "b" and mode == 0))), (k, i)
    # a short workspace is refused before any launch
    assert lib.pcc_optim_sqnorm(d_seg.data_ptr(), len(sizes), d_chunks.data_ptr(), nchunks, partials.data_ptr(), nchunks * 8 - 1,
                                L.stream()) == PCC_EWS


# ---------------------------------------------------------------------------------------------------------------------------------
# version counters and the packed-weight caches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_convolution_after_a_step_uses_the_updated_weights():
    """Every packed-weight cache is keyed on (data_ptr, _version): the forward of a `MinkowskiConvolution` after the step equals
    bit for bit that of a fresh module loaded with the updated weights."""
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from tests.util import cloud_keys, t
    from oracle import coords as co
    C = co.unpack_keys(cloud_keys(0, 12, 0.3)).astype(np.int32)
    rng = np.random.default_rng(0)
    x = ME.SparseTensor(coordinates=t(C), features=t(rng.standard_normal((len(C), 32)).astype(np.float32)))
    conv = ME.MinkowskiConvolution(32, 32, kernel_size=3, stride=1, bias=True, dimension=3).to(dev())
    with torch.no_grad():
        before = conv(x).F.clone()                       # fills the module's packed-weight cache
    opt = _O().FusedOptimizer(conv.parameters(), lr=1e-2, max_norm=1.0)
    for p in conv.parameters():
        p.grad = torch.randn(p.shape, device=dev(), generator=torch.Generator(dev()).manual_seed(1))
    opt.step()
    fresh = ME.MinkowskiConvolution(32, 32, kernel_size=3, stride=1, bias=True, dimension=3).to(dev())
    fresh.load_state_dict(conv.state_dict())
    with torch.no_grad():
        after, want = conv(x).F, fresh(x).F
    assert np.array_equal(bits(after), bits(want))
    assert not np.array_equal(bits(after), bits(before))


# ---------------------------------------------------------------------------------------------------------------------------------
# state dicts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["adam", "sgd"])
@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_dict_moves_between_torch_and_the_kernel(mode, direction):
    """4 steps in one optimiser, its state dict loaded into the other kind, 3 more steps there: within the bound of float32 torch
    that simply continues (and the reverse)."""
    O = _O()
    sizes, lr, max_norm = [3, 257, 1000, 6], 1e-2, 1.0
    host, a_leaves = _params(sizes, 7)
    _, y_leaves = _params(sizes, 7)
    make_fused = lambda leaves: O.FusedOptimizer(leaves, lr=lr, mode=mode, max_norm=max_norm)
    first = _torch_opt(a_leaves, mode, lr) if direction == "torch_to_fused" else make_fused(a_leaves)
    yard = _torch_opt(y_leaves, mode, lr)
    params64, state64 = [h.astype(np.float64) for h in host], R.State(len(sizes))
    rng = np.random.default_rng(8)

    def one_step(opt_a):
        grads = _grads(sizes, rng, 1.0)
        _set_grads(a_leaves, grads), _set_grads(y_leaves, grads)
        if not isinstance(opt_a, O.FusedOptimizer):
            torch.nn.utils.clip_grad_norm_(a_leaves, max_norm, foreach=True)
        opt_a.step()
        torch.nn.utils.clip_grad_norm_(y_leaves, max_norm, foreach=True)
        yard.step()
        R.step(params64, grads, state64, lr, mode=mode, max_norm=max_norm)

    for _ in range(4):
        one_step(first)
    sd = first.state_dict()
    ref_sd = yard.state_dict()
    assert sorted(sd["param_groups"][0]) == sorted(ref_sd["param_groups"][0])        # torch's layout, key for key
    assert sorted(sd["state"]) == sorted(ref_sd["state"]) and all(sorted(sd["state"][k]) == sorted(ref_sd["state"][k]) for k in sd["state"])
    second = make_fused(a_leaves) if direction == "torch_to_fused" else _torch_opt(a_leaves, mode, lr)
    second.load_state_dict(sd)
    for _ in range(3):
        one_step(second)
    fused = second if direction == "torch_to_fused" else first
    if direction == "fused_to_torch":                    # compare the states torch carried on with
        s1 = "exp_avg" if mode == "adam" else "momentum_buffer"
        _bounded(f"{mode}/{direction} {s1}", _err(_state_of(second, a_leaves, s1), state64.s1), _err(_state_of(yard, y_leaves, s1), state64.s1))
        _bounded(f"{mode}/{direction} parameters", _err([n(p) for p in a_leaves], params64), _err([n(p) for p in y_leaves], params64))
        if mode == "adam":
            assert all(int(second.state[p]["step"]) == 7 for p in a_leaves)
    else:
        _compare(f"{mode}/{direction}", mode, fused, a_leaves, yard, y_leaves, params64, state64)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    O = _O()
    from unified_point_cloud_compression_amd.lib import PccError
    good = torch.zeros(8, device=dev(), requires_grad=True)
    with pytest.raises(PccError):
        O.FusedOptimizer([good, torch.zeros((4, 4), device=dev()).t().requires_grad_()], lr=1e-3)       # non-contiguous
    with pytest.raises(PccError):
        O.FusedOptimizer([good, torch.zeros(8, device=dev(), dtype=torch.float16, requires_grad=True)], lr=1e-3)
    with pytest.raises(PccError):
        O.FusedOptimizer([torch.zeros(8, requires_grad=True)], lr=1e-3)                                   # CPU
    with pytest.raises(ValueError):
        O.FusedOptimizer([good], lr=1e-3, mode="rmsprop")
    opt = O.FusedOptimizer([good], lr=1e-3)
    with pytest.raises(PccError):
        opt.add_param_group({"params": [torch.zeros(3, device=dev(), requires_grad=True)]})
    good.grad = torch.ones(8, device=dev())
    opt.step()
    assert int(opt.state[good]["step"]) == 1
    square = torch.zeros((4, 4), device=dev(), requires_grad=True)
    opt = O.FusedOptimizer([square], lr=1e-3)
    square.grad = torch.ones((4, 4), device=dev()).t()
    with pytest.raises(PccError):
        opt.step()                                       # a gradient that is not contiguous
    assert not square.any() and square not in opt.state
