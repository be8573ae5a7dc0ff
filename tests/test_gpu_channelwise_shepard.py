"""GPU suite: `ME.MinkowskiChannelwiseConvolution` (pcc_chconv_fwd / pcc_chconv_wgrad) against a dense grouped conv3d in float64,
and `ShepardsLoss` (`loss.py:161-274`) against a float64 per-tap restatement and against the reference's own formulation over the
union set -- every case with the grid index and with binary search."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests.util import dev, t, n

pytestmark = pytest.mark.gpu

SHEPARD_CFG = {"type": "ShepardsLoss", "loss": "L2", "window_size": 9, "p": 8}
COLOR_LOSS_CFG = {   # `configs/CVPR_inverse_scaling.yaml:58-75`
    "Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
    "ColorLoss": {"type": "ColorLoss", "loss": "L2"},
    "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0},
    "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0},
}
SHEPARD_LOSS_CFG = dict(COLOR_LOSS_CFG, ColorLoss=dict(SHEPARD_CFG))   # `configs/CVPR_inverse_scaling_shepard.yaml`


@pytest.fixture(params=[True, False], ids=["grid", "bsearch"])
def lookup_mode(request):
    from unified_point_cloud_compression_amd import sparse as S
    old = S.USE_GRID
    S.USE_GRID = request.param
    yield request.param
    S.USE_GRID = old


def _cloud(seed, size=10, p=0.3, ts=1, nb=2):
    """Random voxels of `nb` batches on a stride-ts lattice, the corners of the box included (points at the lattice edges)."""
    rng = np.random.default_rng(seed)
    Cs = []
    for b in range(nb):
        occ = rng.random((size, size, size)) < p
        occ[0, 0, 0] = occ[-1, -1, -1] = occ[0, -1, 0] = occ[-1, 0, -1] = True
        xyz = np.argwhere(occ) * ts
        Cs.append(np.concatenate([np.full((len(xyz), 1), b), xyz], axis=1))
    C = np.concatenate(Cs).astype(np.int32)
    return C[rng.permutation(len(C))]


# ---- dense float64 restatement of the channelwise convolution ------------------------------------------------------------
def _dense_chconv(C, feats, kernel, ks, ts):
    """out[i][c] = sum_k kernel[k][c or 0] * feats[row(x_i + off_k * ts)][c], via F.conv3d(groups=C) over a dense volume."""
    r = ks // 2
    nb = int(C[:, 0].max()) + 1
    lat = torch.from_numpy(C[:, 1:] // ts).long()
    dims = [int(v) + 1 + 2 * r for v in lat.max(0).values]
    c = feats.shape[1]
    vol = torch.zeros((nb, c, *dims), dtype=torch.float64)
    b = torch.from_numpy(C[:, 0]).long()
    x, y, z = lat[:, 0] + r, lat[:, 1] + r, lat[:, 2] + r
    vol = vol.index_put((b[:, None].expand(-1, c), torch.arange(c)[None, :].expand(len(b), c), x[:, None].expand(-1, c),
                         y[:, None].expand(-1, c), z[:, None].expand(-1, c)), feats)
    kw = kernel.expand(-1, c) if kernel.shape[1] == 1 else kernel
    w = kw.reshape(ks, ks, ks, c).permute(3, 2, 1, 0).unsqueeze(1)       # x-fastest [K] -> [c, 1, kx, ky, kz]
    out = Fn.conv3d(vol, w, padding=r, groups=c)
    return out[b[:, None], torch.arange(c)[None, :], x[:, None], y[:, None], z[:, None]]


@pytest.mark.parametrize("ts", [1, 2])
@pytest.mark.parametrize("per_channel", [False, True], ids=["k1", "kC"])
@pytest.mark.parametrize("c", [1, 4, 8])
@pytest.mark.parametrize("ks", [1, 3, 5, 9])
def test_channelwise_forward_matches_dense_conv3d(ks, c, per_channel, ts, lookup_mode):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    C = _cloud(ks * 10 + c, ts=ts)
    rng = np.random.default_rng(c + ks)
    F = rng.random((len(C), c)).astype(np.float32)
    K = ks ** 3
    W = (rng.uniform(-1, 1, (K, c if per_channel else 1)) / K).astype(np.float32)
    m = ME.MinkowskiChannelwiseConvolution(c, kernel_size=ks, stride=1, dimension=3)
    m.kernel = torch.nn.Parameter(torch.from_numpy(W), requires_grad=False)
    m = m.to(dev())
    x = ME.SparseTensor(coordinates=t(C), features=t(F), tensor_stride=ts)
    with torch.no_grad():
        out = m(x)
    assert n(out.C).tolist() == n(x.C).tolist() and out.tensor_stride == [ts] * 3
    ref = _dense_chconv(C, torch.from_numpy(F).double(), torch.from_numpy(W).double(), ks, ts).numpy()
    np.testing.assert_allclose(n(out.F), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("ks,c,per_channel,ts", [(3, 4, True, 1), (5, 8, False, 2), (9, 4, False, 1), (9, 8, True, 2),
                                                 (3, 1, False, 1), (5, 3, True, 1)])
def test_channelwise_gradients_match_dense_autograd(ks, c, per_channel, ts, lookup_mode):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    C = _cloud(ks + 7 * c, ts=ts)
    rng = np.random.default_rng(3 * ks + c)
    F = rng.random((len(C), c)).astype(np.float32)
    K = ks ** 3
    W = (rng.uniform(-1, 1, (K, c if per_channel else 1)) / K).astype(np.float32)
    G = rng.standard_normal((len(C), c)).astype(np.float32)
    m = ME.MinkowskiChannelwiseConvolution(c, kernel_size=ks, stride=1, dimension=3)
    m.kernel = torch.nn.Parameter(torch.from_numpy(W))
    m = m.to(dev())
    f = t(F).requires_grad_(True)
    x = ME.SparseTensor(coordinates=t(C), features=f, tensor_stride=ts)
    (m(x).F * t(G)).sum().backward()
    fr = torch.from_numpy(F).double().requires_grad_(True)
    wr = torch.from_numpy(W).double().requires_grad_(True)
    (_dense_chconv(C, fr, wr, ks, ts) * torch.from_numpy(G).double()).sum().backward()
    np.testing.assert_allclose(n(f.grad), fr.grad.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(n(m.kernel.grad), wr.grad.numpy(), rtol=1e-5, atol=1e-5 * max(1.0, float(wr.grad.abs().max())))


def test_channelwise_bitwise_reproducible_and_paths_agree():
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import sparse as S
    C = _cloud(5, size=16, p=0.4)
    F = np.random.default_rng(1).random((len(C), 8)).astype(np.float32)
    m = ME.MinkowskiChannelwiseConvolution(8, kernel_size=5, dimension=3)
    m.kernel = torch.nn.Parameter(torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, (125, 8)).astype(np.float32)))
    m = m.to(dev())
    outs, grads = [], []
    old = S.USE_GRID
    try:
        for grid in (True, True, False):
            S.USE_GRID = grid
            m.kernel.grad = None
            x = ME.SparseTensor(coordinates=t(C), features=t(F))
            o = m(x)
            o.F.square().sum().backward()
            outs.append(n(o.F))
            grads.append(n(m.kernel.grad))
    finally:
        S.USE_GRID = old
    for o, g in zip(outs[1:], grads[1:]):
        assert np.array_equal(o, outs[0]) and np.array_equal(g, grads[0])


# ---- Shepard's loss -----------------------------------------------------------------------------------------------------
def _pack(C):
    C = np.asarray(C, dtype=np.int64)
    return (C[:, 0] << 48) | ((C[:, 1] + 32768) << 32) | ((C[:, 2] + 32768) << 16) | (C[:, 3] + 32768)


def _shepard_ref(gt_C, gt_F, pr_C, pr_F, q_map, ws=9, p=8, l2=True):
    """float64 restatement: per-tap searchsorted over the packed ground-truth keys, own colour where present, masks by
    finiteness, batch q-weights.  Returns (loss, gt_on_pred) as float64 torch tensors on the GPU (loss differentiable in pr_F)."""
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    win = ShepardsLoss({"id": "c", "loss": "L2", "window_size": ws, "p": p}).window.view(-1).double()
    gk = torch.from_numpy(_pack(gt_C)).to(dev())
    order = torch.argsort(gk)
    gk, gF = gk[order], gt_F[order]
    pk = torch.from_numpy(_pack(pr_C)).to(dev())
    r = ws // 2
    num = torch.zeros((len(pk), gF.shape[1]), dtype=torch.float64, device=dev())
    den = torch.zeros(len(pk), dtype=torch.float64, device=dev())
    for k in range(ws ** 3):
        w = float(win[k])
        if w == 0:
            continue
        dx, dy, dz = k % ws - r, (k // ws) % ws - r, k // (ws * ws) - r
        q = pk + (dx << 32) + (dy << 16) + dz
        i = torch.searchsorted(gk, q).clamp(max=len(gk) - 1)
        hit = gk[i] == q
        num += torch.where(hit[:, None], w * gF[i], 0.0)
        den += torch.where(hit, w, 0.0)
    i = torch.searchsorted(gk, pk).clamp(max=len(gk) - 1)
    own = gk[i] == pk
    gop = torch.where(own[:, None], gF[i], num / den[:, None])
    valid = torch.isfinite(gop).all(dim=1, keepdim=True)
    d = torch.where(valid, gop - pr_F, 0.0)
    e = d * d if l2 else d.abs()
    qb = q_map.double()[torch.from_numpy(np.asarray(pr_C[:, 0], dtype=np.int64)).to(dev()), 1]
    return (e * qb[:, None]).sum() / (valid.sum() * gop.shape[1]), gop


def _shepard_case(seed):
    """Ground truth of two batches; predictions: part of the ground truth, voxels near it, voxels outside its bounding box,
    voxels with no ground truth within radius 4, one of them with a NaN colour."""
    rng = np.random.default_rng(seed)
    gt_C = _cloud(seed, size=14, p=0.15)
    gt_F = rng.random((len(gt_C), 3)).astype(np.float32)
    keep = gt_C[rng.random(len(gt_C)) < 0.5]
    near = gt_C[rng.choice(len(gt_C), 200)] + np.concatenate([np.zeros((200, 1), np.int32),
                                                              rng.integers(-3, 4, (200, 3))], axis=1).astype(np.int32)
    outside = np.array([[0, -2, 0, 0], [1, 15, 13, 13], [0, 5, 16, 2], [1, -1, -1, -1], [0, 13, 13, 17]], np.int32)
    far = np.array([[0, 40, 40, 40], [1, -30, 5, 5], [0, 5, 5, 60]], np.int32)
    pr_C = np.unique(np.concatenate([keep, near, outside, far]), axis=0)
    pr_C = pr_C[rng.permutation(len(pr_C))]
    pr_F = rng.random((len(pr_C), 3)).astype(np.float32)
    far_rows = np.nonzero((pr_C[:, 1:] > 30).any(1) | (pr_C[:, 1:] < -20).any(1))[0]
    pr_F[far_rows[0], 1] = np.nan
    return gt_C, gt_F, pr_C, pr_F, far_rows


@pytest.mark.parametrize("l2", [True, False], ids=["L2", "L1"])
def test_shepard_loss_matches_restatement(l2, lookup_mode):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    gt_C, gt_F, pr_C, pr_F, far_rows = _shepard_case(11)
    q_map = t(np.array([[0.1, 3.0], [0.2, 0.5]], np.float32))
    loss_fn = ShepardsLoss(dict(SHEPARD_CFG, id="ColorLoss", loss="L2" if l2 else "L1"))
    gt = ME.SparseTensor(coordinates=t(gt_C), features=t(gt_F))
    f = t(pr_F).requires_grad_(True)
    pred = ME.SparseTensor(coordinates=t(pr_C), features=f)
    loss = loss_fn(gt, {"prediction": pred, "q_map": q_map})
    assert torch.isfinite(loss)
    loss.backward()
    fr = torch.from_numpy(pr_F).double().to(dev()).requires_grad_(True)
    ref, gop = _shepard_ref(gt_C, t(gt_F).double(), pr_C, fr, q_map, l2=l2)
    ref.backward()
    assert torch.isfinite(ref)
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    np.testing.assert_allclose(n(f.grad), n(fr.grad), rtol=1e-5, atol=1e-7)
    assert np.isfinite(n(f.grad)).all()
    assert not torch.isfinite(gop[far_rows]).any()          # the far rows are invalid (0/0) and carry no gradient
    assert (f.grad[far_rows] == 0).all()
    # interpolated values on the prediction's coordinates (user row order)
    got = n(loss_fn.interpolate_gt_to_pred(gt, pred).F)
    np.testing.assert_allclose(got, n(gop), rtol=1e-5, atol=1e-6, equal_nan=True)


def test_shepard_interpolation_matches_reference_formulation(lookup_mode):
    """`loss.py:236-273` restated with the shim: union set, `conv_sum` over it, `features_at_coordinates`."""
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import sparse as S
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    gt_C, gt_F, pr_C, pr_F, _ = _shepard_case(23)
    loss_fn = ShepardsLoss(dict(SHEPARD_CFG, id="ColorLoss"))
    gt = ME.SparseTensor(coordinates=t(gt_C), features=t(gt_F))
    pred = ME.SparseTensor(coordinates=t(pr_C), features=t(pr_F))
    fast = n(loss_fn.interpolate_gt_to_pred(gt, pred).F)

    loss_fn.conv_sum.to(dev())
    gk = S.pack_keys(gt.C)[:len(gt_C)]
    ov = torch.isin(S.pack_keys(pred.C)[:len(pr_C)], gk)
    combined_coords = torch.cat([gt.C, pred.C[~ov]])
    comb = ME.SparseTensor(coordinates=combined_coords, features=torch.ones(combined_coords.shape[0], 4, device=dev()))
    ov_c = torch.isin(S.pack_keys(comb.C)[:combined_coords.shape[0]], gk)
    comb.F[~ov_c] = 0.0
    comb.F[ov_c, 1] = 1.0
    comb.F[ov_c, 1:] = gt.features_at_coordinates(comb.C[ov_c].float())
    with torch.no_grad():
        interp = loss_fn.conv_sum(comb)
    at = interp.features_at_coordinates(pred.C[~ov].float())
    raw = at[:, 1:] / at[:, 0].unsqueeze(1)
    gop = torch.zeros((len(pr_C), 3), device=dev())
    gop[ov] = gt.features_at_coordinates(pred.C[ov].float())
    gop[~ov] = raw
    np.testing.assert_allclose(fast, n(gop), rtol=1e-6, atol=1e-6, equal_nan=True)
    assert np.isnan(fast).any() and np.isfinite(fast).any()


# ---- full size and the training step --------------------------------------------------------------------------------------
def _configs3_forward():
    """The configs[3] batch as `bench.train_step_setup` cuts it, and one training forward of its model."""
    import bench
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from unified_point_cloud_compression_amd import synth
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = copy.deepcopy(bench.R2_CONFIG)
    cfg["entropy_model"].update(adaptive_BN=True, quantization_offset=True, inverse_rescaling=True)
    torch.manual_seed(0)
    model = UnifiedModel(cfg).to(dev()).train()
    pc = synth.surface_cloud(0, 10, shuffle=False)
    cubes = []
    for origin in ((512, 300, 500), (300, 512, 420), (640, 512, 600), (512, 512, 300)):
        o = np.array(origin)
        m = np.all((pc[:, :3] >= o) & (pc[:, :3] < o + 128), axis=1)
        if m.sum() >= 300:
            cubes.append(pc[m])
    coords, feats = ME.utils.sparse_collate([c[:, :3] - c[:, :3].min(0) for c in cubes], [c[:, 3:] for c in cubes])
    nb = len(cubes)
    q = torch.tensor([[0.4, 0.7]] * nb, device=dev())
    Lam = torch.tensor([[5.0, 400.0], [4.0, 300.0], [6.0, 100.0], [5.0, 50.0]][:nb], device=dev())
    x = ME.SparseTensor(coordinates=coords.to(dev()), features=feats.float().to(dev()))
    with torch.no_grad():
        out = model(x, q, Lam)
    return x, out


def _host_reads(fn):
    """Run fn() counting the host reads the project makes (Tensor.item / tolist / cpu / numpy and lib.read)."""
    from unified_point_cloud_compression_amd import lib as L
    count = [0]
    saved = []
    for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "cpu"), (torch.Tensor, "numpy"),
                        (L, "read"), (L, "read_many")):
        orig = getattr(owner, name)
        saved.append((owner, name, orig))

        def wrapped(*a, _orig=orig, **k):
            count[0] += 1
            return _orig(*a, **k)
        setattr(owner, name, wrapped)
    try:
        res = fn()
    finally:
        for owner, name, orig in saved:
            setattr(owner, name, orig)
    return res, count[0]


def test_shepard_loss_full_size(lookup_mode):
    from unified_point_cloud_compression_amd.loss import ShepardsLoss
    x, out = _configs3_forward()
    pred = out["prediction"]
    assert x._cset.n > 70000 and pred._cset.n > 10000
    loss_fn = ShepardsLoss(dict(SHEPARD_CFG, id="ColorLoss"))
    first = loss_fn(x, out)
    torch.cuda.synchronize()
    # second call: no host read (sync debug mode where this build honours it, and counted host reads always)
    honoured = True
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device=dev()).item()
            honoured = False
        except RuntimeError:
            pass
        second, reads = _host_reads(lambda: loss_fn(x, out))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == 0
    assert torch.equal(first, second)
    print(f"sync debug mode honoured: {honoured}")
    pC = n(pred.C)
    ref, _ = _shepard_ref(n(x.C), x.F.double(), pC, pred.F.detach().double(), out["q_map"])
    assert abs(float(first) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))


def test_train_step_with_shepard_loss(lookup_mode):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from oracle import codec
    from tests.util import load_params
    from unified_point_cloud_compression_amd.loss import Loss
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = codec.small_config(adaptive=True, offsets=True, inverse=True)
    Pn = codec.random_params(cfg, 3, gain=4.0)
    rng = np.random.default_rng(0)
    Cs, Fs = [], []
    for b in range(2):                                 # the batch of test_gpu_train_step
        occ = rng.random((24, 24, 24)) < 0.1
        xyz = np.argwhere(occ)
        Cs.append(np.concatenate([np.full((len(xyz), 1), b), xyz], axis=1))
        Fs.append(rng.random((len(xyz), 3)).astype(np.float32))
    C, rgb = np.concatenate(Cs).astype(np.int32), np.concatenate(Fs)
    q = t(np.array([[0.3, 0.8], [0.3, 0.8]], np.float32))
    Lam = t(np.array([[4.0, 300.0], [2.0, 100.0]], np.float32))
    model = load_params(UnifiedModel(copy.deepcopy(cfg)), Pn).to(dev()).train()
    noise = {}

    def noise_fn(tag, like):
        if tag not in noise:
            g = torch.Generator(device="cpu").manual_seed(len(noise) + 1)
            noise[tag] = (torch.rand(like.shape, generator=g) - 0.5).to(like.device)
        return noise[tag]
    model.entropy_model.noise_fn = noise_fn
    x = ME.SparseTensor(coordinates=t(C), features=t(rgb))
    out = model(x, q, Lam)
    _, parts_c = Loss(copy.deepcopy(COLOR_LOSS_CFG))(x, out)
    total, parts_s = Loss(copy.deepcopy(SHEPARD_LOSS_CFG))(x, out)
    for name in ("Multiscale_FocalLoss", "bpp-y", "bpp-z"):
        assert torch.equal(parts_s[name].detach(), parts_c[name].detach()), name
    assert torch.isfinite(parts_s["ColorLoss"]) and float(parts_s["ColorLoss"]) > 0
    total.backward()
    grads = {nme: p.grad for nme, p in model.named_parameters() if p.grad is not None}
    assert len(grads) >= 40
    for nme, g in grads.items():
        assert torch.isfinite(g).all(), nme
    assert float(grads["g_s.color_conv.0.kernel"].abs().max()) > 0
    assert float(grads["g_s.color_conv.0.bias"].abs().max()) > 0
