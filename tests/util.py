"""Shared helpers of the test-suite (oracle <-> HIP glue).  The oracle is the checker only."""
import functools

import numpy as np
import torch

from oracle import codec, coords as co

ATOL = 1e-4   # BASELINE.json north_star: fp32 features within 1e-4
RTOL = 1e-4


def dev():
    return torch.device("cuda:0")


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x.to(dtype) if dtype is not None else x


def n(x):
    return x.detach().cpu().numpy()


def cloud_keys(seed, size, p, ts=1, margin=0, batch=1):
    """Random canonical key set on a stride-ts lattice (numpy)."""
    rng = np.random.default_rng(seed)
    Cs = []
    for b in range(batch):
        occ = rng.random((size, size, size)) < p
        xyz = (np.argwhere(occ) + margin) * ts
        Cs.append(np.concatenate([np.full((len(xyz), 1), b, dtype=np.int64), xyz], axis=1))
    C = np.concatenate(Cs, axis=0)
    keys, _ = co.canonicalize(C)
    return keys


def two_batch_keys(seed, ts, shift, sizes=((21, 0.3), (17, 0.2))):
    """Two batch entries of `cloud_keys` (seed, seed + 1) at the given per-batch (size, p), every coordinate moved by
    shift * ts (negative coordinates for shift < 0)."""
    C = []
    for b, (size, p) in enumerate(sizes):
        c = co.unpack_keys(cloud_keys(seed + b, size, p, ts))
        c[:, 0] = b
        c[:, 1:] += shift * ts
        C.append(c)
    return np.unique(co.pack_keys(np.concatenate(C)))


@functools.lru_cache(maxsize=None)
def surface_keys(scale):
    """Voxelised sphere + torus surface (batch 0): ~205 k rows at scale 0.515, ~1.07 M at 1.17 -- the sizes of the training
    step's up-sampled stride-1 candidate sets."""
    from unified_point_cloud_compression_amd import synth
    pc = synth.surface_cloud(0, 10, scale, shuffle=False)
    C = np.concatenate([np.zeros((len(pc), 1), np.int64), pc[:, :3].astype(np.int64)], axis=1)
    return co.canonicalize(C)[0]


@functools.lru_cache(maxsize=None)
def flat_keys():
    """A set flat in z (one z plane): every offset of a 3x3x3 kernel with dz != 0 has no pair."""
    rng = np.random.default_rng(3)
    xy = np.argwhere(rng.random((160, 160)) < 0.5)
    C = np.concatenate([np.zeros((len(xy), 1), np.int64), xy, np.full((len(xy), 1), 7)], axis=1).astype(np.int64)
    return co.canonicalize(C)[0]


def coord_set(keys, ts):
    """The library's CoordSet of canonical keys (numpy) at tensor stride ts, with their bounds."""
    from unified_point_cloud_compression_amd import sparse as S
    C = co.unpack_keys(keys)
    return S.CoordSet(t(keys), len(keys), ts, S.Bounds(int(C[:, 0].max()), C[:, 1:].min(0), C[:, 1:].max(0)))


def shape_rows(x, dist, rng):
    """Feature rows of the float64 kernel tests from Gaussian draws x [n, c]: relu -- non-negative ReLU-like features (about
    half exact zeros); spread -- rows whose magnitudes spread over e^+-6 (one draw of rng per row)."""
    if dist == "relu":
        return np.maximum(x, 0)
    if dist == "spread":
        return x * np.exp(rng.uniform(-6, 6, (x.shape[0], 1))).astype(np.float32)
    raise ValueError(dist)


def conv_sums64(x64, W64, b64, pairs, n_out):
    """The float64 reference of a sparse convolution over the ORACLE's pairs, on the device of x64 (torch float64):
    (sum, sum of squares) [n_out, cout] of the terms of every entry -- b (None: no bias) and x[i][ci] * W[k][ci][co] for every pair
    (i, o) of every offset k.  pairs: [(in_rows, out_rows)] per offset (numpy), or None for the identity (K = 1)."""
    device = x64.device
    ref = torch.zeros((n_out, W64.shape[2]), dtype=torch.float64, device=device)
    sq = torch.zeros_like(ref)
    if b64 is not None:
        ref += b64.reshape(1, -1)
        sq += b64.reshape(1, -1) ** 2
    if pairs is None:
        ref += x64 @ W64[0]
        sq += (x64 * x64) @ (W64[0] * W64[0])
        return ref, sq
    for k, (i, o) in enumerate(pairs):
        if len(i) == 0:
            continue
        xi = x64[torch.from_numpy(i.astype(np.int64)).to(device)]
        oo = torch.from_numpy(o.astype(np.int64)).to(device)
        ref.index_add_(0, oo, xi @ W64[k])
        sq.index_add_(0, oo, (xi * xi) @ (W64[k] * W64[k]))
    return ref, sq


def bits(a):
    """The bit patterns of a float32 device tensor (numpy int32): equality of results bit for bit, NaNs included."""
    return n(a.contiguous().view(torch.int32))


def ratios(got, ref, s2):
    """(max, rms) over the entries of |got - ref| / S2.  Entries without any non-zero term (S2 = 0) must be exactly 0: an
    error there counts as infinite.  The rms runs over the entries with S2 > 0."""
    got = (got if torch.is_tensor(got) else t(got)).double().reshape(ref.shape)
    err = (got - ref).abs()
    on = s2 > 0
    if bool(torch.any(~on & (err != 0))) or not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    if not bool(on.any()):
        return 0.0, 0.0
    r = err[on] / s2[on]
    return float(r.max()), float(torch.sqrt((r * r).mean()))


def load_params(model, P):
    """Copy an oracle parameter dict into a UnifiedModel (same state-dict names)."""
    sd = model.state_dict()
    for k, v in P.items():
        assert k in sd, k
        assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v))
    model.load_state_dict(sd)
    return model


def assert_close(got, want, atol=ATOL, rtol=RTOL, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    bad = err > tol
    rows = np.unique(np.nonzero(bad)[0])[:16].tolist() if bad.ndim >= 1 and bad.any() else []
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} out of tolerance, max err {err.max():.3e} at "
                           f"{np.unravel_index(err.argmax(), err.shape)}; first rows with bad entries {rows}")
