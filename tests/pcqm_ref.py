"""numpy restatement of the PCQM definition in `metrics.pcqm_features` (the test oracle of the two radius kernels), and the
test clouds.  float64 by default; `dtype=np.longdouble` and `reverse=True` (neighbour order reversed) exist to measure the
restatement's own sensitivity (tools/pcqm_tolerances.py -> profiles/pcqm_tolerances.txt).  Loops run over the offset list and
are vectorised over the points."""
import math

import numpy as np

K, C1, C2, C3, C4, C5 = 1.0, 0.002, 0.1, 0.1, 0.002, 0.008
WEIGHTS = (0.0, 0.0, 0.0057, 0.9771, 0.0, 0.0172, 0.0, 0.0)
MIN_FIT = 6
PIVOT_REL = 1e-12
GAP_REL = 1e-3          # a normal is compared only where (l2 - l1) >= GAP_REL * l3 ...
COND_MAX = 1e8          # ... and a fit only where the normal matrix has a condition number <= COND_MAX


def lim_of(radius):
    return math.ceil(radius * radius) - 1


def offsets(radius):
    """Integer offsets with |d|^2 <= ceil(radius^2) - 1 in the order dx, dy, dz ascending."""
    lim = lim_of(radius)
    R = math.isqrt(lim)
    ax = np.arange(-R, R + 1)
    d = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return d[(d * d).sum(axis=1) <= lim]


def canonical(cloud):
    """[N, >= 3] rows -> (rows sorted by (x, y, z) with duplicates dropped, first wins; for every input row the canonical row
    of its cell)."""
    cloud = np.asarray(cloud, dtype=np.float64)
    xyz = np.rint(cloud[:, :3]).astype(np.int64)
    order = np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))          # stable: the first row of a cell stays first
    s = xyz[order]
    first = np.ones(len(s), dtype=bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)
    cell = np.cumsum(first) - 1
    rows = np.empty(len(s), dtype=np.int64)
    rows[order] = cell
    return cloud[order[first]], rows


class Index:
    """Row of every cell of the bounding box grown by `pad` (-1: empty)."""

    def __init__(self, pts, pad):
        self.lo = pts.min(axis=0) - pad
        self.dims = pts.max(axis=0) - self.lo + 1 + pad
        self.grid = np.full(int(np.prod(self.dims)), -1, dtype=np.int64)
        self.flat = self.linear(pts - self.lo)
        self.grid[self.flat] = np.arange(len(pts))

    def linear(self, c):
        return (c[:, 0] * self.dims[1] + c[:, 1]) * self.dims[2] + c[:, 2]

    def rows(self, d):
        """Rows of the cells at offset d from every point (-1: empty)."""
        return self.grid[self.flat + ((d[0] * self.dims[1] + d[1]) * self.dims[2] + d[2])]


def _cholesky(G, g):
    """Vectorised Cholesky solve of G c = g ([n, 6, 6], [n, 6]) in G's dtype: (c, every pivot > PIVOT_REL x the largest
    diagonal entry).  Rows that miss the pivot rule hold garbage."""
    n = G.shape[0]
    U = np.zeros_like(G)
    dmax = np.max(np.stack([G[:, p, p] for p in range(6)], axis=1), axis=1) if n else np.zeros(0, G.dtype)
    ok = np.ones(n, dtype=bool)
    for p in range(6):
        d = G[:, p, p].copy()
        for k in range(p):
            d -= U[:, k, p] * U[:, k, p]
        bad = ~(d > PIVOT_REL * dmax)
        ok &= ~bad
        d[bad] = 1.0
        U[:, p, p] = np.sqrt(d)
        for q in range(p + 1, 6):
            s = G[:, p, q].copy()
            for k in range(p):
                s -= U[:, k, p] * U[:, k, q]
            U[:, p, q] = s / U[:, p, p]
    c = np.zeros_like(g)
    for p in range(6):
        s = g[:, p].copy()
        for k in range(p):
            s -= U[:, k, p] * c[:, k]
        c[:, p] = s / U[:, p, p]
    for p in range(5, -1, -1):
        s = c[:, p].copy()
        for k in range(p + 1, 6):
            s -= U[:, p, k] * c[:, k]
        c[:, p] = s / U[:, p, p]
    return c, ok


def curvature(pts, radius, dtype=np.float64, reverse=False):
    """Curvature field of canonical integer points [n, 3] -> (rho float64 [n], info).  info: `count` neighbourhood sizes,
    `comparable` (>= 6 neighbours, eigen gap and condition number inside the bounds above), `cond` (inf where not fitted),
    `normal`."""
    pts = np.asarray(pts, dtype=np.int64)
    n = len(pts)
    offs = offsets(radius)
    idx = Index(pts, int(np.abs(offs).max()))
    present = np.stack([idx.rows(d) >= 0 for d in offs], axis=1)                 # [n, K]
    cnt = present.sum(axis=1)
    S1 = present.astype(np.int64) @ offs                                          # [n, 3]
    S2 = np.einsum("nk,ki,kj->nij", present.astype(np.int64), offs, offs)
    M = (cnt[:, None, None] * S2 - S1[:, :, None] * S1[:, None, :]).astype(np.float64)
    w, V = np.linalg.eigh(M)
    nv = V[:, :, 0].copy()
    nv /= np.linalg.norm(nv, axis=1, keepdims=True)
    big = np.take_along_axis(nv, np.argmax(np.abs(nv), axis=1)[:, None], axis=1)   # argmax: the first one on a tie
    nv = np.where(big < 0, -nv, nv)
    gap_ok = (w[:, 1] - w[:, 0]) >= GAP_REL * w[:, 2]
    e = np.eye(3)[np.argmin(np.abs(nv), axis=1)]
    u = np.cross(e, nv)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(nv, u)
    nv_, u_, v_ = nv.astype(dtype), u.astype(dtype), v.astype(dtype)
    G = np.zeros((n, 6, 6), dtype=dtype)
    g = np.zeros((n, 6), dtype=dtype)
    ks = range(len(offs) - 1, -1, -1) if reverse else range(len(offs))
    for k in ks:
        sel = np.nonzero(present[:, k])[0]
        if not len(sel):
            continue
        d = offs[k].astype(dtype)
        x, y, z = u_[sel] @ d, v_[sel] @ d, nv_[sel] @ d
        phi = np.stack([x * x, x * y, y * y, x, y, np.ones_like(x)], axis=1)
        G[sel] += phi[:, :, None] * phi[:, None, :]
        g[sel] += phi * z[:, None]
    fit = cnt >= MIN_FIT
    c, ok = _cholesky(G, g)
    ok &= fit
    cond = np.full(n, np.inf)
    if fit.any():
        cond[fit] = np.linalg.cond(G[fit].astype(np.float64))
    if dtype == np.float64:                                                       # the issue's solver where it applies
        good = ok & np.isfinite(cond)
        c = np.zeros_like(g)
        if good.any():
            c[good] = np.linalg.solve(G[good], g[good][:, :, None])[:, :, 0]
        ok = good
    a, b, cc, d1, e1 = (c[:, i] for i in range(5))
    ww = 1 + d1 * d1 + e1 * e1
    rho = np.abs(((1 + e1 * e1) * a - d1 * e1 * b + (1 + d1 * d1) * cc) / (ww * np.sqrt(ww)))
    rho = np.where(ok, rho, 0).astype(np.float64)
    return rho, {"count": cnt, "comparable": fit & gap_ok & (cond <= COND_MAX), "cond": cond, "normal": nv, "fitted": ok}


def rgb_to_lab(rgb, dtype=np.float64):
    c = (np.clip(np.rint(np.asarray(rgb, dtype=np.float64) * 255.0), 0, 255) / 255.0).astype(dtype)
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** dtype(2.4))
    m = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]],
                 dtype=dtype)
    t = (lin @ m.T) / np.array([0.95047, 1.0, 1.08883], dtype=dtype)
    delta = dtype(6.0) / dtype(29.0)
    f = np.where(t > delta ** 3, np.cbrt(np.maximum(t, 0)), t / (3 * delta * delta) + dtype(4.0) / dtype(29.0))
    return np.stack([116 * f[:, 1] - 16, 500 * (f[:, 0] - f[:, 1]), 200 * (f[:, 1] - f[:, 2])], axis=1)


def nearest(a, b):
    """Row of the nearest point of b for every point of a (ties: the smallest row)."""
    out = np.empty(len(a), dtype=np.int64)
    for s in range(0, len(a), 512):
        d = a[s:s + 512, None, :] - b[None, :, :]
        out[s:s + 512] = np.argmin((d * d).sum(axis=2), axis=1)
    return out


def features(pts, table, h, dtype=np.float64, reverse=False, shift=True):
    """Steps 5 and 6: the paired table [n, 10] of canonical points -> features [n, 8] (in `dtype`)."""
    n = len(pts)
    offs = offsets(h)
    idx = Index(np.asarray(pts, dtype=np.int64), int(np.abs(offs).max()))
    t = table.astype(dtype)
    own = t[:, 0::2] if shift else np.zeros((n, 5), dtype=dtype)                 # the centre's R-side value per attribute
    S = np.zeros((n, 17), dtype=dtype)
    inv = dtype(2.0) / (dtype(h) * dtype(h))
    ks = range(len(offs) - 1, -1, -1) if reverse else range(len(offs))
    for k in ks:
        rows = idx.rows(offs[k])
        sel = np.nonzero(rows >= 0)[0]
        if not len(sel):
            continue
        w = np.exp(-dtype(int((offs[k] * offs[k]).sum())) * inv)
        q = t[rows[sel]]
        o = own[sel]
        kr, kd, lr, ld = q[:, 0] - o[:, 0], q[:, 1] - o[:, 0], q[:, 2] - o[:, 1], q[:, 3] - o[:, 1]
        add = [np.ones_like(kr), kr, kd, kr * kr, kd * kd, kr * kd, lr, ld, lr * lr, ld * ld, lr * ld]
        for j in range(3):
            add += [q[:, 4 + 2 * j] - o[:, 2 + j], q[:, 5 + 2 * j] - o[:, 2 + j]]
        S[sel] += w * np.stack(add, axis=1)
    W = S[:, 0]
    zero = dtype(0)
    kmr, kmd, lmr, lmd = S[:, 1] / W, S[:, 2] / W, S[:, 6] / W, S[:, 7] / W
    ksr, ksd = np.sqrt(np.maximum(S[:, 3] / W - kmr * kmr, zero)), np.sqrt(np.maximum(S[:, 4] / W - kmd * kmd, zero))
    kcov = S[:, 5] / W - kmr * kmd
    lsr, lsd = np.sqrt(np.maximum(S[:, 8] / W - lmr * lmr, zero)), np.sqrt(np.maximum(S[:, 9] / W - lmd * lmd, zero))
    lcov = S[:, 10] / W - lmr * lmd
    da, db, dc = ((S[:, 11 + 2 * j] - S[:, 12 + 2 * j]) / W for j in range(3))
    f = np.empty((n, 8), dtype=dtype)
    f[:, 0] = np.abs(kmr - kmd) / (np.maximum(kmr, kmd) + own[:, 0] + K)
    f[:, 1] = np.abs(ksr - ksd) / (np.maximum(ksr, ksd) + K)
    f[:, 2] = np.abs(ksr * ksd - kcov) / (ksr * ksd + K)
    f[:, 3] = 1 - 1 / (C1 * (lmr - lmd) ** 2 + 1)
    f[:, 4] = 1 - (2 * lsr * lsd + C2) / (lsr * lsr + lsd * lsd + C2)
    f[:, 5] = 1 - (lcov + C3) / (lsr * lsd + C3)
    f[:, 6] = 1 - 1 / (C4 * dc * dc + 1)
    f[:, 7] = 1 - 1 / (C5 * np.maximum(da * da + db * db - dc * dc, zero) + 1)
    return f


def pcqm(source, reconstruction, r, h, dtype=np.float64, reverse=False, shift=True):
    """The whole metric: {"pcqm", "f" (means [8]), "features" [n, 8] float64 in R's canonical order, "rows" (canonical row of
    every source row), "rho_r", "rho_d", "info_r", "info_d"}."""
    R, rows = canonical(source)
    D, _ = canonical(reconstruction)
    rp, dp = R[:, :3].astype(np.int64), D[:, :3].astype(np.int64)
    rho_r, info_r = curvature(rp, r, dtype, reverse)
    rho_d, info_d = curvature(dp, r, dtype, reverse)
    nn = nearest(rp, dp)
    lr, ld = rgb_to_lab(R[:, 3:6], dtype), rgb_to_lab(D[:, 3:6], dtype)[nn]
    table = np.stack([rho_r.astype(dtype), rho_d[nn].astype(dtype), lr[:, 0], ld[:, 0], lr[:, 1], ld[:, 1], lr[:, 2], ld[:, 2],
                      np.hypot(lr[:, 1], lr[:, 2]), np.hypot(ld[:, 1], ld[:, 2])], axis=1)
    f = features(rp, table, h, dtype, reverse, shift)
    means = f.mean(axis=0)
    return {"pcqm": float((means * np.array(WEIGHTS, dtype=dtype)).sum()), "f": means.astype(np.float64),
            "features": f.astype(np.float64), "features_native": f, "rows": rows, "rho_r": rho_r, "rho_d": rho_d,
            "info_r": info_r, "info_d": info_d, "pcqm_native": (means * np.array(WEIGHTS, dtype=dtype)).sum()}


# ---- test clouds ------------------------------------------------------------------------------------------------------------
OFFSET = np.array([100, 37, 50])       # the clouds sit away from the origin (bounding lattices whose z extent is no multiple of 64)


def _shell(radius):
    ax = np.arange(-radius - 1, radius + 2)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return p[np.abs(np.sqrt((p * p).sum(axis=1)) - radius) < 0.5]


def positions(name):
    if name == "shell20":
        p = _shell(20)
    elif name == "sheet48":
        x, y = (a.reshape(-1) for a in np.meshgrid(np.arange(48), np.arange(48), indexing="ij"))
        p = np.stack([x, y, np.rint(6 + 4 * np.sin(x / 5) * np.cos(y / 7)).astype(np.int64)], axis=1)
    elif name == "shell30":
        p = _shell(30)
        p = p[p[:, 0] >= 14]                                        # a cap about x: about 3 k of the shell's 11 k points, z extent 55
    elif name == "sparse500":
        p = np.unique(np.random.default_rng(500).integers(0, 40, size=(500, 3)), axis=0)
    elif name == "one":
        p = np.array([[3, 4, 5]])
    elif name == "two":
        p = np.array([[3, 4, 5], [3, 4, 6]])
    else:
        raise KeyError(name)
    return p + OFFSET


def colours(p, seed):
    """Smooth sinusoids of position plus seeded noise, as 8-bit levels / 255."""
    rng = np.random.default_rng(seed)
    q = p.astype(np.float64)
    c = np.stack([0.5 + 0.35 * np.sin(q[:, 0] / 6.0 + q[:, 1] / 9.0), 0.5 + 0.35 * np.cos(q[:, 1] / 5.0 - q[:, 2] / 8.0),
                  0.5 + 0.35 * np.sin(q[:, 2] / 7.0 + q[:, 0] / 11.0)], axis=1)
    c += rng.normal(0.0, 4.0 / 255.0, size=c.shape)
    return np.clip(np.rint(c * 255.0), 0, 255) / 255.0


def cloud(name, seed=1):
    p = positions(name)
    return np.concatenate([p.astype(np.float64), colours(p, seed)], axis=1)


def reconstruction(src, seed=2, keep=0.7, sigma=12.0):
    """A seeded `keep` share of the points with colour noise of `sigma` levels."""
    rng = np.random.default_rng(seed)
    n = len(src)
    sel = np.sort(rng.permutation(n)[:max(1, int(round(keep * n)))])
    out = src[sel].copy()
    out[:, 3:6] = np.clip(np.rint(out[:, 3:6] * 255.0 + rng.normal(0.0, sigma, size=(len(sel), 3))), 0, 255) / 255.0
    return out
