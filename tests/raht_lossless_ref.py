"""numpy / Python-int restatement of the lossless attribute stream -- test infrastructure, no GPU.

The levels, the stage order, the slot pairs, the row order, the groups, the table family and the member choice are those of
`tests/raht_ref.py` (imported, not repeated); what is new here is the arithmetic: YCoCg-R, the integer lifting butterfly, the
prediction of a node's children from the node's own level, and the stored mode.  `encode` must give the bytes
`attributes.encode_attributes_lossless` gives; `decode` returns the uint8 rows that went in.  All divisions are numpy's `//` on
int64 (floor), all shifts arithmetic.  Run as a script it writes profiles/attribute_lossless_rate.json."""
import struct

import numpy as np

from oracle import rans
from tests import raht_ref as R

MAGIC, SEGMENT_SYMBOLS, MAX_C = 0xB5, R.SEGMENT_SYMBOLS, R.MAX_C
HEADER = struct.Struct("<BIBBB")
F_COLOUR, F_PREDICT, F_STORED = 1, 2, 4
SYMBOL_LIMIT = 1023
CELL_WEIGHT = (27, 9, 3, 1)                                                # by the number of non-zero components of b


# ---- arithmetic ----------------------------------------------------------------------------------------------------------
def rgb_to_ycocg(rgb):
    r, g, b = (rgb[:, i].astype(np.int64) for i in range(3))
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    return np.stack([t + (cg >> 1), co, cg], axis=1)


def ycocg_to_rgb(v):
    y, co, cg = v[:, 0], v[:, 1], v[:, 2]
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    return np.stack([b + co, g, b], axis=1)


def ranges(C, colour):
    """(lo [C], hi [C]): the legal range of every channel."""
    lo, hi = np.zeros(C, dtype=np.int64), np.full(C, 255, dtype=np.int64)
    if colour:
        lo[1:], hi[1:] = -255, 255
    return lo, hi


def lift_pair(w1, w2, x1, x2):
    """(L, H, both) of sibling slots with weights w [m] and values x [m, C]; an absent slot has weight 0 and value 0, a lone
    sibling passes through (H is 0 there and not emitted)."""
    both = (w1 > 0) & (w2 > 0)
    w = np.maximum(w1 + w2, 1)[:, None]
    hi = x2 - x1
    lo = x1 + (w2[:, None] * hi) // w
    return np.where(both[:, None], lo, x1 + x2), np.where(both[:, None], hi, 0), both


def unlift_pair(w1, w2, lo, hi):
    both = (w1 > 0) & (w2 > 0)
    w = np.maximum(w1 + w2, 1)[:, None]
    x1 = lo - (w2[:, None] * hi) // w
    x2 = hi + x1
    x1 = np.where(both[:, None], x1, np.where((w1 > 0)[:, None], lo, 0))
    x2 = np.where(both[:, None], x2, np.where((w2 > 0)[:, None], lo, 0))
    return x1, x2


def lift_node(W, X):
    """Three stages over children's weights W [m, 8] and values X [m, 8, C] (absent: 0).  Returns (node value [m, C],
    H [m, 7, C] in row order, E [m, 7]: which butterflies exist)."""
    W, X = W.copy(), X.copy()
    H = np.zeros((X.shape[0], 7, X.shape[2]), dtype=np.int64)
    E = np.zeros((X.shape[0], 7), dtype=bool)
    for t in (3, 4, 5, 6, 1, 2, 0):                                        # stage 1, then 2, then 3; results go to the first slot
        i, j = R.SLOT_OF_ROW[t]
        X[:, i], H[:, t], E[:, t] = lift_pair(W[:, i], W[:, j], X[:, i], X[:, j])
        W[:, i] = W[:, i] + W[:, j]
    return X[:, 0], H, E


def predict_cell(values, present):
    """values [..., 8] of the cells b = bx<<2 | by<<1 | bz and which are present -> floor((num + (den >> 1)) / den)."""
    wt = np.array([CELL_WEIGHT[bin(b).count("1")] for b in range(8)], dtype=np.int64)
    den = (wt * present).sum(axis=-1)
    num = (wt * present * values).sum(axis=-1)
    return (num + (den >> 1)) // den


def level_cells(cells):
    """depth and [level 0, ..., level depth] as int64 [nodes, 3] origin-relative cells in canonical order."""
    rel = cells - cells.min(axis=0)
    depth = max(1, int(rel.max()).bit_length())
    return depth, [np.unique(rel >> (depth - l), axis=0) for l in range(depth + 1)]


def child_predictions(cells, v, kid):
    """Predictions [m, 8, C] of the children of a level's nodes (cells [m, 3], values v [m, C]) from the level itself; 0 where
    kid [m, 8] has no child."""
    m, C = v.shape
    lin = R._lin(cells)
    pred = np.zeros((m, 8, C), dtype=np.int64)
    for j in range(8):
        d = np.array([2 * ((j >> 2) & 1) - 1, 2 * ((j >> 1) & 1) - 1, 2 * (j & 1) - 1], dtype=np.int64)
        vals = np.zeros((m, C, 8), dtype=np.int64)
        have = np.zeros((m, 8), dtype=np.int64)
        for b in range(8):
            q = cells + d * np.array([(b >> 2) & 1, (b >> 1) & 1, b & 1], dtype=np.int64)
            ok = (q >= 0).all(axis=1)
            at = np.searchsorted(lin, R._lin(np.where(ok[:, None], q, 0)))
            at = np.minimum(at, m - 1)
            ok &= lin[at] == R._lin(np.where(ok[:, None], q, 0))
            have[:, b] = ok
            vals[:, :, b] = np.where(ok[:, None], v[at], 0)
        assert have[:, 0].all()
        pred[:, j] = predict_cell(vals, have[:, None, :])
    return np.where((kid >= 0)[:, :, None], pred, 0)


def transform(cells, values, predict, check=None):
    """Bottom-up lifting of values int64 [n, C], then per level the residuals.  Returns (root [C], symbol rows [n - 1, C],
    level 0 first, stage [n - 1], level [n - 1]).  check: a dict that receives max |H| and whether every L stayed inside the
    range (lo, hi) it names."""
    depth, kids = R.level_plan(cells)
    _, lv_cells = level_cells(cells)
    w = R._weights(kids, len(values))
    v = [None] * depth + [values]
    Hs, Es = [None] * depth, [None] * depth
    for l in range(depth - 1, -1, -1):
        W, X = R._gather(kids[l], w[l + 1], v[l + 1])
        v[l], Hs[l], Es[l] = lift_node(W, X)
        if check is not None:
            check["max_abs_h"] = np.maximum(check.get("max_abs_h", 0), np.abs(Hs[l]).max(axis=(0, 1), initial=0))
            check["inside"] = check.get("inside", True) and bool(np.all(v[l] >= check["lo"]) and np.all(v[l] <= check["hi"]))
    rows, stages, lvls = [], [], []
    for l in range(depth):
        H, E = Hs[l], Es[l]
        if predict:
            W, _ = R._gather(kids[l], w[l + 1], v[l + 1])
            _, Hp, Ep = lift_node(W, child_predictions(lv_cells[l], v[l], kids[l]))
            assert np.array_equal(E, Ep)
            H = H - Hp
        rows.append(H[E])
        stages.append(np.broadcast_to(R.STAGE_OF_ROW, E.shape)[E])
        lvls.append(np.full(int(E.sum()), l))
    return v[0][0], np.concatenate(rows), np.concatenate(stages), np.concatenate(lvls)


def inverse(cells, root, sym, predict, lo, hi):
    """Top-down: root [C] and symbol rows [n - 1, C] -> values int64 [n, C]; raises ValueError where the decoder would clamp."""
    depth, kids = R.level_plan(cells)
    _, lv_cells = level_cells(cells)
    n = len(cells)
    w = R._weights(kids, n)
    v = np.asarray(root, dtype=np.int64)[None, :]
    C, at = v.shape[1], 0
    if np.abs(sym).max(initial=0) > SYMBOL_LIMIT:
        raise ValueError("a symbol beyond +-1023")
    for l in range(depth):
        kid = kids[l]
        W7, E = R._butterflies(kid, w[l + 1])
        H = np.zeros((len(kid), 7, C), dtype=np.int64)
        cnt = int(E.sum())
        H[E] = sym[at:at + cnt]
        at += cnt
        if predict:
            W, _ = R._gather(kid, w[l + 1], np.zeros((len(w[l + 1]), C), dtype=np.int64))
            H = H + lift_node(W, child_predictions(lv_cells[l], v, kid))[1]
        X = np.zeros((len(kid), 8, C), dtype=np.int64)
        X[:, 0] = v
        for t in (0, 1, 2, 3, 4, 5, 6):
            i, j = R.SLOT_OF_ROW[t]
            X[:, i], X[:, j] = unlift_pair(W7[t][0], W7[t][1], X[:, i], H[:, t])
            if np.any(X < lo) or np.any(X > hi):
                raise ValueError("a reconstructed value left its channel's range")
        nxt = np.zeros((len(w[l + 1]), C), dtype=np.int64)
        have = kid >= 0
        nxt[kid[have]] = X[have]
        v = nxt
    assert at == len(sym)
    return v


# ---- the stream ------------------------------------------------------------------------------------------------------------
def encode(points, attrs, colour=True, predict=True, segment_symbols=SEGMENT_SYMBOLS, stored=None, report=None):
    """points [N, >= 3] distinct voxels in any order, attrs uint8 [N, C] -> bytes.  stored: None = the stream's own rule (raw
    bytes when the coded stream would be longer than header + n * C), False = never (tests of the coded path at tiny n)."""
    cells, attrs = R.canonical(points, attrs) if len(points) else (np.zeros((0, 3), dtype=np.int64), np.asarray(attrs))
    n, C = attrs.shape
    colour = bool(colour) and C == 3
    flags = (F_COLOUR if colour else 0) | (F_PREDICT if predict else 0)
    if n == 0:
        depth, root, side, body = 0, np.zeros(C, dtype=np.int64), b"", b""
    else:
        depth = level_cells(cells)[0]
        lo, hi = ranges(C, colour)
        values = rgb_to_ycocg(attrs) if colour else attrs.astype(np.int64)
        check = {"lo": lo, "hi": hi} if report is not None else None
        root, rows, stage, lvl = transform(cells, values, predict, check)
        cls = (np.arange(C) > 0).astype(np.int64)
        grp = (lvl[:, None] * 6 + cls[None, :] * 3 + stage[:, None]).reshape(-1)
        sym = rows.reshape(-1)
        sd, hist = R.choose_members(sym, grp, depth * 6)
        side, body = bytes(sd.tolist()), b""
        if report is not None:
            report.update(n=n, depth=depth, symbols=len(sym), escapes=int((np.abs(sym) > 63).sum()), side=sd.reshape(depth, 6), hist=hist,
                          sym=sym, grp=grp, model_bits256=int((hist * R.tables()[1][sd]).sum()), max_abs_h=check["max_abs_h"],
                          inside=check["inside"], max_abs_symbol=int(np.abs(sym).max(initial=0)))
        if n > 1:
            cdf, _ = R.tables()
            idx = sd[grp]
            segs = max(1, min(-(-len(sym) // max(1, int(segment_symbols))), 65536))
            per = -(-len(sym) // segs)
            streams = [rans.encode(sym[s * per:(s + 1) * per], idx[s * per:(s + 1) * per], cdf, R.SIZES, R.OFFSETS) for s in range(segs)]
            body = struct.pack(f"<I{segs}I", segs, *[len(s) // 4 for s in streams]) + b"".join(streams)
            body = struct.pack("<I", len(body)) + body
    out = bytearray(HEADER.pack(MAGIC, n, depth, C, flags))
    for c in range(C):
        out += R._zigzag(root[c])
    out += side + body
    if report is not None:
        report["coded_bytes"] = len(out)
    if stored is None and len(out) > HEADER.size + n * C:
        if report is not None:
            report["stored"] = True
        return HEADER.pack(MAGIC, n, depth, C, F_STORED) + np.ascontiguousarray(attrs, dtype=np.uint8).tobytes()
    return bytes(out)


def decode(data, points):
    """bytes + the geometry (any row order) -> uint8 [n, C] in canonical order."""
    magic, n, depth, C, flags = HEADER.unpack_from(data, 0)
    assert magic == MAGIC
    cells = np.unique(np.floor(np.asarray(points)[:, :3]).astype(np.int64), axis=0) if len(points) else np.zeros((0, 3), dtype=np.int64)
    assert n == len(cells) and depth == (level_cells(cells)[0] if n else 0)
    at = HEADER.size
    if flags & F_STORED:
        assert flags == F_STORED and len(data) == at + n * C
        return np.frombuffer(data, np.uint8, n * C, at).reshape(n, C).copy()
    colour, predict = bool(flags & F_COLOUR), bool(flags & F_PREDICT)
    root = []
    for c in range(C):
        q, at = R._unzigzag(data, at)
        root.append(q)
    if n == 0:
        assert at == len(data)
        return np.zeros((0, C), dtype=np.uint8)
    side = np.frombuffer(data, np.uint8, depth * 6, at).astype(np.int64)
    at += depth * 6
    sym = np.zeros((n - 1, C), dtype=np.int64)
    _, kids = R.level_plan(cells)
    if n > 1:
        w = R._weights(kids, n)
        E_stage, E_lvl = [], []
        for l in range(depth):
            _, E = R._butterflies(kids[l], w[l + 1])
            E_stage.append(np.broadcast_to(R.STAGE_OF_ROW, E.shape)[E])
            E_lvl.append(np.full(int(E.sum()), l))
        stage, lvl = np.concatenate(E_stage), np.concatenate(E_lvl)
        cls = (np.arange(C) > 0).astype(np.int64)
        idx = side[(lvl[:, None] * 6 + cls[None, :] * 3 + stage[:, None]).reshape(-1)]
        nbytes = struct.unpack_from("<I", data, at)[0]
        body = data[at + 4:at + 4 + nbytes]
        at += 4 + nbytes
        segs = struct.unpack_from("<I", body, 0)[0]
        words = struct.unpack_from(f"<{segs}I", body, 4)
        per, p, parts = -(-len(idx) // segs), 4 * (1 + segs), []
        cdf, _ = R.tables()
        for s in range(segs):
            parts.append(rans.decode(body[p:p + 4 * words[s]], idx[s * per:(s + 1) * per], cdf, R.SIZES, R.OFFSETS))
            p += 4 * words[s]
        sym = np.concatenate(parts).astype(np.int64).reshape(n - 1, C)
    assert at == len(data)
    lo, hi = ranges(C, colour)
    v = inverse(cells, root, sym, predict, lo, hi)
    if colour:
        v = ycocg_to_rgb(v)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


# ---- rate ------------------------------------------------------------------------------------------------------------------
def noise_free_colours(pc, bits):
    """The smooth colour field `synth.surface_cloud` adds its noise to, evaluated at the cloud's own voxels."""
    p = np.floor(pc[:, :3]).astype(np.float64) / float(1 << bits)
    return np.stack([0.5 + 0.5 * np.sin(6.0 * p[:, 0] + 1.0), 0.5 + 0.5 * np.cos(5.0 * p[:, 1]), 0.5 + 0.5 * np.sin(4.0 * (p[:, 2] + p[:, 0]))],
                    axis=1).astype(np.float32)


def rate_row(pc, lv, predict):
    rep = {}
    data = encode(pc, lv, predict=predict, report=rep)
    assert np.array_equal(decode(data, pc), R.canonical(pc, lv)[1])
    ent = R.empirical_entropy_bytes(rep["sym"], rep["grp"] // 6)
    streams = -(-rep["symbols"] // SEGMENT_SYMBOLS)
    return {"stream_bytes": len(data), "bits_per_point": round(8 * len(data) / rep["n"], 4), "stored": bool(rep.get("stored")),
            "coded_bytes": rep["coded_bytes"], "streams": streams, "framing_bytes": 12 * streams,
            "member_cost_bytes": round(rep["model_bits256"] / 2048, 1), "member_cost_bits_per_point": round(rep["model_bits256"] / 256 / rep["n"], 4),
            "per_level_empirical_entropy_bytes": round(ent, 1), "entropy_bits_per_point": round(8 * ent / rep["n"], 4),
            "escapes": rep["escapes"], "max_abs_symbol": rep["max_abs_symbol"]}


def rate_report():
    from unified_point_cloud_compression_amd import synth
    out = {}
    s7, s8 = synth.surface_cloud(0, 7), synth.surface_cloud(0, 8)
    for name, pc, colours in (("surface7", s7, s7[:, 3:]), ("surface8", s8, s8[:, 3:]), ("surface8_noise_free", s8, noise_free_colours(s8, 8))):
        lv = R.levels_of(colours)
        out[name] = {"points": len(pc), "raw_bits_per_point": 24, "predict": rate_row(pc, lv, True), "no_predict": rate_row(pc, lv, False)}
    return out


if __name__ == "__main__":
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = {"what": "lossless colour stream (DESIGN.md 7i), numpy reference coder, YCoCg-R on, with and without the prediction from the "
                   "parent level: stream bytes against the integer cost the members were chosen by (member_cost_bytes: no framing, no "
                   "header) and the per-level zeroth-order entropy of the same symbols; framing_bytes = 12 per rANS stream of 1024 symbols; "
                   "every stream was decoded back to the input's levels; surface8_noise_free carries the generator's smooth colour field at surface8's "
                   "voxels; nothing is gated on these figures",
           "clouds": rate_report()}
    with open(os.path.join(root, "profiles", "attribute_lossless_rate.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["clouds"], indent=1))
