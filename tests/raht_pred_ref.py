"""numpy / Python-int restatement of the predicted RAHT attribute stream 0xB9 ("Prediction from the parent
level") -- test infrastructure, no GPU.

The levels, butterflies, quantiser, colour transform, rows, groups, table family, member choice and container are those of
`tests/raht_ref.py`; the 2 x 2 x 2 weighted mean over the parent level is `tests/raht_lossless_ref.child_predictions` (both
imported, not repeated).  What is new here: a node's mean from its DC, the prediction scaled into the children's domain, its
transform Hp, and the closed loop -- a row travels as quantise(H - Hp) with Hp formed from the DCs the DECODER reconstructs.
`encode` must give the bytes `attributes.encode_attributes(..., predict=True)` gives and also returns its own closed-loop
reconstruction; `decode` reads the bytes back to exactly that.  Run as a script it writes profiles/attribute_pred_rate.json."""
import struct

import numpy as np

from oracle import rans
from tests import raht_lossless_ref as LL
from tests import raht_ref as R

MAGIC, SEGMENT_SYMBOLS, HEADER = 0xB9, R.SEGMENT_SYMBOLS, R.HEADER
LIMIT = 1 << 30
MEAN_LIMIT = 1 << 24       # the clamp on a mean: 64 weighted means sum in int32; a valid stream stays below 2^17


# ---- arithmetic ----------------------------------------------------------------------------------------------------------
def mean(dc, w):
    """m = (a D + 2^29) >> 30 with a = isqrt(((1 << 32) / w) << 28), the Q30 factor of "1 of w", clamped to +-2^24: dc int64 [m, C],
    w int64 [m]."""
    a = R.factors(np.ones_like(w), w - 1)[0]
    return np.clip((a[:, None] * dc + (1 << 29)) >> 30, -MEAN_LIMIT, MEAN_LIMIT)


def scale(pred, w):
    """P = (pred s + 2^15) >> 16 with s = isqrt(w << 32), clamped: pred int64 [..., C], w int64 [...] (w = 0 gives 0)."""
    s = R.isqrt(np.asarray(w, dtype=np.uint64) << np.uint64(32)).astype(np.int64)
    return clamp((pred * s[..., None] + (1 << 15)) >> 16)


def clamp(x):
    return np.clip(x, -LIMIT, LIMIT)


def node_forward(W, X):
    """The three stages of `raht_ref.transform` over children's weights W [m, 8] and values X [m, 8, C] (absent: 0): (DC [m, C],
    H [m, 7, C] in row order, E [m, 7])."""
    W, X = W.copy(), X.copy()
    H = np.zeros((X.shape[0], 7, X.shape[2]), dtype=np.int64)
    E = np.zeros((X.shape[0], 7), dtype=bool)
    for t in (3, 4, 5, 6, 1, 2, 0):
        i, j = R.SLOT_OF_ROW[t]
        X[:, i], H[:, t], E[:, t] = R.forward_pair(W[:, i], W[:, j], X[:, i], X[:, j])
        W[:, i] = W[:, i] + W[:, j]
    return X[:, 0], H, E


def node_inverse(kid, w_child, dc, H):
    """The butterflies of `raht_ref.inverse` for one level, every output clamped as the decoder clamps: children's DCs [m, 8, C]."""
    W7, _ = R._butterflies(kid, w_child)
    X = np.zeros((len(kid), 8, dc.shape[1]), dtype=np.int64)
    X[:, 0] = dc
    for t in range(7):
        i, j = R.SLOT_OF_ROW[t]
        both = ((W7[t][0] > 0) & (W7[t][1] > 0))[:, None]
        x1, x2 = R.inverse_pair(W7[t][0], W7[t][1], X[:, i], H[:, t])
        X[:, i], X[:, j] = np.where(both, clamp(x1), x1), np.where(both, clamp(x2), x2)
    return X


def predicted_hp(cells_l, kid, w_node, w_child, dc):
    """Hp [m, 7, C] of a level's nodes from the level's reconstructed DCs: means, the 27 / 9 / 3 / 1 prediction of every present
    child, scaled by sqrt(w_child), through the node's butterflies."""
    pred = LL.child_predictions(cells_l, mean(dc, w_node), kid)
    W, _ = R._gather(kid, w_child, np.zeros((len(w_child), dc.shape[1]), dtype=np.int64))
    return node_forward(W, scale(pred, W))[1]


def level_rebuild(cells_l, kid, w_node, w_child, dc, q, st):
    """What encoder and decoder share: Hp, H' = clamp(clamp(Hp) + clamp(q step)), the inverse butterflies -> children's DCs
    [nodes(l + 1), C].  q [m, 7, C] is 0 where no butterfly exists."""
    Hp = predicted_hp(cells_l, kid, w_node, w_child, dc)
    X = node_inverse(kid, w_child, clamp(dc), clamp(clamp(Hp) + clamp(q * st[None, None, :])))
    nxt = np.zeros((len(w_child), dc.shape[1]), dtype=np.int64)
    have = kid >= 0
    nxt[kid[have]] = X[have]
    return nxt


def closed_loop(cells, values, st, report=None):
    """values int64 [n, C] (Q8) -> (quantised root DC [C], symbol rows [n - 1, C] level 0 first, stage, level, reconstructed
    values [n, C])."""
    depth, kids = R.level_plan(cells)
    lv = LL.level_cells(cells)[1]
    w = R._weights(kids, len(values))
    v, Hs, Es = values, [None] * depth, [None] * depth
    for l in range(depth - 1, -1, -1):                                     # the true, unquantised H of every level
        v, Hs[l], Es[l] = node_forward(*R._gather(kids[l], w[l + 1], v))
    q_root = R.quantise(v[0], st)
    dc = clamp(q_root * st)[None, :]
    rows, stages, lvls = [], [], []
    for l in range(depth):
        E = Es[l]
        Hp = predicted_hp(lv[l], kids[l], w[l], w[l + 1], dc)
        if report is not None:
            report["max_abs_residual"] = max(report.get("max_abs_residual", 0), int(np.abs(Hs[l] - Hp)[E].max(initial=0)))
        q = np.where(E[:, :, None], R.quantise(Hs[l] - clamp(Hp), st[None, None, :]), 0)
        rows.append(q[E])
        stages.append(np.broadcast_to(R.STAGE_OF_ROW, E.shape)[E])
        lvls.append(np.full(int(E.sum()), l))
        dc = level_rebuild(lv[l], kids[l], w[l], w[l + 1], dc, q, st)
    return q_root, np.concatenate(rows), np.concatenate(stages), np.concatenate(lvls), dc


def finish(v, colour):
    return R.ycc_to_rgb(v) if colour else np.clip((v + 128) >> 8, 0, 255).astype(np.uint8)


# ---- the stream ------------------------------------------------------------------------------------------------------------
def encode(points, attrs, qp, chroma_qp_offset=-2, colour=True, segment_symbols=SEGMENT_SYMBOLS, report=None):
    """points [N, >= 3] distinct voxels (N >= 2) in any order, attrs uint8 [N, C] -> (bytes, the uint8 [N, C] levels the decoder
    will return, canonical order)."""
    cells, attrs = R.canonical(points, attrs)
    n, C = attrs.shape
    assert n >= 2, "fewer than two voxels travel as 0xB3"
    depth = R.level_plan(cells)[0]
    colour = bool(colour) and C == 3
    qp = min(max(int(qp), 4), 51)
    st = np.array(R.steps_for(qp, chroma_qp_offset, C), dtype=np.int64)
    q_root, rows, stage, lvl, rec = closed_loop(cells, R.q8_values(attrs, colour), st, report)
    out = bytearray(HEADER.pack(MAGIC, n, depth, C, 1 if colour else 0, qp, chroma_qp_offset))
    for c in range(C):
        out += R._zigzag(q_root[c])
    cls = (np.arange(C) > 0).astype(np.int64)
    grp = (lvl[:, None] * 6 + cls[None, :] * 3 + stage[:, None]).reshape(-1)
    sym = rows.reshape(-1)
    side, hist = R.choose_members(sym, grp, depth * 6)
    out += bytes(side.tolist())
    if report is not None:
        report.update(n=n, depth=depth, symbols=len(sym), escapes=int((np.abs(sym) > 63).sum()), sym=sym, grp=grp,
                      model_bits256=int((hist * R.tables()[1][side]).sum()))
    cdf, _ = R.tables()
    idx = side[grp]
    segs = max(1, min(-(-len(sym) // max(1, int(segment_symbols))), 65536))
    per = -(-len(sym) // segs)
    streams = [rans.encode(sym[s * per:(s + 1) * per], idx[s * per:(s + 1) * per], cdf, R.SIZES, R.OFFSETS) for s in range(segs)]
    body = struct.pack(f"<I{segs}I", segs, *[len(s) // 4 for s in streams]) + b"".join(streams)
    out += struct.pack("<I", len(body)) + body
    return bytes(out), finish(rec, colour)


def decode(data, points):
    """bytes + the geometry (any row order) -> uint8 [n, C] in canonical order."""
    magic, n, depth, C, flags, qp, off = HEADER.unpack_from(data, 0)
    assert magic == MAGIC and n >= 2
    cells = np.unique(np.floor(np.asarray(points)[:, :3]).astype(np.int64), axis=0)
    d2, kids = R.level_plan(cells)
    assert n == len(cells) and depth == d2
    lv = LL.level_cells(cells)[1]
    st = np.array(R.steps_for(qp, off, C), dtype=np.int64)
    at = HEADER.size
    q_root = []
    for c in range(C):
        q, at = R._unzigzag(data, at)
        q_root.append(q)
    side = np.frombuffer(data, np.uint8, depth * 6, at).astype(np.int64)
    at += depth * 6
    w = R._weights(kids, n)
    Es = [R._butterflies(kids[l], w[l + 1])[1] for l in range(depth)]
    stage = np.concatenate([np.broadcast_to(R.STAGE_OF_ROW, E.shape)[E] for E in Es])
    lvl = np.concatenate([np.full(int(E.sum()), l) for l, E in enumerate(Es)])
    cls = (np.arange(C) > 0).astype(np.int64)
    idx = side[(lvl[:, None] * 6 + cls[None, :] * 3 + stage[:, None]).reshape(-1)]
    nbytes = struct.unpack_from("<I", data, at)[0]
    body = data[at + 4:at + 4 + nbytes]
    at += 4 + nbytes
    assert at == len(data)
    segs = struct.unpack_from("<I", body, 0)[0]
    words = struct.unpack_from(f"<{segs}I", body, 4)
    per, p, parts = -(-len(idx) // segs), 4 * (1 + segs), []
    cdf, _ = R.tables()
    for s in range(segs):
        parts.append(rans.decode(body[p:p + 4 * words[s]], idx[s * per:(s + 1) * per], cdf, R.SIZES, R.OFFSETS))
        p += 4 * words[s]
    sym = np.concatenate(parts).astype(np.int64).reshape(n - 1, C)
    dc = clamp(np.array(q_root, dtype=np.int64) * st)[None, :]
    row = 0
    for l in range(depth):
        q = np.zeros((len(kids[l]), 7, C), dtype=np.int64)
        cnt = int(Es[l].sum())
        q[Es[l]] = sym[row:row + cnt]
        row += cnt
        dc = level_rebuild(lv[l], kids[l], w[l], w[l + 1], dc, q, st)
    assert row == n - 1
    return finish(dc, bool(flags & 1))


# ---- rate ------------------------------------------------------------------------------------------------------------------
def rate_pair(pc, lv, qp):
    """One row of profiles/attribute_pred_rate.json: the 0xB3 and the 0xB9 stream of the same input, each decoded."""
    orig = R.canonical(pc, lv)[1]
    rp, rq = {}, {}
    plain = R.encode(pc, lv, qp, report=rp)
    pred, rec = encode(pc, lv, qp, report=rq)
    assert np.array_equal(decode(pred, pc), rec)
    streams = -(-rp["symbols"] // SEGMENT_SYMBOLS)
    row = {"framing_bytes": 12 * streams}
    for name, data, rep, out in (("plain", plain, rp, R.decode(plain, pc)), ("predicted", pred, rq, rec)):
        row[name] = {"stream_bytes": len(data), "member_cost_bytes": round(rep["model_bits256"] / 2048, 1), "escapes": rep["escapes"],
                     "y_psnr_db": round(R.y_psnr(orig, out), 3)}
    row["y_psnr_gain_db"] = round(R.y_psnr(orig, rec) - R.y_psnr(orig, R.decode(plain, pc)), 4)
    row["max_abs_residual"] = rq["max_abs_residual"]
    return row


def rate_report(bits=(7, 8), qps=(22, 28, 34, 40)):
    from unified_point_cloud_compression_amd import synth
    out = {}
    for b in bits:
        pc = synth.surface_cloud(0, b)
        for name, colours in ((f"surface{b}", pc[:, 3:]), (f"surface{b}_noise_free", LL.noise_free_colours(pc, b))):
            lv = R.levels_of(colours)
            out[name] = {"points": len(pc), "qp": {str(qp): rate_pair(pc, lv, qp) for qp in qps}}
    return out


if __name__ == "__main__":
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clouds = rate_report()
    gated = [clouds[k]["qp"][q]["y_psnr_gain_db"] for k in ("surface7", "surface7_noise_free") for q in ("22", "28", "34")]
    doc = {"what": "lossy RAHT colour with and without the prediction from the parent level (streams 0xB9 and 0xB3, DESIGN.md 7f), numpy "
                   "reference coders, chroma_qp_offset -2, colour transform on: stream bytes, the integer cost the members were chosen by "
                   "(member_cost_bytes: no framing, no header), framing_bytes = 12 per rANS stream of 1024 symbols (the same on both "
                   "sides), luma PSNR of the decoded 8-bit colours, y_psnr_gain_db = predicted - plain; every 0xB9 stream was decoded "
                   "back to its encoder's closed-loop reconstruction; worst_y_psnr_shortfall_db is over surface7 and "
                   "surface7_noise_free at qp 22, 28, 34, the cases tests/test_cpu_attributes_pred.py gates",
           "worst_y_psnr_shortfall_db": round(max(0.0, -min(gated)), 4),
           "clouds": clouds}
    with open(os.path.join(root, "profiles", "attribute_pred_rate.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
