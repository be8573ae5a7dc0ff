"""numpy restatement of the inter-frame RAHT attribute stream, format 0xB4 ("Inter frames") -- test
infrastructure, no GPU.

The levels, the butterflies, the quantiser, the family, the member choice and the container are those of `tests/raht_ref.py`
(imported, not repeated); the blocks and the match of every voxel in the motion-compensated reference those of
`tests/raht_lossless_inter_ref.py` (`block_plan`, `match_rows`), the vectors those of `tests/geom_inter_ref.py`.  New here: the
prediction signal P over the current voxels, its forward transform, the per-block mode decision on quantised symbols, the
extra group set and the stream.  `encode` must give the bytes `attributes.encode_attributes(..., reference=, mode=)` gives;
`decode` returns the uint8 rows `attributes.decode_attributes(..., reference=)` returns.  Run as a script it writes
profiles/attribute_inter_lossy_rate.json."""
import functools
import struct

import numpy as np

from oracle import rans
from tests import geom_inter_ref as GI
from tests import raht_lossless_inter_ref as LI
from tests import raht_ref as R

MAGIC, BLOCK_LOG2, SEARCH, MAX_DEPTH = 0xB4, GI.BLOCK_LOG2, GI.SEARCH, 14
HEADER = struct.Struct("<BIBBBBbBBI")
SEGMENT_SYMBOLS = R.SEGMENT_SYMBOLS
LIMIT = 1 << 30
QPS = (4, 28, 40)


# ---- the prediction --------------------------------------------------------------------------------------------------------
def prediction(cells, ref_cells, ref_lv, colour):
    """(P int64 [n, C] Q8, has_match bool [blocks], block row per voxel, match row per voxel): a matched voxel takes its match's
    prepared row, an unmatched one its block's floor-divided mean of the matched rows; a block without a match stays zero."""
    m, _, _ = LI.match_rows(cells, ref_cells)
    _, _, _, blocks, brow = LI.block_plan(cells)
    C = ref_lv.shape[1]
    rv = R.q8_values(ref_lv, colour) if len(ref_lv) else np.zeros((0, C), dtype=np.int64)
    hit = m >= 0
    P = np.zeros((len(cells), C), dtype=np.int64)
    P[hit] = rv[m[hit]]
    cnt = np.bincount(brow[hit], minlength=len(blocks)).astype(np.int64)
    sums = np.zeros((len(blocks), C), dtype=np.int64)
    np.add.at(sums, brow[hit], P[hit])
    mean = sums // np.maximum(cnt, 1)[:, None]                     # floor division: chroma sums are negative
    P[~hit] = mean[brow[~hit]]
    return P, cnt > 0, brow, m


def forward_levels(kids, w, values):
    """`raht_ref.transform` level by level: (H[l] int64 [m, 7, C] unquantised, E[l] bool [m, 7], V[l] the DCs, V[-1] = values)
    of the levels kids[0 .. len(kids) - 1] over children's weights w[l + 1]."""
    C = values.shape[1]
    H, E, V = [None] * len(kids), [None] * len(kids), [None] * len(kids) + [values]
    for l in range(len(kids) - 1, -1, -1):
        W, X = R._gather(kids[l], w[l + 1], V[l + 1])
        H[l] = np.zeros((len(kids[l]), 7, C), dtype=np.int64)
        E[l] = np.zeros((len(kids[l]), 7), dtype=bool)
        for t in (3, 4, 5, 6, 1, 2, 0):
            i, j = R.SLOT_OF_ROW[t]
            X[:, i], H[l][:, t], E[l][:, t] = R.forward_pair(W[:, i], W[:, j], X[:, i], X[:, j])
            W[:, i] = W[:, i] + W[:, j]
        V[l] = X[:, 0]
    return H, E, V


def node_blocks(cells, depth, first, blocks):
    """Per level l >= first the block row of every node."""
    rel = cells - cells.min(axis=0)
    lb = GI._lin(blocks)
    return {l: np.searchsorted(lb, GI._lin(np.unique(rel >> (depth - l), axis=0) >> (l - first))) for l in range(first, depth)}


def _layout(E, nblk, mode, depth, first, C):
    """Group of every symbol: rows of levels >= first inside mode-1 blocks take the groups of level `depth`."""
    grp = []
    cls = (np.arange(C) > 0).astype(np.int64)
    for l in range(depth):
        stage = np.broadcast_to(R.STAGE_OF_ROW, E[l].shape)[E[l]]
        lvl = np.full(len(stage), l, dtype=np.int64)
        if l >= first:
            lvl[np.broadcast_to(mode[nblk[l]][:, None], E[l].shape)[E[l]]] = depth
        grp.append((lvl[:, None] * 6 + cls[None, :] * 3 + stage[:, None]).reshape(-1))
    return np.concatenate(grp)


def _finish(v, colour):
    return R.ycc_to_rgb(v) if colour else np.clip((v + 128) >> 8, 0, 255).astype(np.uint8)


# ---- the stream ------------------------------------------------------------------------------------------------------------
def encode_inter(points, attrs, qp, ref_points, ref_attrs, chroma_qp_offset=-2, colour=True, segment_symbols=SEGMENT_SYMBOLS,
                 report=None):
    """The 0xB4 stream, or None where there is none (depth 15); fewer than two voxels travel as the intra stream."""
    if len(points) < 2:
        return R.encode(points, attrs, qp, chroma_qp_offset, colour, segment_symbols)
    cells, attrs = R.canonical(points, attrs)
    n, C = attrs.shape
    colour = bool(colour) and C == 3
    qp = min(max(int(qp), 4), 51)
    st = np.array(R.steps_for(qp, chroma_qp_offset, C), dtype=np.int64)
    _, depth, bl, blocks, brow = LI.block_plan(cells)
    if depth > MAX_DEPTH:
        return None
    first = depth - bl
    ref_cells, ref_lv = LI.reference_rows(ref_points, ref_attrs, C)
    P, has_match, _, m = prediction(cells, ref_cells, ref_lv, colour)
    _, kids = R.level_plan(cells)
    w = R._weights(kids, n)
    H, E, V = forward_levels(kids, w, R.q8_values(attrs, colour))
    Hp, _, Vp = forward_levels(kids, w, P)
    nblk = node_blocks(cells, depth, first, blocks)
    q0 = {l: R.quantise(H[l], st[None, None, :]) for l in range(first, depth)}
    q1 = {l: R.quantise(H[l] - Hp[l], st[None, None, :]) for l in range(first, depth)}
    cost = np.zeros((2, len(blocks)), dtype=np.int64)
    for l in range(first, depth):
        for k, q in enumerate((q0[l], q1[l])):
            cost[k] += np.bincount(nblk[l], weights=(np.abs(q) * E[l][:, :, None]).sum(axis=(1, 2)), minlength=len(blocks)).astype(np.int64)
    mode = has_match & (cost[1] < cost[0])
    # the levels above the blocks: the prediction's block DCs after the decision
    Hu, _, Vu = forward_levels(kids[:first], w[:first + 1], Vp[first] * mode[:, None])
    dcp = Vu[0][0]
    sym, hp_rows = [], []
    for l in range(depth):
        if l < first:
            sym.append(R.quantise(H[l] - Hu[l], st[None, None, :])[E[l]])
            hp_rows.append(Hu[l][E[l]])
        else:
            keep = mode[nblk[l]][:, None, None]
            sym.append(np.where(keep, q1[l], q0[l])[E[l]])
            hp_rows.append(np.where(keep, Hp[l], 0)[E[l]])
    sym, hp_rows = np.concatenate(sym), np.concatenate(hp_rows)
    root = R.quantise(V[0][0] - dcp, st)
    grp = _layout(E, nblk, mode, depth, first, C)
    flat = sym.reshape(-1)
    groups = (depth + 1) * 6
    side, hist = R.choose_members(flat, grp, groups)
    cdf, _ = R.tables()
    idx = side[grp]
    segs = max(1, min(-(-len(flat) // max(1, int(segment_symbols))), 65536))
    per = -(-len(flat) // segs)
    streams = [rans.encode(flat[s * per:(s + 1) * per], idx[s * per:(s + 1) * per], cdf, R.SIZES, R.OFFSETS) for s in range(segs)]
    body = struct.pack(f"<I{segs}I", segs, *[len(s) // 4 for s in streams]) + b"".join(streams)
    out = bytearray(HEADER.pack(MAGIC, n, depth, C, 1 if colour else 0, qp, chroma_qp_offset, BLOCK_LOG2, SEARCH, len(blocks)))
    for c in range(C):
        out += R._zigzag(root[c])
    out += bytes(side.tolist()) + np.packbits(mode, bitorder="little").tobytes() + struct.pack("<I", len(body)) + body
    if report is not None:
        recon = _finish(R.inverse(kids, dcp + root * st, hp_rows + sym * st[None, :]), colour)
        intra = np.concatenate([R.quantise(H[l], st[None, None, :])[E[l]] for l in range(depth)])
        report.update(n=n, depth=depth, blocks=len(blocks), first=first, modes=mode, mode1_blocks=int(mode.sum()), matched=int((m >= 0).sum()),
                      unmatched_in_mode1=int(((m < 0) & mode[brow]).sum()), has_match=has_match, side=side, hist=hist, sym=sym,
                      intra_sym=intra, grp=grp, recon=recon, root=root, symbols=len(flat), streams=segs,
                      escapes=int((np.abs(flat) > 63).sum()), model_bits256=int((hist * R.tables()[1][side]).sum()), prediction=P)
    return bytes(out)


def encode(points, attrs, qp, ref_points=None, ref_attrs=None, mode="auto", chroma_qp_offset=-2, colour=True,
           segment_symbols=SEGMENT_SYMBOLS, report=None):
    """mode "intra" or no reference: today's 0xB3 stream; "inter": the 0xB4 stream; "auto": the shorter, intra on a tie."""
    assert mode in ("auto", "inter", "intra")
    if mode == "intra" or ref_points is None:
        return R.encode(points, attrs, qp, chroma_qp_offset, colour, segment_symbols)
    inter = encode_inter(points, attrs, qp, ref_points, ref_attrs, chroma_qp_offset, colour, segment_symbols, report)
    if mode == "inter":
        assert inter is not None, "no inter stream beyond depth 14"
        return inter
    intra = R.encode(points, attrs, qp, chroma_qp_offset, colour, segment_symbols)
    return inter if inter is not None and len(inter) < len(intra) else intra


def decode(data, points, ref_points=None, ref_attrs=None):
    """bytes + the geometry (any row order) + the reference -> uint8 [n, C] in canonical order.  ValueError where the decoder
    clamps."""
    if data[0] == R.MAGIC:
        return R.decode(data, points)
    magic, n, depth, C, flags, qp, off, block_log2, search, nblocks = HEADER.unpack_from(data, 0)
    assert magic == MAGIC and ref_points is not None and (block_log2, search) == (BLOCK_LOG2, SEARCH) and not flags & ~1
    colour = bool(flags & 1)
    cells = np.unique(np.floor(np.asarray(points)[:, :3]).astype(np.int64), axis=0)
    _, d2, bl, blocks, brow = LI.block_plan(cells)
    assert n == len(cells) and n >= 2 and depth == d2 and nblocks == len(blocks)
    first = depth - bl
    st = np.array(R.steps_for(qp, off, C), dtype=np.int64)
    at = HEADER.size
    root = []
    for c in range(C):
        q, at = R._unzigzag(data, at)
        root.append(q)
    groups = (depth + 1) * 6
    side = np.frombuffer(data, np.uint8, groups, at).astype(np.int64)
    at += groups
    mbytes = -(-nblocks // 8)
    bits = np.unpackbits(np.frombuffer(data, np.uint8, mbytes, at), bitorder="little")
    assert not bits[nblocks:].any()
    mode = bits[:nblocks].astype(bool)
    at += mbytes
    ref_cells, ref_lv = LI.reference_rows(ref_points, ref_attrs, C)
    P, _, _, _ = prediction(cells, ref_cells, ref_lv, colour)          # zero in a block without a match, whatever its mode bit
    _, kids = R.level_plan(cells)
    w = R._weights(kids, n)
    Hp, E, Vp = forward_levels(kids, w, P * mode[brow][:, None])
    nblk = node_blocks(cells, depth, first, blocks)
    idx = side[_layout(E, nblk, mode, depth, first, C)]
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
    coef = np.concatenate([Hp[l][E[l]] for l in range(depth)]) + sym * st[None, :]
    dc = Vp[0][0] + np.array(root, dtype=np.int64) * st
    if np.abs(sym * st[None, :]).max(initial=0) > LIMIT or np.abs(coef).max(initial=0) > LIMIT or np.abs(dc).max() > LIMIT:
        raise ValueError("a coefficient left the +-2^30 range")
    return _finish(R.inverse(kids, dc, coef), colour)


# ---- the cases: those of the lossless inter coder, at three quantisers -----------------------------------------------------
def cases():
    return LI.cases()


@functools.lru_cache(maxsize=None)
def coded(name, qp, mode="inter"):
    """(bytes, report) of the reference's encoder on a case."""
    c = cases()[name]
    rep = {}
    return encode(*c["cur"], qp, *c["ref"], mode=mode, colour=c["colour"], segment_symbols=c["segment_symbols"], report=rep), rep


@functools.lru_cache(maxsize=None)
def intra_coded(name, qp):
    c = cases()[name]
    return R.encode(*c["cur"], qp, colour=c["colour"], segment_symbols=c["segment_symbols"])


@functools.lru_cache(maxsize=None)
def moved_surface(bits=7, qp=28, other_seed=None):
    """(current points, levels, reference points, reference levels as decoded at qp): `surface_cloud(0, bits)` moved by one voxel
    with its colours carried, against the unmoved cloud's own intra decode; other_seed: against that surface's decode instead."""
    from unified_point_cloud_compression_amd import synth
    pc = synth.surface_cloud(0, bits)
    pts, lv = np.floor(pc[:, :3]).astype(np.float32), R.levels_of(pc[:, 3:])
    rp, rl = pts, lv
    if other_seed is not None:
        o = synth.surface_cloud(other_seed, bits)
        rp, rl = np.floor(o[:, :3]).astype(np.float32), R.levels_of(o[:, 3:])
    ref_cells, _ = R.canonical(rp, rl)
    ref_dec = R.decode(R.encode(rp, rl, qp), rp)
    return pts + np.float32([1, 0, 0]), lv, ref_cells.astype(np.float32), ref_dec


# ---- rate ------------------------------------------------------------------------------------------------------------------
def rate_row(cur, ref, qp):
    rep = {}
    inter = encode(*cur, qp, *ref, mode="inter", report=rep)
    intra = R.encode(*cur, qp)
    truth = R.canonical(*cur)[1]
    dec_inter, dec_intra = decode(inter, cur[0], *ref), R.decode(intra, cur[0])
    assert np.array_equal(dec_inter, rep["recon"])
    return {"points": rep["n"], "blocks": rep["blocks"], "intra_bytes": len(intra), "inter_bytes": len(inter),
            "ratio_inter_over_intra": round(len(inter) / len(intra), 4), "intra_y_psnr_db": round(R.y_psnr(truth, dec_intra), 3),
            "inter_y_psnr_db": round(R.y_psnr(truth, dec_inter), 3), "inter_member_cost_bytes": round(rep["model_bits256"] / 2048, 1),
            "mode1_block_share": round(rep["mode1_blocks"] / rep["blocks"], 4), "matched_voxel_share": round(rep["matched"] / rep["n"], 4)}


def rate_report(qps=(22, 28, 34, 40), bits=(6, 7)):
    out = {}
    for b in bits:
        for qp in qps:
            for name, seed in (("moved", None), ("unrelated_reference", 1)):
                p, l, rp, rl = moved_surface(b, qp, seed)
                out[f"surface{b}_{name}_qp{qp}"] = rate_row((p, l), (rp, rl), qp)
    return out


if __name__ == "__main__":
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = {"what": "inter-frame RAHT colour stream 0xB4 (DESIGN.md 7f), numpy reference coder, chroma_qp_offset -2, colour transform on: "
                   "surface_cloud(0, b) moved by one voxel with its colours carried, coded against the unmoved cloud as decoded at the same "
                   "qp (moved), and against another surface (seed 1) as decoded at that qp (unrelated_reference); intra is the 0xB3 stream "
                   "of the same cloud; stream bytes include header, side bytes, mode bytes and framing; every inter stream was decoded "
                   "and gave the reconstruction the encoder predicted; nothing is gated on these figures",
           "clouds": rate_report()}
    with open(os.path.join(root, "profiles", "attribute_inter_lossy_rate.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["clouds"], indent=1))
