"""numpy restatement of the inter-frame lossless geometry stream, format 0xA8 -- test infrastructure,
no GPU.

Block motion search against a reference cloud, the predicted set, the two symbol populations (nodes absent from / present in
the prediction), the integer rule of the 128-row table family written out again in Python integers, the vector list and
`oracle.rans` for every payload.  `encode` must give the bytes `geometry.encode_geometry(x, reference=r)` gives; `decode`
reads them back.  The intra parts (levels above the blocks, contexts, occupancy bytes) come from `tests/geom_ref.py`."""
import struct

import numpy as np

from oracle import rans
from tests import geom_ref as G

MAGIC_INTER, BLOCK_LOG2, SEARCH = 0xA8, 4, 2
RAW_NODES, SEGMENT_NODES, PRIOR_WEIGHT = G.RAW_NODES, G.SEGMENT_NODES, G.PRIOR_WEIGHT
POP = G.POP
RHO = np.array(sorted(range(256), key=lambda t: (int(POP[t]), t)), dtype=np.int64)      # symbol -> t = s XOR r
RHO_INV = np.argsort(RHO)                                                               # t -> symbol; RHO_INV[0] = 0
SIZES = np.array([257] * 64 + [258] * 64, dtype=np.int32)
OFFSETS = np.array([1] * 64 + [0] * 64, dtype=np.int32)
SIDE = struct.Struct("<8I9III")
_B = 1 << 17


def _lin(c):
    """Linear key of signed cells (|c| < 2^17)."""
    c = np.asarray(c, dtype=np.int64)
    return ((c[:, 0] + _B) << 42) | ((c[:, 1] + _B) << 21) | (c[:, 2] + _B)


def candidates(search):
    """The (2R+1)^3 vectors by |v|^2, then lexicographically: index 0 is the zero vector."""
    r = range(-search, search + 1)
    return sorted(((dx, dy, dz) for dx in r for dy in r for dz in r), key=lambda v: (v[0] ** 2 + v[1] ** 2 + v[2] ** 2, v))


def motion_search(rel, blocks, bl, ref_rel, search):
    """(vector index per block, match counts [blocks, candidates]).  A match: a voxel p of the block with p - v in the
    reference.  Most matches win, ties go to the lowest index."""
    cand = candidates(search)
    have = np.unique(_lin(ref_rel)) if len(ref_rel) else np.zeros(0, dtype=np.int64)
    row = np.searchsorted(_lin(blocks), _lin(rel >> bl))
    score = np.zeros((len(blocks), len(cand)), dtype=np.int64)
    for j, v in enumerate(cand):
        hit = np.isin(_lin(rel - np.array(v)), have)
        score[:, j] = np.bincount(row, weights=hit, minlength=len(blocks)).astype(np.int64)
    return np.argmax(score, axis=1), score


def predicted(blocks, bl, vec, ref_rel, depth, search):
    """pred = { p : p in an occupied block b, reference(p - v_b) occupied }, canonical."""
    cand = candidates(search)
    blin = _lin(blocks)
    out = [np.zeros((0, 3), dtype=np.int64)]
    for j in np.unique(vec):
        p = ref_rel + np.array(cand[int(j)])
        p = p[np.all((p >= 0) & (p < (1 << depth)), axis=1)]
        if not len(p):
            continue
        k = _lin(p >> bl)
        pos = np.minimum(np.searchsorted(blin, k), len(blin) - 1)
        out.append(p[(blin[pos] == k) & (vec[pos] == j)])
    return np.unique(np.concatenate(out), axis=0)


def prediction_bytes(nodes, pnodes, pchildren):
    """(present, r): whether each node is in the predicted level, and the predicted node's child-occupancy byte (0: absent)."""
    if not len(pnodes):
        return np.zeros(len(nodes), dtype=bool), np.zeros(len(nodes), dtype=np.int64)
    rb = G.occupancy(pnodes, pchildren)
    k = _lin(pnodes)
    pos = np.minimum(np.searchsorted(k, _lin(nodes)), len(k) - 1)
    present = k[pos] == _lin(nodes)
    return present, np.where(present, rb[pos], 0)


def histogram(idx, sym):
    h = np.zeros((128, 256), dtype=np.int64)
    np.add.at(h, (idx, sym), 1)
    return h


def _family(counts, first, nsym, cls, classes, hist):
    """64 rows of one population: counts [64, 256] (symbols first .. first + nsym - 1 live), cls[s] the class of live symbol s,
    hist the level's class histogram.  The rule of `geometry.derive_tables`; an empty population (sum(hist) == 0) takes r = 1."""
    n = [[int(v) for v in row[first:first + nsym]] for row in counts]
    total = sum(sum(row) for row in n)
    shift = max(0, total.bit_length() - 20)
    n = [[v >> shift for v in row] for row in n]
    g = [sum(n[c][s] for c in range(64)) for s in range(nsym)]
    gt = sum(g) + nsym
    hist = [int(v) for v in hist]
    ht = sum(hist)
    r = [1 if ht == 0 else 0] * classes
    for k in range(classes):
        if hist[k]:
            e = sum(g[s] + 1 for s in range(nsym) if cls[s] == k)
            r[k] = min(max(((hist[k] * gt) << 12) // (ht * e), 1), 1 << 20)
    rows = []
    for c in range(64):
        w = [n[c][s] * gt + PRIOR_WEIGHT * (g[s] + 1) for s in range(nsym)]
        wt = sum(w)
        v = [(1 + (w[s] << 20) // wt) * r[cls[s]] for s in range(nsym)]
        vt = sum(v)
        f = [1 + v[s] * (65535 - nsym) // vt for s in range(nsym)]
        f[f.index(max(f))] += 65535 - sum(f)
        rows.append(f)
    return rows


def tables(counts, pop, dist):
    """cdf int32 [128, 258]: rows 0..63 the absent nodes (255 bytes + escape, 257 entries), rows 64..127 the present nodes
    (256 symbols + escape, 258 entries)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(128, 256)
    cdf = np.zeros((128, 258), dtype=np.int32)
    for c, f in enumerate(_family(counts[:64], 1, 255, [int(POP[s + 1]) - 1 for s in range(255)], 8, pop)):
        cdf[c, 1:256] = np.cumsum(f)
        cdf[c, 256] = 65536
    for c, f in enumerate(_family(counts[64:], 0, 256, [int(POP[RHO[s]]) for s in range(256)], 9, dist)):
        cdf[64 + c, 1:257] = np.cumsum(f)
        cdf[64 + c, 257] = 65536
    return cdf


def vector_table(hist, k):
    """cdf int32 [1, k + 2] of the vector indices from their histogram hist[k]: f = 1 + hist * (65535 - k) // total, what is left
    of 65535 to the first largest, the escape slot 1."""
    hist = [int(v) for v in hist]
    total = sum(hist)
    f = [1 + hist[i] * (65535 - k) // total for i in range(k)]
    f[f.index(max(f))] += 65535 - sum(f)
    cdf = np.zeros((1, k + 2), dtype=np.int32)
    cdf[0, 1:k + 1] = np.cumsum(f)
    cdf[0, k + 1] = 65536
    return cdf


def _container(sym, idx, cdf, sizes, offsets, segment_nodes):
    n = len(sym)
    segs = max(1, min(-(-n // segment_nodes), 65536))
    rows = -(-n // segs)
    streams = [rans.encode(sym[s * rows:(s + 1) * rows], idx[s * rows:(s + 1) * rows], cdf, sizes, offsets) for s in range(segs)]
    return struct.pack(f"<I{segs}I", segs, *[len(s) // 4 for s in streams]) + b"".join(streams)


def _uncontainer(body, idx, cdf, sizes, offsets):
    m = len(idx)
    segs = struct.unpack_from("<I", body, 0)[0]
    words = struct.unpack_from(f"<{segs}I", body, 4)
    rows, p, parts = -(-m // segs), 4 * (1 + segs), []
    for s in range(segs):
        parts.append(rans.decode(body[p:p + 4 * words[s]], idx[s * rows:(s + 1) * rows], cdf, sizes, offsets))
        p += 4 * words[s]
    return np.concatenate(parts).astype(np.int64)


def encode_vectors(vec, k, segment_nodes):
    if k == 1:
        return b""
    if len(vec) < RAW_NODES:
        return bytes(int(v) for v in vec)
    hist = np.bincount(vec, minlength=k)
    occ = np.flatnonzero(hist)
    body = _container(vec, np.zeros(len(vec), dtype=np.int64), vector_table(hist, k), np.array([k + 2], np.int32), np.zeros(1, np.int32),
                      segment_nodes)
    return struct.pack("<B", len(occ)) + b"".join(struct.pack("<BI", int(i), int(hist[i])) for i in occ) + struct.pack("<I", len(body)) + body


def _reference_cells(reference):
    if reference is None or len(reference) == 0:
        return np.zeros((0, 3), dtype=np.int64)
    return G.unique_cells(reference)


def encode_inter(points, reference, segment_nodes=SEGMENT_NODES, report=None, block_log2=BLOCK_LOG2, search=SEARCH):
    cells = G.unique_cells(points)
    n = len(cells)
    if n == 0:
        return G.encode(points)
    origin = cells.min(axis=0)
    rel = cells - origin
    depth = max(1, int(rel.max()).bit_length())
    first = max(0, depth - block_log2)
    bl = depth - first
    levels = G.level_cells(rel, depth)
    ref_rel = _reference_cells(reference) - origin
    out = bytearray(struct.pack("<BIB3iBB", MAGIC_INTER, n, depth, *[int(v) for v in origin], block_log2, search))
    counts = np.zeros((128, 256), dtype=np.int64)
    rep = {"n": n, "depth": depth, "first": first, "nodes": [len(v) for v in levels[:depth]], "present": [], "absent": []}
    for l in range(first):
        nodes = levels[l]
        byte, ctx = G.occupancy(nodes, levels[l + 1]), G.contexts(nodes)
        if len(nodes) < RAW_NODES:
            out += bytes(byte.tolist())
        else:
            pop = [int((POP[byte] == k + 1).sum()) for k in range(8)]
            body = G._container(byte, ctx, G.tables(counts[:64], pop), segment_nodes)
            out += struct.pack("<8II", *pop, len(body)) + body
        counts = (counts >> 1) + histogram(ctx, byte)
    blocks = levels[first]
    vec, score = motion_search(rel, blocks, bl, ref_rel, search)
    vbytes = encode_vectors(vec, (2 * search + 1) ** 3, segment_nodes)
    out += vbytes
    pred = predicted(blocks, bl, vec, ref_rel, depth, search)
    plv = [np.unique(pred >> (depth - l), axis=0) for l in range(depth + 1)]
    for l in range(first, depth):
        nodes = levels[l]
        byte, ctx = G.occupancy(nodes, levels[l + 1]), G.contexts(nodes)
        present, r = prediction_bytes(nodes, plv[l], plv[l + 1])
        sym = np.where(present, RHO_INV[byte ^ r], byte)
        idx = ctx + 64 * present
        rep["present"].append(int(present.sum()))
        rep["absent"].append(int((~present).sum()))
        if len(nodes) < RAW_NODES:
            out += bytes(byte.tolist())
        else:
            pop = [int(((POP[byte] == k + 1) & ~present).sum()) for k in range(8)]
            dist = [int(((POP[byte ^ r] == d) & present).sum()) for d in range(9)]
            body = _container(sym, idx, tables(counts, pop, dist), SIZES, OFFSETS, segment_nodes)
            out += SIDE.pack(*pop, *dist, int(POP[byte].sum()), len(body)) + body
        counts = (counts >> 1) + histogram(idx, sym)
    rep.update(vectors=vec, scores=score, vector_bytes=len(vbytes), blocks=len(blocks), predicted=len(pred),
               vectors_coded=len(blocks) >= RAW_NODES and search > 0)
    if report is not None:
        report.update(rep)
    return bytes(out)


def encode(points, reference=None, mode="auto", segment_nodes=SEGMENT_NODES, report=None):
    """mode "intra": today's stream; "inter": the 0xA8 stream; "auto": the shorter of the two, intra on a tie or without a
    reference."""
    assert mode in ("auto", "inter", "intra")
    if mode == "intra" or reference is None or len(G.unique_cells(points)) == 0:
        return G.encode(points, segment_nodes=segment_nodes)
    inter = encode_inter(points, reference, segment_nodes, report)
    if mode == "inter":
        return inter
    intra = G.encode(points, segment_nodes=segment_nodes)
    return inter if len(inter) < len(intra) else intra


def decode(data, reference=None):
    """bytes -> int64 [n, 3] voxels in canonical order."""
    if data[0] == G.MAGIC:
        return G.decode(data)
    magic, n, depth, ox, oy, oz, block_log2, search = struct.unpack_from("<BIB3iBB", data, 0)
    assert magic == MAGIC_INTER and reference is not None
    origin = np.array([ox, oy, oz])
    ref_rel = _reference_cells(reference) - origin
    first = max(0, depth - block_log2)
    bl = depth - first
    k = (2 * search + 1) ** 3
    at = 20
    nodes = np.zeros((1, 3), dtype=np.int64)
    counts = np.zeros((128, 256), dtype=np.int64)
    plv = None
    for l in range(depth):
        m = len(nodes)
        if l == first:
            if k == 1:
                vec = np.zeros(m, dtype=np.int64)
            elif m < RAW_NODES:
                vec = np.frombuffer(data, np.uint8, m, at).astype(np.int64)
                at += m
            else:
                occ = data[at]
                hist = np.zeros(k, dtype=np.int64)
                for j in range(occ):
                    i, c = struct.unpack_from("<BI", data, at + 1 + 5 * j)
                    hist[i] = c
                at += 1 + 5 * occ
                nbytes = struct.unpack_from("<I", data, at)[0]
                at += 4
                vec = _uncontainer(data[at:at + nbytes], np.zeros(m, dtype=np.int64), vector_table(hist, k), np.array([k + 2], np.int32),
                                   np.zeros(1, np.int32))
                at += nbytes
            assert vec.max() < k
            pred = predicted(nodes, bl, vec, ref_rel, depth, search)
            plv = [np.unique(pred >> (depth - j), axis=0) for j in range(depth + 1)]
        ctx = G.contexts(nodes)
        if l < first:
            present, r = np.zeros(m, dtype=bool), np.zeros(m, dtype=np.int64)
        else:
            present, r = prediction_bytes(nodes, plv[l], plv[l + 1])
        idx = ctx + 64 * present
        if m < RAW_NODES:
            byte = np.frombuffer(data, np.uint8, m, at).astype(np.int64)
            at += m
            sym = np.where(present, RHO_INV[byte ^ r], byte)
        elif l < first:
            *pop, nbytes = struct.unpack_from("<8II", data, at)
            at += 36
            sym = byte = _uncontainer(data[at:at + nbytes], ctx, G.tables(counts[:64], pop), G.SIZES, G.OFFSETS)
            at += nbytes
        else:
            side = SIDE.unpack_from(data, at)
            at += SIDE.size
            sym = _uncontainer(data[at:at + side[18]], idx, tables(counts, side[:8], side[8:17]), SIZES, OFFSETS)
            at += side[18]
            byte = np.where(present, RHO[np.clip(sym, 0, 255)] ^ r, sym)
            assert int(POP[byte].sum()) == side[17]
        assert byte.min() >= 1 and byte.max() <= 255
        counts = (counts >> 1) + histogram(idx, sym)
        kids = []
        for j in range(8):
            sel = nodes[(byte >> j) & 1 == 1]
            kids.append(sel * 2 + np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1]))
        nodes = np.unique(np.concatenate(kids), axis=0)
    assert at == len(data) and len(nodes) == n
    return nodes + origin


# ---- the clouds of the inter tests: the smallest shapes at which each mechanism can still go wrong -------------------------
def cases():
    """name -> (current frame, reference), float32 [N, 3] rows, (a)..(h) of the tests."""
    from unified_point_cloud_compression_amd import synth
    a = np.floor(synth.surface_cloud(0, 7)[:, :3]).astype(np.float32)
    a8 = np.floor(synth.surface_cloud(0, 8)[:, :3]).astype(np.float32)
    half = a.copy()
    half[a[:, 0] >= 64] += np.array([1, 1, 0], dtype=np.float32)
    wave = a.copy()
    wave[:, 2] += np.floor(1.5 * np.sin(2 * np.pi * a[:, 0] / 128) + 0.5).astype(np.float32)
    small = G.clouds()
    blk = synth.random_block(0, 64, 0.05)[:, :3]
    return {
        "a_identical": (a, a),
        "b_shift_100": (a + np.array([1, 0, 0], dtype=np.float32), a),
        "b_shift_2m12": (a + np.array([2, -1, 2], dtype=np.float32), a),
        "c_half_moved": (half, a),
        "d_wave": (wave, a),
        "e_other_surface": (np.floor(synth.surface_cloud(1, 7)[:, :3]).astype(np.float32), a),
        "f_unrelated": (synth.random_block(1, 64, 0.05)[:, :3], blk),
        "g_one_point": (small["one_point"], small["one_point"]),
        "g_full_cube8": (small["full_cube8"], small["full_cube8"]),
        "g_reference_outside": (blk, blk + np.array([200, 0, 0], dtype=np.float32)),
        "g_reference_empty": (blk, np.zeros((0, 3), dtype=np.float32)),
        "g_reference_shifted": (blk, blk + np.array([-100, -7, 33], dtype=np.float32)),
        # negative coordinates and another origin with matches left: both clouds at (-100, -7, 33), the reference one step further
        "g_negative_origin": (blk + np.array([-100, -7, 33], dtype=np.float32), blk + np.array([-101, -7, 35], dtype=np.float32)),
        "h_surface8_shift": (a8 + np.array([1, 0, 0], dtype=np.float32), a8),
    }


SEGMENTED = ("b_shift_100", "b_shift_2m12")        # (i): coded again with SEGMENTED_NODES so that the last level spans three streams
SEGMENTED_NODES = 1300


def rate_report(names=None):
    """Per case: points, intra / inter / auto stream bytes of the reference coder, the vector bytes and the share of zero
    vectors."""
    out = {}
    for name, (cur, ref) in cases().items():
        if names is not None and name not in names:
            continue
        rep = {}
        inter = encode(cur, ref, "inter", report=rep)
        intra = G.encode(cur)
        out[name] = {"points": rep["n"], "depth": rep["depth"], "blocks": rep["blocks"], "intra_bytes": len(intra), "inter_bytes": len(inter),
                     "auto_bytes": len(encode(cur, ref, "auto")), "ratio_inter_over_intra": round(len(inter) / len(intra), 4),
                     "vector_bytes": rep["vector_bytes"], "zero_vector_share": round(float((rep["vectors"] == 0).mean()), 4),
                     "present_nodes_per_inter_level": rep["present"], "absent_nodes_per_inter_level": rep["absent"]}
    return out
