"""numpy restatement of the wide-search inter streams: geometry 0xAA, lossless colour 0xB7, RAHT colour 0xB8 (DESIGN.md sections
7e "Wide search", 7f, 7i) -- test infrastructure, no GPU.

The block motion search over [-search, search]^3 for search up to 7 (exhaustive; most matches, then the shorter vector, then the
lexicographically smaller one: the "lowest index of candidates(search)" of `tests/geom_inter_ref.py`), the vector list coded per
component, and `encode_inter` / `decode` of 0xAA.  The levels are coded by `geom_inter_ref.encode_inter` itself, run with the wide
search and the component vector list in place of its own; the colour streams are `raht_lossless_inter_ref` / `raht_inter_ref`
run with another range and magic byte (no vector travels in them)."""
import contextlib
import functools
import struct

import numpy as np

from tests import geom_inter_ref as GI
from tests import geom_ref as G

MAGIC_WIDE, MAGIC_LOSSLESS_WIDE, MAGIC_RAHT_WIDE = 0xAA, 0xB7, 0xB8
MIN_SEARCH, MAX_SEARCH = 3, 7
RAW_NODES, SEGMENT_NODES, BLOCK_LOG2 = GI.RAW_NODES, GI.SEGMENT_NODES, GI.BLOCK_LOG2


@functools.lru_cache(maxsize=None)
def _orders(search):
    """(vectors in lexicographic order [K^3, 3], candidate index -> lexicographic rank, lexicographic rank -> candidate index)."""
    r = range(-search, search + 1)
    lex = [(dx, dy, dz) for dx in r for dy in r for dz in r]
    rank = {v: i for i, v in enumerate(lex)}
    to_lex = np.array([rank[v] for v in GI.candidates(search)], dtype=np.int64)
    return np.array(lex, dtype=np.int64), to_lex, np.argsort(to_lex)


def match_counts(rel, blocks, bl, ref_rel, search):
    """int64 [blocks, (2 search + 1)^3], lexicographic (dx, dy, dz): the voxels p of each block with p - v in the reference."""
    lex, _, _ = _orders(search)
    rel = np.asarray(rel, dtype=np.int64)
    lo, hi = rel.min(axis=0) - search, rel.max(axis=0) + search
    occ = np.zeros(tuple(hi - lo + 1), dtype=bool)
    if len(ref_rel):
        inside = ref_rel[np.all((ref_rel >= lo) & (ref_rel <= hi), axis=1)] - lo
        occ[inside[:, 0], inside[:, 1], inside[:, 2]] = True
    row = np.searchsorted(GI._lin(blocks), GI._lin(rel >> bl))
    counts = np.zeros((len(blocks), len(lex)), dtype=np.int64)
    for j, v in enumerate(lex):
        q = rel - v - lo
        counts[:, j] = np.bincount(row, weights=occ[q[:, 0], q[:, 1], q[:, 2]], minlength=len(blocks)).astype(np.int64)
    return counts


def _index_search(rel, blocks, bl, ref_rel, search):
    """`geom_inter_ref.motion_search` for any range, by way of an occupancy array: (index into candidates(search), counts in
    candidate order)."""
    _, to_lex, _ = _orders(search)
    score = match_counts(rel, blocks, bl, ref_rel, search)[:, to_lex]
    return np.argmax(score, axis=1), score


def motion_search(rel, blocks, bl, ref_rel, search):
    """(displacement per block int64 [blocks, 3], match counts [blocks, K^3] in lexicographic order)."""
    idx, score = _index_search(rel, blocks, bl, ref_rel, search)
    lex, to_lex, to_cand = _orders(search)
    return lex[to_lex[idx]], score[:, to_cand]


def components(idx, search):
    """[blocks, 3] (dx + search, dy + search, dz + search) of indices into candidates(search)."""
    lex, to_lex, _ = _orders(search)
    return lex[to_lex[np.asarray(idx, dtype=np.int64)]] + search


def indices(comp, search):
    _, _, to_cand = _orders(search)
    k = 2 * search + 1
    comp = np.asarray(comp, dtype=np.int64)
    return to_cand[(comp[:, 0] * k + comp[:, 1]) * k + comp[:, 2]]


def _vector_tables(hists, k):
    return np.concatenate([GI.vector_table(h, k) for h in hists]), np.full(3, k + 2, np.int32), np.zeros(3, np.int32)


def encode_vectors(comp, search, segment_nodes=SEGMENT_NODES, hists=None):
    """The vector list of an 0xAA stream from the components [blocks, 3].  `hists` overrides the transmitted histograms (the damage
    tests code a component the histograms do not announce)."""
    comp = np.asarray(comp, dtype=np.int64)
    k = 2 * search + 1
    if len(comp) < RAW_NODES:
        return bytes(comp.reshape(-1).tolist())
    hists = [np.bincount(comp[:, c], minlength=k)[:k] for c in range(3)] if hists is None else hists
    out = bytearray()
    for h in hists:
        occ = np.flatnonzero(h)
        out += struct.pack("<B", len(occ)) + b"".join(struct.pack("<BI", int(i), int(h[i])) for i in occ)
    body = GI._container(comp.reshape(-1), np.tile(np.arange(3), len(comp)), *_vector_tables(hists, k), segment_nodes)
    return bytes(out) + struct.pack("<I", len(body)) + body


def decode_vectors(data, at, blocks, search):
    """(components [blocks, 3], end)."""
    k = 2 * search + 1
    if blocks < RAW_NODES:
        comp = np.frombuffer(data, np.uint8, 3 * blocks, at).astype(np.int64).reshape(blocks, 3)
        return comp, at + 3 * blocks
    hists = []
    for _ in range(3):
        h = np.zeros(k, dtype=np.int64)
        for j in range(data[at]):
            i, c = struct.unpack_from("<BI", data, at + 1 + 5 * j)
            h[i] = c
        at += 1 + 5 * data[at]
        hists.append(h)
    nbytes = struct.unpack_from("<I", data, at)[0]
    at += 4
    comp = GI._uncontainer(data[at:at + nbytes], np.tile(np.arange(3), blocks), *_vector_tables(hists, k))
    return comp.reshape(blocks, 3), at + nbytes


@contextlib.contextmanager
def _wide(search, segment_nodes=SEGMENT_NODES, modules=()):
    """Run the narrow reference coders with the wide search: `geom_inter_ref` searches by `_index_search` and writes the component
    vector list, and each of `modules` = (module, magic) takes `search` and the magic byte for its constants."""
    saved = (GI.motion_search, GI.encode_vectors, [(m, m.SEARCH, m.MAGIC) for m, _ in modules])
    GI.motion_search = _index_search
    GI.encode_vectors = lambda vec, k, seg: encode_vectors(components(vec, search), search, seg)
    for m, magic in modules:
        m.SEARCH, m.MAGIC = search, magic
    try:
        yield
    finally:
        GI.motion_search, GI.encode_vectors = saved[:2]
        for m, s, magic in saved[2]:
            m.SEARCH, m.MAGIC = s, magic


def encode_inter(points, reference, search=MAX_SEARCH, segment_nodes=SEGMENT_NODES, report=None):
    """The 0xAA stream (an empty cloud still travels as intra).  report["vectors"] are indices into candidates(search),
    report["displacements"] the vectors themselves, report["scores"] the match counts in candidate order."""
    assert MIN_SEARCH <= search <= MAX_SEARCH
    rep = {}
    with _wide(search, segment_nodes):
        data = GI.encode_inter(points, reference, segment_nodes, rep, search=search)
    if rep:
        rep["displacements"] = components(rep["vectors"], search) - search
        data = bytes([MAGIC_WIDE]) + data[1:]
    if report is not None:
        report.update(rep)
    return data


def encode(points, reference=None, mode="auto", search=MAX_SEARCH, segment_nodes=SEGMENT_NODES, report=None):
    """search 2: `geom_inter_ref.encode`; 3..7: 0xAA; "auto": the shorter of 2 and 7, 2 on a tie.  mode as in `geom_inter_ref`."""
    if mode == "intra" or reference is None or len(G.unique_cells(points)) == 0:
        return G.encode(points, segment_nodes=segment_nodes)
    if search == "auto":
        a, b = GI.encode_inter(points, reference, segment_nodes), encode_inter(points, reference, MAX_SEARCH, segment_nodes)
        inter = b if len(b) < len(a) else a
    elif search == 2:
        inter = GI.encode_inter(points, reference, segment_nodes, report)
    else:
        inter = encode_inter(points, reference, search, segment_nodes, report)
    if mode == "inter":
        return inter
    intra = G.encode(points, segment_nodes=segment_nodes)
    return inter if len(inter) < len(intra) else intra


def decode(data, reference=None):
    """bytes -> int64 [n, 3] voxels in canonical order (0xA7 and 0xA8 through the narrow references)."""
    if data[0] != MAGIC_WIDE:
        return GI.decode(data, reference)
    _, n, depth, ox, oy, oz, block_log2, search = struct.unpack_from("<BIB3iBB", data, 0)
    assert reference is not None and MIN_SEARCH <= search <= MAX_SEARCH
    origin = np.array([ox, oy, oz])
    ref_rel = GI._reference_cells(reference) - origin
    first = max(0, depth - block_log2)
    bl = depth - first
    at = 20
    nodes = np.zeros((1, 3), dtype=np.int64)
    counts = np.zeros((128, 256), dtype=np.int64)
    plv = None
    for l in range(depth):
        m = len(nodes)
        if l == first:
            comp, at = decode_vectors(data, at, m, search)
            assert comp.min() >= 0 and comp.max() <= 2 * search
            pred = GI.predicted(nodes, bl, indices(comp, search), ref_rel, depth, search)
            plv = [np.unique(pred >> (depth - j), axis=0) for j in range(depth + 1)]
        ctx = G.contexts(nodes)
        if l < first:
            present, r = np.zeros(m, dtype=bool), np.zeros(m, dtype=np.int64)
        else:
            present, r = GI.prediction_bytes(nodes, plv[l], plv[l + 1])
        idx = ctx + 64 * present
        if m < RAW_NODES:
            byte = np.frombuffer(data, np.uint8, m, at).astype(np.int64)
            at += m
            sym = np.where(present, GI.RHO_INV[byte ^ r], byte)
        elif l < first:
            *pop, nbytes = struct.unpack_from("<8II", data, at)
            at += 36
            sym = byte = GI._uncontainer(data[at:at + nbytes], ctx, G.tables(counts[:64], pop), G.SIZES, G.OFFSETS)
            at += nbytes
        else:
            side = GI.SIDE.unpack_from(data, at)
            at += GI.SIDE.size
            sym = GI._uncontainer(data[at:at + side[18]], idx, GI.tables(counts, side[:8], side[8:17]), GI.SIZES, GI.OFFSETS)
            at += side[18]
            byte = np.where(present, GI.RHO[np.clip(sym, 0, 255)] ^ r, sym)
            assert int(GI.POP[byte].sum()) == side[17]
        assert byte.min() >= 1 and byte.max() <= 255
        counts = (counts >> 1) + GI.histogram(idx, sym)
        kids = []
        for j in range(8):
            sel = nodes[(byte >> j) & 1 == 1]
            kids.append(sel * 2 + np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1]))
        nodes = np.unique(np.concatenate(kids), axis=0)
    assert at == len(data) and len(nodes) == n
    return nodes + origin


# ---- the colour streams: the narrow references with another range and magic byte -------------------------------------------
def lossless_colour_encode(points, attrs, ref_points, ref_attrs, search=MAX_SEARCH, **kw):
    """0xB7: `raht_lossless_inter_ref.encode_inter` with the wide search."""
    from tests import raht_lossless_inter_ref as LI
    with _wide(search, modules=[(LI, MAGIC_LOSSLESS_WIDE)]):
        return LI.encode_inter(points, attrs, ref_points, ref_attrs, **kw)


def lossless_colour_decode(data, points, ref_points, ref_attrs):
    from tests import raht_lossless_inter_ref as LI
    assert data[0] == MAGIC_LOSSLESS_WIDE
    with _wide(data[LI.HEADER.size - 5], modules=[(LI, MAGIC_LOSSLESS_WIDE)]):
        return LI.decode(data, points, ref_points, ref_attrs)


def raht_colour_encode(points, attrs, qp, ref_points, ref_attrs, search=MAX_SEARCH, **kw):
    """0xB8: `raht_inter_ref.encode_inter` with the wide search."""
    from tests import raht_inter_ref as RI
    from tests import raht_lossless_inter_ref as LI
    with _wide(search, modules=[(RI, MAGIC_RAHT_WIDE), (LI, LI.MAGIC)]):          # (its matches come from LI.match_rows)
        return RI.encode_inter(points, attrs, qp, ref_points, ref_attrs, **kw)


def raht_colour_decode(data, points, ref_points, ref_attrs):
    from tests import raht_inter_ref as RI
    from tests import raht_lossless_inter_ref as LI
    assert data[0] == MAGIC_RAHT_WIDE
    with _wide(data[RI.HEADER.size - 5], modules=[(RI, MAGIC_RAHT_WIDE), (LI, LI.MAGIC)]):
        return RI.decode(data, points, ref_points, ref_attrs)


# ---- the clouds of the wide tests ------------------------------------------------------------------------------------------
MOVE_HIGH, MOVE_LOW = (5, -4, 3), (-6, 2, 0)


def articulated(bits, seed=0):
    """(current, reference, colour levels): the surface cloud with its x >= 2^(bits - 1) half moved by MOVE_HIGH and the other
    half by MOVE_LOW, colours carried; the reference is the unmoved cloud."""
    from unified_point_cloud_compression_amd import synth
    from tests import raht_ref as R
    pc = synth.surface_cloud(seed, bits)
    ref = np.floor(pc[:, :3]).astype(np.float32)
    cur = ref + np.where(ref[:, :1] >= (1 << (bits - 1)), np.float32(MOVE_HIGH), np.float32(MOVE_LOW))
    return cur.astype(np.float32), ref, R.levels_of(pc[:, 3:])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (current frame, reference), float32 [N, 3] rows."""
    from unified_point_cloud_compression_amd import synth
    a7, r7, _ = articulated(7)
    a8, r8, _ = articulated(8)
    blk = synth.random_block(0, 64, 0.05)[:, :3]
    far = np.array([-100, -7, 33], dtype=np.float32)
    cube = G.clouds()["full_cube8"]
    return {
        "articulated7": (a7, r7),                                    # 66 blocks: a raw vector list
        "articulated8": (a8, r8),                                    # 240 blocks: a coded one
        "identical8": (r8, r8),
        "shift_7m76": (r7 + np.array([7, -7, 6], dtype=np.float32), r7),      # the edge of the range
        "shift_800": (r7 + np.array([8, 0, 0], dtype=np.float32), r7),        # just outside it
        "reference_empty": (blk, np.zeros((0, 3), dtype=np.float32)),
        "reference_outside": (blk, blk + np.array([200, 0, 0], dtype=np.float32)),
        "negative_origin": (blk + far, blk + far + np.array([-5, 3, 6], dtype=np.float32)),
        "depth3": (cube, cube + np.array([3, 0, -2], dtype=np.float32)),      # block_log2 = 3
    }


SEGMENTED = ("articulated7", "shift_7m76")       # coded again with SEGMENTED_NODES: the last level spans three rANS streams
SEGMENTED_NODES = GI.SEGMENTED_NODES


def rate_report(bits=(7, 8)):
    """Per articulated cloud: stream bytes of the reference coders, intra / inter at +-2 / inter at +-7, geometry and lossless
    colour, and the cloud against itself."""
    from tests import raht_lossless_inter_ref as LI
    from tests import raht_lossless_ref as Q
    out = {}
    for b in bits:
        cur, ref, lv = articulated(b)
        rep = {}
        wide = encode_inter(cur, ref, MAX_SEARCH, report=rep)
        assert np.array_equal(decode(wide, ref), G.unique_cells(cur))
        narrow, intra = GI.encode_inter(cur, ref), G.encode(cur)
        c_wide = lossless_colour_encode(cur, lv, ref, lv)
        c_narrow, c_intra = LI.encode_inter(cur, lv, ref, lv), Q.encode(cur, lv)
        out[f"articulated{b}"] = {
            "points": rep["n"], "blocks": rep["blocks"], "vector_bytes": rep["vector_bytes"], "vectors_coded": bool(rep["vectors_coded"]),
            "geometry": {"intra_bytes": len(intra), "inter2_bytes": len(narrow), "inter7_bytes": len(wide),
                         "ratio_inter7_over_best_other": round(len(wide) / min(len(intra), len(narrow)), 4)},
            "lossless_colour": {"intra_bytes": len(c_intra), "inter2_bytes": len(c_narrow), "inter7_bytes": len(c_wide),
                                "ratio_inter7_over_intra": round(len(c_wide) / len(c_intra), 4)}}
        same7, same2 = encode_inter(ref, ref, MAX_SEARCH), GI.encode_inter(ref, ref)
        out[f"identical{b}"] = {"geometry": {"inter2_bytes": len(same2), "inter7_bytes": len(same7)}}
    return out


if __name__ == "__main__":
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = {"what": "wide-search inter streams (DESIGN.md 7e \"Wide search\"), numpy reference coders: surface_cloud(0, bits) with its "
                   f"x >= 2^(bits-1) half moved by {MOVE_HIGH} and the other half by {MOVE_LOW}, colours carried, against the unmoved "
                   "cloud; geometry 0xA7 / 0xA8 / 0xAA and lossless colour 0xB5 / 0xB6 / 0xB7; every 0xAA stream was decoded back; "
                   "nothing is gated on these figures",
           "clouds": rate_report()}
    with open(os.path.join(root, "profiles", "geometry_wide_rate.json"), "w") as f:
        json.dump(doc, f, indent=1)
