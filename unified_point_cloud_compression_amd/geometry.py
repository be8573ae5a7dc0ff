"""Lossless geometry of one block on the device: `encode_geometry` / `decode_geometry`.

A breadth-first octree over the block's unique voxels.  Level l (0 = root, `depth` = the voxels) is the set at pitch
2^(depth - l) of the origin-relative cells -- the project's own stride chain -- in canonical key order on both sides.  A node's
symbol is its child-occupancy byte (1..255), its context the 6-bit pattern of face neighbours present in its own level, which
the decoder knows completely before it decodes the level's bytes.

    stream  = u8 0xA7 | u32 n | u8 depth | 3 x i32 origin | level 0 | level 1 | ... | level depth-1
    level   = raw:    the bytes of its nodes                           (fewer than RAW_NODES nodes)
              coded:  8 x u32 popcount histogram | u32 length | rANS container of pcc_rans_encode_streams
                      (one channel, one group, `ceil(nodes / segment_nodes)` row segments; the count is the container's first word)

Node counts are not transmitted: level 0 has one node and a level's child total -- the sum of the popcounts of a raw level's
bytes, sum (k + 1) * hist[k] of a coded one -- is the next level's node count, so `parse_header` walks the whole stream on the
host and refuses it unless every level fits (children >= nodes, <= n, = n after the last level) and the length is exact.
Tables are never transmitted either: `derive_tables` builds the 64 frequency rows of a level from the (context, byte) counts
of the levels before it and the level's own popcount histogram, in integer arithmetic only.

There is no CPU fallback: the symbols are produced and consumed by the kernels of csrc/pcc_geom.hip and coded by the rANS
stream kernels.  Device->host reads, by construction: encode 5 (bounds, level sizes, histograms of all levels, raw levels'
bytes, the payload; one more for the canonicalisation's count when tensor rows are not yet in canonical order); decode ONE,
at the end (every level's rANS status, byte check, child total, popcount histogram and row count, and the bounds of `as_set`):
the decoder derives its tables on the device (`pcc_geom_tables`, the same integer rule) and sizes everything by the header.

Inter streams (`encode_geometry(x, reference=r)`, DESIGN.md section 7e "Inter frames"): with a reference cloud both sides hold,
the levels at and below the block pitch 2^BLOCK_LOG2 are coded against a motion-compensated prediction.

    stream  = u8 0xA8 | u32 n | u8 depth | 3 x i32 origin | u8 block_log2 | u8 search
              | levels 0 .. first-1 as above | vectors | levels first .. depth-1          (first = max(0, depth - block_log2))
    vectors = one index into `candidates(search)` per node of level `first` (a block), in canonical order:
              raw:    one byte each                                            (fewer than RAW_NODES blocks)
              coded:  u8 m | m x (u8 index, u32 count) ascending | u32 length | rANS container over the table of `vector_table`
              nothing at all when search = 0
    level   = raw:    the occupancy bytes of its nodes, as above
              coded:  8 x u32 popcount classes of the nodes absent from the prediction | 9 x u32 distance classes of the present
                      ones | u32 child total | u32 length | rANS container, table row = context + 64 * present

The prediction is the reference displaced per block by the block's vector and clipped to the block; a node present in it codes
rho^-1(byte XOR predicted byte), rho = 0..255 by (popcount, value), with table rows, adaptive counts and class correction of its
own (`derive_tables_inter`).  The kernels are those of csrc/pcc_geom_inter.hip; the encoder's vectors ride in the read that
fetches the raw levels' bytes, the decoder still reads ONCE, at the end.  `encode_sequence` / `decode_sequence` chain frames.

Wide search (`encode_geometry(x, reference=r, search=3..7)`, DESIGN.md section 7e "Wide search"): the same stream with the block
vectors searched over [-search, search]^3 by `pcc_geom_wide_motion` and listed as displacements, one component at a time.

    stream  = u8 0xAA | the rest of the 0xA8 layout, search in 3 .. 7, with
    vectors = per block, in canonical order, the components (dx + search, dy + search, dz + search), each in 0 .. 2 * search:
              raw:    three bytes each, x y z                                  (fewer than RAW_NODES blocks)
              coded:  3 x [u8 m | m x (u8 value, u32 count) ascending], one histogram per component, each summing to the blocks
                      | u32 length | ONE rANS container over the [blocks, 3] components, table row = component, the three rows
                      built by the rule of `vector_table` with K = 2 * search + 1

Most matches win; ties go to the smaller dx^2 + dy^2 + dz^2, then to the lexicographically smaller (dx, dy, dz) -- the lowest index
of `candidates(search)`, so the rule of 0xA8.  search = None or 2 writes 0xA8 byte for byte; "auto" codes at 2 and at 7 and keeps
the shorter stream (2 on a tie).  An 0xA8 stream whose search byte is not 0..2 and an 0xAA stream whose is not 3..7 are refused.

Global motion (`encode_geometry(x, reference=r, global_motion=...)`, DESIGN.md section 7e "Global motion"): one rigid transform
moves the whole reference before the blocks look at it.

    stream  = u8 0xA9 | 9 x i32 M (Q24, row by row) | 3 x i32 t (Q8 voxels) | an 0xA7, 0xA8 or 0xAA stream as above  (49 bytes + it)

The stream behind the transform is coded against `motion.warp_cloud(reference, T)`, an integer warp both sides repeat
(`pcc_motion_warp`).  `parse_header` checks the transform's ranges on the host; the decoder warps the reference rows as they
come (no canonicalisation first: the set of warped cells does not depend on their order), which costs the one read the
canonicalisation of the reference would have cost, and decodes the inner stream as before.

Several references (`encode_geometry(x, reference=[r0, (r1, T), ...])`, DESIGN.md section 7e "Several references"): up to four
reference slots, every block predicted from the slot that matches it best.

    stream  = u8 0xAB | u8 K (2..4) | K x slot | inner
    slot    = u8 source (an index into the clouds the decoder is handed) | u8 warped (0 / 1) | if warped: 12 x i32 transform
    inner   = a complete 0xA8 or 0xAA stream, magic byte included, with the selector list immediately before the vector list
    selectors = one slot number per block, in canonical order:
              raw:    one byte each                                            (fewer than RAW_NODES blocks)
              coded:  u8 m | m x (u8 slot, u32 count) ascending | u32 length | rANS container over `vector_table(hist)` of the K slots

Every slot is searched as a single reference would be (a warped slot as `motion.warp_set(cloud, T)`); a block takes the slot
with the most matches under that slot's vector, the lower slot on a tie, and lists that slot's vector.  The kernel is
`pcc_geom_multi_block_bits` (csrc/pcc_geom_multi.hip); the selectors ride in the encoder's read of the raw levels' bytes, and the
decoder's one read carries the selector list's rANS status and range flag.
"""
import ctypes as C
import itertools
import struct

import numpy as np
import torch

from . import lib as L
from . import motion as M
from . import rans as R
from . import sparse as S

MAGIC = 0xA7              # format version 1
RAW_NODES = 128           # levels with fewer nodes travel as raw bytes (a coded level costs 36 bytes of side information + 20 of framing)
SEGMENT_NODES = 512       # nodes per rANS stream of a coded level: streams = ceil(nodes / SEGMENT_NODES), 12 bytes of framing each
#                           (3.5 % of the ~340 bytes 512 surface nodes code to; a stream is decoded serially by one wave at
#                           ~0.27 us per symbol, so the length of a stream is the decode time of a level)
MAX_DEPTH = 15            # cells fit the 16-bit key fields (coordinates below 2^15 after the bias)
HEADER = struct.Struct("<BIB3i")
SIDE = struct.Struct("<8II")
N_CTX, N_SYM = 64, 255
PRIOR_WEIGHT = 16         # observations the global byte distribution is worth inside a context
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def segments_for(nodes, segment_nodes=SEGMENT_NODES):
    """Row segments (= rANS streams) of a coded level."""
    return R.segments_for(nodes, segment_nodes, 65536)


def derive_tables(counts, pop):
    """Quantised CDF rows [64, 257] int32 of one level (255 bytes + the rANS escape slot, which never occurs and gets
    frequency 1), from the adaptive counts [64, 256] and this level's popcount histogram pop[8].  Integers only:
      1. the counts are shifted right until their total is below 2^20 (N), G[s] = sum_c N[c][s], Gt = sum G;
      2. context mix  W[c][s] = N[c][s] * (Gt + 255) + PRIOR_WEIGHT * (G[s] + 1)      (N/Nc blended with (G + 1)/(Gt + 255))
         q[c][s] = 1 + W[c][s] * 2^20 // sum_s W[c][s];
      3. popcount correction  r[k] = clamp(pop[k] * (Gt + 255) * 2^12 // (sum(pop) * E[k]), 1, 2^20), E[k] = sum of G[s] + 1 over
         the bytes with k + 1 bits; r[k] = 0 when pop[k] = 0 (no byte of that class occurs in the level);
         w[c][s] = q[c][s] * r[popcount(s) - 1];
      4. f[c][s] = 1 + w[c][s] * (65535 - 255) // sum_s w[c][s]; what is left of 65535 goes to the row's first largest f."""
    N = np.asarray(counts, dtype=np.int64).reshape(N_CTX, 256)[:, 1:]
    total = int(N.sum())
    shift = max(0, total.bit_length() - 20)
    N = N >> shift
    G = N.sum(axis=0)
    gt = int(G.sum()) + N_SYM
    W = N * gt + PRIOR_WEIGHT * (G + 1)[None, :]
    q = 1 + (W << 20) // W.sum(axis=1, keepdims=True)
    pc = POPCOUNT[1:] - 1
    pop = [int(v) for v in pop]
    ptot = sum(pop)
    r = np.zeros(8, dtype=np.int64)
    for k in range(8):
        if pop[k] > 0:
            e = int((G[pc == k] + 1).sum())
            r[k] = min(max((pop[k] * gt << 12) // (ptot * e), 1), 1 << 20)
    w = q * r[pc][None, :]
    f = 1 + w * (65535 - N_SYM) // w.sum(axis=1, keepdims=True)
    rows = np.arange(N_CTX)
    f[rows, np.argmax(f, axis=1)] += 65535 - f.sum(axis=1)
    cdf = np.zeros((N_CTX, N_SYM + 2), dtype=np.int64)
    cdf[:, 1:N_SYM + 1] = np.cumsum(f, axis=1)
    cdf[:, N_SYM + 1] = 65536
    return np.ascontiguousarray(cdf.astype(np.int32))


TABLE_SIZES = np.full(N_CTX, N_SYM + 2, dtype=np.int32)
TABLE_OFFSETS = np.ones(N_CTX, dtype=np.int32)

# ---- the inter stream, format 0xA8 (module docstring; DESIGN.md section 7e "Inter frames") -----------------------------------
MAGIC_INTER = 0xA8
MAGIC_GLOBAL = 0xA9       # wrapper: u8 0xA9 | 12 x i32 transform | an 0xA7 or 0xA8 stream coded against the warped reference
GLOBAL_HEADER = 1 + M.PACKED.size
BLOCK_LOG2 = 4            # blocks are the nodes at pitch 16: one motion vector each
SEARCH = 2                # vectors in [-2, 2]^3: 125 candidates, an index fits a byte
MAX_SEARCH = 2
MAGIC_WIDE = 0xAA         # the 0xA8 layout with search in WIDE_SEARCH and the vectors listed as displacements, per component
WIDE_SEARCH = (3, 7)      # dx + 8 fits the 4 bits of a packed displacement, a window column of 16 + 2 * 7 z cells fits a word
MAGIC_MULTI = 0xAB        # wrapper: u8 0xAB | u8 K | K slots | an 0xA8 or 0xAA stream with a selector list before its vector list
MAX_SLOTS = 4
HEADER_INTER = struct.Struct("<BIB3iBB")
SIDE_INTER = struct.Struct("<8I9III")      # popcount classes of the absent nodes | distance classes of the present | children | length
N_ROWS = 2 * N_CTX        # table rows: context + 64 * present
INTER_STRIDE = 258        # present rows: 256 symbols + the escape slot
RHO = np.array(sorted(range(256), key=lambda t: (int(POPCOUNT[t]), t)), dtype=np.int64)     # symbol -> t = byte XOR prediction
RHO_INV = np.argsort(RHO)
INTER_SIZES = np.array([N_SYM + 2] * N_CTX + [INTER_STRIDE] * N_CTX, dtype=np.int32)
INTER_OFFSETS = np.array([1] * N_CTX + [0] * N_CTX, dtype=np.int32)


def candidates(search=SEARCH):
    """The (2 * search + 1)^3 motion vectors by |v|^2, then lexicographically; index 0 is the zero vector."""
    r = range(-search, search + 1)
    return sorted(((dx, dy, dz) for dx in r for dy in r for dz in r), key=lambda v: (v[0] ** 2 + v[1] ** 2 + v[2] ** 2, v))


def _family_rows(N, cls, classes, hist):
    """Frequencies [64, nsym] of one population (steps 1-4 of `derive_tables`): N the live columns of its counts, cls the class
    of each live symbol, hist the level's class histogram.  A population without a node in the level takes r = 1."""
    nsym = N.shape[1]
    shift = max(0, int(N.sum()).bit_length() - 20)
    N = N >> shift
    G = N.sum(axis=0)
    gt = int(G.sum()) + nsym
    W = N * gt + PRIOR_WEIGHT * (G + 1)[None, :]
    q = 1 + (W << 20) // W.sum(axis=1, keepdims=True)
    hist = [int(v) for v in hist]
    ht = sum(hist)
    r = np.full(classes, 1 if ht == 0 else 0, dtype=np.int64)
    for k in range(classes):
        if hist[k] > 0:
            e = int((G[cls == k] + 1).sum())
            r[k] = min(max((hist[k] * gt << 12) // (ht * e), 1), 1 << 20)
    w = q * r[cls][None, :]
    f = 1 + w * (65535 - nsym) // w.sum(axis=1, keepdims=True)
    f[np.arange(N_CTX), np.argmax(f, axis=1)] += 65535 - f.sum(axis=1)
    return f


def derive_tables_inter(counts, pop, dist):
    """Quantised CDF rows [128, 258] int32 of one inter level.  Rows 0..63, the nodes absent from the prediction: the rule of
    `derive_tables` on counts[:64] and the popcount histogram of those nodes (257 entries).  Rows 64..127, the present nodes:
    the same rule over the 256 symbols rho^-1(byte XOR prediction) with the 9 classes popcount(byte XOR prediction) and their
    histogram dist[9] (258 entries).  The two populations are rescaled, mixed and corrected separately."""
    counts = np.asarray(counts, dtype=np.int64).reshape(N_ROWS, 256)
    cdf = np.zeros((N_ROWS, INTER_STRIDE), dtype=np.int64)
    cdf[:N_CTX, 1:N_SYM + 1] = np.cumsum(_family_rows(counts[:N_CTX, 1:], POPCOUNT[1:] - 1, 8, pop), axis=1)
    cdf[:N_CTX, N_SYM + 1] = 65536
    cdf[N_CTX:, 1:257] = np.cumsum(_family_rows(counts[N_CTX:], POPCOUNT[RHO], 9, dist), axis=1)
    cdf[N_CTX:, 257] = 65536
    return np.ascontiguousarray(cdf.astype(np.int32))


def vector_table(hist):
    """CDF row [1, K + 2] of the vector indices from their transmitted histogram hist[K]: f = 1 + hist * (65535 - K) // blocks,
    what is left of 65535 to the first largest f, 1 for the escape slot."""
    k = len(hist)
    total = sum(int(v) for v in hist)
    f = [1 + int(v) * (65535 - k) // total for v in hist]
    f[f.index(max(f))] += 65535 - sum(f)
    cdf = np.zeros((1, k + 2), dtype=np.int32)
    cdf[0, 1:k + 1] = np.cumsum(f)
    cdf[0, k + 1] = 65536
    return cdf


def _container_streams(data, at, nbytes, symbols, what):
    """The stream count a container of `nbytes` bytes at data[at:] claims for `symbols` symbols; refuses what cannot be one."""
    if nbytes < 8 or nbytes % 4 or at + nbytes > len(data):
        raise L.PccError(f"geometry stream truncated inside the payload of {what}")
    streams = int.from_bytes(data[at:at + 4], "little")
    if not 1 <= streams <= min(symbols, 65536) or nbytes < 4 * (1 + streams):
        raise L.PccError(f"geometry stream: {what} claims {streams} rANS streams for {symbols} symbols")
    return streams


def _parse_vectors(data, at, blocks, k):
    """The vector list behind the levels above the blocks: (dict(raw, payload, hist, streams), end)."""
    if k == 1:
        return {"raw": True, "payload": (at, at), "hist": [blocks], "streams": 0}, at
    if blocks < RAW_NODES:
        if at + blocks > len(data):
            raise L.PccError("geometry stream truncated inside the vector list")
        if max(data[at:at + blocks]) >= k:
            raise L.PccError(f"geometry stream: a vector index outside the {k} candidates")
        return {"raw": True, "payload": (at, at + blocks), "hist": None, "streams": 0}, at + blocks
    if at + 1 > len(data) or at + 1 + 5 * data[at] + 4 > len(data):
        raise L.PccError("geometry stream truncated inside the vector histogram")
    hist, last = [0] * k, -1
    for j in range(data[at]):
        i, c = struct.unpack_from("<BI", data, at + 1 + 5 * j)
        if not last < i < k or c == 0:
            raise L.PccError("geometry stream: the vector histogram lists indices in ascending order, each with a count")
        hist[i], last = c, i
    if sum(hist) != blocks:
        raise L.PccError(f"geometry stream: the vector histogram counts {sum(hist)} of {blocks} blocks")
    at += 1 + 5 * data[at]
    nbytes = int.from_bytes(data[at:at + 4], "little")
    at += 4
    streams = _container_streams(data, at, nbytes, blocks, "the vector list")
    return {"raw": False, "payload": (at, at + nbytes), "hist": hist, "streams": streams}, at + nbytes


def _parse_vectors_wide(data, at, blocks, search):
    """The vector list of an 0xAA stream: (dict(raw, payload, hist, streams), end); hist = the three component histograms."""
    k = 2 * search + 1
    if blocks < RAW_NODES:
        if at + 3 * blocks > len(data):
            raise L.PccError("geometry stream truncated inside the vector list")
        if max(data[at:at + 3 * blocks]) >= k:
            raise L.PccError(f"geometry stream: a vector component outside 0..{k - 1}")
        return {"raw": True, "payload": (at, at + 3 * blocks), "hist": None, "streams": 0}, at + 3 * blocks
    hists = []
    for axis in "xyz":
        if at + 1 > len(data) or at + 1 + 5 * data[at] > len(data):
            raise L.PccError("geometry stream truncated inside the vector histograms")
        hist, last = [0] * k, -1
        for j in range(data[at]):
            i, c = struct.unpack_from("<BI", data, at + 1 + 5 * j)
            if not last < i < k or c == 0:
                raise L.PccError(f"geometry stream: the {axis} histogram of the vectors lists components 0..{k - 1} in ascending order, "
                                 "each with a count")
            hist[i], last = c, i
        if sum(hist) != blocks:
            raise L.PccError(f"geometry stream: the {axis} histogram of the vectors counts {sum(hist)} of {blocks} blocks")
        at += 1 + 5 * data[at]
        hists.append(hist)
    if at + 4 > len(data):
        raise L.PccError("geometry stream truncated inside the vector histograms")
    nbytes = int.from_bytes(data[at:at + 4], "little")
    at += 4
    streams = _container_streams(data, at, nbytes, 3 * blocks, "the vector list")
    return {"raw": False, "payload": (at, at + nbytes), "hist": hists, "streams": streams}, at + nbytes


def _parse_selectors(data, at, blocks, k):
    """The selector list of an 0xAB stream's inner stream, the layout of `_parse_vectors` over the k slots."""
    if blocks < RAW_NODES:
        if at + blocks > len(data):
            raise L.PccError("geometry stream truncated inside the selector list")
        if max(data[at:at + blocks]) >= k:
            raise L.PccError(f"geometry stream: a selector outside the {k} reference slots")
        return {"raw": True, "payload": (at, at + blocks), "hist": None, "streams": 0}, at + blocks
    if at + 1 > len(data) or at + 1 + 5 * data[at] + 4 > len(data):
        raise L.PccError("geometry stream truncated inside the selector histogram")
    hist, last = [0] * k, -1
    for j in range(data[at]):
        i, c = struct.unpack_from("<BI", data, at + 1 + 5 * j)
        if not last < i < k or c == 0:
            raise L.PccError(f"geometry stream: the selector histogram lists the slots 0..{k - 1} in ascending order, each with a count")
        hist[i], last = c, i
    if sum(hist) != blocks:
        raise L.PccError(f"geometry stream: the selector histogram counts {sum(hist)} of {blocks} blocks")
    at += 1 + 5 * data[at]
    nbytes = int.from_bytes(data[at:at + 4], "little")
    at += 4
    streams = _container_streams(data, at, nbytes, blocks, "the selector list")
    return {"raw": False, "payload": (at, at + nbytes), "hist": hist, "streams": streams}, at + nbytes


def _parse_multi(data, have_reference, clouds):
    """The dictionary of an 0xAB stream: that of its inner stream with `slots` = [(source, RigidTransform or None)], `selectors`
    and `inner`, the byte the payload spans count from."""
    clouds = (1 if have_reference else 0) if clouds is None else int(clouds)
    if not have_reference or clouds < 1:
        raise L.PccError("geometry stream: a stream with several references (0xab) decodes against reference clouds, none was given")
    if len(data) < 2:
        raise L.PccError("geometry stream truncated inside the slot table")
    k = data[1]
    if not 2 <= k <= MAX_SLOTS:
        raise L.PccError(f"geometry stream (0xab): {k} reference slots, this build reads 2..{MAX_SLOTS}")
    at, slots = 2, []
    for s in range(k):
        if at + 2 > len(data):
            raise L.PccError("geometry stream truncated inside the slot table")
        source, warped = data[at], data[at + 1]
        at += 2
        if source >= clouds:
            raise L.PccError(f"geometry stream (0xab): slot {s} names reference cloud {source}, {clouds} {'was' if clouds == 1 else 'were'} given")
        if warped > 1:
            raise L.PccError(f"geometry stream (0xab): slot {s} has the warped byte {warped}, this build reads 0 and 1")
        T = None
        if warped:
            if at + M.PACKED.size > len(data):
                raise L.PccError("geometry stream truncated inside the transform of a reference slot")
            T = M.RigidTransform.unpack(data[at:at + M.PACKED.size])        # (refuses entries outside the ranges)
            at += M.PACKED.size
        slots.append((source, T))
    if at >= len(data):
        raise L.PccError("geometry stream truncated behind the slot table")
    if data[at] not in (MAGIC_INTER, MAGIC_WIDE):
        raise L.PccError(f"geometry stream (0xab): the stream behind the slot table has the magic byte {data[at]:#x}, not {MAGIC_INTER:#x} or "
                         f"{MAGIC_WIDE:#x}")
    hdr = parse_header(bytes(data[at:]), True, _selectors=k)
    hdr.update(slots=slots, inner=at)
    return hdr


def parse_header(data, have_reference=True, clouds=None, _selectors=0):
    """Walk the stream on the host: {n, depth, origin, levels}; levels[l] = dict(nodes, children, raw, payload=(begin, end),
    pop).  An inter stream (0xA8, or 0xAA: the wide search, whose `vectors["hist"]` are three component histograms) adds
    inter=True, block_log2, search, first (the level of the blocks) and vectors = dict(raw,
    payload, hist, streams); its levels carry `inter` (coded against the prediction) and, coded ones of those, `dist`.  Raises PccError on a bad magic byte, depth, n, block size or search
    range, on an inter stream when the caller has no reference, on truncated or inconsistent side information and on trailing
    bytes -- before any GPU work.  A global-motion wrapper (0xA9) is refused without a reference too; its transform's ranges are
    checked here, the stream behind it is parsed as above (and must not be a wrapper again) and its dictionary is returned with
    `transform` (a RigidTransform) and `inner` = 49, the byte the payload spans count from.  A stream with several references
    (0xAB) is refused without a reference, with a slot count outside 2..4, a slot whose `source` is not below `clouds` (the number
    of reference clouds the caller holds; None: one when there is a reference), a warped byte above 1, a transform 0xA9 would
    refuse or another magic byte than 0xA8 / 0xAA behind the slot table; its dictionary is that of the stream behind the table
    with `slots` = [(source, RigidTransform or None)], `selectors` = dict(raw, payload, hist, streams) and `inner`."""
    if len(data) >= 1 and data[0] == MAGIC_MULTI and not _selectors:
        return _parse_multi(data, have_reference, clouds)
    if len(data) >= 1 and data[0] == MAGIC_GLOBAL:
        if not have_reference:
            raise L.PccError("geometry stream: a global-motion stream (0xa9) decodes against a reference cloud, none was given")
        if len(data) < GLOBAL_HEADER:
            raise L.PccError("geometry stream truncated inside the global-motion transform")
        transform = M.RigidTransform.unpack(data[1:GLOBAL_HEADER])          # (refuses entries outside the ranges)
        if len(data) > GLOBAL_HEADER and data[GLOBAL_HEADER] == MAGIC_GLOBAL:
            raise L.PccError("geometry stream: a global-motion stream wraps an intra or an inter stream, not another wrapper")
        hdr = parse_header(bytes(data[GLOBAL_HEADER:]), have_reference)
        hdr.update(transform=transform, inner=GLOBAL_HEADER)
        return hdr
    if len(data) < HEADER.size:
        raise L.PccError("geometry stream truncated inside the header")
    magic, n, depth, ox, oy, oz = HEADER.unpack_from(data, 0)
    if magic not in (MAGIC, MAGIC_INTER, MAGIC_WIDE):
        raise L.PccError(f"geometry stream: magic byte {magic:#x}, this build reads {MAGIC:#x}, {MAGIC_INTER:#x}, {MAGIC_GLOBAL:#x}, "
                         f"{MAGIC_WIDE:#x} and {MAGIC_MULTI:#x}")
    inter, wide = magic != MAGIC, magic == MAGIC_WIDE
    at, first, k, block_log2, search = HEADER.size, depth, 1, 0, 0
    if inter:
        if not have_reference:
            raise L.PccError(f"geometry stream: an inter stream ({magic:#x}) decodes against a reference cloud, none was given")
        if len(data) < HEADER_INTER.size:
            raise L.PccError("geometry stream truncated inside the header")
        block_log2, search = data[at], data[at + 1]
        at = HEADER_INTER.size
        lo, hi = WIDE_SEARCH if wide else (0, MAX_SEARCH)
        if block_log2 != BLOCK_LOG2 or not lo <= search <= hi:
            raise L.PccError(f"geometry stream ({magic:#x}): block_log2 {block_log2} / search {search}, this build reads {BLOCK_LOG2} / {lo}..{hi}")
        if n == 0:
            raise L.PccError("geometry stream: an empty cloud travels as an intra stream")
        first, k = max(0, depth - block_log2), (2 * search + 1) ** 3
    if n == 0:
        if depth != 0 or len(data) != HEADER.size:
            raise L.PccError("geometry stream: an empty cloud has depth 0 and no levels")
        return {"n": 0, "depth": 0, "origin": (ox, oy, oz), "levels": []}
    if not 1 <= depth <= MAX_DEPTH:
        raise L.PccError(f"geometry stream: depth {depth} outside 1..{MAX_DEPTH}")
    if n > 8 ** min(depth, 10) or n >= (1 << 31):
        raise L.PccError(f"geometry stream: header claims {n} points at depth {depth}")
    reach = (1 << (depth - 1)) if depth > 1 else 0            # the largest cell has bit depth - 1 set (depth is minimal)
    if min(ox, oy, oz) < -S.BIAS + 64 or max(ox, oy, oz) + reach >= S.BIAS - 64:
        raise L.PccError(f"geometry stream: origin {(ox, oy, oz)} at depth {depth} leaves the 16-bit key range")
    nodes, levels, vectors, selectors = 1, [], None, None
    for lvl in range(depth):
        if inter and lvl == first:
            if _selectors:
                selectors, at = _parse_selectors(data, at, nodes, _selectors)
            vectors, at = _parse_vectors_wide(data, at, nodes, search) if wide else _parse_vectors(data, at, nodes, k)
        if nodes < RAW_NODES:
            if at + nodes > len(data):
                raise L.PccError(f"geometry stream truncated inside raw level {lvl}")
            body = data[at:at + nodes]
            if 0 in body:
                raise L.PccError(f"geometry stream: raw level {lvl} holds an empty node")
            children = sum(int(POPCOUNT[b]) for b in body)
            lv = {"nodes": nodes, "children": children, "raw": True, "payload": (at, at + nodes), "pop": None}
            at += nodes
        elif lvl >= first:
            if at + SIDE_INTER.size > len(data):
                raise L.PccError(f"geometry stream truncated inside the side information of level {lvl}")
            side = SIDE_INTER.unpack_from(data, at)
            pop, dist, children, nbytes = list(side[:8]), list(side[8:17]), side[17], side[18]
            at += SIDE_INTER.size
            if sum(pop) + sum(dist) != nodes:
                raise L.PccError(f"geometry stream: level {lvl} has {nodes} nodes, its class histograms count {sum(pop) + sum(dist)}")
            streams = _container_streams(data, at, nbytes, nodes, f"level {lvl}")
            lv = {"nodes": nodes, "children": children, "raw": False, "payload": (at, at + nbytes), "pop": pop, "dist": dist,
                  "streams": streams}
            at += nbytes
        else:
            if at + SIDE.size > len(data):
                raise L.PccError(f"geometry stream truncated inside the side information of level {lvl}")
            *pop, nbytes = SIDE.unpack_from(data, at)
            at += SIDE.size
            if sum(pop) != nodes:
                raise L.PccError(f"geometry stream: level {lvl} has {nodes} nodes, its popcount histogram counts {sum(pop)}")
            streams = _container_streams(data, at, nbytes, nodes, f"level {lvl}")
            children = sum((k_ + 1) * v for k_, v in enumerate(pop))
            lv = {"nodes": nodes, "children": children, "raw": False, "payload": (at, at + nbytes), "pop": pop, "streams": streams}
            at += nbytes
        if inter:
            lv["inter"] = lvl >= first
        # a zero byte is unrepresentable: a level's child total is at least its node count, and never more than n
        if not nodes <= children <= n:
            raise L.PccError(f"geometry stream: level {lvl} expands {nodes} nodes to {children} for {n} points")
        levels.append(lv)
        nodes = children
    if nodes != n:
        raise L.PccError(f"geometry stream: the last level gives {nodes} points, the header says {n}")
    if at != len(data):
        raise L.PccError("geometry stream: trailing bytes")
    hdr = {"n": n, "depth": depth, "origin": (ox, oy, oz), "levels": levels}
    if inter:                                  # (an intra stream's dictionary is what it always was)
        hdr.update(inter=True, block_log2=block_log2, search=search, first=first, vectors=vectors)
    if _selectors:
        hdr["selectors"] = selectors
    return hdr


# ------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------
def _key_of(x, y, z):
    return ((x + S.BIAS) << 32) | ((y + S.BIAS) << 16) | (z + S.BIAS)


def canonical_rows(x, what="encode_geometry"):
    """(set, perm, keep): the canonical, de-duplicated pitch-1 single-batch CoordSet of the input with exact bounds, and for
    tensor rows the permutation / surviving rows of `sparse.coordset_from_coords` (None, None for a set, whose rows already
    are canonical).  `what` names the caller in the refusals."""
    if isinstance(x, S.CoordSet):
        if x.ts != 1:
            raise L.PccError(f"{what}: a pitch-1 coordinate set is required, got pitch {x.ts}")
        if x.bounds.bmax > 0:
            raise L.PccError(f"{what} codes one block: batched input is not supported")
        if x.n == 0:
            return x, None, None
        b = S.bounds_of(x.coords())               # a set's own bounds may be conservative; the header needs the minimum
        if b.bmax > 0:
            raise L.PccError(f"{what} codes one block: batched input is not supported")
        cs = S.CoordSet(x.keys, x.n, 1, b, on_lattice=True)        # a set of our own: the caller's object is not touched
        if b.lo == x.bounds.lo and b.hi == x.bounds.hi:
            cs.share_grid(x)
        return cs, None, None
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] < 3:
        raise L.PccError(f"{what}: an [N, >= 3] tensor or a CoordSet is required")
    if not x.is_cuda:
        raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
    xyz = x[:, :3]
    xyz = torch.floor(xyz).to(torch.int32) if xyz.dtype.is_floating_point else xyz.to(torch.int32)
    c4 = torch.cat([torch.zeros((x.shape[0], 1), dtype=torch.int32, device=x.device), xyz], dim=1).contiguous()
    cs, perm, keep = S.coordset_from_coords(c4, 1)
    if cs.bounds.bmax > 0:
        raise L.PccError(f"{what} codes one block: batched input is not supported")
    return cs, perm, keep


def _input_set(x):
    """Canonical, de-duplicated pitch-1 single-batch CoordSet of the input, with exact bounds."""
    return canonical_rows(x)[0]


def level_sets(cs, origin, depth):
    """[level 0 (root), ..., level depth (the voxels)] as CoordSets of origin-relative cells (shared with attributes.py)."""
    dev = cs.device
    ext = [cs.bounds.hi[i] - origin[i] for i in range(3)]
    if all(v == 0 for v in origin):
        base = cs
    else:
        keys = cs.keys[:cs.n] - ((origin[0] << 32) + (origin[1] << 16) + origin[2])
        base = S.CoordSet(keys, cs.n, 1, S.Bounds(0, (0, 0, 0), ext), on_lattice=True)
    strides = [1 << s for s in range(1, depth)]
    if strides:
        pend = base.stride_chain_begin(strides)
        if pend is not None:
            S.resolve(pend)
    sets, cur = [base], base
    for m in strides:
        cur = cur.stride(m)
        sets.append(cur)
    root = S.CoordSet(torch.tensor([_key_of(0, 0, 0)], dtype=torch.int64, device=dev), 1, 1 << depth, S.Bounds(0, (0, 0, 0), (0, 0, 0)))
    sets.append(root)
    return sets[::-1]


def reference_set(reference, what="encode_geometry"):
    """The reference cloud of an inter stream as a canonical pitch-1 single-batch CoordSet in absolute coordinates (the rules of
    `canonical_rows`), or None for an empty one."""
    if torch.is_tensor(reference) and reference.dim() == 2 and reference.shape[1] >= 3 and reference.is_cuda and reference.shape[0] == 0:
        return None
    rs = canonical_rows(reference, f"{what} (reference)")[0]
    return rs if rs.n else None


@torch.no_grad()
def encode_geometry(x, segment_nodes=SEGMENT_NODES, timings=None, reference=None, mode="auto", global_motion=None, search=None):
    """[N, >= 3] GPU tensor (any row order, duplicates allowed, floats floored) or pitch-1 CoordSet -> bytes.
    segment_nodes: nodes per rANS stream (tests lower it to cut small levels into several streams; the decoder reads the
    stream count from each container).  timings: a dict that receives per-level device events (tools/geometry_timing.py).
    reference: a voxel cloud the decoder holds too (same kinds of input as x), against which the levels at and below the block
    pitch are predicted.  mode "auto": the shorter of the inter (0xA8) and the intra (0xA7) stream, intra on a tie -- never
    longer than without a reference; "inter": the inter stream (an empty cloud still travels as intra); "intra", or no
    reference: today's stream byte for byte.
    global_motion (DESIGN.md section 7e "Global motion"): None -- the streams above.  A `motion.RigidTransform` T -- the wrapper
    stream u8 0xA9 | 12 x i32 T | the stream above coded against `motion.warp_cloud(reference, T)` under `mode` (a reference
    is required).  "auto" -- T = `motion.estimate_rigid(x, reference)`; the wrapper and the plain stream are both coded and
    the shorter one is returned, the plain one on a tie, when nothing matches or T is the identity: never longer than without
    global motion.
    search (DESIGN.md section 7e "Wide search"): the range of the block vectors of an inter stream.  None or 2 -- [-2, 2]^3, the
    0xA8 stream, today's bytes.  3 .. 7 -- [-search, search]^3, the 0xAA stream.  "auto" -- coded at 2 and at 7, the shorter stream
    is kept, 2 on a tie; with mode "auto" that stream is then compared with the intra one as before, so a wider search never
    costs bytes, only encode time.  0 and 1 are refused: the encoder has never written them.
    Several references (DESIGN.md section 7e "Several references"): reference may be a list or tuple of 1 .. 4 entries, each a
    cloud or a pair (cloud, RigidTransform) -- that cloud warped; the transform travels in the stream.  A one-entry list is that
    entry, a lone pair is the 0xA9 call; with a list global_motion must be None.  Two or more entries: every block takes the
    entry that matches it best (stream 0xAB).  mode "inter" forces that stream; "auto" returns the shorter of it and of the same
    call with the first entry alone, that one on a tie -- more references never cost bytes.  search "auto" codes the 0xAB stream
    at 2 and at 7.  global_motion="both" with a single reference: shorthand for [reference, (reference, estimate_rigid(x,
    reference))], the plain call when there is no estimate or it is the identity."""
    if mode not in ("auto", "inter", "intra"):
        raise L.PccError(f"encode_geometry: mode {mode!r} is not one of auto, inter, intra")
    search = check_search(search, "encode_geometry")
    if not (global_motion is None or isinstance(global_motion, M.RigidTransform) or (isinstance(global_motion, str) and global_motion in ("auto", "both"))):
        raise L.PccError(f"encode_geometry: global_motion {global_motion!r} is not None, \"auto\", \"both\" or a RigidTransform")
    cs = _input_set(x)
    if isinstance(reference, (list, tuple)):
        slots = reference_slots(reference, "encode_geometry")
        if global_motion is not None:
            raise L.PccError("encode_geometry: with a list of references global_motion must be None (a transform travels with its entry: "
                             "(cloud, RigidTransform))")
        if len(slots) == 1:                            # a one-entry list is that entry; a lone pair is the 0xA9 call
            return encode_geometry(cs, segment_nodes, timings, slots[0][0], mode, slots[0][1], search)
        return _encode_multi(cs, slots, mode, segment_nodes, timings, search)
    if isinstance(global_motion, str) and global_motion == "both":
        if reference is None or mode == "intra" or cs.n == 0:
            return _encode(cs, INTRA, segment_nodes, timings)
        rs = reference_set(reference)
        T = M.estimate_rigid(cs, rs) if rs is not None else None
        if T is None or T.is_identity():
            return _encode_against(cs, rs, mode, segment_nodes, timings, search)
        return _encode_multi(cs, [(rs, None), (rs, T)], mode, segment_nodes, timings, search)
    if isinstance(global_motion, M.RigidTransform):
        if reference is None:
            raise L.PccError("encode_geometry: a global motion transform needs the reference it moves")
        return _encode_global(cs, reference_set(reference), global_motion, mode, segment_nodes, timings, search)
    if reference is None or mode == "intra" or cs.n == 0:
        return _encode(cs, INTRA, segment_nodes, timings)
    rs = reference_set(reference)
    plain = _encode_against(cs, rs, mode, segment_nodes, timings, search)
    if global_motion is None or rs is None:
        return plain
    T = M.estimate_rigid(cs, rs)
    if T is None or T.is_identity():
        return plain
    tw = {} if timings is not None else None
    wrapped = _encode_global(cs, rs, T, mode, segment_nodes, tw, search)
    take = len(wrapped) < len(plain)
    if timings is not None:
        if take:                                   # the events of the stream that is returned, not of the discarded one
            timings.clear()
            timings.update(tw)
        timings["global_bytes"], timings["plain_bytes"] = len(wrapped), len(plain)
    return wrapped if take else plain


def _encode_global(cs, rs, T, mode, segment_nodes, timings, search=SEARCH):
    """The wrapper stream (0xA9) of the canonical set `cs`: the transform, then `cs` against the warped reference set."""
    ws = M.warp_set(rs, T) if rs is not None else None
    if ws is not None and ws.n == 0:
        ws = None
    inner = _encode(cs, INTRA, segment_nodes, timings) if (mode == "intra" or cs.n == 0) else _encode_against(cs, ws, mode, segment_nodes, timings, search)
    return bytes([MAGIC_GLOBAL]) + T.pack() + inner


def _is_pair(entry):
    return isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], M.RigidTransform)


def reference_slots(reference, what):
    """[(cloud, RigidTransform or None)] of a `reference=` argument: a cloud, a pair (cloud, RigidTransform) -- that cloud warped --
    or a list / tuple of 1..MAX_SLOTS of either."""
    if _is_pair(reference):
        return [(reference[0], reference[1])]
    if not isinstance(reference, (list, tuple)):
        return [(reference, None)]
    if not 1 <= len(reference) <= MAX_SLOTS:
        raise L.PccError(f"{what}: a list of references holds 1..{MAX_SLOTS} entries, got {len(reference)}")
    slots = []
    for e in reference:
        if _is_pair(e):
            slots.append((e[0], e[1]))
        elif e is None or isinstance(e, (list, tuple)):
            raise L.PccError(f"{what}: an entry of a list of references is a cloud or a pair (cloud, RigidTransform)")
        else:
            slots.append((e, None))
    return slots


def slot_sources(slots):
    """(the distinct clouds of the slots in order of first appearance, the index of each slot's cloud among them): entries that
    are the same object share a source, so `[r, (r, T)]` decodes against `r` alone and against the same list alike."""
    clouds, sources = [], []
    for cloud, _ in slots:
        at = next((i for i, c in enumerate(clouds) if c is cloud), len(clouds))
        if at == len(clouds):
            clouds.append(cloud)
        sources.append(at)
    return clouds, sources


def _slot_sets(slots, what):
    """(the reference set of every slot -- None: empty --, its source): each distinct cloud canonicalised once, a warped slot
    through `motion.warp_set` of that set."""
    clouds, sources = slot_sources(slots)
    plain = [reference_set(c, what) for c in clouds]
    sets = []
    for (_, T), src in zip(slots, sources):
        rs = plain[src]
        if T is not None and rs is not None:
            rs = M.warp_set(rs, T)
            rs = rs if rs.n else None
        sets.append(rs)
    return sets, sources


def _encode_multi(cs, slots, mode, segment_nodes, timings, search):
    """`encode_geometry` with two or more reference slots [(cloud, RigidTransform or None)]: the 0xAB stream under mode "inter",
    the shorter of it and of the same call with the first entry alone under "auto" (that entry on a tie)."""
    if mode == "intra" or cs.n == 0:
        return _encode(cs, INTRA, segment_nodes, timings)
    sets, sources = _slot_sets(slots, "encode_geometry")
    head = bytearray([MAGIC_MULTI, len(slots)])
    for (_, T), src in zip(slots, sources):
        head += bytes([src, 0 if T is None else 1]) + (b"" if T is None else T.pack())
    if search == "auto":
        multi = _encode(cs, sets, segment_nodes, timings)
        tw = {} if timings is not None else None
        widest = _encode(cs, sets, segment_nodes, tw, WIDE_SEARCH[1])
        if len(widest) < len(multi):
            multi = widest
            if timings is not None:
                timings.clear()
                timings.update(tw)
    else:
        multi = _encode(cs, sets, segment_nodes, timings, search)
    multi = bytes(head) + multi
    if mode == "inter":
        return multi
    cloud, T = slots[0]
    single = encode_geometry(cs, segment_nodes, None, cloud, mode, T, search)
    if timings is not None:
        timings["multi_bytes"], timings["single_bytes"] = len(multi), len(single)
    return multi if len(multi) < len(single) else single


def multi_prediction(cs, sets, origin, depth, level_sets_=None, search=SEARCH, counts=False):
    """(blocks set, block_log2 of this cloud, int32 slot per block, int32 packed displacement per block, the predicted pyramids,
    int32 match counts [blocks, slots] or None) of the canonical set `cs` against the reference sets `sets` (None: an empty slot):
    every slot searched by `pcc_geom_wide_motion` -- for search <= 2 the vector `pcc_geom_inter_motion` picks --, the slot chosen
    per block by `pcc_geom_multi_block_bits`."""
    lib = L.load()
    dev = cs.device
    lv = level_sets(cs, origin, depth) if level_sets_ is None else level_sets_
    first = max(0, depth - BLOCK_LOG2)
    bl = depth - first
    blocks, voxels = lv[first], lv[depth]
    nb, k = blocks.n, len(sets)
    pw = lib.pcc_geom_inter_pyramid_words()
    cur = torch.empty(nb * pw, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("pcc_geom_inter_block_bits", L.ptr(blocks.keys), nb, bl, L.ptr(voxels.keys), voxels.n,
           *S.grid_args(voxels.grid() if S.USE_GRID else None), 0, 0, 0, None, SEARCH, L.ptr(cur), L.ptr(bad), L.stream())
    vecs = torch.empty((k, nb), dtype=torch.int32, device=dev)
    for s, rs in enumerate(sets):
        L.call("pcc_geom_wide_motion", L.ptr(blocks.keys), nb, bl, L.ptr(cur), *ref_args(rs), *origin, search, None,
               vecs.data_ptr() + 4 * s * nb, L.stream())
    sel = torch.empty(nb, dtype=torch.int32, device=dev)
    disp = torch.empty(nb, dtype=torch.int32, device=dev)
    pred = torch.empty(nb * pw, dtype=torch.int64, device=dev)
    cnt = torch.empty((nb, k), dtype=torch.int32, device=dev) if counts else None
    multi_block_bits(blocks.keys, nb, bl, sets, origin, vecs, search, cur, sel, disp, pred, cnt, L.ptr(bad))
    return blocks, bl, sel, disp, pred, cnt


def multi_block_bits(bkeys, nb, bl, sets, origin, vecs, search, cur, sel, disp, pred, counts, bad_ptr):
    """One launch of `pcc_geom_multi_block_bits` over the reference sets `sets` (None: an empty slot); cur None: the decoder form."""
    k = len(sets)
    args = [ref_args(rs) for rs in sets]
    hs = [a[4] for a in args]                                         # (the host headers stay alive until the call returns)
    L.call("pcc_geom_multi_block_bits", L.ptr(bkeys), nb, bl, k,
           (C.c_void_p * k)(*[a[0] for a in args]), (C.c_int64 * k)(*[a[1] for a in args]), (C.c_void_p * k)(*[a[2] for a in args]),
           (C.c_void_p * k)(*[a[3] for a in args]), (C.c_void_p * k)(*[None if h is None else C.addressof(h) for h in hs]),
           *origin, L.ptr(vecs), search, L.ptr(cur), L.ptr(sel), L.ptr(disp), L.ptr(pred), L.ptr(counts), bad_ptr, L.stream())


_DISP_LUT = {}


def _disp_luts(dev):
    """(int32 [4096] packed displacement -> index into candidates(SEARCH), int32 [256] index -> packed displacement) on `dev`.
    An index the table does not hold maps to a word no range accepts, which `pcc_geom_multi_block_bits` flags."""
    key = str(dev)
    if key not in _DISP_LUT:
        packed = [(dx + 8) | ((dy + 8) << 4) | ((dz + 8) << 8) for dx, dy, dz in candidates(SEARCH)]
        to_index = np.zeros(4096, dtype=np.int32)
        to_index[packed] = np.arange(len(packed), dtype=np.int32)
        to_disp = np.full(256, 1 << 12, dtype=np.int32)
        to_disp[:len(packed)] = packed
        _DISP_LUT[key] = (torch.from_numpy(to_index).to(dev), torch.from_numpy(to_disp).to(dev))
    return _DISP_LUT[key]


def check_search(search, what):
    """The search range an encoder was asked for: SEARCH for None, an int in 2 .. 7, or "auto" (shared with attributes.py)."""
    if search is None:
        return SEARCH
    if isinstance(search, str) and search == "auto":
        return search
    if isinstance(search, bool) or not isinstance(search, int) or not SEARCH <= search <= WIDE_SEARCH[1]:
        raise L.PccError(f"{what}: search {search!r} is not None, \"auto\" or an int in {SEARCH} .. {WIDE_SEARCH[1]} (ranges 0 and 1 are read "
                         "but never written)")
    return search


def _multi_inner(data):
    """The byte an 0xAB stream's inner stream begins at (0 for any other stream); nothing is validated here."""
    if len(data) < 2 or data[0] != MAGIC_MULTI:
        return 0
    at = 2
    for _ in range(data[1]):
        at += 2 + (M.PACKED.size if at + 1 < len(data) and data[at + 1] == 1 else 0)
    return at


def stream_search(data):
    """The search range a geometry stream ended with: its header's byte for an inter stream (0xA8 / 0xAA, also behind a global-motion
    wrapper or the slot table of 0xAB), SEARCH for an intra one -- the range a colour coder that follows the geometry uses."""
    at = GLOBAL_HEADER if len(data) >= 1 and data[0] == MAGIC_GLOBAL else _multi_inner(data)
    if len(data) >= at + HEADER_INTER.size and data[at] in (MAGIC_INTER, MAGIC_WIDE):
        return data[at + HEADER_INTER.size - 1]
    return SEARCH


def _encode_against(cs, rs, mode, segment_nodes, timings, search=SEARCH):
    """The stream of the canonical non-empty set `cs` against the reference set `rs` (None: empty) under mode "inter" / "auto"
    with the search range `search` (an int, or "auto": the shorter of SEARCH and the widest range, SEARCH on a tie)."""
    if search == "auto":
        inter = _encode(cs, rs, segment_nodes, timings)
        tw = {} if timings is not None else None
        widest = _encode(cs, rs, segment_nodes, tw, WIDE_SEARCH[1])
        if len(widest) < len(inter):
            inter = widest
            if timings is not None:                    # the events of the stream that is kept
                timings.clear()
                timings.update(tw)
    else:
        inter = _encode(cs, rs, segment_nodes, timings, search)
    if mode == "inter":
        return inter
    intra = _encode(cs, INTRA, segment_nodes, None)
    if timings is not None:
        timings["inter_bytes"], timings["intra_bytes"] = len(inter), len(intra)
    return inter if len(inter) < len(intra) else intra


def ref_args(rs):
    """Kernel arguments (keys, n, bits, rank, h) of a reference set; None: the empty reference."""
    if rs is None:
        return None, 0, None, None, None
    return (L.ptr(rs.keys), rs.n, *S.grid_args(rs.grid() if S.USE_GRID else None))


class Phases:
    """Device time between consecutive marks, under the later mark's name (a mark without a name only starts a span); inert
    when the caller asked for no timings.  Two series run side by side and do not cut each other's spans: the marks that carry
    a level (a level number -- an intra stream's rows, tools/geometry_timing.py -- or any other key) and the marks that carry
    none (the phases of a whole call, tools/geometry_inter_timing.py)."""

    def __init__(self, on):
        self.marks = [] if on else None

    def mark(self, name=None, level=None):
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, level, ev))

    def report(self, level=None):
        """name -> ms of the series `level` belongs to, summed over the marks of `level`."""
        series = [m for m in self.marks if (m[1] is None) == (level is None)]
        out = {}
        for (_, _, a), (name, at, b) in zip(series[:-1], series[1:]):
            if name is not None and at == level:
                out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


def motion_vectors(cs, rs, origin, depth, sets=None, counts=False, search=SEARCH):
    """(blocks set, block_log2 of this cloud, current pyramid, int32 vector index per block[, int32 match counts [blocks, K]]) of
    the canonical set `cs` against the reference `rs`: `pcc_geom_inter_block_bits` on the frame itself, `pcc_geom_inter_motion`.
    search above 2: `pcc_geom_wide_motion`, which gives packed displacements (dx + 8) | (dy + 8) << 4 | (dz + 8) << 8 in place of
    indices and the counts in lexicographic (dx, dy, dz) order."""
    lib = L.load()
    dev = cs.device
    sets = level_sets(cs, origin, depth) if sets is None else sets
    first = max(0, depth - BLOCK_LOG2)
    bl = depth - first
    blocks, voxels = sets[first], sets[depth]
    pw = lib.pcc_geom_inter_pyramid_words()
    cur = torch.empty(blocks.n * pw, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    vec = torch.empty(blocks.n, dtype=torch.int32, device=dev)
    cnt = torch.empty((blocks.n, (2 * search + 1) ** 3), dtype=torch.int32, device=dev) if counts else None
    L.call("pcc_geom_inter_block_bits", L.ptr(blocks.keys), blocks.n, bl, L.ptr(voxels.keys), voxels.n,
           *S.grid_args(voxels.grid() if S.USE_GRID else None), 0, 0, 0, None, SEARCH, L.ptr(cur), L.ptr(bad), L.stream())
    L.call("pcc_geom_wide_motion" if search > MAX_SEARCH else "pcc_geom_inter_motion", L.ptr(blocks.keys), blocks.n, bl, L.ptr(cur),
           *ref_args(rs), *origin, search, L.ptr(cnt), L.ptr(vec), L.stream())
    return (blocks, bl, cur, vec, cnt) if counts else (blocks, bl, cur, vec)


INTRA = object()          # `_encode(cs, INTRA, ...)`: no reference at all (None is the empty reference of an inter stream)


def _encode(cs, rs, segment_nodes, timings, search=SEARCH):
    """The stream of the canonical set `cs`: intra (0xA7) when `rs` is INTRA, else inter (0xA8; 0xAA when `search` is above 2)
    against the reference set `rs` (None: empty).  A LIST of reference sets: the inner stream of 0xAB, every block predicted from
    the set `pcc_geom_multi_block_bits` chose for it, the selector list in front of the vector list.  One walk over the levels: those above `first` (= depth for an intra stream) take the intra kernels, the
    others the inter ones.  Device->host reads: bounds, level sizes, every level's histograms, the raw levels' bytes (an inter
    stream's vectors ride in that read), the payload."""
    n = cs.n
    if n == 0:
        return HEADER.pack(MAGIC, 0, 0, 0, 0, 0)
    inter = rs is not INTRA
    multi = isinstance(rs, list)                                         # the inner stream of 0xAB: one reference set per slot
    origin = tuple(cs.bounds.lo)
    depth = max(1, max(cs.bounds.hi[i] - origin[i] for i in range(3)).bit_length())
    first = max(0, depth - BLOCK_LOG2) if inter else depth
    rows = N_ROWS if inter else N_CTX
    wide = inter and search > MAX_SEARCH
    k_vec = (2 * search + 1) if wide else (2 * SEARCH + 1) ** 3          # the alphabet of a vector symbol: a component, or an index
    per = 3 if wide else 1                                               # symbols per block in the vector list
    dev = cs.device
    lib = L.load()
    ph = Phases(timings is not None)
    with torch.cuda.device(dev):
        ph.mark()
        sets = level_sets(cs, origin, depth)
        ph.mark("level_sets_ms")
        nodes = [s.n for s in sets[:depth]]
        at = np.concatenate([[0], np.cumsum(nodes)]).tolist()
        sym = torch.empty(at[-1], dtype=torch.int32, device=dev)        # what the rANS coder sees
        idx = torch.empty(at[-1], dtype=torch.int32, device=dev)        # its table row: context (+ 64 * present in an inter level)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        words = [lib.pcc_geom_hist_words()] * first
        nb = 0
        if inter:
            if multi:                                                   # per slot a search, per block the best slot and its pyramid
                blocks, bl, sel, vec, pred, _ = multi_prediction(cs, rs, origin, depth, sets, search)
                ph.mark("motion_search_ms")
                nb = blocks.n
                if not wide:                                            # what an 0xA8 vector list codes: indices
                    vec = _disp_luts(dev)[0][vec.long()]
            else:
                blocks, bl, _, vec = motion_vectors(cs, rs, origin, depth, sets, search=search)
                ph.mark("motion_search_ms")
                nb = blocks.n
                pred = torch.empty(nb * lib.pcc_geom_inter_pyramid_words(), dtype=torch.int64, device=dev)
                L.call("pcc_geom_wide_block_bits" if wide else "pcc_geom_inter_block_bits", L.ptr(blocks.keys), nb, bl, *ref_args(rs), *origin,
                       L.ptr(vec), search, L.ptr(pred), L.ptr(bad), L.stream())
            bgrid = blocks.grid() if (first and S.USE_GRID) else None
            if wide:                                                    # what the vector list codes: [blocks, 3] components
                disp, vec = vec, torch.empty(3 * nb, dtype=torch.int32, device=dev)
                L.call("pcc_geom_wide_unpack", L.ptr(disp), nb, search, L.ptr(vec), L.stream())
            ph.mark("compensation_ms")
            byte = torch.empty(at[-1], dtype=torch.int32, device=dev)   # the occupancy bytes of the inter levels (raw levels travel as these)
            words += [lib.pcc_geom_inter_hist_words()] * (depth - first)
        h_at = [0, *itertools.accumulate(words)]
        hist = torch.zeros(h_at[-1], dtype=torch.int32, device=dev)
        for l in range(depth):
            node, child = sets[l], sets[l + 1]
            sp, ip, hp = sym.data_ptr() + 4 * at[l], idx.data_ptr() + 4 * at[l], hist.data_ptr() + 4 * h_at[l]
            ph.mark(None, l)                                               # (a set without a grid index builds it in `grid()`: the level's time)
            ngrid = S.grid_args(node.grid() if (l and S.USE_GRID) else None)
            cgrid = S.grid_args(child.grid() if S.USE_GRID else None)
            if l < first:
                L.call("pcc_geom_occ_ctx", L.ptr(node.keys), node.n, node.ts, *ngrid, L.ptr(child.keys), child.n, *cgrid, sp, ip, L.stream())
                ph.mark("occ_ctx_ms", l)
                L.call("pcc_geom_hist", sp, ip, node.n, hp, L.ptr(bad), L.stream())
            else:
                L.call("pcc_geom_inter_occ_ctx", L.ptr(node.keys), node.n, node.ts, *ngrid, L.ptr(child.keys), child.n, *cgrid,
                       L.ptr(blocks.keys), nb, *S.grid_args(bgrid), bl, L.ptr(pred), byte.data_ptr() + 4 * at[l], sp, None, ip, L.stream())
                L.call("pcc_geom_inter_hist", sp, ip, node.n, hp, L.ptr(bad), L.stream())
            ph.mark("hist_ms", l)
        ph.mark("symbols_hist_ms")
        h_hist = hist.cpu().numpy().astype(np.int64)                       # one read: every level's histograms
        raw_lv = [l for l in range(depth) if nodes[l] < RAW_NODES]
        parts = [(sym if l < first else byte)[at[l]:at[l + 1]] for l in raw_lv] + ([vec] if inter else []) + ([sel] if multi else [])
        raw_bytes, h_vec, h_sel = {}, None, None
        if parts:
            got = torch.cat(parts).to(torch.uint8).cpu().numpy()           # one read: the raw levels' bytes and the vectors
            p = 0
            for l in raw_lv:
                raw_bytes[l] = got[p:p + nodes[l]].tobytes()
                p += nodes[l]
            h_vec = got[p:p + per * nb]
            h_sel = got[p + per * nb:p + per * nb + nb] if multi else None
        # containers: the vector list (when it is coded) and the coded levels, tables from the levels before, one rANS launch each
        # into a shared blob [sizes | containers]
        code_vec = inter and k_vec > 1 and nb >= RAW_NODES
        symbols = {l: nodes[l] for l in range(depth) if nodes[l] >= RAW_NODES}
        if code_vec:
            symbols = {"vec": per * nb, **symbols}
        code_sel = multi and nb >= RAW_NODES
        if code_sel:
            symbols = {"sel": nb, **symbols}
        jobs = list(symbols)
        plans = {j: R.Plan(symbols[j], 1, 1, segments_for(symbols[j], segment_nodes)) for j in jobs}
        caps = {j: R.align8(plans[j].capacity) for j in jobs}
        head = 8 * max(len(jobs), 1)
        blob = torch.zeros(head + sum(caps.values()), dtype=torch.uint8, device=dev)
        begin, keep, where = head, [], {}

        def run(job, tabs, sp, ip):
            nonlocal begin
            keep.append(tabs)
            ph.mark(None, job)
            R.encode(tabs, plans[job], sp, ip, blob.data_ptr() + begin, blob.data_ptr() + 8 * jobs.index(job))
            ph.mark("rans_ms", job)
            where[job] = (begin, caps[job])
            begin += caps[job]

        if code_sel:
            s_hist = np.bincount(h_sel, minlength=len(rs))
            s_idx = torch.zeros(nb, dtype=torch.int32, device=dev)
            keep.append(s_idx)
            run("sel", R.fresh_cdf_tables(f"geometry_selectors{len(rs)}", dev, vector_table(s_hist), np.full(1, len(rs) + 2, dtype=np.int32),
                                          np.zeros(1, dtype=np.int32)), L.ptr(sel), L.ptr(s_idx))
        if code_vec:
            v_hist = [np.bincount(h_vec[c::per], minlength=k_vec) for c in range(per)]
            v_idx = torch.arange(per * nb, dtype=torch.int32, device=dev) % per        # table row = component (one row: an index)
            keep.append(v_idx)
            run("vec", R.fresh_cdf_tables(f"geometry_vectors{per}x{k_vec}", dev, np.concatenate([vector_table(h) for h in v_hist]),
                                          np.full(per, k_vec + 2, dtype=np.int32), np.zeros(per, dtype=np.int32)), L.ptr(vec), L.ptr(v_idx))
        # backward-adaptive (row, byte) counts: after every level (raw ones included) the old counts are halved and the level's are added
        state = np.zeros((rows, 256), dtype=np.int64)
        side = {}
        for l in range(depth):
            h = h_hist[h_at[l]:h_at[l + 1]]
            r = N_CTX if l < first else N_ROWS
            if l in plans:
                side[l] = [int(v) for v in h[r * 256:]]                      # popcount classes (8), then an inter level's distance classes (9)
                if l < first:
                    tabs = R.fresh_cdf_tables("geometry", dev, derive_tables(state[:N_CTX], side[l]), TABLE_SIZES, TABLE_OFFSETS)
                else:
                    tabs = R.fresh_cdf_tables("geometry_inter", dev, derive_tables_inter(state, side[l][:8], side[l][8:]), INTER_SIZES, INTER_OFFSETS)
                run(l, tabs, sym.data_ptr() + 4 * at[l], idx.data_ptr() + 4 * at[l])
            state >>= 1
            state[:r] += h[:r * 256].reshape(r, 256)
        ph.mark("tables_rans_ms")
        host = blob.cpu().numpy()                                          # one read: sizes + containers
        sizes = host[:head].view(np.int64)
        ph.mark("payload_read_ms")

    def container(job):
        b0, cap = where[job]
        got = int(sizes[jobs.index(job)])
        if not 0 < got <= cap:
            raise L.PccError(f"encode_geometry: {'container' if inter else 'level'} {job} produced {got} bytes for a capacity of {cap}")
        return host[b0:b0 + got].tobytes()

    out = bytearray(HEADER_INTER.pack(MAGIC_WIDE if wide else MAGIC_INTER, n, depth, *origin, BLOCK_LOG2, search) if inter
                    else HEADER.pack(MAGIC, n, depth, *origin))
    for l in range(depth):
        if l == first and code_sel:
            body = container("sel")
            occ = np.flatnonzero(s_hist)
            out += struct.pack("<B", len(occ)) + b"".join(struct.pack("<BI", int(i), int(s_hist[i])) for i in occ)
            out += struct.pack("<I", len(body)) + body
        elif l == first and multi:
            out += h_sel.tobytes()
        if l == first and k_vec > 1:
            if code_vec:
                body = container("vec")
                for h in v_hist:
                    occ = np.flatnonzero(h)
                    out += struct.pack("<B", len(occ)) + b"".join(struct.pack("<BI", int(i), int(h[i])) for i in occ)
                out += struct.pack("<I", len(body)) + body
            else:
                out += h_vec.tobytes()
        if l in raw_bytes:
            out += raw_bytes[l]
            continue
        body = container(l)
        if l < first:
            out += SIDE.pack(*side[l], len(body))
        else:
            # (the distance classes do not give the child total, so it travels: the next level's node count)
            out += SIDE_INTER.pack(*side[l], nodes[l + 1] if l + 1 < depth else n, len(body))
        out += body
    if timings is not None:
        torch.cuda.synchronize(dev)
        if inter:
            timings.update(inter=ph.report(), blocks=nb, zero_vectors=int((h_vec.reshape(nb, per) == (search if wide else 0)).all(axis=1).sum()))
        else:
            timings["levels"] = [{"level": l, "nodes": nodes[l], **ph.report(l)} for l in range(depth)]
        # by construction, not counted: the input's bounds, the stride chain's sizes, the histograms | the raw levels' bytes + the
        # vectors | the payload (tensor rows that are not yet canonical add the canonicalisation's count)
        timings["host_reads_by_construction"] = 3 + (1 if parts else 0) + 1
    return bytes(out)


def _canonical_children(keys, n, pitch, depth_level, dev, counts_ptr):
    """Canonical order of a level's child keys (inside the level's 2^l cube by construction): through the occupancy bitmap of
    that cube while it is small enough, else by radix sort (the level then has no grid index and the context kernel searches).
    The bitmap path leaves (distinct keys, off-lattice flag) at counts_ptr (device int64 [2]) for the deferred check; rows past
    the distinct count keep the cube's corner cell, so a level decoded from a damaged stream still holds in-lattice keys only."""
    lib = L.load()
    side = 1 << depth_level
    lat = S.Lattice((0, 0, 0), (side, side, side), pitch, 1)
    if S.USE_GRID and lat.fits(S.GRID_MAX_BYTES // 4):
        bits, rank, ws = lat.alloc(dev)
        out = torch.full((n,), _key_of(0, 0, 0), dtype=torch.int64, device=dev)
        first = torch.empty(n, dtype=torch.int32, device=dev)
        L.call("pcc_keys_canonicalize_grid", L.ptr(keys), n, lat.h, L.ptr(bits), L.ptr(rank), L.ptr(out), L.ptr(first), counts_ptr,
               L.ptr(ws), ws.numel(), L.stream())
        return out, S.GridIndex(bits, rank, lat.h)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    mask = 0
    for sh in (32, 16, 0):
        mask |= S._field_mask(0, (side - 1) * pitch) << sh
    ws = L.workspace(lib.pcc_sort_ws_bytes(n), dev)
    L.call("pcc_sort_keys", L.ptr(keys), n, mask, L.ptr(out), None, L.ptr(ws), ws.numel(), L.stream())
    return out, None


def _payloads(data, levels, vectors=None, blocks=0, selectors=None):
    """Host buffers for ONE upload each: the coded levels' rANS containers (`rans.stage`) and the raw levels' bytes as int32
    symbols.  An inter stream's vector list rides as the job "vec": its container when it is coded, else one index per block
    behind the raw levels' bytes (zeros when the stream carries none); an 0xAB stream's selector list likewise as "sel"."""
    jobs = [l for l, lv in enumerate(levels) if not lv["raw"]]
    spans = [levels[l]["payload"] for l in jobs]
    raw_at, raw = {}, []
    for l, lv in enumerate(levels):
        if lv["raw"]:
            raw_at[l] = len(raw)
            raw.extend(data[lv["payload"][0]:lv["payload"][1]])
    if vectors is not None and vectors["raw"]:
        b0, b1 = vectors["payload"]
        raw_at["vec"] = len(raw)
        raw.extend(data[b0:b1] if b1 > b0 else [0] * blocks)               # (one index, or three components, per block)
    elif vectors is not None:
        jobs, spans = jobs + ["vec"], spans + [vectors["payload"]]
    if selectors is not None and selectors["raw"]:                         # (an 0xAB stream's selector list rides the same way: "sel")
        raw_at["sel"] = len(raw)
        raw.extend(data[selectors["payload"][0]:selectors["payload"][1]])
    elif selectors is not None:
        jobs, spans = jobs + ["sel"], spans + [selectors["payload"]]
    buf, offsets = R.stage(data, spans)
    return buf, dict(zip(jobs, offsets)), np.asarray(raw, dtype=np.int32), raw_at          # (level 0 is one node: always raw)


def _decode(hdr, data, dev, rs, as_set, timings):
    """The level walk of `decode_geometry` for a non-empty cloud; `rs` is the reference set of an inter stream (None: empty).
    Levels above `first` (= depth for an intra stream) decode against the contexts alone.  In an inter stream, once the
    blocks (level `first`) are known the vectors are decoded (or uploaded), the predicted pyramids are built from the
    reference, and every level from there on draws `present` and the prediction byte from them.  Sizes come from the header
    alone (the pyramids from the block level's node count), so there is ONE device->host read, at the end; it also carries
    the vector list's rANS status and range check and both class histograms of every inter level.  A wrong reference or a
    damaged payload can only give wrong keys inside the cube until that read."""
    n, depth, origin, levels = hdr["n"], hdr["depth"], hdr["origin"], hdr["levels"]
    inter = bool(hdr.get("inter"))
    first = hdr["first"] if inter else depth
    lib = L.load()
    words = [lib.pcc_geom_hist_words()] * first
    ph = Phases(timings is not None)
    with torch.cuda.device(dev):
        ph.mark()
        vh, nb = (hdr["vectors"], levels[first]["nodes"]) if inter else (None, 0)
        sh = hdr.get("selectors")                                          # an 0xAB stream: `rs` is the list of its slots' reference sets
        multi = sh is not None
        h_buf, where, h_raw, raw_at = _payloads(data, levels, vh, nb, sh)
        d_buf, d_raw = torch.from_numpy(h_buf).to(dev), torch.from_numpy(h_raw).to(dev)
        const = R.fixed_tables("geometry", dev, None, TABLE_SIZES, TABLE_OFFSETS)
        # the level's cdf and decoder blob are derived on the device (`pcc_geom_tables`), in place, before each coded level
        tabs = R.Tables(torch.empty((N_CTX, N_SYM + 2), dtype=torch.int32, device=dev), const.sizes, const.offsets,
                        dec=torch.zeros(lib.pcc_geom_dec_table_bytes(), dtype=torch.uint8, device=dev))
        if inter:
            search, bl = hdr["search"], depth - first
            wide = search > MAX_SEARCH
            k_vec = (2 * search + 1) if wide else (2 * search + 1) ** 3
            per = 3 if wide else 1
            words += [lib.pcc_geom_inter_hist_words()] * (depth - first)
            consti = R.fixed_tables("geometry_inter", dev, None, INTER_SIZES, INTER_OFFSETS)
            tabsi = R.Tables(torch.empty((N_ROWS, INTER_STRIDE), dtype=torch.int32, device=dev), consti.sizes, consti.offsets,
                             dec=torch.zeros(lib.pcc_geom_inter_dec_table_bytes(), dtype=torch.uint8, device=dev))
            bkeys = bgrid = pred = None
        state = torch.zeros((N_ROWS if inter else N_CTX) * 256, dtype=torch.int64, device=dev)
        h_at = [0, *itertools.accumulate(words)]
        hist = torch.zeros(h_at[-1], dtype=torch.int32, device=dev)
        # per level: status | bad byte | child total (i64) | distinct, off-lattice (i64 x 2); an inter stream's row `depth`: the
        # vector list's status | bad index; an 0xAB stream's row `depth + 1`: the selector list's status | selector or vector out of range
        flags = torch.zeros((depth + inter + multi, 8), dtype=torch.int32, device=dev)
        keys = torch.tensor([_key_of(0, 0, 0)], dtype=torch.int64, device=dev)
        grid, by_grid = None, []
        for l, lv in enumerate(levels):
            m, pitch, total = lv["nodes"], 1 << (depth - l), lv["children"]
            fp, hp = flags.data_ptr() + 32 * l, hist.data_ptr() + 4 * h_at[l]
            nbytes = lv["payload"][1] - lv["payload"][0]
            ph.mark(None, l)
            if l == first:
                vp = flags.data_ptr() + 32 * depth
                if vh["raw"]:
                    vec = d_raw[raw_at["vec"]:raw_at["vec"] + per * nb]
                else:
                    v_hists = vh["hist"] if wide else [vh["hist"]]
                    v_cdf, v_sizes = np.concatenate([vector_table(h) for h in v_hists]), np.full(per, k_vec + 2, dtype=np.int32)
                    v_const = R.fixed_tables(f"geometry_vectors{per}x{k_vec}", dev, None, v_sizes, np.zeros(per, dtype=np.int32))
                    vt = R.Tables(torch.from_numpy(v_cdf).to(dev), v_const.sizes, v_const.offsets,     # (the header's histograms: host work)
                                  dec=torch.from_numpy(R._dec_blob(v_cdf, v_sizes)).to(dev))
                    vec = torch.empty(per * nb, dtype=torch.int32, device=dev)
                    R.decode(vt, d_buf.data_ptr() + where["vec"], vh["payload"][1] - vh["payload"][0],
                             torch.arange(per * nb, dtype=torch.int32, device=dev) % per, per * nb, 1, 1, vh["streams"], vec, vp)
                if wide:                                                # components -> displacements; one above 2 * search sets the flag
                    comps, vec = vec.contiguous(), torch.empty(nb, dtype=torch.int32, device=dev)
                    L.call("pcc_geom_wide_pack", L.ptr(comps), nb, search, L.ptr(vec), vp + 4, L.stream())
                bkeys, bgrid = keys, grid
                pred = torch.empty(nb * lib.pcc_geom_inter_pyramid_words(), dtype=torch.int64, device=dev)
                if multi:
                    mp = flags.data_ptr() + 32 * (depth + 1)
                    if sh["raw"]:
                        sel = d_raw[raw_at["sel"]:raw_at["sel"] + nb].contiguous()
                    else:
                        s_cdf, s_sizes = vector_table(sh["hist"]), np.full(1, len(rs) + 2, dtype=np.int32)
                        s_const = R.fixed_tables(f"geometry_selectors{len(rs)}", dev, None, s_sizes, np.zeros(1, dtype=np.int32))
                        st = R.Tables(torch.from_numpy(s_cdf).to(dev), s_const.sizes, s_const.offsets,
                                      dec=torch.from_numpy(R._dec_blob(s_cdf, s_sizes)).to(dev))
                        sel = torch.empty(nb, dtype=torch.int32, device=dev)
                        R.decode(st, d_buf.data_ptr() + where["sel"], sh["payload"][1] - sh["payload"][0],
                                 torch.zeros(nb, dtype=torch.int32, device=dev), nb, 1, 1, sh["streams"], sel, mp)
                    if not wide:                                        # indices -> displacements; one outside the table: a word the kernel flags
                        vec = _disp_luts(dev)[1][vec.clamp(0, 255).long()]
                    multi_block_bits(bkeys, nb, bl, rs, origin, vec.contiguous(), search, None, sel, None, pred, None, mp + 4)
                else:
                    L.call("pcc_geom_wide_block_bits" if wide else "pcc_geom_inter_block_bits", L.ptr(bkeys), nb, bl, *ref_args(rs), *origin,
                           L.ptr(vec), search, L.ptr(pred), vp + 4, L.stream())
                ph.mark("vectors_compensation_ms")
            if l < first:
                ctx = torch.empty(m, dtype=torch.int32, device=dev)
                L.call("pcc_geom_occ_ctx", L.ptr(keys), m, pitch, *S.grid_args(grid), None, 0, None, None, None, None, L.ptr(ctx), L.stream())
                ph.mark("ctx_ms", l)
                if lv["raw"]:
                    byte = d_raw[raw_at[l]:raw_at[l] + m]
                else:
                    L.call("pcc_geom_tables", L.ptr(state), (C.c_uint32 * 8)(*lv["pop"]), L.ptr(tabs.cdf), L.ptr(tabs.dec), L.stream())
                    byte = torch.empty(m, dtype=torch.int32, device=dev)
                    R.decode(tabs, d_buf.data_ptr() + where[l], nbytes, ctx, m, 1, 1, lv["streams"], byte, fp)
                ph.mark("symbols_ms", l)
                L.call("pcc_geom_hist", L.ptr(byte), L.ptr(ctx), m, hp, fp + 4, L.stream())
                L.call("pcc_geom_state_update", L.ptr(state), hp, L.stream())
            else:
                idx = torch.empty(m, dtype=torch.int32, device=dev)
                r = torch.empty(m, dtype=torch.int32, device=dev)
                L.call("pcc_geom_inter_occ_ctx", L.ptr(keys), m, pitch, *S.grid_args(grid), None, 0, None, None, None, L.ptr(bkeys), nb,
                       *S.grid_args(bgrid), bl, L.ptr(pred), None, None, L.ptr(r), L.ptr(idx), L.stream())
                if lv["raw"]:
                    byte = d_raw[raw_at[l]:raw_at[l] + m]
                    sym = torch.empty(m, dtype=torch.int32, device=dev)
                    L.call("pcc_geom_inter_map", L.ptr(byte), L.ptr(idx), L.ptr(r), m, 0, L.ptr(sym), fp + 4, L.stream())
                else:
                    L.call("pcc_geom_inter_tables", L.ptr(state), (C.c_uint32 * 8)(*lv["pop"]), (C.c_uint32 * 9)(*lv["dist"]), L.ptr(tabsi.cdf),
                           L.ptr(tabsi.dec), L.stream())
                    sym = torch.empty(m, dtype=torch.int32, device=dev)
                    R.decode(tabsi, d_buf.data_ptr() + where[l], nbytes, idx, m, 1, 1, lv["streams"], sym, fp)
                    byte = torch.empty(m, dtype=torch.int32, device=dev)
                    L.call("pcc_geom_inter_map", L.ptr(sym), L.ptr(idx), L.ptr(r), m, 1, L.ptr(byte), fp + 4, L.stream())
                L.call("pcc_geom_inter_hist", L.ptr(sym), L.ptr(idx), m, hp, fp + 4, L.stream())
                L.call("pcc_geom_state_update", L.ptr(state), hp, L.stream())
                L.call("pcc_geom_state_update", state.data_ptr() + 8 * N_CTX * 256, hp + 4 * N_CTX * 256, L.stream())
            ph.mark("symbols_ms")
            off = torch.empty(m + 1, dtype=torch.int32, device=dev)
            ws = L.workspace(lib.pcc_geom_offsets_ws_bytes(m), dev)
            L.call("pcc_geom_child_offsets", L.ptr(byte), m, L.ptr(off), fp + 8, fp + 4, L.ptr(ws), ws.numel(), L.stream())
            ph.mark("hist_scan_ms", l)
            # sized by the header's child count; slots a damaged payload leaves unwritten hold the cube's corner cell
            child = torch.full((total,), _key_of(0, 0, 0), dtype=torch.int64, device=dev)
            L.call("pcc_geom_expand", L.ptr(keys), L.ptr(byte), L.ptr(off), m, pitch >> 1, L.ptr(child), total, L.stream())
            keys, grid = _canonical_children(child, total, pitch >> 1, l + 1, dev, fp + 16)
            by_grid.append(grid is not None)
            ph.mark("expand_canonical_ms", l)
            ph.mark("expand_canonical_ms")
        xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
        akeys = torch.empty(n, dtype=torch.int64, device=dev) if as_set else None
        L.call("pcc_geom_finish", L.ptr(keys), n, origin[0], origin[1], origin[2], L.ptr(akeys), L.ptr(xyz), L.stream())
        # every level's class histograms, the words behind its (row, byte) counts: one strided view per kind of level
        parts = [flags.reshape(-1)]
        if first:
            parts.append(hist[:h_at[first]].view(first, -1)[:, N_CTX * 256:].reshape(-1))
        if first < depth:
            parts.append(hist[h_at[first]:].view(depth - first, -1)[:, N_ROWS * 256:].reshape(-1))
        if as_set:
            parts += [xyz.amin(dim=0), xyz.amax(dim=0)]
        back = torch.cat(parts).cpu().numpy()                                  # the decode's one device->host read
        ph.mark("finish_read_ms")
        p = flags.numel()
        fl = back[:p].reshape(-1, 8)
        if inter and (fl[depth, 0] != 0 or fl[depth, 1] != 0):
            raise L.PccError(f"geometry stream: malformed vector list (status {int(fl[depth, 0])}, index out of range {int(fl[depth, 1])})")
        if multi and (fl[depth + 1, 0] != 0 or fl[depth + 1, 1] != 0):
            raise L.PccError(f"geometry stream: malformed selector list (status {int(fl[depth + 1, 0])}, selector or vector out of range "
                             f"{int(fl[depth + 1, 1])})")
        for l, lv in enumerate(levels):
            width = words[l] - (N_CTX if l < first else N_ROWS) * 256
            got, p = [int(v) for v in back[p:p + width]], p + width
            total, distinct, off_lattice = (int(v) for v in fl[l, 2:8].view(np.int64))
            if fl[l, 0] != 0:
                raise L.PccError(f"geometry stream: malformed rANS container in level {l} (status {int(fl[l, 0])})")
            if fl[l, 1] != 0 or total != lv["children"]:
                raise L.PccError(f"geometry stream: level {l} decodes to {total} children, the header gives {lv['children']}")
            if not lv["raw"] and got != [int(v) for v in lv["pop"]] + [int(v) for v in lv.get("dist", [])]:
                raise L.PccError(f"geometry stream: level {l} does not decode to its {'class histograms' if inter else 'popcount histogram'}")
            if by_grid[l] and (off_lattice or distinct != lv["children"]):
                raise L.PccError(f"geometry stream: level {l} expands to {distinct} distinct cells, the header gives {lv['children']}")
        if timings is not None:
            torch.cuda.synchronize(dev)
            if inter:
                timings["inter"] = ph.report()
            else:
                timings["levels"] = [{"level": l, "nodes": lv["nodes"], "raw": lv["raw"], **ph.report(l)} for l, lv in enumerate(levels)]
            timings["host_reads_by_construction"] = 1
        if not as_set:
            return xyz
        lo_hi = back[p:].reshape(2, 3).tolist()
        return S.CoordSet(akeys, n, 1, S.Bounds(0, lo_hi[0], lo_hi[1]), on_lattice=True)


@torch.no_grad()
def decode_geometry(data, device, as_set=False, reference=None, timings=None):
    """bytes -> int32 [n, 3] rows (x, y, z) in canonical order on `device`; as_set=True: the canonical pitch-1 CoordSet
    instead (no caller re-sorts).  Raises PccError on a malformed stream; never returns anything but exactly the header's n
    rows.  reference: the cloud an inter stream (0xA8, 0xAA) was coded against (same kinds of input as `encode_geometry` takes);
    an intra stream ignores it, an inter stream without one is refused.  A stream with several references (0xAB) takes the list
    `encode_geometry` took (or the clouds its slots name, in that order: entries that are the same object count once, a pair's
    transform is read from the stream); any other stream decodes against the first entry of a list.

    Every buffer and launch is sized by what `parse_header` derived on the host (each level's nodes <= children <= n); the
    tables are derived on the device from the histograms the kernels leave there (`pcc_geom_tables`), so no level waits for
    the host.  What the payload decodes to -- rANS status, bytes outside 1..255, every level's child total and popcount
    histogram, the canonicalisation's row count -- is compared with the header's figures in ONE read at the end; until then
    a damaged payload can only produce wrong keys inside the level's cube, never a write past a buffer."""
    slots_in = reference_slots(reference, "decode_geometry") if isinstance(reference, (list, tuple)) else None
    clouds = slot_sources(slots_in)[0] if slots_in is not None else ([] if reference is None else [reference])
    hdr = parse_header(data, have_reference=reference is not None, clouds=len(clouds))
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.PccError("decode_geometry runs on a GPU (no CPU fallback)")
    transform = hdr.get("transform")
    if transform is not None or "slots" in hdr:
        data = bytes(data[hdr["inner"]:])              # (the payload spans of the dictionary count from here)
    if hdr["n"] == 0:
        empty = torch.empty((0, 3), dtype=torch.int32, device=dev)
        return S.CoordSet(torch.empty(1, dtype=torch.int64, device=dev), 0, 1, S.Bounds(0, (0, 0, 0), (0, 0, 0))) if as_set else empty
    rs = None
    if slots_in is not None:                           # any other stream against a list: its first entry's cloud, as the encoder's "auto"
        reference = slots_in[0][0]
    if "slots" in hdr:
        rs = _slot_sets([(clouds[src], T) for src, T in hdr["slots"]], "decode_geometry")[0]
    elif hdr.get("inter") and transform is None:
        rs = reference_set(reference, "decode_geometry")
    elif hdr.get("inter"):
        # the warp takes the reference rows as they are -- the set of warped cells does not depend on their order -- and
        # its one read (row count and bounds of the warped set) stands where the canonicalisation of the reference stood;
        # every launch of it is sized by the reference's row count
        rs = M.warp_set(reference, transform)
        rs = rs if rs.n else None
    return _decode(hdr, data, dev, rs, as_set, timings)


# ------------------------------------------------------------------------------------------------------------------------
# sequences: frame i against frame i - 1
# ------------------------------------------------------------------------------------------------------------------------
def stream_transform(data):
    """The RigidTransform of a global-motion stream (0xA9), None for any other stream.  PccError when the 49 bytes are cut short
    or an entry is out of range."""
    if len(data) < 1 or data[0] != MAGIC_GLOBAL:
        return None
    if len(data) < GLOBAL_HEADER:
        raise L.PccError("geometry stream truncated inside the global-motion transform")
    return M.RigidTransform.unpack(data[1:GLOBAL_HEADER])


def stream_slots(data):
    """The slots of a stream with several references (0xAB) as [(source, RigidTransform or None)] -- None for a plain slot --,
    None for any other stream.  PccError when the slot table is cut short or malformed."""
    if len(data) < 1 or data[0] != MAGIC_MULTI:
        return None
    if len(data) < 2 or not 2 <= data[1] <= MAX_SLOTS:
        raise L.PccError("geometry stream (0xab): the slot table is cut short or names a slot count outside 2..4")
    at, out = 2, []
    for _ in range(data[1]):
        if at + 2 > len(data) or data[at + 1] > 1 or at + 2 + data[at + 1] * M.PACKED.size > len(data):
            raise L.PccError("geometry stream (0xab): the slot table is cut short or holds a warped byte above 1")
        T = M.RigidTransform.unpack(data[at + 2:at + 2 + M.PACKED.size]) if data[at + 1] else None
        out.append((data[at], T))
        at += 2 + data[at + 1] * M.PACKED.size
    return out


def encode_sequence(frames, intra_period=32, mode="auto", segment_nodes=SEGMENT_NODES, global_motion=None, search=None, references=1):
    """One stream per frame: frame i is coded against frame i - 1, every `intra_period`-th frame (0, intra_period, ...) without a
    reference.  The coder is lossless, so the decoder's previous frame is the encoder's.  mode and global_motion as in
    `encode_geometry` (global_motion applies to the frames that have a reference; `decode_sequence` reads it from the streams);
    search as in `encode_geometry`, for the frames that have a reference.  references=2: a frame whose two predecessors both lie
    inside its intra period is coded against [frame i - 1, frame i - 2] (0xAB where that is shorter under "auto"), and
    global_motion="both" adds frame i - 1 warped by its estimate as a third slot; references=1: today's list byte for byte."""
    if int(intra_period) < 1:
        raise L.PccError(f"encode_sequence: intra_period {intra_period} must be at least 1")
    if references not in (1, 2):
        raise L.PccError(f"encode_sequence: references {references!r} is not 1 or 2")
    out, prev, prev2 = [], None, None
    for i, frame in enumerate(frames):
        cs = _input_set(frame)
        at = i % int(intra_period)
        ref = None if at == 0 else prev
        if references == 2 and at >= 2 and cs.n:
            slots = [prev, prev2]
            if isinstance(global_motion, str) and global_motion == "both" and prev.n:
                T = M.estimate_rigid(cs, prev)
                if T is not None and not T.is_identity():
                    slots.append((prev, T))
            elif global_motion is not None:
                raise L.PccError("encode_sequence: with references=2 global_motion is None or \"both\"")
            out.append(encode_geometry(cs, segment_nodes=segment_nodes, reference=slots, mode=mode, search=search))
        else:
            out.append(encode_geometry(cs, segment_nodes=segment_nodes, reference=ref, mode=mode,
                                       global_motion=global_motion if ref is not None else None, search=search))
        prev, prev2 = cs, prev
    return out


def decode_sequence(streams, device, as_set=False):
    """The frames of `encode_sequence`, in order: int32 [n, 3] tensors, or canonical CoordSets with as_set=True."""
    out, prev, prev2 = [], None, None
    for data in streams:
        held = [prev, prev2] if prev2 is not None else prev          # (the last two frames: what an 0xAB stream's slots name)
        prev, prev2 = decode_geometry(data, device, as_set=True, reference=held), prev
        out.append(prev if as_set else prev.coords()[:, 1:].contiguous())
    return out
