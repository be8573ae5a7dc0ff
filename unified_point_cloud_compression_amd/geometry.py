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
"""
import ctypes as C
import struct

import numpy as np
import torch

from . import lib as L
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


class TableState:
    """Backward-adaptive (context, byte) counts.  After every level (raw ones included) the old counts are halved and the
    level's histogram [64, 256] is added."""

    def __init__(self):
        self.counts = np.zeros((N_CTX, 256), dtype=np.int64)

    def update(self, hist):
        self.counts = (self.counts >> 1) + np.asarray(hist, dtype=np.int64).reshape(N_CTX, 256)


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


def parse_header(data):
    """Walk the stream on the host: {n, depth, origin, levels}; levels[l] = dict(nodes, children, raw, payload=(begin, end),
    pop).  Raises PccError on a bad magic byte, depth or n, on truncated or inconsistent side information and on trailing
    bytes -- before any GPU work."""
    if len(data) < HEADER.size:
        raise L.PccError("geometry stream truncated inside the header")
    magic, n, depth, ox, oy, oz = HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise L.PccError(f"geometry stream: magic byte {magic:#x}, this build reads {MAGIC:#x}")
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
    at, nodes, levels = HEADER.size, 1, []
    for lvl in range(depth):
        if nodes < RAW_NODES:
            if at + nodes > len(data):
                raise L.PccError(f"geometry stream truncated inside raw level {lvl}")
            body = data[at:at + nodes]
            if 0 in body:
                raise L.PccError(f"geometry stream: raw level {lvl} holds an empty node")
            children = sum(int(POPCOUNT[b]) for b in body)
            lv = {"nodes": nodes, "children": children, "raw": True, "payload": (at, at + nodes), "pop": None}
            at += nodes
        else:
            if at + SIDE.size > len(data):
                raise L.PccError(f"geometry stream truncated inside the side information of level {lvl}")
            *pop, nbytes = SIDE.unpack_from(data, at)
            at += SIDE.size
            if sum(pop) != nodes:
                raise L.PccError(f"geometry stream: level {lvl} has {nodes} nodes, its popcount histogram counts {sum(pop)}")
            if nbytes < 8 or nbytes % 4 or at + nbytes > len(data):
                raise L.PccError(f"geometry stream truncated inside the payload of level {lvl}")
            streams = int.from_bytes(data[at:at + 4], "little")
            if not 1 <= streams <= min(nodes, 65536) or nbytes < 4 * (1 + streams):
                raise L.PccError(f"geometry stream: level {lvl} claims {streams} rANS streams for {nodes} nodes")
            children = sum((k + 1) * v for k, v in enumerate(pop))
            lv = {"nodes": nodes, "children": children, "raw": False, "payload": (at, at + nbytes), "pop": pop, "streams": streams}
            at += nbytes
        # a zero byte is unrepresentable: a level's child total is at least its node count, and never more than n
        if not nodes <= children <= n:
            raise L.PccError(f"geometry stream: level {lvl} expands {nodes} nodes to {children} for {n} points")
        levels.append(lv)
        nodes = children
    if nodes != n:
        raise L.PccError(f"geometry stream: the last level gives {nodes} points, the header says {n}")
    if at != len(data):
        raise L.PccError("geometry stream: trailing bytes")
    return {"n": n, "depth": depth, "origin": (ox, oy, oz), "levels": levels}


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


@torch.no_grad()
def encode_geometry(x, segment_nodes=SEGMENT_NODES, timings=None):
    """[N, >= 3] GPU tensor (any row order, duplicates allowed, floats floored) or pitch-1 CoordSet -> bytes.
    segment_nodes: nodes per rANS stream (tests lower it to cut small levels into several streams; the decoder reads the
    stream count from each container).  timings: a dict that receives per-level device events (tools/geometry_timing.py)."""
    cs = _input_set(x)
    n = cs.n
    origin = tuple(cs.bounds.lo)
    if n == 0:
        return HEADER.pack(MAGIC, 0, 0, 0, 0, 0)
    depth = max(1, max(cs.bounds.hi[i] - origin[i] for i in range(3)).bit_length())
    dev = cs.device
    lib = L.load()
    with torch.cuda.device(dev):
        sets = level_sets(cs, origin, depth)
        hw = lib.pcc_geom_hist_words()
        nodes = [s.n for s in sets[:depth]]
        at = np.concatenate([[0], np.cumsum(nodes)]).tolist()
        sym = torch.empty(at[-1], dtype=torch.int32, device=dev)
        ctx = torch.empty(at[-1], dtype=torch.int32, device=dev)
        hist = torch.zeros((depth, hw), dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        ev = []
        for l in range(depth):
            node, child = sets[l], sets[l + 1]
            if timings is not None:
                ev.append([torch.cuda.Event(enable_timing=True) for _ in range(3)])
                ev[l][0].record()
            L.call("pcc_geom_occ_ctx", L.ptr(node.keys), node.n, node.ts, *S.grid_args(node.grid() if (l and S.USE_GRID) else None),
                   L.ptr(child.keys), child.n, *S.grid_args(child.grid() if S.USE_GRID else None), sym.data_ptr() + 4 * at[l], ctx.data_ptr() + 4 * at[l],
                   L.stream())
            if timings is not None:
                ev[l][1].record()
            L.call("pcc_geom_hist", sym.data_ptr() + 4 * at[l], ctx.data_ptr() + 4 * at[l], node.n, hist[l].data_ptr(), L.ptr(bad),
                   L.stream())
            if timings is not None:
                ev[l][2].record()
        h_hist = hist.cpu().numpy().astype(np.int64)                       # one read: every level's histograms
        raw_lv = [l for l in range(depth) if nodes[l] < RAW_NODES]
        raw_bytes = {}
        if raw_lv:
            got = torch.cat([sym[at[l]:at[l + 1]] for l in raw_lv]).to(torch.uint8).cpu().numpy().tobytes()   # one read
            p = 0
            for l in raw_lv:
                raw_bytes[l] = got[p:p + nodes[l]]
                p += nodes[l]
        # coded levels: tables from the levels before, one rANS launch each into a shared blob [sizes | containers]
        state = TableState()
        coded = [l for l in range(depth) if nodes[l] >= RAW_NODES]
        plans = {l: R.Plan(nodes[l], 1, 1, segments_for(nodes[l], segment_nodes)) for l in coded}
        caps = {l: R.align8(plans[l].capacity) for l in coded}
        head = 8 * max(len(coded), 1)
        blob = torch.zeros(head + sum(caps.values()), dtype=torch.uint8, device=dev)
        begin, keep, where = head, [], {}
        t_code = []
        for l in range(depth):
            if l in plans:
                tabs = R.fresh_cdf_tables("geometry", dev, derive_tables(state.counts, h_hist[l, N_CTX * 256:]), TABLE_SIZES, TABLE_OFFSETS)
                keep.append(tabs)
                if timings is not None:
                    t_code.append((l, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    t_code[-1][1].record()
                R.encode(tabs, plans[l], sym.data_ptr() + 4 * at[l], ctx.data_ptr() + 4 * at[l], blob.data_ptr() + begin,
                         blob.data_ptr() + 8 * coded.index(l))
                if timings is not None:
                    t_code[-1][2].record()
                where[l] = (begin, caps[l])
                begin += caps[l]
            state.update(h_hist[l, :N_CTX * 256])
        host = blob.cpu().numpy()                                          # one read: sizes + containers
        sizes = host[:head].view(np.int64)
    out = bytearray(HEADER.pack(MAGIC, n, depth, *origin))
    for l in range(depth):
        if l in raw_bytes:
            out += raw_bytes[l]
        else:
            b0, cap = where[l]
            nb = int(sizes[coded.index(l)])
            if not 0 < nb <= cap:
                raise L.PccError(f"encode_geometry: level {l} produced {nb} bytes for a capacity of {cap}")
            out += SIDE.pack(*[int(v) for v in h_hist[l, N_CTX * 256:]], nb)
            out += host[b0:b0 + nb].tobytes()
    if timings is not None:
        torch.cuda.synchronize(dev)
        timings["levels"] = [{"level": l, "nodes": nodes[l], "occ_ctx_ms": ev[l][0].elapsed_time(ev[l][1]),
                              "hist_ms": ev[l][1].elapsed_time(ev[l][2])} for l in range(depth)]
        for l, a, b in t_code:
            timings["levels"][l]["rans_ms"] = a.elapsed_time(b)
        # by construction, not counted: the input's bounds, the stride chain's sizes, the histograms, the raw levels' bytes,
        # the payload (tensor rows that are not yet canonical add the canonicalisation's count)
        timings["host_reads_by_construction"] = 3 + (1 if raw_lv else 0) + 1
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


def _payloads(data, levels):
    """Host buffers for ONE upload each: the coded levels' rANS containers (`rans.stage`) and the raw levels' bytes as int32
    symbols."""
    coded = [l for l, lv in enumerate(levels) if not lv["raw"]]
    buf, offsets = R.stage(data, [levels[l]["payload"] for l in coded])
    raw_at, raw = {}, []
    for l, lv in enumerate(levels):
        if lv["raw"]:
            raw_at[l] = len(raw)
            raw.extend(data[lv["payload"][0]:lv["payload"][1]])
    return buf, dict(zip(coded, offsets)), np.asarray(raw if raw else [1], dtype=np.int32), raw_at


@torch.no_grad()
def decode_geometry(data, device, as_set=False, timings=None):
    """bytes -> int32 [n, 3] rows (x, y, z) in canonical order on `device`; as_set=True: the canonical pitch-1 CoordSet
    instead (no caller re-sorts).  Raises PccError on a malformed stream; never returns anything but exactly the header's n
    rows.

    Every buffer and launch is sized by what `parse_header` derived on the host (each level's nodes <= children <= n); the
    tables are derived on the device from the histograms the kernels leave there (`pcc_geom_tables`), so no level waits for
    the host.  What the payload decodes to -- rANS status, bytes outside 1..255, every level's child total and popcount
    histogram, the canonicalisation's row count -- is compared with the header's figures in ONE read at the end; until then
    a damaged payload can only produce wrong keys inside the level's cube, never a write past a buffer."""
    hdr = parse_header(data)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.PccError("decode_geometry runs on a GPU (no CPU fallback)")
    n, depth, origin = hdr["n"], hdr["depth"], hdr["origin"]
    if n == 0:
        empty = torch.empty((0, 3), dtype=torch.int32, device=dev)
        return S.CoordSet(torch.empty(1, dtype=torch.int64, device=dev), 0, 1, S.Bounds(0, (0, 0, 0), (0, 0, 0))) if as_set else empty
    lib = L.load()
    hw = lib.pcc_geom_hist_words()
    levels = hdr["levels"]
    with torch.cuda.device(dev):
        h_buf, where, h_raw, raw_at = _payloads(data, levels)
        d_buf, d_raw = torch.from_numpy(h_buf).to(dev), torch.from_numpy(h_raw).to(dev)
        const = R.fixed_tables("geometry", dev, None, TABLE_SIZES, TABLE_OFFSETS)
        state = torch.zeros(N_CTX * 256, dtype=torch.int64, device=dev)
        hist = torch.zeros((depth, hw), dtype=torch.int32, device=dev)
        flags = torch.zeros((depth, 8), dtype=torch.int32, device=dev)     # status | bad byte | child total (i64) | distinct, off-lattice (i64 x 2)
        # the level's cdf and decoder blob are derived on the device (`pcc_geom_tables`), in place, before each coded level
        tabs = R.Tables(torch.empty((N_CTX, N_SYM + 2), dtype=torch.int32, device=dev), const.sizes, const.offsets,
                        dec=torch.zeros(lib.pcc_geom_dec_table_bytes(), dtype=torch.uint8, device=dev))
        keys = torch.tensor([_key_of(0, 0, 0)], dtype=torch.int64, device=dev)
        grid, by_grid, tl = None, [], []
        for l, lv in enumerate(levels):
            m, pitch, total = lv["nodes"], 1 << (depth - l), lv["children"]
            fp = flags.data_ptr() + 32 * l
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timings is not None else None
            if evs:
                evs[0].record()
            ctx = torch.empty(m, dtype=torch.int32, device=dev)
            L.call("pcc_geom_occ_ctx", L.ptr(keys), m, pitch, *S.grid_args(grid), None, 0, None, None, None, None, L.ptr(ctx), L.stream())
            if evs:
                evs[1].record()
            if lv["raw"]:
                sym = d_raw[raw_at[l]:raw_at[l] + m]
            else:
                nb = lv["payload"][1] - lv["payload"][0]
                L.call("pcc_geom_tables", L.ptr(state), (C.c_uint32 * 8)(*lv["pop"]), L.ptr(tabs.cdf), L.ptr(tabs.dec), L.stream())
                sym = torch.empty(m, dtype=torch.int32, device=dev)
                R.decode(tabs, d_buf.data_ptr() + where[l], nb, ctx, m, 1, 1, lv["streams"], sym, fp)
            if evs:
                evs[2].record()
            L.call("pcc_geom_hist", L.ptr(sym), L.ptr(ctx), m, hist[l].data_ptr(), fp + 4, L.stream())
            L.call("pcc_geom_state_update", L.ptr(state), hist[l].data_ptr(), L.stream())
            off = torch.empty(m + 1, dtype=torch.int32, device=dev)
            ws = L.workspace(lib.pcc_geom_offsets_ws_bytes(m), dev)
            L.call("pcc_geom_child_offsets", L.ptr(sym), m, L.ptr(off), fp + 8, fp + 4, L.ptr(ws), ws.numel(), L.stream())
            if evs:
                evs[3].record()
            # sized by the header's child count; slots a damaged payload leaves unwritten hold the cube's corner cell
            child = torch.full((total,), _key_of(0, 0, 0), dtype=torch.int64, device=dev)
            L.call("pcc_geom_expand", L.ptr(keys), L.ptr(sym), L.ptr(off), m, pitch >> 1, L.ptr(child), total, L.stream())
            keys, grid = _canonical_children(child, total, pitch >> 1, l + 1, dev, fp + 16)
            by_grid.append(grid is not None)
            if evs:
                evs[4].record()
                tl.append((l, m, lv["raw"], evs))
        xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
        akeys = torch.empty(n, dtype=torch.int64, device=dev) if as_set else None
        L.call("pcc_geom_finish", L.ptr(keys), n, origin[0], origin[1], origin[2], L.ptr(akeys), L.ptr(xyz), L.stream())
        parts = [flags.reshape(-1), hist[:, N_CTX * 256:].reshape(-1)]
        if as_set:
            parts += [xyz.amin(dim=0), xyz.amax(dim=0)]
        back = torch.cat(parts).cpu().numpy()                                  # the decode's one device->host read
        fl, pops = back[:8 * depth].reshape(depth, 8), back[8 * depth:16 * depth].reshape(depth, 8)
        for l, lv in enumerate(levels):
            total, distinct, off_lattice = (int(v) for v in fl[l, 2:8].view(np.int64))
            if fl[l, 0] != 0:
                raise L.PccError(f"geometry stream: malformed rANS container in level {l} (status {int(fl[l, 0])})")
            if fl[l, 1] != 0 or total != lv["children"]:
                raise L.PccError(f"geometry stream: level {l} decodes to {total} children, the header gives {lv['children']}")
            if not lv["raw"] and [int(v) for v in pops[l]] != [int(v) for v in lv["pop"]]:
                raise L.PccError(f"geometry stream: level {l} does not decode to its popcount histogram")
            if by_grid[l] and (off_lattice or distinct != lv["children"]):
                raise L.PccError(f"geometry stream: level {l} expands to {distinct} distinct cells, the header gives {lv['children']}")
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["levels"] = [{"level": l, "nodes": m, "raw": raw, "ctx_ms": e[0].elapsed_time(e[1]),
                                  "symbols_ms": e[1].elapsed_time(e[2]), "hist_scan_ms": e[2].elapsed_time(e[3]),
                                  "expand_canonical_ms": e[3].elapsed_time(e[4])} for l, m, raw, e in tl]
            timings["host_reads_by_construction"] = 1
        if not as_set:
            return xyz
        lo_hi = back[16 * depth:].reshape(2, 3).tolist()
        return S.CoordSet(akeys, n, 1, S.Bounds(0, lo_hi[0], lo_hi[1]), on_lattice=True)
