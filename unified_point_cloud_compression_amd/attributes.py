"""Colour (any 8-bit attribute) of one block on the device: `encode_attributes` / `decode_attributes`, a RAHT coder over the
level sets of the octree geometry coder.  With `geometry.encode_geometry` it forms the anchor the
reference draws every RD plot against -- `tmc3 --transformType=0`, octree geometry + RAHT colour (`utils.py:505-529`) -- in
this project's own stream: no G-PCC syntax and no bit-compatibility claim, the stance section 7e takes for geometry.

    stream = u8 0xB3 | u32 n | u8 depth | u8 C | u8 flags (bit 0: colour transform) | u8 qp | i8 chroma_qp_offset
             | C zig-zag LEB128 varints (the quantised root DC) | depth x 6 side bytes | u32 length | rANS container
    (no length and no container when n <= 1)

The geometry is not in the stream: the decoder is handed it and refuses a stream whose n or depth differ from the set's.
Level l of the transform is level l of the octree (`geometry.level_sets`); inside a node three stages of weighted Haar
butterflies merge the children along z, y and x, all in integers (Q8 values, Q30 factors from an exact integer square root),
so the kernels of csrc/pcc_raht.hip and the numpy restatement of the test-suite give the same bits.  A coefficient is
quantised with step(qp) (channel 0) or step(qp + chroma_qp_offset) (the others).  All n - 1 coefficient rows of all levels
form ONE symbol vector, coded by the rANS stream kernels with per symbol the member of a fixed family of 64 two-sided
geometric tables its (level, class, stage) group chose: 6 side bytes per level, no adaptive state, every level decodes in
parallel.  Everything on this side -- the steps, the family, the member choice, the header -- is Python integers or int64.

There is no CPU fallback.  Device->host reads: encode 2 beyond building the level sets (the histograms with the root DC, the
container); decode ONE at the end (the rANS status and the clamp flag; either raises PccError).  `parse_header` rejects a
damaged stream on the host before any GPU work, and every buffer and launch is sized by the geometry set, never by the
payload.

`encode_attributes_lossless` / `decode_attributes_lossless` (second half of this file) are a separate coder
over the same levels, rows, groups, family and container with a reversible arithmetic and their own stream:

    stream = u8 0xB5 | u32 n | u8 depth | u8 C | u8 flags (bit 0: YCoCg-R, bit 1: prediction, bit 2: stored)
             | C zig-zag varints (root values) | depth x 6 side bytes | u32 length | rANS container
    stored:  u8 0xB5 | u32 n | u8 depth | u8 C | u8 4 | n x C raw levels in canonical order
"""
import ctypes as C
import struct

import numpy as np
import torch

from . import geometry as G
from . import lib as L
from . import rans as R
from . import sparse as S

MAGIC = 0xB3               # format version 1
SEGMENT_SYMBOLS = 1024     # symbols per rANS stream: streams = ceil(symbols / SEGMENT_SYMBOLS), 12 bytes of framing each
MAX_STREAMS = 65536
MAX_C = 8
MAX_POINTS = 1 << 26       # a DC value stays below 2^29 and every product below 2^60
LIMIT = 1 << 30            # the decoder's clamp on q * step and on every butterfly output
QP_MIN, QP_MAX = 4, 51
HEADER = struct.Struct("<BIBBBBb")
STEP_TABLE = (256, 287, 323, 362, 406, 456)                 # Q8: 2^(k / 6), k = 0..5
THETA = (55109, 46341, 38968, 32768)                        # Q16: 2^(-k / 4), k = 1..4
N_TABLES, N_SLOTS, ESCAPE, MAX_ABS = 64, 128, 127, 63       # slots 0..126: the values -63..63; slot 127: the escape
TABLE_SIZES = np.full(N_TABLES, N_SLOTS + 1, dtype=np.int32)
TABLE_OFFSETS = np.full(N_TABLES, -MAX_ABS, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------------
# the integer rule, host side
# ------------------------------------------------------------------------------------------------------------------------
def step(qp):
    """Quantiser step in Q8 of a qp clamped to 4..51: doubles every 6, step(4) = 1.0."""
    qp = min(max(int(qp), QP_MIN), QP_MAX)
    return STEP_TABLE[(qp - QP_MIN) % 6] << ((qp - QP_MIN) // 6)


def steps_for(qp, chroma_qp_offset, channels):
    """Per channel: channel 0 takes qp, every other channel qp + chroma_qp_offset."""
    qp = min(max(int(qp), QP_MIN), QP_MAX)
    return [step(qp)] + [step(qp + int(chroma_qp_offset))] * (channels - 1)


def quantise(value, st):
    """sign(value) * ((|value| + step / 2) // step), Python integers."""
    value, st = int(value), int(st)
    q = (abs(value) + (st >> 1)) // st
    return -q if value < 0 else q


def theta(k):
    """Q16 ratio of family member k: 2^(-(40 - k) / 4) below 40, 1 - 2^(-(k - 36) / 4 - 2) from 40 on."""
    if k < 40:
        return THETA[(39 - k) % 4] >> ((39 - k) // 4)
    return 65536 - (THETA[(k - 40) % 4] >> ((k - 40) // 4 + 3))


def member_frequencies(k):
    """The 128 frequencies of member k (sum 65536, all >= 1): W[0] = 2^24, W[m + 1] = W[m] * theta >> 16; a value v weighs
    W[|v|], the escape 2 * sum W[64..4095]; f = 1 + W * (65536 - 128) // sum W and what is left goes to the first largest f."""
    th = theta(k)
    w = [1 << 24]
    for _ in range(4095):
        w.append((w[-1] * th) >> 16)
    slot = [w[abs(v)] for v in range(-MAX_ABS, MAX_ABS + 1)] + [2 * sum(w[MAX_ABS + 1:])]
    total = sum(slot)
    f = [1 + s * (65536 - N_SLOTS) // total for s in slot]
    f[f.index(max(f))] += 65536 - sum(f)
    return f


_FAMILY = None


def table_family():
    """(cdf int32 [64, 129], cost int64 [64, 128]): cost[k][s] = 16 * 256 - floor(256 * log2 f) (bit_length(f^256) - 1 is
    that floor exactly), and 16 * 256 more for the escape slot's bypass digits."""
    global _FAMILY
    if _FAMILY is None:
        cdf = np.zeros((N_TABLES, N_SLOTS + 1), dtype=np.int32)
        cost = np.zeros((N_TABLES, N_SLOTS), dtype=np.int64)
        log = {}
        for k in range(N_TABLES):
            f = member_frequencies(k)
            acc = 0
            for s, v in enumerate(f):
                acc += v
                cdf[k, s + 1] = acc
                if v not in log:
                    log[v] = (v ** 256).bit_length() - 1
                cost[k, s] = 16 * 256 - log[v] + (16 * 256 if s == ESCAPE else 0)
        _FAMILY = (cdf, cost)
    return _FAMILY


def choose_members(hist):
    """Side bytes of the groups from their histograms [groups, 128]: the member of least integer cost sum_s hist[s] * cost_k[s]
    (below 2^43: int64 is exact), ties to the smaller member, 0 for an empty group."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1, N_SLOTS)
    total = hist @ table_family()[1].T
    side = np.argmin(total, axis=1)                   # the first of equal minima
    side[hist.sum(axis=1) == 0] = 0
    return [int(v) for v in side]


def segments_for(symbols, segment_symbols=SEGMENT_SYMBOLS):
    """rANS streams of the symbol vector."""
    return R.segments_for(symbols, segment_symbols, MAX_STREAMS)


def _zigzag(v):
    u = (v << 1) if v >= 0 else ((-v) << 1) - 1
    out = bytearray()
    while True:
        out.append((u & 0x7F) | (0x80 if u > 0x7F else 0))
        u >>= 7
        if not u:
            return bytes(out)


def _container_span(data, at, symbols, name):
    """((begin, end), streams) of the `u32 length | rANS container` at `at`, its lengths checked against the data and each other."""
    if at + 4 > len(data):
        raise L.PccError(f"{name} truncated before the container")
    nbytes = int.from_bytes(data[at:at + 4], "little")
    at += 4
    if nbytes < 8 or nbytes % 4 or at + nbytes > len(data):
        raise L.PccError(f"{name} truncated inside the container")
    streams = int.from_bytes(data[at:at + 4], "little")
    if not 1 <= streams <= min(symbols, MAX_STREAMS) or nbytes < 4 * (1 + streams):
        raise L.PccError(f"{name}: the container claims {streams} rANS streams for {symbols} symbols")
    words = int(np.frombuffer(data, dtype="<u4", count=streams, offset=at + 4).astype(np.int64).sum())
    if 4 * (1 + streams + words) != nbytes:
        raise L.PccError(f"{name}: the container's length disagrees with its stream lengths")
    return (at, at + nbytes), streams


def parse_header(data):
    """{n, depth, channels, colour, qp, chroma_qp_offset, steps, dc (quantised root DC per channel), side (depth * 6 members),
    payload=(begin, end) or None, streams}.  Raises PccError on a bad magic byte, on channels, qp or depth out of range, on a
    root DC or side byte out of range, on truncation, on trailing bytes and on a length that disagrees with the data --
    before any GPU work."""
    if len(data) < HEADER.size:
        raise L.PccError("attribute stream truncated inside the header")
    magic, n, depth, ch, flags, qp, cqo = HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise L.PccError(f"attribute stream: magic byte {magic:#x}, this build reads {MAGIC:#x}")
    if not 1 <= ch <= MAX_C:
        raise L.PccError(f"attribute stream: {ch} channels outside 1..{MAX_C}")
    if flags & ~1 or (flags & 1 and ch != 3):
        raise L.PccError(f"attribute stream: flags {flags:#x} with {ch} channels")
    if not QP_MIN <= qp <= QP_MAX:
        raise L.PccError(f"attribute stream: qp {qp} outside {QP_MIN}..{QP_MAX}")
    if n >= MAX_POINTS:
        raise L.PccError(f"attribute stream: header claims {n} points, the limit is 2^26 - 1")
    if (n == 0 and depth != 0) or (n > 0 and not 1 <= depth <= G.MAX_DEPTH) or n > 8 ** min(depth, 10):
        raise L.PccError(f"attribute stream: header claims {n} points at depth {depth}")
    steps = steps_for(qp, cqo, ch)
    at, dc = HEADER.size, []
    for c in range(ch):
        u, sh = 0, 0
        while True:
            if at >= len(data) or sh > 28:
                raise L.PccError("attribute stream truncated inside the root DC")
            b = data[at]
            at += 1
            u |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        q = (u >> 1) if not u & 1 else -((u + 1) >> 1)
        if abs(q) * steps[c] > LIMIT:
            raise L.PccError(f"attribute stream: root DC {q} of channel {c} is out of range")
        dc.append(q)
    if at + depth * 6 > len(data):
        raise L.PccError("attribute stream truncated inside the side bytes")
    side = list(data[at:at + depth * 6])
    at += depth * 6
    if side and max(side) >= N_TABLES:
        raise L.PccError(f"attribute stream: side byte {max(side)} names no table (64 members)")
    hdr = {"n": n, "depth": depth, "channels": ch, "colour": bool(flags & 1), "qp": qp, "chroma_qp_offset": cqo, "steps": steps,
           "dc": dc, "side": side, "payload": None, "streams": 0}
    if n > 1:
        hdr["payload"], hdr["streams"] = _container_span(data, at, (n - 1) * ch, "attribute stream")
        at = hdr["payload"][1]
    if at != len(data):
        raise L.PccError("attribute stream: trailing bytes")
    return hdr


# ------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------
def _tables(dev):
    """The family on the device, with its encoder entries and decoder blob: one upload per device."""
    return R.fixed_tables("raht", dev, table_family()[0], TABLE_SIZES, TABLE_OFFSETS, enc=True, dec=True)


def _depth_of(cs):
    return max(1, max(cs.bounds.hi[i] - cs.bounds.lo[i] for i in range(3)).bit_length())


def _level_args(node, child):
    """The eight leading arguments of the per-level entry points: the nodes, their children, the children's grid index."""
    return (L.ptr(node.keys), node.n, node.ts, L.ptr(child.keys), child.n, *S.grid_args(child.grid() if S.USE_GRID else None))


def _plan(sets, depth, dev):
    """Per level the child-occupancy bytes and their exclusive scan (a node's first coefficient row), and the scan's checks
    [depth, 4] int32 (child total as int64, bad-byte flag) for the caller's read."""
    lib = L.load()
    masks, offs = [], []
    checks = torch.zeros((depth, 4), dtype=torch.int32, device=dev)
    for l in range(depth):
        node = sets[l]
        mask = torch.empty(node.n, dtype=torch.int32, device=dev)
        off = torch.empty(node.n + 1, dtype=torch.int32, device=dev)
        L.call("pcc_raht_mask", *_level_args(node, sets[l + 1]), L.ptr(mask), L.stream())
        ws = L.workspace(lib.pcc_geom_offsets_ws_bytes(node.n), dev)
        L.call("pcc_geom_child_offsets", L.ptr(mask), node.n, L.ptr(off), checks.data_ptr() + 16 * l, checks.data_ptr() + 16 * l + 8,
               L.ptr(ws), ws.numel(), L.stream())
        masks.append(mask)
        offs.append(off)
    return masks, offs, checks


def _check_plan(checks, sets, what):
    for l, row in enumerate(checks.reshape(-1, 4)):
        if int(row[:2].view(np.int64)[0]) != sets[l + 1].n or row[2] != 0:
            raise L.PccError(f"{what}: level {l} of the geometry does not expand to level {l + 1}")


def _fill_index(masks, offs, sets, depth, channels, side, idx, rows):
    for l in range(depth):
        L.call("pcc_raht_index", L.ptr(masks[l]), L.ptr(offs[l]), sets[l].n, l, channels, L.ptr(side), L.ptr(idx), sets[l].n - 1, rows,
               L.stream())


def _attribute_rows(cloud, attrs, what):
    """(geometry input, uint8 [N, C] levels in the caller's row order); refusals that need no launch come first."""
    if attrs is None:
        if not torch.is_tensor(cloud) or cloud.dim() != 2 or cloud.shape[1] != 6:
            raise L.PccError(f"{what}: an [N, 6] cloud (xyz, rgb in [0, 1]) is required when attrs is not given")
        if not cloud.is_cuda:
            raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
        return cloud, torch.round(cloud[:, 3:6].to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8).contiguous()
    if not torch.is_tensor(attrs) or attrs.dim() != 2 or attrs.dtype != torch.uint8:
        raise L.PccError(f"{what}: attrs must be an [N, C] uint8 tensor")
    if not 1 <= attrs.shape[1] <= MAX_C:
        raise L.PccError(f"{what}: {attrs.shape[1]} channels outside 1..{MAX_C}")
    if not attrs.is_cuda:
        raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
    rows = cloud.n if isinstance(cloud, S.CoordSet) else (cloud.shape[0] if torch.is_tensor(cloud) and cloud.dim() == 2 else -1)
    if rows != attrs.shape[0]:
        raise L.PccError(f"{what}: {attrs.shape[0]} attribute rows for {rows} points")
    return cloud, attrs.contiguous()


@torch.no_grad()
def encode_attributes(cloud, qp, chroma_qp_offset=-2, colour=True, attrs=None, segment_symbols=SEGMENT_SYMBOLS, timings=None):
    """[N, 6] GPU tensor (xyz, then rgb in [0, 1]: colours become round(255 c)), or a pitch-1 CoordSet / [N, >= 3] rows with
    `attrs` uint8 [N, C], 1 <= C <= 8 -> bytes.  Any row order (attributes follow their rows into canonical order; a set's
    attributes are in the set's order).  Duplicate voxels, CPU tensors and batched input raise PccError.  colour: the integer
    BT.709 transform in front of the RAHT (three channels only).  segment_symbols: symbols per rANS stream (tests lower it).
    timings: a dict that receives per-stage device events (tools/anchor_rd.py)."""
    what = "encode_attributes"
    cloud, levels = _attribute_rows(cloud, attrs, what)
    if not -128 <= int(chroma_qp_offset) <= 127:
        raise L.PccError(f"{what}: chroma_qp_offset {chroma_qp_offset} does not fit the header's signed byte")
    qp, cqo = min(max(int(qp), QP_MIN), QP_MAX), int(chroma_qp_offset)
    cs, perm, keep = G.canonical_rows(cloud, what)
    if keep is not None:
        raise L.PccError(f"{what}: {levels.shape[0] - cs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    n, ch = cs.n, levels.shape[1]
    if n >= MAX_POINTS:
        raise L.PccError(f"{what}: {n} points, the limit is 2^26 - 1")
    colour = bool(colour) and ch == 3
    if n == 0:
        return HEADER.pack(MAGIC, 0, 0, ch, int(colour), qp, cqo) + b"\x00" * ch
    dev = cs.device
    if levels.device != dev:
        raise L.PccError(f"{what}: points and attrs are on different devices")
    steps = steps_for(qp, cqo, ch)
    h_steps = (C.c_int32 * ch)(*steps)
    origin, depth = tuple(cs.bounds.lo), _depth_of(cs)
    rows = n - 1
    with torch.cuda.device(dev):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timings is not None else None
        sets = G.level_sets(cs, origin, depth)
        if ev:
            ev[0].record()
        values = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_raht_prepare", L.ptr(levels), L.ptr(perm), n, ch, int(colour), L.ptr(values), L.stream())
        masks, offs, checks = _plan(sets, depth, dev)
        if ev:
            ev[1].record()
        coef = torch.zeros((max(rows, 1), ch), dtype=torch.int32, device=dev)
        w_child, v_child = None, values
        for l in range(depth - 1, -1, -1):
            w = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            v = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_raht_forward", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(w_child), L.ptr(v_child), ch, h_steps,
                   L.ptr(w), L.ptr(v), L.ptr(coef), sets[l].n - 1, rows, L.stream())
            w_child, v_child = w, v
        if ev:
            ev[2].record()
        parts = [v_child.reshape(-1), checks.reshape(-1)]
        if rows:
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            hist = torch.empty(depth * 6 * N_SLOTS, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, None, idx, rows)
            L.call("pcc_raht_hist", L.ptr(coef), L.ptr(idx), rows * ch, depth * 6, L.ptr(hist), L.stream())
            parts.append(hist)
        back = torch.cat(parts).cpu().numpy()                              # one read: root DC, the plan's checks, the histograms
        _check_plan(back[ch:ch + 4 * depth], sets, what)
        dc = [quantise(int(back[c]), steps[c]) for c in range(ch)]
        side = choose_members(back[ch + 4 * depth:]) if rows else [0] * (depth * 6)
        if ev:
            ev[3].record()
        body = b""
        if rows:
            d_side = torch.tensor(side, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
            tabs = _tables(dev)
            plan = R.Plan(rows * ch, 1, 1, segments_for(rows * ch, segment_symbols))
            cap = R.align8(plan.capacity)
            blob = torch.zeros(8 + cap, dtype=torch.uint8, device=dev)
            R.encode(tabs, plan, coef, idx, blob.data_ptr() + 8, blob.data_ptr())
            if ev:
                ev[4].record()
            host = blob.cpu().numpy()                                      # one read: size + container
            nb = int(host[:8].view(np.int64)[0])
            if not 0 < nb <= cap:
                raise L.PccError(f"{what}: the coder produced {nb} bytes for a capacity of {cap}")
            body = struct.pack("<I", nb) + host[8:8 + nb].tobytes()
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["stages_ms"] = {"prepare_plan": ev[0].elapsed_time(ev[1]), "forward": ev[1].elapsed_time(ev[2]),
                                    "index_hist_choose": ev[2].elapsed_time(ev[3]),
                                    "index_rans": ev[3].elapsed_time(ev[4]) if rows else 0.0}
            timings["host_reads_by_construction"] = 2 if rows else 1       # beyond those of building the level sets
    out = bytearray(HEADER.pack(MAGIC, n, depth, ch, int(colour), qp, cqo))
    for q in dc:
        out += _zigzag(q)
    out += bytes(side)
    return bytes(out + body)


@torch.no_grad()
def decode_attributes(data, geometry, device=None):
    """bytes + the block's geometry (the pitch-1 CoordSet `decode_geometry(..., as_set=True)` returns, or [n, >= 3] rows) ->
    uint8 [n, C] in the canonical order `decode_geometry` returns.  device=None: the geometry's.  Raises PccError on a
    malformed stream, on a stream whose n or depth differ from the geometry's, and on a payload that does not decode; never
    returns anything but exactly [n, C]."""
    what = "decode_attributes"
    hdr = parse_header(data)
    if torch.is_tensor(geometry) and device is not None:
        geometry = geometry.to(device)
    cs = G.canonical_rows(geometry, what)[0]
    dev = cs.device
    if dev.type != "cuda" or (device is not None and torch.device(device).type != "cuda"):
        raise L.PccError(f"{what} runs on a GPU (no CPU fallback)")
    n, depth, ch, steps = hdr["n"], hdr["depth"], hdr["channels"], hdr["steps"]
    if cs.n != n or (n and _depth_of(cs) != depth):
        raise L.PccError(f"{what}: the stream codes {n} points at depth {depth}, the geometry has {cs.n} at depth "
                         f"{_depth_of(cs) if cs.n else 0}")
    if n == 0:
        return torch.empty((0, ch), dtype=torch.uint8, device=dev)
    h_steps = (C.c_int32 * ch)(*steps)
    rows = n - 1
    with torch.cuda.device(dev):
        sets = G.level_sets(cs, tuple(cs.bounds.lo), depth)
        masks, offs, checks = _plan(sets, depth, dev)
        weights = [None] * (depth + 1)                                      # the voxels weigh 1: no array
        for l in range(depth - 1, -1, -1):
            weights[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            L.call("pcc_raht_weights", *_level_args(sets[l], sets[l + 1]), L.ptr(weights[l + 1]), L.ptr(weights[l]), L.stream())
        status = torch.zeros(2, dtype=torch.int32, device=dev)             # rANS status | clamp flag
        coef = torch.zeros(max(rows, 1) * ch, dtype=torch.int32, device=dev)
        if rows:
            b0, b1 = hdr["payload"]
            d_buf = torch.from_numpy(R.stage(data, [(b0, b1)])[0]).to(dev)
            d_side = torch.tensor(hdr["side"], dtype=torch.int32, device=dev)
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
            R.decode(_tables(dev), d_buf, b1 - b0, idx, rows * ch, 1, 1, hdr["streams"], coef, status.data_ptr())
        v = torch.tensor([[q * s for q, s in zip(hdr["dc"], steps)]], dtype=torch.int32, device=dev)
        for l in range(depth):
            cv = torch.zeros((sets[l + 1].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_raht_inverse", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v), ch, h_steps,
                   L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), status.data_ptr() + 4, L.stream())
            v = cv
        out = torch.empty((n, ch), dtype=torch.uint8, device=dev)
        L.call("pcc_raht_finish", L.ptr(v), n, ch, int(hdr["colour"]), L.ptr(out), L.stream())
        back = torch.cat([status, checks.reshape(-1)]).cpu().numpy()         # the decode's one device->host read
    _check_plan(back[2:], sets, what)
    if back[0] != 0:
        raise L.PccError(f"attribute stream: malformed rANS container (status {int(back[0])})")
    if back[1] != 0:
        raise L.PccError("attribute stream: a coefficient or a reconstructed value left the +-2^30 range")
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the lossless coder: the same levels, rows, groups, family and container; a reversible arithmetic
# ------------------------------------------------------------------------------------------------------------------------
LOSSLESS_MAGIC = 0xB5      # format version 1
LOSSLESS_HEADER = struct.Struct("<BIBBB")
F_COLOUR, F_PREDICT, F_STORED = 1, 2, 4
SYMBOL_LIMIT = 1023        # the decoder's clamp on a symbol; a valid one is within +-1020


def channel_ranges(channels, colour):
    """[(lo, hi)] per channel: 0..255, and -255..255 for Co and Cg of YCoCg-R."""
    return [(0, 255)] + [(-255, 255) if colour else (0, 255)] * (channels - 1)


def parse_lossless_header(data):
    """{n, depth, channels, colour, predict, stored, root (per channel), side (depth * 6 members), payload=(begin, end) or None,
    streams, raw=(begin, end) or None}.  Raises PccError on a bad magic byte, an unknown flag, the colour flag without three
    channels, channels, n or depth out of range, a root outside its channel's range, a side byte that names no table,
    truncation, trailing bytes, a container length that disagrees with the data and a stored body of the wrong size --
    before any GPU work."""
    if len(data) < LOSSLESS_HEADER.size:
        raise L.PccError("lossless attribute stream truncated inside the header")
    magic, n, depth, ch, flags = LOSSLESS_HEADER.unpack_from(data, 0)
    if magic != LOSSLESS_MAGIC:
        raise L.PccError(f"lossless attribute stream: magic byte {magic:#x}, this build reads {LOSSLESS_MAGIC:#x}")
    if not 1 <= ch <= MAX_C:
        raise L.PccError(f"lossless attribute stream: {ch} channels outside 1..{MAX_C}")
    if flags & ~7 or (flags & F_COLOUR and ch != 3) or (flags & F_STORED and flags != F_STORED):
        raise L.PccError(f"lossless attribute stream: flags {flags:#x} with {ch} channels")
    if n >= MAX_POINTS:
        raise L.PccError(f"lossless attribute stream: header claims {n} points, the limit is 2^26 - 1")
    if (n == 0 and depth != 0) or (n > 0 and not 1 <= depth <= G.MAX_DEPTH) or n > 8 ** min(depth, 10):
        raise L.PccError(f"lossless attribute stream: header claims {n} points at depth {depth}")
    colour = bool(flags & F_COLOUR)
    hdr = {"n": n, "depth": depth, "channels": ch, "colour": colour, "predict": bool(flags & F_PREDICT), "stored": bool(flags & F_STORED),
           "root": [], "side": [], "payload": None, "streams": 0, "raw": None}
    at = LOSSLESS_HEADER.size
    if hdr["stored"]:
        if len(data) != at + n * ch:
            raise L.PccError(f"lossless attribute stream: a stored body of {len(data) - at} bytes for {n} x {ch} levels")
        hdr["raw"] = (at, at + n * ch)
        return hdr
    for c, (lo, hi) in enumerate(channel_ranges(ch, colour)):
        u, sh = 0, 0
        while True:
            if at >= len(data) or sh > 14:
                raise L.PccError("lossless attribute stream truncated inside the root values")
            b = data[at]
            at += 1
            u |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        q = (u >> 1) if not u & 1 else -((u + 1) >> 1)
        if not lo <= q <= hi or (n == 0 and q):
            raise L.PccError(f"lossless attribute stream: root value {q} of channel {c} outside {lo}..{hi}")
        hdr["root"].append(q)
    if at + depth * 6 > len(data):
        raise L.PccError("lossless attribute stream truncated inside the side bytes")
    hdr["side"] = list(data[at:at + depth * 6])
    at += depth * 6
    if hdr["side"] and max(hdr["side"]) >= N_TABLES:
        raise L.PccError(f"lossless attribute stream: side byte {max(hdr['side'])} names no table (64 members)")
    if n > 1:
        hdr["payload"], hdr["streams"] = _container_span(data, at, (n - 1) * ch, "lossless attribute stream")
        at = hdr["payload"][1]
    if at != len(data):
        raise L.PccError("lossless attribute stream: trailing bytes")
    return hdr


def _node_level_args(node, child, root):
    """The eleven leading arguments of the entry points that also probe the node level: the nodes with their own grid index
    (the root's single node is searched), their children with theirs."""
    use = S.USE_GRID and not root
    return (L.ptr(node.keys), node.n, node.ts, *S.grid_args(node.grid() if use else None), L.ptr(child.keys), child.n,
            *S.grid_args(child.grid() if S.USE_GRID else None))


@torch.no_grad()
def encode_attributes_lossless(cloud, colour=True, attrs=None, predict=True, segment_symbols=SEGMENT_SYMBOLS, timings=None):
    """The input forms and refusals of `encode_attributes` -> bytes that `decode_attributes_lossless` turns back into the very
    uint8 levels (colours of an [N, 6] cloud become round(255 c) first).  colour: YCoCg-R in front of the lifting (three
    channels only).  predict: code every butterfly against its prediction from the parent level.  When the coded stream would
    be longer than header + n * C bytes, the raw levels are stored instead.  timings: a dict that receives per-stage device
    events (tools/lossless_timing.py)."""
    what = "encode_attributes_lossless"
    cloud, levels = _attribute_rows(cloud, attrs, what)
    cs, perm, keep = G.canonical_rows(cloud, what)
    if keep is not None:
        raise L.PccError(f"{what}: {levels.shape[0] - cs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    n, ch = cs.n, levels.shape[1]
    if n >= MAX_POINTS:
        raise L.PccError(f"{what}: {n} points, the limit is 2^26 - 1")
    colour, predict = bool(colour) and ch == 3, bool(predict)
    if n == 0:
        return LOSSLESS_HEADER.pack(LOSSLESS_MAGIC, 0, 0, ch, F_STORED)
    dev = cs.device
    if levels.device != dev:
        raise L.PccError(f"{what}: points and attrs are on different devices")
    origin, depth = tuple(cs.bounds.lo), _depth_of(cs)
    rows = n - 1
    with torch.cuda.device(dev):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)] if timings is not None else None
        sets = G.level_sets(cs, origin, depth)
        if ev:
            ev[0].record()
        values = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_lift_prepare", L.ptr(levels), L.ptr(perm), n, ch, int(colour), L.ptr(values), L.stream())
        masks, offs, checks = _plan(sets, depth, dev)
        if ev:
            ev[1].record()
        coef = torch.zeros((max(rows, 1), ch), dtype=torch.int32, device=dev)
        w, v = [None] * (depth + 1), [None] * depth + [values]
        for l in range(depth - 1, -1, -1):
            w[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            v[l] = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_lift_forward", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(w[l + 1]), L.ptr(v[l + 1]), ch, L.ptr(w[l]),
                   L.ptr(v[l]), L.ptr(coef), sets[l].n - 1, rows, L.stream())
        if ev:
            ev[2].record()
        if predict and rows:
            for l in range(depth):
                L.call("pcc_lift_residual", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(w[l + 1]), L.ptr(v[l]), ch,
                       L.ptr(coef), sets[l].n - 1, rows, L.stream())
        if ev:
            ev[3].record()
        parts = [v[0].reshape(-1), checks.reshape(-1)]
        if rows:
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            hist = torch.empty(depth * 6 * N_SLOTS, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, None, idx, rows)
            L.call("pcc_raht_hist", L.ptr(coef), L.ptr(idx), rows * ch, depth * 6, L.ptr(hist), L.stream())
            parts.append(hist)
        back = torch.cat(parts).cpu().numpy()                              # one read: root values, the plan's checks, the histograms
        _check_plan(back[ch:ch + 4 * depth], sets, what)
        root = [int(back[c]) for c in range(ch)]
        side = choose_members(back[ch + 4 * depth:]) if rows else [0] * (depth * 6)
        if ev:
            ev[4].record()
        body = b""
        if rows:
            d_side = torch.tensor(side, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
            tabs = _tables(dev)
            plan = R.Plan(rows * ch, 1, 1, segments_for(rows * ch, segment_symbols))
            cap = R.align8(plan.capacity)
            blob = torch.zeros(8 + cap, dtype=torch.uint8, device=dev)
            R.encode(tabs, plan, coef, idx, blob.data_ptr() + 8, blob.data_ptr())
            if ev:
                ev[5].record()
            host = blob.cpu().numpy()                                      # one read: size + container
            nb = int(host[:8].view(np.int64)[0])
            if not 0 < nb <= cap:
                raise L.PccError(f"{what}: the coder produced {nb} bytes for a capacity of {cap}")
            body = struct.pack("<I", nb) + host[8:8 + nb].tobytes()
        out = bytearray(LOSSLESS_HEADER.pack(LOSSLESS_MAGIC, n, depth, ch, (F_COLOUR if colour else 0) | (F_PREDICT if predict else 0)))
        for q in root:
            out += _zigzag(q)
        out += bytes(side) + body
        stored = len(out) > LOSSLESS_HEADER.size + n * ch
        if stored:                                                         # a third read, of the raw levels, in this case alone
            raw = levels if perm is None else levels[perm]
            out = LOSSLESS_HEADER.pack(LOSSLESS_MAGIC, n, depth, ch, F_STORED) + raw.cpu().numpy().tobytes()
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["stages_ms"] = {"prepare_plan": ev[0].elapsed_time(ev[1]), "forward": ev[1].elapsed_time(ev[2]),
                                    "residual": ev[2].elapsed_time(ev[3]), "index_hist_choose": ev[3].elapsed_time(ev[4]),
                                    "index_rans": ev[4].elapsed_time(ev[5]) if rows else 0.0}
            timings["host_reads_by_construction"] = (2 if rows else 1) + int(stored)       # beyond those of building the level sets
            timings["stored"] = stored
    return bytes(out)


@torch.no_grad()
def decode_attributes_lossless(data, geometry, device=None):
    """bytes + the block's geometry (the pitch-1 CoordSet `decode_geometry(..., as_set=True)` returns, or [n, >= 3] rows) ->
    uint8 [n, C] in the canonical order `decode_geometry` returns: the levels the encoder was given.  device=None: the
    geometry's.  Raises PccError on a malformed stream, on a stream whose n or depth differ from the geometry's, and on a
    payload that does not decode to legal values; never returns anything but exactly [n, C]."""
    what = "decode_attributes_lossless"
    hdr = parse_lossless_header(data)
    if torch.is_tensor(geometry) and device is not None:
        geometry = geometry.to(device)
    cs = G.canonical_rows(geometry, what)[0]
    dev = cs.device
    if dev.type != "cuda" or (device is not None and torch.device(device).type != "cuda"):
        raise L.PccError(f"{what} runs on a GPU (no CPU fallback)")
    n, depth, ch, colour, predict = hdr["n"], hdr["depth"], hdr["channels"], hdr["colour"], hdr["predict"]
    if cs.n != n or (n and _depth_of(cs) != depth):
        raise L.PccError(f"{what}: the stream codes {n} points at depth {depth}, the geometry has {cs.n} at depth "
                         f"{_depth_of(cs) if cs.n else 0}")
    if n == 0:
        return torch.empty((0, ch), dtype=torch.uint8, device=dev)
    if hdr["stored"]:
        b0, b1 = hdr["raw"]
        return torch.from_numpy(np.frombuffer(data, np.uint8, b1 - b0, b0).reshape(n, ch).copy()).to(dev)
    rows = n - 1
    with torch.cuda.device(dev):
        sets = G.level_sets(cs, tuple(cs.bounds.lo), depth)
        masks, offs, checks = _plan(sets, depth, dev)
        weights = [None] * (depth + 1)                                      # the voxels weigh 1: no array
        for l in range(depth - 1, -1, -1):
            weights[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            L.call("pcc_raht_weights", *_level_args(sets[l], sets[l + 1]), L.ptr(weights[l + 1]), L.ptr(weights[l]), L.stream())
        status = torch.zeros(2, dtype=torch.int32, device=dev)             # rANS status | clamp flag
        coef = torch.zeros(max(rows, 1) * ch, dtype=torch.int32, device=dev)
        if rows:
            b0, b1 = hdr["payload"]
            d_buf = torch.from_numpy(R.stage(data, [(b0, b1)])[0]).to(dev)
            d_side = torch.tensor(hdr["side"], dtype=torch.int32, device=dev)
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
            R.decode(_tables(dev), d_buf, b1 - b0, idx, rows * ch, 1, 1, hdr["streams"], coef, status.data_ptr())
        v = torch.tensor([hdr["root"]], dtype=torch.int32, device=dev)
        for l in range(depth):
            cv = torch.zeros((sets[l + 1].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_lift_inverse", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v), ch,
                   int(colour), int(predict), L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), status.data_ptr() + 4, L.stream())
            v = cv
        out = torch.empty((n, ch), dtype=torch.uint8, device=dev)
        L.call("pcc_lift_finish", L.ptr(v), n, ch, int(colour), L.ptr(out), status.data_ptr() + 4, L.stream())
        back = torch.cat([status, checks.reshape(-1)]).cpu().numpy()         # the decode's one device->host read
    _check_plan(back[2:], sets, what)
    if back[0] != 0:
        raise L.PccError(f"lossless attribute stream: malformed rANS container (status {int(back[0])})")
    if back[1] != 0:
        raise L.PccError("lossless attribute stream: a symbol, a reconstructed value or a level left its legal range")
    return out
