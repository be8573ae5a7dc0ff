"""Colour (any 8-bit attribute) of one block on the device: `encode_attributes` / `decode_attributes`, a RAHT coder over the
level sets of the octree geometry coder.  With `geometry.encode_geometry` it forms the anchor the
reference draws every RD plot against -- `tmc3 --transformType=0`, octree geometry + RAHT colour (`utils.py:505-529`) -- in
this project's own stream: no G-PCC syntax and no bit-compatibility claim, the stance section 7e takes for geometry.

    stream = u8 0xB3 | u32 n | u8 depth | u8 C | u8 flags (bit 0: colour transform) | u8 qp | i8 chroma_qp_offset
             | C zig-zag LEB128 varints (the quantised root DC) | depth x 6 side bytes | u32 length | rANS container
    (no length and no container when n <= 1)
    inter:   u8 0xB4 | u32 n | u8 depth | u8 C | u8 flags | u8 qp | i8 chroma_qp_offset | u8 block_log2 | u8 search | u32 blocks
             | C zig-zag varints (the quantised root DC residual) | (depth + 1) x 6 side bytes
             | ceil(blocks / 8) mode bytes (block b: bit b & 7 of byte b >> 3) | u32 length | rANS container
             (coded against a reference cloud the decoder holds, in the coefficient domain; no vector travels; "Inter frames" in 7f)
    wide:    u8 0xB8 | the 0xB4 layout byte for byte, search in 3 .. 7: the matches come from block vectors searched over
             [-search, search]^3 (`encode_attributes(..., search=)`; the decoder re-runs that search; 0xB4 itself reads 2 only)
    predicted: u8 0xB9 | the 0xB3 layout byte for byte, n >= 2: every coefficient travels as quantise(H - Hp), Hp the transform of
             a prediction of the node's children from the parent level as the decoder has reconstructed it
             (`encode_attributes(..., predict=)`; "Prediction from the parent level" in 7f)

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
payload.  All seven headers of this file are one layout with optional parts: the table `KINDS` says per magic byte which parts a
stream has and what its fields may hold, `_parse` (behind `parse_header` and `parse_lossless_header`) reads it and `_stream`
writes it.

`encode_attributes_lossless` / `decode_attributes_lossless` (second half of this file) are a separate coder
over the same levels, rows, groups, family and container with a reversible arithmetic and their own stream:

    stream = u8 0xB5 | u32 n | u8 depth | u8 C | u8 flags (bit 0: YCoCg-R, bit 1: prediction, bit 2: stored)
             | C zig-zag varints (root values) | depth x 6 side bytes | u32 length | rANS container
    stored:  u8 0xB5 | u32 n | u8 depth | u8 C | u8 4 | n x C raw levels in canonical order
    inter:   u8 0xB6 | u32 n | u8 depth | u8 C | u8 flags (bit 1, and bit 0 for YCoCg-R) | u8 block_log2 | u8 search | u32 blocks
             | C zig-zag varints | (depth + 1) x 6 side bytes | ceil(blocks / 8) mode bytes (block b: bit b & 7 of byte b >> 3)
             | u32 length | rANS container            (coded against a reference cloud the decoder holds; no vector travels)
    wide:    u8 0xB7 | the 0xB6 layout byte for byte, search in 3 .. 7 (`encode_attributes_lossless(..., search=)`, as 0xB8 above)
"""
import collections
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
INTER_LOSSY_MAGIC = 0xB4   # inter frames, format version 1: coefficients predicted from a reference cloud
WIDE_LOSSY_MAGIC = 0xB8    # the 0xB4 layout byte for byte with the block vectors searched over +-3 .. +-7 (the header's search byte)
PRED_MAGIC = 0xB9          # intra, the 0xB3 layout byte for byte: coefficients predicted from the parent level (closed loop)
INTER_LOSSY_HEADER = struct.Struct("<BIBBBBbBBI")
LOSSLESS_MAGIC = 0xB5      # the lossless coder (second half of this file), format version 1
LOSSLESS_HEADER = struct.Struct("<BIBBB")
F_COLOUR, F_PREDICT, F_STORED = 1, 2, 4
SYMBOL_LIMIT = 1023        # the lossless decoder's clamp on a symbol; a valid one is within +-1020
INTER_MAGIC = 0xB6         # inter frames, format version 1: the last level may be predicted from a reference cloud
WIDE_MAGIC = 0xB7          # the 0xB6 layout byte for byte with the block vectors searched over +-3 .. +-7 (the header's search byte)
INTER_HEADER = struct.Struct("<BIBBBBBI")
INTER_MAX_DEPTH = 14       # (depth + 1) * 6 groups within the 90 of pcc_raht_hist
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


# ------------------------------------------------------------------------------------------------------------------------
# the stream headers, host side: one table of the seven streams, one reader, one writer
# ------------------------------------------------------------------------------------------------------------------------
def _check_range(name, block_log2, search, wide):
    """The block size and search range of an inter header: G.SEARCH under the narrow magic bytes, G.WIDE_SEARCH under the wide ones."""
    lo, hi = G.WIDE_SEARCH if wide else (G.SEARCH, G.SEARCH)
    if block_log2 != G.BLOCK_LOG2 or not lo <= search <= hi:
        reads = f"{lo}..{hi}" if wide else f"{G.SEARCH}"
        raise L.PccError(f"{name}: block_log2 {block_log2}, search {search}; this build reads {G.BLOCK_LOG2} and {reads}")


def channel_ranges(channels, colour):
    """[(lo, hi)] per channel of the lossless coder: 0..255, and -255..255 for Co and Cg of YCoCg-R."""
    return [(0, 255)] + [(-255, 255) if colour else (0, 255)] * (channels - 1)


def _dc_rule(hdr, c, q):
    """What is wrong with the quantised root DC q of channel c (RAHT streams), or None: q * step stays within the decoder's clamp."""
    return f"root DC {q} of channel {c} is out of range" if abs(q) * hdr["steps"][c] > LIMIT else None


def _root_rule(hdr, c, q):
    """What is wrong with the root value q of channel c (lossless streams), or None: inside the channel's range, 0 without a voxel."""
    lo, hi = channel_ranges(hdr["channels"], hdr["colour"])[c]
    return f"root value {q} of channel {c} outside {lo}..{hi}" if not lo <= q <= hi or (hdr["n"] == 0 and q) else None


# One stream form: head (the struct of its fixed fields) and the names of those behind magic, n, depth, channels, flags; its name in
# refusals; inter, wide; the legal flag bytes; the largest shift a root varint may reach and the rule its value obeys (`_dc_rule`
# marks the RAHT streams: qp and steps in the header, "dc" in the result); the levels of side-byte groups beyond `depth`
# ((depth + extra) * 6 side bytes).
_Kind = collections.namedtuple("_Kind", "head more name inter wide flags shift rule extra")
_QP, _BLOCKS = ("qp", "chroma_qp_offset"), ("block_log2", "search", "blocks")
_CODED = (0, F_COLOUR, F_PREDICT, F_PREDICT | F_COLOUR)
KINDS = {
    MAGIC: _Kind(HEADER, _QP, "attribute stream", False, False, (0, F_COLOUR), 28, _dc_rule, 0),
    PRED_MAGIC: _Kind(HEADER, _QP, "predicted attribute stream", False, False, (0, F_COLOUR), 28, _dc_rule, 0),
    INTER_LOSSY_MAGIC: _Kind(INTER_LOSSY_HEADER, _QP + _BLOCKS, "inter attribute stream", True, False, (0, F_COLOUR), 28, _dc_rule, 1),
    WIDE_LOSSY_MAGIC: _Kind(INTER_LOSSY_HEADER, _QP + _BLOCKS, "inter attribute stream", True, True, (0, F_COLOUR), 28, _dc_rule, 1),
    LOSSLESS_MAGIC: _Kind(LOSSLESS_HEADER, (), "lossless attribute stream", False, False, _CODED + (F_STORED,), 14, _root_rule, 0),
    INTER_MAGIC: _Kind(INTER_HEADER, _BLOCKS, "inter lossless attribute stream", True, False, _CODED[2:], 14, _root_rule, 1),
    WIDE_MAGIC: _Kind(INTER_HEADER, _BLOCKS, "inter lossless attribute stream", True, True, _CODED[2:], 14, _root_rule, 1),
}


def _unzigzag(data, at, max_shift):
    """(value, the offset behind it) of the zig-zag LEB128 varint at `at`; (None, at) where the data end inside it or it runs
    past max_shift."""
    u, sh = 0, 0
    while True:
        if at >= len(data) or sh > max_shift:
            return None, at
        b = data[at]
        at += 1
        u |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            return ((u >> 1) if not u & 1 else -((u + 1) >> 1)), at


def _parse(data, have_reference, family, reads):
    """The one walk of a colour stream: fixed fields -> root varints -> side bytes -> mode bytes -> container -> trailing bytes, the
    checks in the order the streams have always been refused in.  family: the magic bytes the calling entry point reads, its
    intra stream first (which also names the refusal of anything else); reads: how the refusal of a foreign magic byte lists them."""
    kind = KINDS[data[0] if len(data) and data[0] in family else family[0]]
    name, lossy = kind.name, kind.rule is _dc_rule
    if kind.inter and not have_reference:
        raise L.PccError(f"{name}: the stream is coded against a reference cloud and none was given")
    if len(data) < kind.head.size:
        raise L.PccError(f"{name} truncated inside the header")
    f = dict(zip(("magic", "n", "depth", "channels", "flags") + kind.more, kind.head.unpack_from(data, 0)))
    n, depth, ch, flags = f["n"], f["depth"], f["channels"], f["flags"]
    if f["magic"] not in family:
        raise L.PccError(f"{name}: magic byte {f['magic']:#x}, this build reads {reads}")
    if not 1 <= ch <= MAX_C:
        raise L.PccError(f"{name}: {ch} channels outside 1..{MAX_C}")
    if flags not in kind.flags or (flags & F_COLOUR and ch != 3):
        raise L.PccError(f"{name}: flags {flags:#x} with {ch} channels")
    if lossy and not QP_MIN <= f["qp"] <= QP_MAX:
        raise L.PccError(f"{name}: qp {f['qp']} outside {QP_MIN}..{QP_MAX}")
    if lossy or not kind.inter:                    # (0xB6 / 0xB7 word these two in their own way, below)
        if n >= MAX_POINTS:
            raise L.PccError(f"{name}: header claims {n} points, the limit is 2^26 - 1")
        if (n == 0 and depth != 0) or (n > 0 and not 1 <= depth <= G.MAX_DEPTH) or n > 8 ** min(depth, 10):
            raise L.PccError(f"{name}: header claims {n} points at depth {depth}")
    hdr = {"n": n, "depth": depth, "channels": ch, "colour": bool(flags & F_COLOUR), "side": [], "payload": None, "streams": 0,
           "inter": kind.inter}
    if lossy:
        hdr.update(qp=f["qp"], chroma_qp_offset=f["chroma_qp_offset"], steps=steps_for(f["qp"], f["chroma_qp_offset"], ch))
        if f["magic"] == PRED_MAGIC:                   # the only RAHT stream with this key: the others' results stay as they were
            if n < 2:
                raise L.PccError(f"{name}: header claims {n} points, a predicted stream codes 2 .. 2^26 - 1")
            hdr["predict"] = True
    else:
        hdr.update(predict=bool(flags & F_PREDICT), stored=bool(flags & F_STORED), raw=None)
    if kind.inter:
        _check_range(name, f["block_log2"], f["search"], kind.wide)
        if not 2 <= n < MAX_POINTS:
            raise L.PccError(f"{name}: header claims {n} points, an inter stream codes 2 .. 2^26 - 1")
        if lossy and depth > INTER_MAX_DEPTH:
            raise L.PccError(f"{name}: header claims depth {depth} (inter streams exist up to depth {INTER_MAX_DEPTH})")
        if not lossy and (not 1 <= depth <= INTER_MAX_DEPTH or n > 8 ** min(depth, 10)):
            raise L.PccError(f"{name}: header claims {n} points at depth {depth} (inter streams exist up to depth {INTER_MAX_DEPTH})")
        if not 1 <= f["blocks"] <= n:
            raise L.PccError(f"{name}: header claims {f['blocks']} blocks for {n} points")
        hdr.update(block_log2=f["block_log2"], search=f["search"], blocks=f["blocks"])
    at = kind.head.size
    key, word = ("dc", "root DC") if lossy else ("root", "root values")
    hdr[key] = []
    if not lossy and hdr["stored"]:                # the stored form of 0xB5: the raw levels and nothing else
        if len(data) != at + n * ch:
            raise L.PccError(f"{name}: a stored body of {len(data) - at} bytes for {n} x {ch} levels")
        hdr["raw"] = (at, at + n * ch)
        return hdr
    for c in range(ch):
        q, at = _unzigzag(data, at, kind.shift)
        if q is None:
            raise L.PccError(f"{name} truncated inside the {word}")
        why = kind.rule(hdr, c, q)
        if why:
            raise L.PccError(f"{name}: {why}")
        hdr[key].append(q)
    groups = (depth + kind.extra) * 6
    if at + groups > len(data):
        raise L.PccError(f"{name} truncated inside the side bytes")
    hdr["side"] = list(data[at:at + groups])
    at += groups
    if hdr["side"] and max(hdr["side"]) >= N_TABLES:
        raise L.PccError(f"{name}: side byte {max(hdr['side'])} names no table (64 members)")
    if kind.inter:
        mbytes = (hdr["blocks"] + 7) // 8
        if at + mbytes > len(data):
            raise L.PccError(f"{name} truncated inside the mode bytes")
        if hdr["blocks"] % 8 and data[at + mbytes - 1] >> (hdr["blocks"] % 8):
            raise L.PccError(f"{name}: padding bits of the mode bytes are set")
        hdr["modes"] = (at, at + mbytes)
        at += mbytes
    if n > 1:                                           # no voxel, or one: no row, no length and no container
        hdr["payload"], hdr["streams"] = _container_span(data, at, (n - 1) * ch, name)
        at = hdr["payload"][1]
    if at != len(data):
        raise L.PccError(f"{name}: trailing bytes")
    return hdr


def parse_header(data, have_reference=True):
    """{n, depth, channels, colour, qp, chroma_qp_offset, steps, dc (quantised root DC per channel), side (depth * 6 members),
    payload=(begin, end) or None, streams, inter}.  Raises PccError on a bad magic byte, on channels, qp or depth out of range,
    on a root DC or side byte out of range, on truncation, on trailing bytes and on a length that disagrees with the data --
    before any GPU work.  A predicted stream (0xB9: the 0xB3 layout) has predict=True besides, the only one with that key, and is
    refused with fewer than two points.  An inter stream (0xB4, or 0xB8: the same layout searched over +-3 .. +-7) has
    inter=True, dc = the quantised root DC residual, (depth + 1) * 6 side bytes and block_log2, search, blocks, modes=(begin, end) besides; refused
    for it as well: a block size or search range other than this build's, depth > 14, n < 2, a block count of 0 or above n, set
    padding bits of the mode bytes, and have_reference=False.  A 0xB5 .. 0xB7 stream is refused by its magic byte."""
    return _parse(data, have_reference, (MAGIC, INTER_LOSSY_MAGIC, WIDE_LOSSY_MAGIC, PRED_MAGIC),
                  f"{MAGIC:#x}, {INTER_LOSSY_MAGIC:#x} and {WIDE_LOSSY_MAGIC:#x}")


def parse_lossless_header(data, have_reference=True):
    """{n, depth, channels, colour, predict, stored, root (per channel), side (depth * 6 members), payload=(begin, end) or None,
    streams, raw=(begin, end) or None, inter}.  Raises PccError on a bad magic byte, an unknown flag, the colour flag without
    three channels, channels, n or depth out of range, a root outside its channel's range, a side byte that names no table,
    truncation, trailing bytes, a container length that disagrees with the data and a stored body of the wrong size --
    before any GPU work.  An inter stream (0xB6, or 0xB7: the same layout searched over +-3 .. +-7) has inter=True,
    (depth + 1) * 6 side bytes and block_log2, search, blocks, modes=(begin, end) besides; refused for it as well: a block size
    or search range other than this build's, depth > 14, n < 2, a block count of 0 or above n, set padding bits of the mode
    bytes, and have_reference=False.  A 0xB3, 0xB4, 0xB8 or 0xB9 stream is refused by its magic byte."""
    return _parse(data, have_reference, (LOSSLESS_MAGIC, INTER_MAGIC, WIDE_MAGIC), f"{LOSSLESS_MAGIC:#x}")


def _stream(magic, fields, roots=(), side=(), modes=None, body=b""):
    """The bytes of a stream from its parts: the fixed fields behind the magic byte, the root values (zig-zag varints), the side
    bytes, one int per block (the mode bytes of an inter stream; None: none), and `u32 length | rANS container` or raw levels."""
    out = KINDS[magic].head.pack(magic, *fields) + b"".join(_zigzag(int(q)) for q in roots) + bytes(side)
    if modes is not None:
        out += np.packbits(np.asarray(modes).astype(bool), bitorder="little").tobytes()
    return out + body


# ------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------
def _colour_search(search, what):
    """The search range of a colour encoder: an int in 2 .. 7 (None: 2).  "auto" belongs to the geometry coder -- the colour follows
    the range the geometry stream ended with (`geometry.stream_search`)."""
    search = G.check_search(search, what)
    if search == "auto":
        raise L.PccError(f"{what}: search \"auto\" is the geometry coder's; give the range its stream ended with (geometry.stream_search)")
    return search


def _tables(dev):
    """The family on the device, with its encoder entries and decoder blob: one upload per device."""
    return R.fixed_tables("raht", dev, table_family()[0], TABLE_SIZES, TABLE_OFFSETS, enc=True, dec=True)


def _depth_of(cs):
    return max(1, max(cs.bounds.hi[i] - cs.bounds.lo[i] for i in range(3)).bit_length())


def _level_args(node, child):
    """The eight leading arguments of the per-level entry points: the nodes, their children, the children's grid index."""
    return (L.ptr(node.keys), node.n, node.ts, L.ptr(child.keys), child.n, *S.grid_args(child.grid() if S.USE_GRID else None))


def _node_level_args(node, child, root):
    """The eleven leading arguments of the entry points that also probe the node level: the nodes with their own grid index
    (the root's single node is searched), their children with theirs."""
    use = S.USE_GRID and not root
    return (L.ptr(node.keys), node.n, node.ts, *S.grid_args(node.grid() if use else None), L.ptr(child.keys), child.n,
            *S.grid_args(child.grid() if S.USE_GRID else None))


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


def _reference_rows(reference, reference_attrs, channels, predict, what):
    """(set or None for an empty reference, its uint8 [M, C] levels, the permutation that brings them into the set's order or
    None) of the reference cloud of an inter stream: an [M, 6] cloud, or a pitch-1 set / [M, >= 3] rows with `reference_attrs`.
    Refused: the input forms `encode_attributes` refuses, rows that repeat a voxel (their colours would be ambiguous), another
    channel count than the stream's, and a stream without prediction."""
    who = f"{what} (reference)"
    if not predict:
        raise L.PccError(f"{what}: a reference needs the prediction (predict=True)")
    cloud, levels = _attribute_rows(reference, reference_attrs, who)
    if levels.shape[1] != channels:
        raise L.PccError(f"{who}: {levels.shape[1]} channels, the cloud has {channels}")
    if (cloud.n if isinstance(cloud, S.CoordSet) else cloud.shape[0]) == 0:
        return None, None, None
    rs, perm, keep = G.canonical_rows(cloud, who)
    if keep is not None:
        raise L.PccError(f"{who}: {levels.shape[0] - rs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    if levels.device != rs.device:
        raise L.PccError(f"{who}: points and attrs are on different devices")
    return rs, levels, perm


def _encoder_input(what, cloud, attrs, reference, reference_attrs, mode, predict, chroma_qp_offset=0):
    """The opening of both encoders: (canonical set, uint8 levels, their permutation, reference rows or None, depth, whether an
    inter stream is coded).  Refusals in this order, those that need no launch first: the mode, the cloud's rows, the chroma
    offset, the reference's rows, rows that repeat a voxel, too many points, attrs on another device, "inter" beyond depth 14.
    An empty cloud comes back with depth 0 before the device is looked at."""
    if mode not in ("auto", "inter", "intra"):
        raise L.PccError(f"{what}: mode {mode!r} is not one of auto, inter, intra")
    cloud, levels = _attribute_rows(cloud, attrs, what)
    if not -128 <= int(chroma_qp_offset) <= 127:
        raise L.PccError(f"{what}: chroma_qp_offset {chroma_qp_offset} does not fit the header's signed byte")
    ref = None
    if reference is not None and mode != "intra":                         # "intra" never looks at the reference
        ref = _reference_rows(reference, reference_attrs, levels.shape[1], predict, what)
    cs, perm, keep = G.canonical_rows(cloud, what)
    if keep is not None:
        raise L.PccError(f"{what}: {levels.shape[0] - cs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    if cs.n >= MAX_POINTS:
        raise L.PccError(f"{what}: {cs.n} points, the limit is 2^26 - 1")
    if cs.n == 0:
        return cs, levels, perm, None, 0, False
    if levels.device != cs.device:
        raise L.PccError(f"{what}: points and attrs are on different devices")
    depth = _depth_of(cs)
    inter = ref is not None and cs.n >= 2
    if inter and depth > INTER_MAX_DEPTH:
        if mode == "inter":
            raise L.PccError(f"{what}: inter streams exist up to depth {INTER_MAX_DEPTH}, the cloud has depth {depth}")
        inter = False
    return cs, levels, perm, ref, depth, inter


def _inter_state(cs, sets, origin, depth, ref, channels, colour, d_flag, prepare="pcc_lift_prepare", search=G.SEARCH):
    """What both sides of an inter stream (0xB6 and 0xB4) recompute from the geometry and the reference: (the block arguments of
    the pcc_lift_inter_* / pcc_raht_inter_* entry points, the block count, int32 match row per voxel, int32 [M, C] prepared
    reference values or None, M).  `geometry.motion_vectors` gives the vectors; the tensors the arguments point into live in
    `sets` and the result.  prepare: the entry point that turns the reference's levels into the coder's values (plain or
    YCoCg-R levels for the lossless coder, Q8 with BT.709 for the RAHT coder: "pcc_raht_prepare").  search above 2: the wide search,
    whose vectors are packed displacements (`pcc_lift_inter_match_wide`)."""
    rs, levels, perm = ref
    dev = cs.device
    blocks, bl, _, vec = G.motion_vectors(cs, rs, origin, depth, sets, search=search)
    grid = blocks.grid() if (depth > bl and S.USE_GRID) else None         # the root's single node is searched
    bargs = (L.ptr(blocks.keys), blocks.n, *S.grid_args(grid), bl)
    match = torch.empty(cs.n, dtype=torch.int32, device=dev)
    L.call("pcc_lift_inter_match_wide" if search > G.MAX_SEARCH else "pcc_lift_inter_match", L.ptr(sets[depth].keys), cs.n, *bargs, L.ptr(vec),
           search, *G.ref_args(rs), *origin, L.ptr(match), d_flag, L.stream())
    if rs is None:
        return bargs, blocks.n, match, None, 0, (vec, grid)
    if levels.device != dev:
        raise L.PccError("the reference is on another device than the cloud")
    tv = torch.empty((rs.n, channels), dtype=torch.int32, device=dev)
    L.call(prepare, L.ptr(levels), L.ptr(perm), rs.n, channels, int(colour), L.ptr(tv), L.stream())
    return bargs, blocks.n, match, tv, rs.n, (vec, grid)


def _rans_body(coef, idx, symbols, segment_symbols, dev, what, ph=None):
    """`u32 length | rANS container` of the symbol vector; one device->host read (size + container).  ph: `geometry.Phases`
    that get the mark "index_rans" behind the coder's launches."""
    plan = R.Plan(symbols, 1, 1, segments_for(symbols, segment_symbols))
    cap = R.align8(plan.capacity)
    blob = torch.zeros(8 + cap, dtype=torch.uint8, device=dev)
    R.encode(_tables(dev), plan, coef, idx, blob.data_ptr() + 8, blob.data_ptr())
    if ph is not None:
        ph.mark("index_rans")
    host = blob.cpu().numpy()
    nb = int(host[:8].view(np.int64)[0])
    if not 0 < nb <= cap:
        raise L.PccError(f"{what}: the coder produced {nb} bytes for a capacity of {cap}")
    return struct.pack("<I", nb) + host[8:8 + nb].tobytes()


def _forward_pass(sets, offs, values, depth, ch, h_steps, coef, rows):
    """The bottom-up pass of an intra stream, one launch per level: the rows of `coef` become quantise(H) under h_steps (every step
    1: H itself).  Returns (the root's DC [1, C], int32 weights per level, None for the voxels)."""
    dev = values.device
    weights, v_child = [None] * (depth + 1), values
    for l in range(depth - 1, -1, -1):
        weights[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
        v = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_raht_forward", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v_child), ch, h_steps,
               L.ptr(weights[l]), L.ptr(v), L.ptr(coef), sets[l].n - 1, rows, L.stream())
        v_child = v
    return v_child, weights


def _check_predict(what, predict):
    if predict is not None and predict is not False and predict is not True and predict != "auto":
        raise L.PccError(f"{what}: predict {predict!r} is not one of None, False, True, \"auto\"")
    return predict or False


def _predicted_rows(sets, offs, values, depth, ch, h_steps, rows):
    """(symbol rows [rows, C] of a 0xB9 stream, the root's true DC [1, C]), rows >= 1.  Closed loop: the bottom-up pass with every
    step 1 leaves the true H at the rows; then from the root down, one launch per level, `pcc_raht_pred_encode` forms Hp from the
    level's DCs and means AS THE DECODER RECONSTRUCTS THEM, writes quantise(H - Hp) and rebuilds the children's DCs and means with
    the decoder's own device function.  The clamp flag is not read: the encoder's values are within the quantisation error of the
    source (DESIGN.md 7f bounds), and the decoder reads its own."""
    dev, n = values.device, sets[depth].n
    h_true = torch.zeros((rows, ch), dtype=torch.int32, device=dev)
    v_root, weights = _forward_pass(sets, offs, values, depth, ch, (C.c_int32 * ch)(*([1] * ch)), h_true, rows)
    coef = torch.zeros((rows, ch), dtype=torch.int32, device=dev)
    d_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    v = torch.empty((1, ch), dtype=torch.int32, device=dev)
    m = torch.empty((1, ch), dtype=torch.int32, device=dev)
    L.call("pcc_raht_pred_root", L.ptr(v_root), n, ch, h_steps, L.ptr(v), L.ptr(m), L.ptr(d_flag), L.stream())
    for l in range(depth):
        cv = torch.zeros((sets[l + 1].n, ch), dtype=torch.int32, device=dev)
        cm = torch.empty((sets[l + 1].n, ch), dtype=torch.int32, device=dev) if l + 1 < depth else None    # nothing reads the voxels' means
        L.call("pcc_raht_pred_encode", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v),
               L.ptr(m), ch, h_steps, L.ptr(h_true), L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), L.ptr(cm), L.ptr(d_flag), L.stream())
        v, m = cv, cm
    return coef, v_root


def _intra_tail(what, sets, masks, offs, checks, coef, v_root, depth, ch, rows, segment_symbols, dev, ph):
    """(root values as they are, side bytes, `u32 length | rANS container`) of an intra stream (0xB3, 0xB5) from the coded rows
    and the root's values: the groups, their histograms, the member choice (one read), the member index and the coder (one
    read).  ph: the caller's `geometry.Phases`."""
    parts = [v_root.reshape(-1), checks.reshape(-1)]
    if rows:
        idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
        hist = torch.empty(depth * 6 * N_SLOTS, dtype=torch.int32, device=dev)
        _fill_index(masks, offs, sets, depth, ch, None, idx, rows)
        L.call("pcc_raht_hist", L.ptr(coef), L.ptr(idx), rows * ch, depth * 6, L.ptr(hist), L.stream())
        parts.append(hist)
    back = torch.cat(parts).cpu().numpy()                              # one read: root DC, the plan's checks, the histograms
    _check_plan(back[ch:ch + 4 * depth], sets, what)
    root = [int(back[c]) for c in range(ch)]
    side = choose_members(back[ch + 4 * depth:]) if rows else [0] * (depth * 6)
    ph.mark("index_hist_choose")
    body = b""
    if rows:
        d_side = torch.tensor(side, dtype=torch.int32, device=dev)
        _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
        body = _rans_body(coef, idx, rows * ch, segment_symbols, dev, what, ph)    # one read: size + container
    return root, side, body


def _inter_index(masks, offs, sets, depth, first, ch, bargs, d_mode, d_side, idx, coef_p, coef, rows, d_flag):
    """idx of all rows of an inter RAHT stream: the levels above the blocks as in the intra stream, the levels inside them by
    their block's mode.  d_side None: groups; coef given (encoder): the intra symbols of mode-0 blocks are copied into coef_p."""
    _fill_index(masks, offs, sets, first, ch, d_side, idx, rows)
    for l in range(first, depth):
        L.call("pcc_raht_inter_select", L.ptr(sets[l].keys), L.ptr(masks[l]), L.ptr(offs[l]), sets[l].n, l, depth, ch, *bargs, L.ptr(d_mode),
               L.ptr(d_side), L.ptr(idx), L.ptr(coef_p), L.ptr(coef), sets[l].n - 1, rows, d_flag, L.stream())


def _encode_inter_lossy(what, cs, levels, perm, ref, qp, cqo, colour, mode, segment_symbols, timings, search=G.SEARCH, predict=False):
    """The inter half of `encode_attributes` (n >= 2, depth <= 14): the 0xB4 stream (0xB8 when `search` is above 2) and, for
    mode "auto", the 0xB3 stream from
    the same forward pass (predict True: the 0xB9 stream in its place, "auto": the shorter of those two, 0xB3 on a tie); the
    shorter is returned, intra on a tie.  Device->host reads beyond the level sets: 2 for the inter stream (modes, root DCs and
    histograms; the container), 2 more for every intra stream of "auto"."""
    n, ch, dev = cs.n, levels.shape[1], cs.device
    steps = steps_for(qp, cqo, ch)
    h_steps = (C.c_int32 * ch)(*steps)
    origin, depth = tuple(cs.bounds.lo), _depth_of(cs)
    rows = n - 1
    with torch.cuda.device(dev):
        ph = G.Phases(timings is not None)
        sets = G.level_sets(cs, origin, depth)
        ph.mark("start")
        d_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        bargs, nb, match, tv, nr, _keep = _inter_state(cs, sets, origin, depth, ref, ch, colour, L.ptr(d_flag), "pcc_raht_prepare", search)
        first = depth - bargs[-1]
        ph.mark("motion_match_ms")
        values = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_raht_prepare", L.ptr(levels), L.ptr(perm), n, ch, int(colour), L.ptr(values), L.stream())
        masks, offs, checks = _plan(sets, depth, dev)
        fill_sums = torch.empty((nb, ch + 1), dtype=torch.int32, device=dev)
        pred = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_raht_inter_fill", L.ptr(sets[depth].keys), n, *bargs, L.ptr(match), L.ptr(tv), nr, ch, None, L.ptr(fill_sums), L.ptr(pred),
               L.ptr(d_flag), L.stream())
        ph.mark("prepare_plan_fill_ms")
        coef = torch.zeros((rows, ch), dtype=torch.int32, device=dev)      # the intra symbols of every row
        coef_p = torch.zeros((rows, ch), dtype=torch.int32, device=dev)    # the inter stream's symbols
        sums = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
        d_mode = torch.empty(nb, dtype=torch.int32, device=dev)
        w_child, v_child, p_child = None, values, pred
        for l in range(depth - 1, -1, -1):                                  # the levels above the blocks come after the decision
            w = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            v = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
            p = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_raht_inter_forward", *_level_args(sets[l], sets[l + 1]), *bargs, L.ptr(offs[l]), L.ptr(w_child), L.ptr(v_child),
                   L.ptr(p_child), ch, h_steps, L.ptr(w), L.ptr(v), L.ptr(p), L.ptr(coef), L.ptr(coef_p), sets[l].n - 1, rows,
                   L.ptr(sums) if l >= first else None, L.ptr(d_flag), L.stream())
            if l == first:
                L.call("pcc_raht_inter_modes", L.ptr(sums), L.ptr(fill_sums), nb, ch, L.ptr(d_mode), L.ptr(p), L.stream())
            w_child, v_child, p_child = w, v, p
        ph.mark("forward_modes_ms")
        groups = (depth + 1) * 6
        idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
        hist = torch.empty(groups * N_SLOTS, dtype=torch.int32, device=dev)
        _inter_index(masks, offs, sets, depth, first, ch, bargs, d_mode, None, idx, coef_p, coef, rows, L.ptr(d_flag))
        L.call("pcc_raht_hist", L.ptr(coef_p), L.ptr(idx), rows * ch, groups, L.ptr(hist), L.stream())
        back = torch.cat([v_child.reshape(-1), p_child.reshape(-1), checks.reshape(-1), d_flag, d_mode, hist]).cpu().numpy()      # one read
        at = 2 * ch + 4 * depth
        _check_plan(back[2 * ch:at], sets, what)
        if back[at] != 0:
            raise L.PccError(f"{what}: the blocks, vectors or matches of the cloud are inconsistent")
        root = [quantise(int(back[c]) - int(back[ch + c]), steps[c]) for c in range(ch)]
        modes = back[at + 1:at + 1 + nb]
        side = choose_members(back[at + 1 + nb:])
        ph.mark("select_hist_choose_ms")
        d_side = torch.tensor(side, dtype=torch.int32, device=dev)
        _inter_index(masks, offs, sets, depth, first, ch, bargs, d_mode, d_side, idx, None, None, rows, L.ptr(d_flag))
        body = _rans_body(coef_p, idx, rows * ch, segment_symbols, dev, what)          # one read: size + container
        ph.mark("index_rans_ms")
        out = _stream(WIDE_LOSSY_MAGIC if search > G.MAX_SEARCH else INTER_LOSSY_MAGIC, (n, depth, ch, int(colour), qp, cqo, G.BLOCK_LOG2, search, nb),
                      root, side, modes, body)
        intra = None
        if mode == "auto":
            for magic in ([MAGIC] if not predict else [PRED_MAGIC] if predict is True else [MAGIC, PRED_MAGIC]):
                sym, v_root = (coef, v_child) if magic == MAGIC else _predicted_rows(sets, offs, values, depth, ch, h_steps, rows)
                dc, side0, body0 = _intra_tail(what, sets, masks, offs, checks, sym, v_root, depth, ch, rows, segment_symbols, dev, G.Phases(False))
                data = _stream(magic, (n, depth, ch, int(colour), qp, cqo), [quantise(q, st) for q, st in zip(dc, steps)], side0, None, body0)
                intra = data if intra is None or len(data) < len(intra) else intra
            ph.mark("intra_stream_ms")
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["inter_stages_ms"] = ph.report()
            timings["inter_bytes"], timings["intra_bytes"] = len(out), (len(intra) if intra is not None else None)
            timings["mode1_blocks"], timings["blocks"] = int(modes.sum()), nb
            timings["host_reads_by_construction"] = (6 if predict == "auto" else 4) if mode == "auto" else 2   # beyond those of building the level sets
    return out if intra is None or len(out) < len(intra) else intra


@torch.no_grad()
def encode_attributes(cloud, qp, chroma_qp_offset=-2, colour=True, attrs=None, segment_symbols=SEGMENT_SYMBOLS, timings=None,
                      reference=None, reference_attrs=None, mode="auto", search=None, predict=None):
    """[N, 6] GPU tensor (xyz, then rgb in [0, 1]: colours become round(255 c)), or a pitch-1 CoordSet / [N, >= 3] rows with
    `attrs` uint8 [N, C], 1 <= C <= 8 -> bytes.  Any row order (attributes follow their rows into canonical order; a set's
    attributes are in the set's order).  Duplicate voxels, CPU tensors and batched input raise PccError.  colour: the integer
    BT.709 transform in front of the RAHT (three channels only).  segment_symbols: symbols per rANS stream (tests lower it).
    timings: a dict that receives per-stage device events (tools/anchor_rd.py, tools/anchor_inter_timing.py).
    reference: a cloud the decoder holds too, with the levels the DECODER holds (the previous frame as decoded) -- [M, 6], or a
    pitch-1 set / [M, >= 3] rows with `reference_attrs` uint8 [M, C] in its row order; distinct voxels, the cloud's channel
    count.  mode "auto": the shorter of the inter (0xB4) and the intra (0xB3) stream, intra on a tie and at depth 15 -- by
    stream length alone: against an unrelated reference the shorter stream may decode to a lower PSNR than the intra one
    (DESIGN.md 7f); "inter": the inter stream (fewer than two voxels still travel as intra; depth 15 raises); "intra", or no
    reference: today's stream byte for byte.  search: the range of the block vectors the inter stream's matches come from --
    None or 2: 0xB4 as ever; 3 .. 7: the stream 0xB8, the 0xB4 layout with that range in its header (no vector travels: the
    decoder re-runs the wide search).
    predict: the form of the INTRA stream wherever one is produced (no reference, mode "intra", the intra candidate of mode
    "auto"; the inter streams are untouched).  None / False: 0xB3, today's bytes; True: 0xB9, every coefficient predicted from
    the parent level in a closed loop (fewer than two voxels still travel as 0xB3); "auto": the shorter of the two, 0xB3 on a
    tie -- by stream length alone.  The closed loop costs a second pass over the levels; the decoder needs no argument."""
    what = "encode_attributes"
    predict = _check_predict(what, predict)
    search = _colour_search(search, what)
    cs, levels, perm, ref, depth, inter = _encoder_input(what, cloud, attrs, reference, reference_attrs, mode, True, chroma_qp_offset)
    qp, cqo = min(max(int(qp), QP_MIN), QP_MAX), int(chroma_qp_offset)
    n, ch, dev = cs.n, levels.shape[1], cs.device
    colour = bool(colour) and ch == 3
    if n == 0:
        return _stream(MAGIC, (0, 0, ch, int(colour), qp, cqo), [0] * ch)
    if inter:
        return _encode_inter_lossy(what, cs, levels, perm, ref, qp, cqo, colour, mode, segment_symbols, timings, search, predict)
    steps = steps_for(qp, cqo, ch)
    h_steps = (C.c_int32 * ch)(*steps)
    rows = n - 1
    with torch.cuda.device(dev):
        ph = G.Phases(timings is not None)
        sets = G.level_sets(cs, tuple(cs.bounds.lo), depth)
        ph.mark()
        values = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_raht_prepare", L.ptr(levels), L.ptr(perm), n, ch, int(colour), L.ptr(values), L.stream())
        masks, offs, checks = _plan(sets, depth, dev)
        ph.mark("prepare_plan")
        out = None
        for magic in ([MAGIC] if not predict or not rows else [PRED_MAGIC] if predict is True else [MAGIC, PRED_MAGIC]):
            if magic == MAGIC:
                coef = torch.zeros((max(rows, 1), ch), dtype=torch.int32, device=dev)
                v_root = _forward_pass(sets, offs, values, depth, ch, h_steps, coef, rows)[0]
                ph.mark("forward")
            else:
                coef, v_root = _predicted_rows(sets, offs, values, depth, ch, h_steps, rows)
                ph.mark("forward_predict")
            root, side, body = _intra_tail(what, sets, masks, offs, checks, coef, v_root, depth, ch, rows, segment_symbols, dev, ph)
            data = _stream(magic, (n, depth, ch, int(colour), qp, cqo), [quantise(q, st) for q, st in zip(root, steps)], side, None, body)
            out = data if out is None or len(data) < len(out) else out
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["stages_ms"] = ph.report()
            timings["stages_ms"].setdefault("index_rans", 0.0)             # (a single voxel has no rows to code)
            timings["host_reads_by_construction"] = (4 if predict == "auto" else 2) if rows else 1   # beyond those of building the level sets
    return out


def _decoder_input(what, hdr, geometry, device, reference, reference_attrs):
    """(canonical set of the geometry on the GPU, the reference rows of an inter stream or None) of both decoders; refuses a
    reference an inter stream cannot use, a geometry off the GPU and one whose n or depth are not the header's."""
    ref = _reference_rows(reference, reference_attrs, hdr["channels"], True, what) if hdr["inter"] else None
    if torch.is_tensor(geometry) and device is not None:
        geometry = geometry.to(device)
    cs = G.canonical_rows(geometry, what)[0]
    if cs.device.type != "cuda" or (device is not None and torch.device(device).type != "cuda"):
        raise L.PccError(f"{what} runs on a GPU (no CPU fallback)")
    n, depth = hdr["n"], hdr["depth"]
    if cs.n != n or (n and _depth_of(cs) != depth):
        raise L.PccError(f"{what}: the stream codes {n} points at depth {depth}, the geometry has {cs.n} at depth "
                         f"{_depth_of(cs) if cs.n else 0}")
    return cs, ref


def _decoder_plan(cs, depth, ch, ph):
    """What both decoders build from the geometry alone: (level sets, masks, offsets and checks of `_plan`, int32 weights per
    level, the status words rANS status | clamp flag, the zeroed coefficient rows)."""
    dev = cs.device
    ph.mark("start")
    sets = G.level_sets(cs, tuple(cs.bounds.lo), depth)
    ph.mark("level_sets_ms")
    masks, offs, checks = _plan(sets, depth, dev)
    weights = [None] * (depth + 1)                                          # the voxels weigh 1: no array
    for l in range(depth - 1, -1, -1):
        weights[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
        L.call("pcc_raht_weights", *_level_args(sets[l], sets[l + 1]), L.ptr(weights[l + 1]), L.ptr(weights[l]), L.stream())
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    coef = torch.zeros(max(cs.n - 1, 1) * ch, dtype=torch.int32, device=dev)
    ph.mark("plan_weights_ms")
    return sets, masks, offs, checks, weights, status, coef


def _block_modes(data, hdr, blocks, dev):
    """int32 mode per block of an inter stream, from the header's mode bytes."""
    m0, m1 = hdr["modes"]
    bits = np.unpackbits(np.frombuffer(data, np.uint8, m1 - m0, m0), bitorder="little")[:blocks]
    return torch.from_numpy(bits.astype(np.int32)).to(dev)


def _decoder_read(what, name, left, status, checks, sets, ph, timings):
    """The decode's one device->host read and what it refuses: a geometry that does not expand level by level, a malformed
    container, a value that `left` its range.  name: the stream's name in the refusals."""
    back = torch.cat([status, checks.reshape(-1)]).cpu().numpy()
    if timings is not None:
        torch.cuda.synchronize(status.device)
        timings["stages_ms"] = ph.report()
    _check_plan(back[2:], sets, what)
    if back[0] != 0:
        raise L.PccError(f"{name}: malformed rANS container (status {int(back[0])})")
    if back[1] != 0:
        raise L.PccError(f"{name}: {left}")


@torch.no_grad()
def decode_attributes(data, geometry, device=None, reference=None, reference_attrs=None, timings=None):
    """bytes + the block's geometry (the pitch-1 CoordSet `decode_geometry(..., as_set=True)` returns, or [n, >= 3] rows) ->
    uint8 [n, C] in the canonical order `decode_geometry` returns.  device=None: the geometry's.  reference, reference_attrs:
    the reference cloud `encode_attributes` was given; an inter stream (0xB4) needs it with its levels, an intra stream (0xB3, or
    0xB9: coefficients predicted from the parent level, rebuilt level by level from the root) ignores it.  For an inter stream
    the decoder re-runs the motion search and the matching, forms the prediction's transform from the reference it was handed,
    compares the header's block count with the geometry's and sizes every buffer from the geometry.  Raises PccError on
    a malformed stream, on a stream whose n, depth or block count differ from the geometry's, and on a payload that does not
    decode; never returns anything but exactly [n, C].  timings: a dict that receives per-stage device events
    (tools/anchor_inter_timing.py); asking for them adds a synchronisation at the end."""
    what = "decode_attributes"
    hdr = parse_header(data, have_reference=reference is not None)
    inter = hdr["inter"]
    cs, ref = _decoder_input(what, hdr, geometry, device, reference, reference_attrs)
    dev = cs.device
    n, depth, ch, steps = hdr["n"], hdr["depth"], hdr["channels"], hdr["steps"]
    if n == 0:
        return torch.empty((0, ch), dtype=torch.uint8, device=dev)
    h_steps = (C.c_int32 * ch)(*steps)
    rows = n - 1
    with torch.cuda.device(dev):
        ph = G.Phases(timings is not None)
        sets, masks, offs, checks, weights, status, coef = _decoder_plan(cs, depth, ch, ph)
        first, hp, p_root = depth, None, None
        if inter:
            first = max(0, depth - G.BLOCK_LOG2)
            if hdr["blocks"] != sets[first].n:
                raise L.PccError(f"{what}: the stream codes {hdr['blocks']} blocks, the geometry has {sets[first].n}")
            flag = status.data_ptr() + 4
            bargs, nb, match, tv, nr, _keep = _inter_state(cs, sets, tuple(cs.bounds.lo), depth, ref, ch, hdr["colour"], flag,
                                                           "pcc_raht_prepare", hdr["search"])
            d_mode = _block_modes(data, hdr, nb, dev)
            ph.mark("motion_match_ms")
            # the prediction's transform: P with the mode-0 blocks zeroed, then the same forward pass, rows left unquantised
            fill_sums = torch.empty((nb, ch + 1), dtype=torch.int32, device=dev)
            p_child = torch.empty((n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_raht_inter_fill", L.ptr(sets[depth].keys), n, *bargs, L.ptr(match), L.ptr(tv), nr, ch, L.ptr(d_mode), L.ptr(fill_sums),
                   L.ptr(p_child), flag, L.stream())
            hp = torch.zeros(rows * ch, dtype=torch.int32, device=dev)
            for l in range(depth - 1, -1, -1):
                p = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
                L.call("pcc_raht_inter_predict", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(p_child), ch,
                       L.ptr(p), L.ptr(hp), sets[l].n - 1, rows, L.stream())
                p_child = p
            p_root = p_child
            ph.mark("fill_predict_ms")
        if rows:
            b0, b1 = hdr["payload"]
            d_buf = torch.from_numpy(R.stage(data, [(b0, b1)])[0]).to(dev)
            d_side = torch.tensor(hdr["side"], dtype=torch.int32, device=dev)
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            if inter:
                _inter_index(masks, offs, sets, depth, first, ch, bargs, d_mode, d_side, idx, None, None, rows, status.data_ptr() + 4)
            else:
                _fill_index(masks, offs, sets, depth, ch, d_side, idx, rows)
            R.decode(_tables(dev), d_buf, b1 - b0, idx, rows * ch, 1, 1, hdr["streams"], coef, status.data_ptr())
        ph.mark("index_rans_ms")
        v = torch.tensor([[q * s for q, s in zip(hdr["dc"], steps)]], dtype=torch.int32, device=dev)
        predicted, m = bool(hdr.get("predict")), None
        if predicted:                                       # 0xB9: the root's DC as it stands (q * step again) and its mean
            root, m = v, torch.empty((1, ch), dtype=torch.int32, device=dev)
            v = torch.empty((1, ch), dtype=torch.int32, device=dev)
            L.call("pcc_raht_pred_root", L.ptr(root), n, ch, h_steps, L.ptr(v), L.ptr(m), status.data_ptr() + 4, L.stream())
        for l in range(depth):
            cv = torch.zeros((sets[l + 1].n, ch), dtype=torch.int32, device=dev)
            if predicted:
                cm = torch.empty((sets[l + 1].n, ch), dtype=torch.int32, device=dev) if l + 1 < depth else None
                L.call("pcc_raht_pred_inverse", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v),
                       L.ptr(m), ch, h_steps, L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), L.ptr(cm), status.data_ptr() + 4, L.stream())
                m = cm
            elif inter:
                L.call("pcc_raht_inter_inverse", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v),
                       L.ptr(p_root) if l == 0 else None, ch, h_steps, L.ptr(coef), L.ptr(hp), sets[l].n - 1, rows, L.ptr(cv),
                       status.data_ptr() + 4, L.stream())
            else:
                L.call("pcc_raht_inverse", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v), ch, h_steps,
                       L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), status.data_ptr() + 4, L.stream())
            v = cv
        out = torch.empty((n, ch), dtype=torch.uint8, device=dev)
        L.call("pcc_raht_finish", L.ptr(v), n, ch, int(hdr["colour"]), L.ptr(out), L.stream())
        ph.mark("inverse_finish_ms")
        _decoder_read(what, "attribute stream", "a coefficient or a reconstructed value left the +-2^30 range", status, checks, sets, ph,
                      timings)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the lossless coder: the same levels, rows, groups, family and container; a reversible arithmetic
# ------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encode_attributes_lossless(cloud, colour=True, attrs=None, predict=True, segment_symbols=SEGMENT_SYMBOLS, timings=None,
                               reference=None, reference_attrs=None, mode="auto", search=None):
    """The input forms and refusals of `encode_attributes` -> bytes that `decode_attributes_lossless` turns back into the very
    uint8 levels (colours of an [N, 6] cloud become round(255 c) first).  colour: YCoCg-R in front of the lifting (three
    channels only).  predict: code every butterfly against its prediction from the parent level.  When the coded stream would
    be longer than header + n * C bytes, the raw levels are stored instead.  timings: a dict that receives per-stage device
    events (tools/lossless_timing.py, tools/lossless_inter_timing.py).
    reference: a cloud the decoder holds too -- [M, 6], or a pitch-1 set / [M, >= 3] rows with `reference_attrs` uint8 [M, C]
    in its row order; distinct voxels, the cloud's channel count, predict=True.  mode "auto": the shorter of the inter (0xB6)
    and the intra (0xB5) stream, intra on a tie and at depth 15 -- never longer than without a reference; "inter": the inter
    stream (fewer than two voxels still travel as intra; depth 15 raises); "intra", or no reference: today's stream byte for
    byte.  search: the range of the block vectors the matches come from -- None or 2: 0xB6 as ever; 3 .. 7: the stream 0xB7, the
    0xB6 layout with that range in its header (no vector travels: the decoder re-runs the wide search)."""
    what = "encode_attributes_lossless"
    search = _colour_search(search, what)
    cs, levels, perm, ref, depth, inter = _encoder_input(what, cloud, attrs, reference, reference_attrs, mode, bool(predict))
    n, ch, dev = cs.n, levels.shape[1], cs.device
    colour, predict = bool(colour) and ch == 3, bool(predict)
    if n == 0:
        return _stream(LOSSLESS_MAGIC, (0, 0, ch, F_STORED))
    origin = tuple(cs.bounds.lo)
    rows = n - 1
    with torch.cuda.device(dev):
        ph = G.Phases(timings is not None)          # the stages of every stream, and under the key "inter" those only an inter stream has
        sets = G.level_sets(cs, origin, depth)
        if inter:
            ph.mark(None, "inter")
            d_flag = torch.zeros(1, dtype=torch.int32, device=dev)
            bargs, nb, match, tv, nr, _keep = _inter_state(cs, sets, origin, depth, ref, ch, colour, L.ptr(d_flag), search=search)
            ph.mark("motion_match_ms", "inter")
        ph.mark()
        values = torch.empty((n, ch), dtype=torch.int32, device=dev)
        L.call("pcc_lift_prepare", L.ptr(levels), L.ptr(perm), n, ch, int(colour), L.ptr(values), L.stream())
        masks, offs, checks = _plan(sets, depth, dev)
        ph.mark("prepare_plan")
        coef = torch.zeros((max(rows, 1), ch), dtype=torch.int32, device=dev)
        w, v = [None] * (depth + 1), [None] * depth + [values]
        for l in range(depth - 1, -1, -1):
            w[l] = torch.empty(sets[l].n, dtype=torch.int32, device=dev)
            v[l] = torch.empty((sets[l].n, ch), dtype=torch.int32, device=dev)
            L.call("pcc_lift_forward", *_level_args(sets[l], sets[l + 1]), L.ptr(offs[l]), L.ptr(w[l + 1]), L.ptr(v[l + 1]), ch, L.ptr(w[l]),
                   L.ptr(v[l]), L.ptr(coef), sets[l].n - 1, rows, L.stream())
        ph.mark("forward")
        last = depth - 1
        if predict and rows:
            for l in range(last if inter else depth):
                L.call("pcc_lift_residual", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(w[l + 1]), L.ptr(v[l]), ch,
                       L.ptr(coef), sets[l].n - 1, rows, L.stream())
        if inter:                                                          # the last level: both residual sets, coef as the intra coder's
            coef_t = torch.empty((rows - (sets[last].n - 1), ch), dtype=torch.int32, device=dev)
            sums = torch.empty((nb, 2), dtype=torch.int32, device=dev)
            L.call("pcc_lift_inter_residual", *_node_level_args(sets[last], sets[depth], last == 0), *bargs, L.ptr(offs[last]), L.ptr(v[last]),
                   ch, L.ptr(match), L.ptr(tv), nr, L.ptr(coef), L.ptr(coef_t), sets[last].n - 1, rows, L.ptr(sums), L.ptr(d_flag), L.stream())
        ph.mark("residual")
        out, stored = None, False
        if not inter or mode == "auto":
            root, side, body = _intra_tail(what, sets, masks, offs, checks, coef, v[0], depth, ch, rows, segment_symbols, dev, ph)
            out = _stream(LOSSLESS_MAGIC, (n, depth, ch, (F_COLOUR if colour else 0) | (F_PREDICT if predict else 0)), root, side, None, body)
            stored = len(out) > LOSSLESS_HEADER.size + n * ch
            if stored:                                                     # a third read, of the raw levels, in this case alone
                raw = levels if perm is None else levels[perm]
                out = _stream(LOSSLESS_MAGIC, (n, depth, ch, F_STORED), body=raw.cpu().numpy().tobytes())
        if inter:
            # the select pass: modes from the block sums, the temporal rows of mode-1 blocks into coef, their rows into the groups
            # of level `depth`; then the members, the member index and the container as above
            ph.mark(None, "inter")
            groups = (depth + 1) * 6
            node = sets[last]
            d_mode = torch.empty(nb, dtype=torch.int32, device=dev)
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            hist = torch.empty(groups * N_SLOTS, dtype=torch.int32, device=dev)
            sel = (L.ptr(node.keys), L.ptr(masks[last]), L.ptr(offs[last]), node.n, last, ch, *bargs)
            _fill_index(masks, offs, sets, last, ch, None, idx, rows)
            L.call("pcc_lift_inter_select", *sel, L.ptr(sums), L.ptr(d_mode), None, L.ptr(idx), L.ptr(coef), L.ptr(coef_t), node.n - 1, rows,
                   L.ptr(d_flag), L.stream())
            L.call("pcc_raht_hist", L.ptr(coef), L.ptr(idx), rows * ch, groups, L.ptr(hist), L.stream())
            back = torch.cat([v[0].reshape(-1), checks.reshape(-1), d_flag, d_mode, hist]).cpu().numpy()      # one read
            _check_plan(back[ch:ch + 4 * depth], sets, what)
            at = ch + 4 * depth
            if back[at] != 0:
                raise L.PccError(f"{what}: the blocks, vectors or matches of the cloud are inconsistent")
            modes = back[at + 1:at + 1 + nb]
            side = choose_members(back[at + 1 + nb:])
            ph.mark("select_hist_choose_ms", "inter")
            d_side = torch.tensor(side, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, last, ch, d_side, idx, rows)
            L.call("pcc_lift_inter_select", *sel, None, L.ptr(d_mode), L.ptr(d_side), L.ptr(idx), None, None, node.n - 1, rows, L.ptr(d_flag),
                   L.stream())
            body = _rans_body(coef, idx, rows * ch, segment_symbols, dev, what)          # one read: size + container
            ph.mark("inter_index_rans_ms", "inter")
            coded = _stream(WIDE_MAGIC if search > G.MAX_SEARCH else INTER_MAGIC,
                            (n, depth, ch, F_PREDICT | (F_COLOUR if colour else 0), G.BLOCK_LOG2, search, nb), back[:ch], side, modes, body)
            if timings is not None:
                timings["inter_bytes"], timings["intra_bytes"] = len(coded), (len(out) if out is not None else None)
                timings["mode1_blocks"], timings["blocks"] = int(modes.sum()), nb
            if out is None or len(coded) < len(out):
                out = coded
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["stages_ms"] = ph.report()
            if not inter or mode == "auto":
                timings["stages_ms"].setdefault("index_rans", 0.0)         # (a single voxel has no rows to code)
                timings["host_reads_by_construction"] = (2 if rows else 1) + int(stored)   # beyond those of building the level sets
                timings["stored"] = stored
            if inter:
                timings["inter_stages_ms"] = ph.report("inter")
    return out


@torch.no_grad()
def decode_attributes_lossless(data, geometry, device=None, reference=None, reference_attrs=None, timings=None):
    """bytes + the block's geometry (the pitch-1 CoordSet `decode_geometry(..., as_set=True)` returns, or [n, >= 3] rows) ->
    uint8 [n, C] in the canonical order `decode_geometry` returns: the levels the encoder was given.  device=None: the
    geometry's.  reference, reference_attrs: the reference cloud `encode_attributes_lossless` was given; an inter stream (0xB6)
    needs it with its colours, an intra stream ignores it.  The decoder re-runs the motion search and the matching on the
    geometry, compares the header's block count with the geometry's and sizes every buffer from the geometry.  Raises PccError
    on a malformed stream, on a stream whose n, depth or block count differ from the geometry's, and on a payload that does not
    decode to legal values; never returns anything but exactly [n, C].  timings: a dict that receives per-stage device events
    (tools/lossless_inter_timing.py); asking for them adds a synchronisation at the end."""
    what = "decode_attributes_lossless"
    hdr = parse_lossless_header(data, have_reference=reference is not None)
    inter = hdr["inter"]
    cs, ref = _decoder_input(what, hdr, geometry, device, reference, reference_attrs)
    dev = cs.device
    n, depth, ch, colour, predict = hdr["n"], hdr["depth"], hdr["channels"], hdr["colour"], hdr["predict"]
    if n == 0:
        return torch.empty((0, ch), dtype=torch.uint8, device=dev)
    if hdr["stored"]:
        b0, b1 = hdr["raw"]
        return torch.from_numpy(np.frombuffer(data, np.uint8, b1 - b0, b0).reshape(n, ch).copy()).to(dev)
    rows = n - 1
    with torch.cuda.device(dev):
        ph = G.Phases(timings is not None)
        sets, masks, offs, checks, weights, status, coef = _decoder_plan(cs, depth, ch, ph)
        last = depth - 1
        if inter:
            if hdr["blocks"] != sets[max(0, depth - G.BLOCK_LOG2)].n:
                raise L.PccError(f"{what}: the stream codes {hdr['blocks']} blocks, the geometry has {sets[max(0, depth - G.BLOCK_LOG2)].n}")
            bargs, nb, match, tv, nr, _keep = _inter_state(cs, sets, tuple(cs.bounds.lo), depth, ref, ch, colour, status.data_ptr() + 4,
                                                           search=hdr["search"])
            d_mode = _block_modes(data, hdr, nb, dev)
            ph.mark("motion_match_ms")
        if rows:
            b0, b1 = hdr["payload"]
            d_buf = torch.from_numpy(R.stage(data, [(b0, b1)])[0]).to(dev)
            d_side = torch.tensor(hdr["side"], dtype=torch.int32, device=dev)
            idx = torch.empty(rows * ch, dtype=torch.int32, device=dev)
            _fill_index(masks, offs, sets, last if inter else depth, ch, d_side, idx, rows)
            if inter:
                L.call("pcc_lift_inter_select", L.ptr(sets[last].keys), L.ptr(masks[last]), L.ptr(offs[last]), sets[last].n, last, ch, *bargs,
                       None, L.ptr(d_mode), L.ptr(d_side), L.ptr(idx), None, None, sets[last].n - 1, rows, status.data_ptr() + 4, L.stream())
            R.decode(_tables(dev), d_buf, b1 - b0, idx, rows * ch, 1, 1, hdr["streams"], coef, status.data_ptr())
        ph.mark("index_rans_ms")
        v = torch.tensor([hdr["root"]], dtype=torch.int32, device=dev)
        for l in range(depth):
            cv = torch.zeros((sets[l + 1].n, ch), dtype=torch.int32, device=dev)
            if inter and l == last:
                L.call("pcc_lift_inter_inverse", *_node_level_args(sets[l], sets[l + 1], l == 0), *bargs, L.ptr(d_mode), L.ptr(offs[l]), L.ptr(v),
                       ch, int(colour), L.ptr(match), L.ptr(tv), nr, L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), status.data_ptr() + 4,
                       L.stream())
            else:
                L.call("pcc_lift_inverse", *_node_level_args(sets[l], sets[l + 1], l == 0), L.ptr(offs[l]), L.ptr(weights[l + 1]), L.ptr(v),
                       ch, int(colour), int(predict), L.ptr(coef), sets[l].n - 1, rows, L.ptr(cv), status.data_ptr() + 4, L.stream())
            v = cv
        out = torch.empty((n, ch), dtype=torch.uint8, device=dev)
        L.call("pcc_lift_finish", L.ptr(v), n, ch, int(colour), L.ptr(out), status.data_ptr() + 4, L.stream())
        ph.mark("inverse_finish_ms")
        _decoder_read(what, "lossless attribute stream", "a symbol, a reconstructed value or a level left its legal range", status, checks,
                      sets, ph, timings)
    return out
