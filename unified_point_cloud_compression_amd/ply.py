"""PLY point clouds in and out (`evaluate.py:30-37,105`, `data/utils/RawLoader.py:47`, `utils.save_ply`, `model.py:409` of the
reference go through PLY at every edge).  The header -- small and irregular -- is parsed and written here in Python; the body
is converted on the device (`csrc/pcc_ply.hip`): binary records of any layout and either endianness, and ASCII bodies read as
a stream of whitespace-separated tokens, the way rply reads them.

ASCII numbers are converted on the device only where that is exact arithmetic (integers; decimals of at most 15 significant
digits with a power of ten within +-22).  Every other token is handed back and converted here with `float()`, so the result
is `np.float32(float(token))` for every token either way; `FALLBACK_CAPACITY` bounds how many the device hands back before
the whole body is converted here instead.
"""
import ctypes as C
import os
import re
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import lib as L
from .lib import PccError

FALLBACK_CAPACITY = 65536
HEADER_LIMIT = 64 * 1024
MAX_PROPS = 32
FORMATS = ("ascii", "binary_little_endian", "binary_big_endian")
# name -> (PCC_PLY_* code, bytes)
TYPES = {"char": (0, 1), "uchar": (1, 1), "short": (2, 2), "ushort": (3, 2), "int": (4, 4), "uint": (5, 4), "float": (6, 4),
         "double": (7, 8), "int8": (0, 1), "uint8": (1, 1), "int16": (2, 2), "uint16": (3, 2), "int32": (4, 4), "uint32": (5, 4),
         "float32": (6, 4), "float64": (7, 8)}
_RANGE = {0: (-128, 127), 1: (0, 255), 2: (-32768, 32767), 3: (0, 65535), 4: (-2 ** 31, 2 ** 31 - 1), 5: (0, 2 ** 32 - 1)}
COLOUR_NAMES = (("red", "green", "blue"), ("r", "g", "b"), ("diffuse_red", "diffuse_green", "diffuse_blue"))
NORMAL_NAMES = (("nx", "ny", "nz"), ("normal_x", "normal_y", "normal_z"))
_INT_RE = re.compile(rb"[+-]?[0-9]+\Z")
_FLOAT_RE = re.compile(rb"[+-]?(([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?|nan|inf|infinity)\Z", re.I)
_WS_RE = re.compile(rb"[ \t\r\n]+")                      # PLY whitespace, as the kernels see it

PlyHeader = namedtuple("PlyHeader", "format n_vertex properties stride body_offset")
PlyCloud = namedtuple("PlyCloud", "cloud normals extra header fallback_count host_path")


def read_ply_header(data):
    """Header of a PLY file from its first bytes (pure Python).  `properties` are the vertex element's (name, type) in file
    order, `stride` the bytes of a binary vertex record (None for ascii), `body_offset` the first byte after `end_header`."""
    head = bytes(data[:HEADER_LIMIT])
    m = re.search(rb"(?:\A|\n)end_header\r?\n", head)
    lines = head[:m.start() if m else len(head)].split(b"\n")
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    if lines[0].strip() != b"ply":
        raise PccError(f"not a PLY file: the first line is {lines[0][:40]!r}, not 'ply'")
    if m is None:
        raise PccError(f"PLY header: no 'end_header' line within the first {HEADER_LIMIT} bytes")
    fmt, n_vertex, props, element, n_elements = None, None, [], None, 0
    for raw in lines[1:]:
        line = raw.decode("latin-1")
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            if len(w) != 3 or w[1] not in FORMATS or w[2] != "1.0" or fmt is not None:
                raise PccError(f"PLY header: unsupported format line {line!r}")
            fmt = w[1]
        elif w[0] == "element":
            count = int(w[2]) if len(w) == 3 and re.fullmatch(r"[0-9]+", w[2]) else None
            if count is None:
                raise PccError(f"PLY header: element count is not a non-negative integer: {line!r}")
            if n_elements == 0 and w[1] != "vertex":
                raise PccError(f"PLY header: 'vertex' must be the first element: {line!r}")
            if n_elements > 0 and w[1] == "vertex":
                raise PccError(f"PLY header: a second vertex element: {line!r}")
            element, n_elements = w[1], n_elements + 1
            if element == "vertex":
                n_vertex = count
        elif w[0] == "property":
            if element is None:
                raise PccError(f"PLY header: property before any element: {line!r}")
            if element != "vertex":
                continue                                   # later elements (faces): their data is never read
            if len(w) >= 2 and w[1] == "list":
                raise PccError(f"PLY header: list property in the vertex element: {line!r}")
            if len(w) != 3:
                raise PccError(f"PLY header: malformed property line {line!r}")
            if w[1] not in TYPES:
                raise PccError(f"PLY header: unknown type in {line!r}")
            if any(w[2] == name for name, _ in props):
                raise PccError(f"PLY header: property named twice: {line!r}")
            if len(props) == MAX_PROPS:
                raise PccError(f"PLY header: more than {MAX_PROPS} vertex properties: {line!r}")
            props.append((w[2], w[1]))
        else:
            raise PccError(f"PLY header: unknown line {line!r}")
    if fmt is None:
        raise PccError("PLY header: no format line")
    if n_vertex is None:
        raise PccError("PLY header: no vertex element")
    names = [name for name, _ in props]
    for axis in "xyz":
        if axis not in names:
            raise PccError(f"PLY header: the vertex element has no property '{axis}' (it has: {' '.join(names) or 'none'})")
    stride = None if fmt == "ascii" else sum(TYPES[t][1] for _, t in props)
    return PlyHeader(fmt, n_vertex, tuple(props), stride, m.end())


def _select(header, extra, normals):
    """[(property index, byte offset, name, type code, array, column, scale)] of the properties to read, by NAME."""
    names = [name for name, _ in header.properties]
    offsets = np.cumsum([0] + [TYPES[t][1] for _, t in header.properties]).tolist()
    sel = []

    def take(name, arr, col, colour=False):
        p = names.index(name)
        code = TYPES[header.properties[p][1]][0]
        if colour and code not in (1, 6, 7):
            raise PccError(f"PLY colour '{name}' has type {header.properties[p][1]}; uchar, float or double colours are read")
        sel.append((p, offsets[p], name, code, arr, col, int(colour and code == 1)))

    for c, axis in enumerate("xyz"):
        take(axis, 0, c)
    colours = next((fam for fam in COLOUR_NAMES if all(nm in names for nm in fam)), None)
    for c, nm in enumerate(colours or ()):
        take(nm, 0, 3 + c, colour=True)
    fam_n = next((fam for fam in NORMAL_NAMES if all(nm in names for nm in fam)), None) if normals else None
    for c, nm in enumerate(fam_n or ()):
        take(nm, 1, c)
    extra = tuple(extra)
    for c, nm in enumerate(extra):
        if nm not in names:
            raise PccError(f"PLY file has no vertex property '{nm}' (it has: {' '.join(names)})")
        if any(nm == s[2] for s in sel):
            raise PccError(f"extra property '{nm}' is already read (as a coordinate, colour, normal or earlier extra)")
        take(nm, 2, c)
    return sel, 6 if colours else 3, fam_n is not None, extra


def _table(sel, where):
    flat = [v for s in sel for v in (s[where], s[3], s[4], s[5], s[6])]
    return (C.c_int32 * len(flat))(*flat)


def _upload(buf, start, stop, device):
    """Bytes [start, stop) of a host buffer as a device tensor of their own (so its base is aligned whatever `start` is)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (a read-only buffer: it is only ever copied from)
        host = torch.frombuffer(buf, dtype=torch.uint8, count=stop - start, offset=start)
    return host.to(device)


def _host_value(tok, code, what):
    """`float32(float(token))` of one token under the device's grammar, or PccError."""
    if code < 6:
        if not _INT_RE.match(tok) or not _RANGE[code][0] <= int(tok) <= _RANGE[code][1]:
            raise PccError(f"PLY body: {tok[:48]!r} is not a value of an integer property ({what})")
        return np.float32(int(tok))
    if not _FLOAT_RE.match(tok):
        raise PccError(f"PLY body: {tok[:48]!r} is not a number ({what})")
    return np.float32(float(tok))


def _token(view, at):
    """The token that starts at byte `at` of the body."""
    m = _WS_RE.search(view, at)
    return bytes(view[at:m.start() if m else len(view)])


def _where(header, t):
    P = len(header.properties)
    return f"vertex {t // P}, property '{header.properties[t % P][0]}'"


def _parse_on_host(header, body, sel, outs):
    """The whole ASCII body converted here (the device's fallback list overflowed): same tokens, same values."""
    P, n = len(header.properties), header.n_vertex
    toks = [t for t in _WS_RE.split(body) if t]
    if len(toks) < n * P:
        raise PccError(f"PLY body: {len(toks)} values, {n} vertices of {P} properties need {n * P}")
    for p, _, _, code, arr, col, scale in sel:
        v = np.array([_host_value(toks[i * P + p], code, _where(header, i * P + p)) for i in range(n)], dtype=np.float32)
        if scale:
            v = v / np.float32(255.0)
        t = torch.from_numpy(v).to(outs[arr].device)
        if arr == 2:
            outs[2][col].copy_(t)
        else:
            outs[arr][:, col].copy_(t)


def _unpack_binary(header, body, sel, outs):
    """Queues the conversion of an uploaded binary body into `outs` = (cloud, normals, extra)."""
    L.call("pcc_ply_unpack_binary", L.ptr(body), body.numel(), header.n_vertex, header.stride, _table(sel, 1), len(sel),
           int(header.format == "binary_big_endian"), L.ptr(outs[0]), outs[0].shape[1], L.ptr(outs[1]), L.ptr(outs[2]),
           0 if outs[2] is None else outs[2].shape[0], L.stream())


def _parse_ascii(header, body, sel, outs):
    """Queues the token passes over an uploaded ASCII body; returns the device state (4 status words, then the fallback
    list) without reading it."""
    n, P, device = header.n_vertex, len(header.properties), body.device
    nb = body.numel()
    tile = L.load().pcc_ply_tile_bytes()
    counts = torch.zeros((nb + tile - 1) // tile, dtype=torch.int32, device=device)
    L.call("pcc_ply_count_tokens", L.ptr(body), nb, L.ptr(counts), L.stream())
    base = torch.cumsum(counts, 0, dtype=torch.int32) - counts            # exclusive scan of the tiles
    starts = torch.empty(n * P, dtype=torch.int32, device=device)
    cap = int(FALLBACK_CAPACITY)
    state = torch.empty(4 + 2 * cap, dtype=torch.int64, device=device)    # status words, then the fallback list
    L.call("pcc_ply_parse_ascii", L.ptr(body), nb, n, P, _table(sel, 0), len(sel), L.ptr(base), L.ptr(starts), L.ptr(outs[0]),
           outs[0].shape[1], L.ptr(outs[1]), L.ptr(outs[2]), 0 if outs[2] is None else outs[2].shape[0], state.data_ptr(),
           state.data_ptr() + 32, cap, L.stream())
    return state


def _finish_ascii(header, view, state, sel, outs):
    """Reads the status words (the one device->host read of an ordinary file), raises on bad data, and converts what the
    device handed back; `view` is the body on the host.  Returns (fallback count, whether the whole body took the host path)."""
    n, P, device = header.n_vertex, len(header.properties), state.device
    cap = (state.numel() - 4) // 2
    tokens, n_fallback, err, _ = state[:4].tolist()
    if tokens < n * P:
        raise PccError(f"PLY body: {tokens} values, {n} vertices of {P} properties need {n * P}")
    if err != -1:
        t, at = err >> 32, err & 0xFFFFFFFF
        tok = _token(view, at)
        raise PccError(f"PLY body: {tok[:48]!r} is not a number of type {header.properties[t % P][1]} ({_where(header, t)})")
    if n_fallback > cap:
        _parse_on_host(header, bytes(view), sel, outs)
        return n_fallback, True
    if n_fallback:
        by_prop = {s[0]: s for s in sel}
        rows = {0: [], 1: [], 2: []}
        for t, at in state[4:4 + 2 * n_fallback].view(-1, 2).tolist():
            _, _, _, code, arr, col, scale = by_prop[t % P]
            v = _host_value(_token(view, at), code, _where(header, t))
            v = v / np.float32(255.0) if scale else v
            flat = col * n + t // P if arr == 2 else (t // P) * outs[arr].shape[1] + col
            rows[arr].append((flat, v))
        for arr, items in rows.items():
            if items:
                idx = torch.tensor([i for i, _ in items], dtype=torch.int64, device=device)
                val = torch.from_numpy(np.array([v for _, v in items], dtype=np.float32)).to(device)
                outs[arr].view(-1)[idx] = val
    return n_fallback, False


def read_ply(path_or_bytes, device, extra=(), normals=True):
    """A PLY file (path, or its bytes) as device tensors: `.cloud` float32 [N,6] (x y z r g b, colours in [0,1]) or [N,3] when
    the file has no colours; `.normals` [N,3] or None; `.extra[name]` [N] for the names asked for; `.header`.  Properties are
    found by name, in any order.  Integer types and double round to the nearest fp32; uchar colours become k / 255."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        buf = path_or_bytes
    else:
        with open(path_or_bytes, "rb") as f:
            buf = bytearray(os.fstat(f.fileno()).st_size)
            f.readinto(buf)
    header = read_ply_header(buf)
    sel, cols, has_normals, extra = _select(header, extra, normals)
    device = torch.device(device)
    n = header.n_vertex
    binary = header.format != "ascii"
    if binary and header.body_offset + n * header.stride > len(buf):
        raise PccError(f"PLY body: {n} records of {header.stride} bytes need {n * header.stride} bytes, the file holds "
                       f"{len(buf) - header.body_offset}")
    if device.type != "cuda":
        raise PccError("read_ply converts the body on the GPU (no CPU fallback): pass a cuda device")
    with torch.cuda.device(device):
        cloud = torch.empty((n, cols), dtype=torch.float32, device=device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=device) if has_normals else None
        ext = torch.empty((len(extra), n), dtype=torch.float32, device=device) if extra else None
        n_fallback, host_path = 0, False
        outs, off = (cloud, nrm, ext), header.body_offset
        if n > 0 and binary:
            _unpack_binary(header, _upload(buf, off, off + n * header.stride, device), sel, outs)   # later elements are not uploaded
        elif n > 0:
            body = _upload(buf, off, len(buf), device) if len(buf) > off else torch.empty(0, dtype=torch.uint8, device=device)
            state = _parse_ascii(header, body, sel, outs)
            n_fallback, host_path = _finish_ascii(header, memoryview(buf)[off:], state, sel, outs)
    return PlyCloud(cloud, nrm, {nm: ext[c] for c, nm in enumerate(extra)}, header, n_fallback, host_path)


def ply_header_text(n, colours, normals=False, ascii=False, coords="float"):
    """The header `write_ply` writes, as bytes."""
    if coords not in ("float", "int"):
        raise PccError(f"coords is 'float' or 'int', not {coords!r}")
    lines = ["ply", "format ascii 1.0" if ascii else "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property {coords} {a}" for a in "xyz"]
    if normals:
        lines += [f"property float {a}" for a in ("nx", "ny", "nz")]
    if colours:
        lines += [f"property uchar {a}" for a in ("red", "green", "blue")]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, cloud, normals=None, ascii=False, coords="float"):
    """A GPU float32 [N,3] or [N,6] cloud (what `decompress` returns) as a PLY file.  Colours are written as uchar
    clamp(rint(255 f), 0, 255).  Binary (little-endian): records x y z [nx ny nz] [r g b], coordinates float or, with
    coords='int', int32.  ascii=True: one vertex per line, coordinates as integers under either `coords` (the header then
    says float or int accordingly: `utils.save_ply`'s file has a float header over integer text).  Coordinates that have to
    be integers and are not raise PccError."""
    if not (torch.is_tensor(cloud) and cloud.is_cuda and cloud.dtype == torch.float32 and cloud.dim() == 2 and cloud.shape[1] in (3, 6)):
        raise PccError("write_ply takes a GPU float32 tensor of shape [N,3] or [N,6]")
    n, cols = int(cloud.shape[0]), int(cloud.shape[1])
    if normals is not None:
        if ascii:
            raise PccError("write_ply: normals are written in binary files only")
        if not (torch.is_tensor(normals) and normals.is_cuda and normals.dtype == torch.float32 and tuple(normals.shape) == (n, 3)):
            raise PccError("write_ply: normals must be a GPU float32 tensor of shape [N,3]")
        normals = normals.contiguous()
    header = ply_header_text(n, cols == 6, normals is not None, ascii, coords)
    cloud = cloud.contiguous()
    body = None
    not_integral = PccError("write_ply: a coordinate is not an integer (of int32 range); coords='int' and ascii=True need integers")
    with torch.cuda.device(cloud.device):
        if n > 0 and ascii:
            flag = torch.empty(1, dtype=torch.int32, device=cloud.device)
            lengths = torch.empty(n, dtype=torch.int32, device=cloud.device)
            L.call("pcc_ply_row_lengths", L.ptr(cloud), cols, n, L.ptr(lengths), L.ptr(flag), L.stream())
            offs = torch.zeros(n + 1, dtype=torch.int64, device=cloud.device)
            offs[1:] = torch.cumsum(lengths, 0, dtype=torch.int64)
            total, bad = torch.cat([offs[-1:], flag.to(torch.int64)]).tolist()    # size and flag in one read
            if bad:
                raise not_integral
            out = torch.empty(total, dtype=torch.uint8, device=cloud.device)
            L.call("pcc_ply_format_ascii", L.ptr(cloud), cols, n, L.ptr(offs), L.ptr(out), total, L.stream())
            body = out.cpu()
        elif n > 0:
            stride = 12 + (12 if normals is not None else 0) + (3 if cols == 6 else 0)
            flag = torch.empty(1, dtype=torch.int32, device=cloud.device)
            out = torch.empty(n * stride, dtype=torch.uint8, device=cloud.device)
            L.call("pcc_ply_pack_binary", L.ptr(cloud), cols, L.ptr(normals), n, int(coords == "int"), L.ptr(out), out.numel(),
                   L.ptr(flag), L.stream())
            if coords == "int" and flag.item():
                raise not_integral
            body = out.cpu()
    with open(path, "wb") as f:
        f.write(header)
        if body is not None:
            f.write(memoryview(body.numpy()))
