"""Plain numpy / Python restatement of PLY reading and writing (the yardstick of tests/test_*_ply.py and the CPU column of
tools/ply_timing.py).  It shares no code with unified_point_cloud_compression_amd/ply.py: its own header parser, binary
bodies through `np.frombuffer` with a structured dtype, ASCII bodies as `body.split()` with `int()` / `float()` per token,
writers with `struct.pack` / "%d"."""
import struct

import numpy as np

NP_TYPE = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
           "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
COLOURS = [("red", "green", "blue"), ("r", "g", "b"), ("diffuse_red", "diffuse_green", "diffuse_blue")]
NORMALS = [("nx", "ny", "nz"), ("normal_x", "normal_y", "normal_z")]


def parse_header(data):
    """{'format', 'n', 'props': [(name, type)], 'offset'} of the vertex element (files the tests build: always well-formed)."""
    end = data.index(b"end_header")
    offset = data.index(b"\n", end) + 1
    out = {"format": None, "n": None, "props": [], "offset": offset}
    in_vertex = False
    for line in data[:end].decode("ascii").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            out["format"] = w[1]
        elif w[0] == "element":
            in_vertex = w[1] == "vertex"
            if in_vertex:
                out["n"] = int(w[2])
        elif w[0] == "property" and in_vertex:
            out["props"].append((w[2], w[1]))
    return out


def _columns(h, data):
    """name -> float64-or-native numpy column of every vertex property."""
    n, props = h["n"], h["props"]
    body = data[h["offset"]:]
    if h["format"] == "ascii":
        toks = body.split()
        assert len(toks) >= n * len(props)
        cols = {}
        for p, (name, typ) in enumerate(props):
            conv = float if NP_TYPE[typ][0] == "f" else int
            cols[name] = np.array([conv(toks[i * len(props) + p]) for i in range(n)], dtype="f8" if conv is float else "i8")
        return cols
    order = "<" if h["format"] == "binary_little_endian" else ">"
    rec = np.dtype([(name, order + NP_TYPE[typ]) for name, typ in props])
    arr = np.frombuffer(body, dtype=rec, count=n)
    return {name: arr[name] for name, _ in props}


def read(data, extra=(), normals=True):
    """(cloud float32 [n, 3|6], normals float32 [n,3] or None, {name: float32 [n]}) of a PLY file's bytes."""
    h = parse_header(data)
    cols = _columns(h, data)
    types = dict(h["props"])
    f32 = {k: v.astype(np.float32) for k, v in cols.items()}            # round to nearest, from any type
    out = [f32[a] for a in "xyz"]
    fam = next((f for f in COLOURS if all(c in cols for c in f)), None)
    for c in fam or ():
        out.append(f32[c] / np.float32(255.0) if NP_TYPE[types[c]] == "u1" else f32[c])
    cloud = np.stack(out, axis=1).astype(np.float32).reshape(h["n"], len(out))
    fam_n = next((f for f in NORMALS if all(c in cols for c in f)), None) if normals else None
    nrm = np.stack([f32[c] for c in fam_n], axis=1).reshape(h["n"], 3) if fam_n else None
    return cloud, nrm, {k: f32[k] for k in extra}


def header_text(n, colours, normals=False, ascii=False, coords="float"):
    s = "ply\nformat %s 1.0\nelement vertex %d\n" % ("ascii" if ascii else "binary_little_endian", n)
    for a in "xyz":
        s += "property %s %s\n" % (coords, a)
    if normals:
        s += "property float nx\nproperty float ny\nproperty float nz\n"
    if colours:
        s += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    return (s + "end_header\n").encode("ascii")


def levels(rgb):
    """clamp(rint(255 f), 0, 255) in fp32, as the decoder's last step rounds colours."""
    return np.clip(np.rint(np.float32(255.0) * rgb.astype(np.float32)), 0, 255).astype(np.uint8)


def write(cloud, normals=None, ascii=False, coords="float"):
    """The file's bytes for a float32 [n, 3|6] cloud (integral coordinates where text or int coordinates are asked for)."""
    n, c = cloud.shape
    out = [header_text(n, c == 6, normals is not None, ascii, coords)]
    lv = levels(cloud[:, 3:]) if c == 6 else None
    for i in range(n):
        xyz = cloud[i, :3]
        if ascii:
            vals = [int(v) for v in xyz] + ([int(v) for v in lv[i]] if c == 6 else [])
            out.append((" ".join("%d" % v for v in vals) + "\n").encode("ascii"))
            continue
        rec = struct.pack("<3i", *[int(v) for v in xyz]) if coords == "int" else struct.pack("<3f", *xyz)
        if normals is not None:
            rec += struct.pack("<3f", *normals[i])
        if c == 6:
            rec += struct.pack("<3B", *lv[i])
        out.append(rec)
    return b"".join(out)
