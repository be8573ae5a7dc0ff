"""CPU suite: the PLY header parser and writer of unified_point_cloud_compression_amd/ply.py (pure Python, no GPU), against
the independent restatement tests/ply_ref.py."""
import pytest

from tests import ply_ref as R
from unified_point_cloud_compression_amd import ply
from unified_point_cloud_compression_amd.lib import PccError

SIZES = {"char": 1, "uchar": 1, "short": 2, "ushort": 2, "int": 4, "uint": 4, "float": 4, "double": 8, "int8": 1, "uint8": 1,
         "int16": 2, "uint16": 2, "int32": 4, "uint32": 4, "float32": 4, "float64": 8}


def header(fmt="ascii", n=3, props=(("x", "float"), ("y", "float"), ("z", "float")), before=(), after=(), eol="\n", magic="ply",
           fmt_line=None, end="end_header"):
    lines = [magic, fmt_line or f"format {fmt} 1.0", *before, f"element vertex {n}"]
    lines += [f"property {t} {name}" for name, t in props]
    return (eol.join([*lines, *after, end]) + eol).encode("ascii")


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_header_round_trip_formats_and_line_ends(fmt, eol):
    props = (("x", "double"), ("y", "double"), ("z", "double"), ("green", "uchar"), ("blue", "uchar"), ("red", "uchar"),
             ("reflectance", "ushort"))                                         # permuted colour order
    data = header(fmt, 12345, props, before=("comment made by a test", "obj_info 1 2 3"),
                  after=("element face 0", "property list uchar int vertex_indices"), eol=eol) + b"BODY"
    h = ply.read_ply_header(data)
    assert h.format == fmt and h.n_vertex == 12345 and h.properties == props
    assert h.stride == (None if fmt == "ascii" else 29)
    assert data[h.body_offset:] == b"BODY"
    r = R.parse_header(data)
    assert (r["format"], r["n"], tuple(r["props"]), r["offset"]) == (h.format, h.n_vertex, h.properties, h.body_offset)


def test_header_every_type_name_and_alias():
    names = list(SIZES)
    props = (("x", "float"), ("y", "float"), ("z", "float")) + tuple((f"p{i}", t) for i, t in enumerate(names))
    h = ply.read_ply_header(header("binary_little_endian", 1, props))
    assert h.properties == props and h.stride == 12 + sum(SIZES.values())
    for alias, base in (("int8", "char"), ("uint8", "uchar"), ("int16", "short"), ("uint16", "ushort"), ("int32", "int"),
                        ("uint32", "uint"), ("float32", "float"), ("float64", "double")):
        assert ply.TYPES[alias] == ply.TYPES[base] and ply.TYPES[base][1] == SIZES[base]
    assert len({ply.TYPES[t][0] for t in names}) == 8


def test_header_32_properties_are_accepted_and_zero_vertices():
    props = (("x", "float"), ("y", "float"), ("z", "float")) + tuple((f"p{i}", "uchar") for i in range(29))
    h = ply.read_ply_header(header("binary_big_endian", 0, props))
    assert len(h.properties) == 32 and h.n_vertex == 0 and h.stride == 41


XYZ = (("x", "float"), ("y", "float"), ("z", "float"))
REFUSALS = {
    "no ply magic": (header(magic="plx"), "plx"),
    "no end_header within 64 KB": (header(before=tuple("comment " + "x" * 100 for _ in range(700))), "end_header"),
    "no end_header at all": (header(end="end_of_header"), "end_header"),
    "vertex not the first element": (header(before=("element face 2", "property list uchar int vertex_indices")), "element face 2"),
    "list property inside vertex": (header(props=XYZ + (("uchar int vertex_indices", "list"),)), "property list uchar int vertex_indices"),
    "unknown type": (header(props=XYZ + (("a", "half"),)), "property half a"),
    "more than 32 vertex properties": (header(props=XYZ + tuple((f"p{i}", "uchar") for i in range(30))), "property uchar p29"),
    "negative count": (header(n=-3), "element vertex -3"),
    "non-integer count": (header(n="2.5"), "element vertex 2.5"),
    "missing z": (header(props=(("x", "float"), ("y", "float"), ("nz", "float"))), "'z'"),
    "missing x": (header(props=(("y", "float"), ("z", "float"))), "'x'"),
    "unknown format": (header(fmt_line="format binary_middle_endian 1.0"), "format binary_middle_endian 1.0"),
    "unknown version": (header(fmt_line="format ascii 2.0"), "format ascii 2.0"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_header_refusals_name_the_offending_line(case):
    data, needle = REFUSALS[case]
    with pytest.raises(PccError) as e:
        ply.read_ply_header(data)
    assert needle in str(e.value), str(e.value)


def test_refusals_launch_nothing(tmp_path):
    """read_ply on a bad header, and on a binary body one byte short, raises from the host checks: no device is asked for
    (the device argument here does not exist on any machine)."""
    with pytest.raises(PccError):
        ply.read_ply(header(magic="plx"), "cuda:63")
    p = tmp_path / "short.ply"
    p.write_bytes(header("binary_little_endian", 2) + b"\0" * 23)
    with pytest.raises(PccError) as e:
        ply.read_ply(str(p), "cuda:63")
    assert "24" in str(e.value) and "23" in str(e.value)
    with pytest.raises(PccError):
        ply.read_ply(header("binary_little_endian", 0), "cuda:63", extra=("alpha",))       # unknown extra name
    rgb_short = XYZ + (("red", "short"), ("green", "short"), ("blue", "short"))
    with pytest.raises(PccError):
        ply.read_ply(header("binary_little_endian", 0, rgb_short), "cuda:63")             # colours of another type


@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("normals,ascii", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("coords", ["float", "int"])
def test_written_header_equals_the_restatement(colours, normals, ascii, coords):
    for n in (0, 1, 787502):
        text = ply.ply_header_text(n, colours, normals, ascii, coords)
        assert text == R.header_text(n, colours, normals, ascii, coords)
        h = ply.read_ply_header(text)
        assert h.n_vertex == n and h.body_offset == len(text) and h.format == ("ascii" if ascii else "binary_little_endian")
        assert h.stride == (None if ascii else 12 + 12 * normals + 3 * colours)


def test_package_exports_ply():
    import unified_point_cloud_compression_amd as pkg
    assert pkg.read_ply is ply.read_ply and pkg.write_ply is ply.write_ply and pkg.read_ply_header is ply.read_ply_header
    assert pkg.ply is ply and {"read_ply", "write_ply", "read_ply_header"} <= set(pkg.__all__)


def test_tile_sizes_are_host_queries():
    from unified_point_cloud_compression_amd import lib
    L = lib.load()
    assert L.pcc_ply_tile_bytes() == 4096
    assert L.pcc_ply_block_records(15) == 1024 and L.pcc_ply_block_records(27) == 16384 // 27 and L.pcc_ply_block_records(30) == 546
    assert L.pcc_ply_block_records(0) == 0 and L.pcc_ply_block_records(256) == 64
