"""GPU suite: PLY bodies read and written on the device (unified_point_cloud_compression_amd/ply.py, csrc/pcc_ply.hip) against
the numpy restatement tests/ply_ref.py, bit for bit.

The two tile sizes of the kernels are read from the library: TILE body bytes per workgroup of the ASCII token passes, and
block_records(stride) records per workgroup of the binary reader.  The sizes 0 / 1 / 257 / 4099 are: nothing to launch, one
row, one row past a workgroup's 256 threads, and (asserted below) more than one workgroup of every kernel with a partial
last one; the ASCII bodies are shifted so that chosen bytes land exactly on a multiple of TILE."""
import numpy as np
import pytest
import torch

from tests import ply_ref as R
from tests.util import dev, n as to_np
from unified_point_cloud_compression_amd import lib, ply
from unified_point_cloud_compression_amd.lib import PccError

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 257, 4099)
TILE = lib.load().pcc_ply_tile_bytes()


def block_records(stride):
    return lib.load().pcc_ply_block_records(stride)


def bits_equal(got, want):
    got = to_np(got) if torch.is_tensor(got) else got
    return got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_read(data, extra=(), normals=True, source=None):
    """read_ply of `data` (as bytes, or through a file when `source` is a path) equals the restatement bit for bit."""
    if source is not None:
        source.write_bytes(data)
    pc = ply.read_ply(str(source) if source is not None else data, dev(), extra=extra, normals=normals)
    cloud, nrm, ext = R.read(data, extra=extra, normals=normals)
    assert pc.cloud.dtype == torch.float32 and pc.cloud.is_contiguous() and pc.cloud.data_ptr() % 8 == 0
    assert bits_equal(pc.cloud, cloud), "cloud"
    assert (pc.normals is None) == (nrm is None)
    if nrm is not None:
        assert bits_equal(pc.normals, nrm), "normals"
    assert sorted(pc.extra) == sorted(ext)
    for k in ext:
        assert pc.extra[k].shape == (cloud.shape[0],) and bits_equal(pc.extra[k].contiguous(), ext[k]), k
    return pc


# ---- binary read ---------------------------------------------------------------------------------------------------
F3 = [("x", "float"), ("y", "float"), ("z", "float")]
RGB = [("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
LAYOUTS = {
    "xyz_rgb_15": (F3 + RGB, 15, ()),
    "normals_between_27": (F3 + [("nx", "float"), ("ny", "float"), ("nz", "float")] + RGB, 27, ()),
    # doubles at odd byte offsets 1, 9, 17; G-PCC's colour order; two extras
    "double_gpcc_30": ([("alpha", "uchar"), ("x", "double"), ("y", "double"), ("z", "double"), ("reflectance", "ushort"),
                        ("green", "uchar"), ("blue", "uchar"), ("red", "uchar")], 30, ("reflectance", "alpha")),
    "int_xyz_rgb_15": ([("x", "int"), ("y", "int"), ("z", "int")] + RGB, 15, ()),
}


def binary_file(props, n, big, seed):
    rng = np.random.default_rng(seed)
    order = ">" if big else "<"
    arr = np.zeros(n, dtype=np.dtype([(name, order + R.NP_TYPE[t]) for name, t in props]))
    for name, t in props:
        k = R.NP_TYPE[t]
        if k == "f8":
            arr[name] = rng.uniform(-5000, 5000, n)                 # not fp32 values: the rounding is checked
        elif k == "f4":
            arr[name] = rng.uniform(-1100, 1100, n).astype(np.float32)
        elif k == "i4":
            arr[name] = rng.integers(-2 ** 31, 2 ** 31, n)          # above 2^24: round to nearest
        else:
            info = np.iinfo(k)
            arr[name] = rng.integers(info.min, info.max + 1, n)
    head = "ply\nformat binary_%s_endian 1.0\ncomment binary test\nelement vertex %d\n" % ("big" if big else "little", n)
    head += "".join("property %s %s\n" % (t, name) for name, t in props) + "end_header\n"
    return head.encode() + arr.tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("big", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_binary_read(layout, big, n, tmp_path):
    props, stride, extra = LAYOUTS[layout]
    rb = block_records(stride)
    assert 1 < rb < SIZES[-1] and SIZES[-1] % rb != 0                # 4099 records: several workgroups, the last one partial
    data = binary_file(props, n, big, seed=n + 7 * big)
    pc = check_read(data, extra=extra, source=tmp_path / "b.ply")
    assert pc.header.stride == stride and pc.cloud.shape == (n, 6)
    assert (pc.normals is not None) == (layout == "normals_between_27")
    if layout == "double_gpcc_30" and n:                             # colours were mapped by name
        raw = np.frombuffer(data[pc.header.body_offset:], dtype=np.uint8).reshape(n, 30)
        assert np.array_equal(np.rint(to_np(pc.cloud)[:, 3:] * 255).astype(np.uint8), raw[:, [29, 27, 28]])


def test_binary_read_ignores_face_data_and_skips_normals():
    props, _, _ = LAYOUTS["normals_between_27"]
    data = binary_file(props, 300, False, 3)
    data = data.replace(b"end_header\n", b"element face 1\nproperty list uchar int vertex_indices\nend_header\n") + b"\x03" + b"\0" * 12
    pc = check_read(data, normals=False)
    assert pc.normals is None and pc.cloud.shape == (300, 6)


def test_uchar_colour_levels_are_true_quotients():
    props = F3 + RGB
    arr = np.zeros(256, dtype=np.dtype([(name, "<" + R.NP_TYPE[t]) for name, t in props]))
    arr["red"] = arr["green"] = arr["blue"] = np.arange(256)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 256\n" + "".join(f"property {t} {nm}\n" for nm, t in props) + "end_header\n"
    pc = ply.read_ply(head.encode() + arr.tobytes(), dev())
    want = np.array([np.float32(k / 255.0) for k in range(256)], dtype=np.float32)
    for c in range(3, 6):
        assert bits_equal(pc.cloud[:, c].contiguous(), want)


# ---- ASCII read ----------------------------------------------------------------------------------------------------
ASCII_PROPS = F3 + RGB
ASCII_HEAD = "ply\nformat ascii 1.0\nelement vertex %d\n" + "".join(f"property {t} {nm}\n" for nm, t in ASCII_PROPS) + "end_header\n"
SPECIAL = ["-0", "+7", "007", "1.", ".5", "1e3", "2.5E-3", "123.000000", "123456789012345e22", "1.23456789012345e-8",
           "123456789012345e-22", "-9.99999999999999E+22", "0.000", "16777217", "-1023", "1e-22", "1E22"]


def ascii_lines(n, seed):
    """n vertex lines: float-typed coordinates drawn from plain integers, decimals and the special tokens; uchar colours."""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        xyz = []
        for a in range(3):
            kind = (i + a) % 4
            if kind == 0:
                xyz.append(SPECIAL[(i // 4 + a) % len(SPECIAL)])
            elif kind == 1:
                xyz.append(str(int(rng.integers(0, 1024))))
            elif kind == 2:
                xyz.append("%.6f" % rng.uniform(-2000, 2000))
            else:
                xyz.append("%.9e" % (rng.uniform(1, 9.9) * rng.choice([-1, 1]) * 10.0 ** int(rng.integers(-12, 12))))   # 10^-21 .. 10^2 after the point
        lines.append(" ".join(xyz + [str(int(v)) for v in rng.integers(0, 256, 3)]))
    return lines


def shifted_body(lines, kind):
    """The lines as a body whose byte at offset TILE is the first byte of a token ("start"), a byte inside a token
    ("middle") or a line end ("newline"): the first line is padded with blanks."""
    body = "\n".join(lines) + "\n"
    for i in range(len(lines[0]) + 1, min(TILE, len(body) - 1)):        # any position after the first line will do
        c, before, after = body[i], body[i - 1], body[i + 1]
        if {"start": c not in " \n" and before in " \n", "middle": c not in " \n" and before not in " \n" and after not in " \n",
                "newline": c == "\n"}[kind]:
            out = " " * (TILE - i) + body
            assert len(out) > TILE and out[TILE] == c
            return out
    raise AssertionError("body too short to reach a tile boundary")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["start", "middle", "newline"])
def test_ascii_read_tile_boundaries(n, kind, tmp_path):
    lines = ascii_lines(n, seed=n)
    body = shifted_body(lines, kind) if n >= 257 else "".join(ln + "\n" for ln in lines)
    if n >= 257:
        assert len(body) > TILE + 16, "more than one pass-1 tile"
    if n == SIZES[-1]:
        assert len(body) > 8 * TILE and n * len(ASCII_PROPS) > 256      # many tiles; several workgroups of the token pass
    pc = check_read((ASCII_HEAD % n).encode() + body.encode(), source=tmp_path / "a.ply")
    assert pc.fallback_count == 0 and not pc.host_path                 # ordinary tokens never take the fallback
    assert pc.cloud.shape == (n, 6)


def test_ascii_read_layouts():
    """CRLF, tabs, blank lines, two vertices on one line, one vertex over two lines, no final newline, face lines after
    the vertices, and every special token."""
    lines = ascii_lines(80, seed=5)
    toks = [ln.split() for ln in lines]
    body = "  \t" + lines[0] + "\r\n"
    body += "\t".join(toks[1]) + "\r\n\r\n\n"
    body += lines[2] + "   " + lines[3] + "\n"                            # two vertices on one line
    body += " ".join(toks[4][:2]) + "\n" + " ".join(toks[4][2:]) + " \t \n"  # one vertex over two lines
    body += "".join(ln + "\r\n" for ln in lines[5:40]) + "\n".join(lines[40:]) + "\n"
    body += "3 0 1 2\n3 1 2 3"                                            # faces, no final newline
    head = (ASCII_HEAD % 80).replace("end_header\n", "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    pc = check_read(head.encode() + body.encode())
    assert pc.fallback_count == 0
    seen = {t for row in toks for t in row[:3]}
    assert set(SPECIAL) <= seen
    no_newline = (ASCII_HEAD % 2).replace("\n", "\r\n") + "1 2 3 4 5 6\r\n-7 8e0 9. 255 0 1"
    pc = check_read(no_newline.encode())
    assert to_np(pc.cloud)[1].tolist()[:3] == [-7.0, 8.0, 9.0]


def test_ascii_read_integer_coordinates_and_extras():
    head = ("ply\nformat ascii 1.0\nelement vertex 3\nproperty int x\nproperty int y\nproperty int z\nproperty float nx\n"
            "property float ny\nproperty float nz\nproperty uchar blue\nproperty uchar red\nproperty uchar green\n"
            "property ushort refl\nend_header\n")
    body = "-0 +7 007 0.5 -.5 1e0 0 128 255 65535\n2147483647 -2147483648 16777217 0 0 1 1 2 3 0\n1 2 3 1 0 0 255 254 253 9\n"
    pc = check_read((head + body).encode(), extra=("refl",))
    assert pc.normals is not None and to_np(pc.cloud)[0, :3].tolist() == [0.0, 7.0, 7.0]


FALLBACK_TOKENS = ["12345678901234567", "0.12345678901234567", "-1234567890.1234567", "1234567890123456789012", "3.14159265358979323846",
                   "1.0000000000000000001e5", "99999999999999999e-3", "nan", "inf"]


def fallback_file():
    lines = [ln.split() for ln in ascii_lines(600, seed=11)]
    where = [(0, 0), (5, 1), (77, 2), (255, 0), (256, 1), (400, 2), (599, 2), (300, 0), (301, 1)]   # known (vertex, axis)
    for (v, a), tok in zip(where, FALLBACK_TOKENS):
        lines[v][a] = tok
    return (ASCII_HEAD % 600).encode() + "".join(" ".join(ln) + "\n" for ln in lines).encode(), where


def test_ascii_fallback_tokens_are_converted_by_the_host():
    data, where = fallback_file()
    cloud, _, _ = R.read(data)
    pc = ply.read_ply(data, dev())
    assert pc.fallback_count == 9 and not pc.host_path
    got = to_np(pc.cloud)
    assert np.array_equal(got, cloud, equal_nan=True)
    ok = ~np.isnan(cloud)
    assert np.array_equal(got.view(np.uint32)[ok], cloud.view(np.uint32)[ok])
    assert np.isnan(got[300, 0]) and np.isinf(got[301, 1]) and got[0, 0] == np.float32(12345678901234567.0)


def test_ascii_fallback_overflow_takes_the_host_path(monkeypatch):
    data, _ = fallback_file()
    cloud, _, _ = R.read(data)
    monkeypatch.setattr(ply, "FALLBACK_CAPACITY", 4)
    pc = ply.read_ply(data, dev())
    assert pc.fallback_count == 9 and pc.host_path
    got = to_np(pc.cloud)
    assert np.array_equal(got, cloud, equal_nan=True)
    ok = ~np.isnan(cloud)
    assert np.array_equal(got.view(np.uint32)[ok], cloud.view(np.uint32)[ok])


# ---- errors: bounded reads of bad data ---------------------------------------------------------------------------------
def still_usable():
    pc = check_read((ASCII_HEAD % 2).encode() + b"1 2 3 4 5 6\n7 8 9 10 11 12\n")
    assert pc.cloud.shape == (2, 6)
    torch.cuda.synchronize()


def test_error_ascii_body_one_token_short():
    lines = ascii_lines(300, seed=2)
    body = "\n".join(lines)
    body = body[:body.rindex(" ")]                                         # drops the last token
    with pytest.raises(PccError) as e:
        ply.read_ply((ASCII_HEAD % 300).encode() + body.encode(), dev())
    assert "1799" in str(e.value) and "1800" in str(e.value)
    still_usable()


def test_error_token_that_is_no_number_names_vertex_and_property():
    lines = [ln.split() for ln in ascii_lines(300, seed=3)]
    lines[3][1] = "12x4"
    with pytest.raises(PccError) as e:
        ply.read_ply((ASCII_HEAD % 300).encode() + "".join(" ".join(ln) + "\n" for ln in lines).encode(), dev())
    assert "vertex 3" in str(e.value) and "'y'" in str(e.value) and "12x4" in str(e.value)
    still_usable()


def test_error_decimal_point_in_uchar_property():
    lines = [ln.split() for ln in ascii_lines(300, seed=4)]
    lines[290][4] = "12."
    with pytest.raises(PccError) as e:
        ply.read_ply((ASCII_HEAD % 300).encode() + "".join(" ".join(ln) + "\n" for ln in lines).encode(), dev())
    assert "vertex 290" in str(e.value) and "'green'" in str(e.value)
    still_usable()


def test_error_binary_body_one_byte_short():
    props, _, _ = LAYOUTS["xyz_rgb_15"]
    data = binary_file(props, 300, False, 1)
    with pytest.raises(PccError):
        ply.read_ply(data[:-1], dev())
    L = lib.load()                                                       # the C entry point refuses it too, before any launch
    body = torch.zeros(4499, dtype=torch.uint8, device=dev())
    out = torch.zeros((300, 6), device=dev())
    table = ply._table(ply._select(ply.read_ply_header(data), (), True)[0], 1)
    assert L.pcc_ply_unpack_binary(lib.ptr(body), 4499, 300, 15, table, 6, 0, lib.ptr(out), 6, None, None, 0, None) == -1
    table[0] = 12                                                        # a float at bytes [12, 16) of a 15-byte record
    assert L.pcc_ply_unpack_binary(lib.ptr(body), 4499, 299, 15, table, 6, 0, lib.ptr(out), 6, None, None, 0, None) == -1
    still_usable()


# ---- write ------------------------------------------------------------------------------------------------------------
COORDS = [0, -1, 9, 10, -9, -10, 99, 100, 99999, 100000, -99999, 2 ** 24 - 1, -(2 ** 24 - 1), 5, 1023, 1024]


def write_cloud(n, colours=True):
    """Integer coordinates over the digit-count edges; colours over all 256 levels, their neighbourhoods and the clamp."""
    i = np.arange(n)
    xyz = np.stack([np.array(COORDS)[(i + s) % len(COORDS)] for s in (0, 5, 11)], axis=1).astype(np.float32)
    if not colours:
        return xyz
    k = (np.float32(1) * (i % 256)) / np.float32(255.0)
    pool = np.stack([k, k + np.float32(1e-4), k - np.float32(1e-4)], axis=1).astype(np.float32)
    pool[i % 7 == 3, 1] = 1.2
    pool[i % 7 == 5, 2] = -0.1
    return np.concatenate([xyz, pool], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", ["binary", "binary_normals", "binary_int", "ascii_float", "ascii_int", "ascii_xyz_only", "binary_xyz_only"])
def test_write_equals_the_restatement(n, variant, tmp_path):
    assert SIZES[-1] > 256 and SIZES[-1] % 256 != 0                      # the writers take 256 rows per workgroup
    cloud = write_cloud(n, colours="xyz_only" not in variant)
    nrm = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32) if variant == "binary_normals" else None
    kw = dict(ascii=variant.startswith("ascii"), coords="int" if variant.endswith("_int") else "float")
    path = tmp_path / "w.ply"
    ply.write_ply(str(path), torch.from_numpy(cloud).to(dev()), normals=None if nrm is None else torch.from_numpy(nrm).to(dev()), **kw)
    want = R.write(cloud, normals=nrm, **kw)
    got = path.read_bytes()
    assert len(got) == len(want) and got == want
    if n and not kw["ascii"]:
        assert (len(got) - ply.read_ply_header(got).body_offset) // n == {"binary": 15, "binary_int": 15, "binary_normals": 27, "binary_xyz_only": 12}[variant]


def test_write_float_coordinates_need_not_be_integers(tmp_path):
    cloud = np.random.default_rng(0).uniform(-100, 100, (300, 6)).astype(np.float32)
    ply.write_ply(str(tmp_path / "f.ply"), torch.from_numpy(cloud).to(dev()))
    assert (tmp_path / "f.ply").read_bytes() == R.write(cloud)


@pytest.mark.parametrize("kw", [dict(coords="int"), dict(ascii=True), dict(ascii=True, coords="int")], ids=["binary_int", "ascii_float", "ascii_int"])
@pytest.mark.parametrize("bad", [0.5, float("nan"), 3e9])
def test_write_refuses_non_integral_coordinates(kw, bad, tmp_path):
    cloud = write_cloud(700)
    cloud[613, 1] = bad
    with pytest.raises(PccError):
        ply.write_ply(str(tmp_path / "x.ply"), torch.from_numpy(cloud).to(dev()), **kw)
    still_usable()


def test_write_refuses_ascii_normals_and_bad_arguments(tmp_path):
    x = torch.from_numpy(write_cloud(4)).to(dev())
    with pytest.raises(PccError):
        ply.write_ply(str(tmp_path / "x.ply"), x, normals=torch.zeros((4, 3), device=dev()), ascii=True)
    with pytest.raises(PccError):
        ply.write_ply(str(tmp_path / "x.ply"), x.cpu())
    with pytest.raises(PccError):
        ply.write_ply(str(tmp_path / "x.ply"), x, coords="double")


# ---- round trips -------------------------------------------------------------------------------------------------------
def decoded_like(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, 1024, (n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.float32) / np.float32(255.0)
    return np.concatenate([xyz, rgb], axis=1).astype(np.float32)


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
@pytest.mark.parametrize("coords", ["float", "int"])
def test_round_trip_is_bit_equal(ascii, coords, tmp_path):
    x = decoded_like(4099, 1)
    x[:256, 3] = np.arange(256, dtype=np.float32) / np.float32(255.0)     # every level
    path = str(tmp_path / "r.ply")
    ply.write_ply(path, torch.from_numpy(x).to(dev()), ascii=ascii, coords=coords)
    pc = ply.read_ply(path, dev())
    assert bits_equal(pc.cloud, x) and pc.fallback_count == 0


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
def test_compress_of_a_read_file_equals_compress_of_its_source(ascii, tmp_path):
    import copy
    from oracle import codec
    from tests.util import load_params
    from unified_point_cloud_compression_amd import synth
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = copy.deepcopy(codec.small_config())
    cfg["entropy_model"]["entropy_coder"] = "pcc_streams"
    model = load_params(UnifiedModel(cfg), codec.random_params(cfg, 0, gain=4.0)).to(dev()).eval()
    model.update()
    pc = synth.random_block(0, 64, 0.05)
    pc[:, 3:] = np.rint(pc[:, 3:] * 255).astype(np.float32) / np.float32(255.0)      # a decoded-like cloud: 8-bit colour levels
    x = torch.from_numpy(pc).to(dev())
    q = torch.tensor([[0.5, 0.5]], device=dev())
    path = str(tmp_path / "c.ply")
    ply.write_ply(path, x, ascii=ascii)
    y = ply.read_ply(path, dev()).cloud
    assert y.data_ptr() % 8 == 0 and y.is_contiguous() and torch.equal(x, y)
    a, b = model.compress(x, q), model.compress(y, q)
    assert len(a[0]) == 1                                                     # one block: the intake fast path
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])
