"""CPU suite: the lattice / grid-index types of the host layer (`sparse.Lattice`, `GridIndex`, `grid_args`).

Needs the built library for the pure host size query `pcc_grid_words` only (as tests/test_cpu_abi.py does); no kernel runs.
Every expected integer is written out by hand from the definitions: dims = (hi - lo) // pitch + 1 per axis,
cells = batches * dx * dy * dz, words = ceil(cells / 64) rounded up to an even number."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _S():
    from unified_point_cloud_compression_amd import sparse as S, lib as L
    return S, L


# bounds lo = (-8, -16, 8), hi = (24, 8, 40): extents 32, 24, 32
HEADERS = {
    (1, 0): ([-8, -16, 8, 33, 25, 33, 1, 1], 27225, 426),      # 27225 / 64 = 425.4 -> 426
    (2, 0): ([-8, -16, 8, 17, 13, 17, 2, 1], 3757, 60),        # 58.7 -> 59 -> 60
    (8, 0): ([-8, -16, 8, 5, 4, 5, 8, 1], 100, 2),             # 1.6 -> 2
    (1, 3): ([-8, -16, 8, 33, 25, 33, 1, 4], 108900, 1702),    # 1701.6 -> 1702
    (2, 3): ([-8, -16, 8, 17, 13, 17, 2, 4], 15028, 236),      # 234.8 -> 235 -> 236
    (8, 3): ([-8, -16, 8, 5, 4, 5, 8, 4], 400, 8),             # 6.25 -> 7 -> 8
}


@pytest.mark.parametrize("pitch,bmax", sorted(HEADERS))
def test_header_of_bounds_with_negative_lo(pitch, bmax):
    S, L = _S()
    want_h, want_cells, want_words = HEADERS[pitch, bmax]
    lat = S.Lattice.of(S.Bounds(bmax, (-8, -16, 8), (24, 8, 40)), pitch)
    assert list(lat.h) == want_h and len(lat.h) == 8
    assert lat.dims == tuple(want_h[3:6]) and lat.cells == want_cells
    assert lat.words == L.load().pcc_grid_words(lat.h) == want_words and lat.words % 2 == 0
    # the explicit form (the octree cube) gives the same object
    same = S.Lattice(want_h[0:3], want_h[3:6], pitch, bmax + 1)
    assert list(same.h) == want_h and (same.dims, same.cells, same.words) == (lat.dims, lat.cells, lat.words)


def test_strided_bounds_give_the_coarse_lattices():
    S, _ = _S()
    b = S.Bounds(1, (-7, -16, 3), (20, 9, 40))
    s4 = b.strided(4)                                              # floor towards -inf to multiples of 4
    assert (s4.bmax, s4.lo, s4.hi) == (1, (-8, -16, 0), (20, 8, 40))
    assert list(S.Lattice.of(s4, 4).h) == [-8, -16, 0, 8, 7, 11, 4, 2]
    s32 = b.strided(32)
    assert (s32.lo, s32.hi) == ((-32, -32, 0), (0, 0, 32))
    assert list(S.Lattice.of(s32, 32).h) == [-32, -32, 0, 2, 2, 2, 32, 2]
    assert b.strided(2).strided(4).lo == s4.lo and b.strided(2).strided(4).hi == s4.hi   # a chain may stride the root's bounds


@pytest.mark.parametrize("ksize,step,want", [
    (2, 1, [-8, -16, 8, 34, 26, 34, 1, 1]),         # even kernel: offsets 0 .. 1
    (3, 1, [-9, -17, 7, 35, 27, 35, 1, 1]),         # -1 .. 1
    (5, 1, [-10, -18, 6, 37, 29, 37, 1, 1]),        # -2 .. 2
    (2, 4, [-8, -16, 8, 10, 8, 10, 4, 1]),          # offsets 0 .. 4 at pitch 4: extents 36, 28, 36
    (3, 4, [-12, -20, 4, 11, 9, 11, 4, 1]),         # -4 .. 4: extents 40, 32, 40
    (5, 4, [-16, -24, 0, 13, 11, 13, 4, 1]),        # -8 .. 8: extents 48, 40, 48
])
def test_expanded_bounds_give_the_output_lattices(ksize, step, want):
    S, _ = _S()
    ob = S.Bounds(0, (-8, -16, 8), (24, 8, 40)).expanded(ksize, step)
    assert list(ob.lo) == want[0:3] and ob.bmax == 0
    lat = S.Lattice.of(ob, step)
    assert list(lat.h) == want and lat.cells == want[3] * want[4] * want[5]


def test_fits_flips_exactly_at_twelve_bytes_per_word(monkeypatch):
    S, _ = _S()
    lat = S.Lattice.of(S.Bounds(0, (-8, -16, 8), (24, 8, 40)), 1)
    assert lat.words == 426
    assert lat.fits(426 * 12) and not lat.fits(426 * 12 - 1) and lat.fits(426 * 12 + 1)
    assert lat.fits()                                             # the default is the module switch, read at call time
    monkeypatch.setattr(S, "GRID_MAX_BYTES", 426 * 12 - 1)
    assert not lat.fits()
    monkeypatch.setattr(S, "GRID_MAX_BYTES", 426 * 12)
    assert lat.fits()
    # 2^31 words or more never fit, whatever the byte limit (the kernels index words with 32 bits)
    huge = S.Lattice((0, 0, 0), (8192, 8192, 4096), 1, 1)
    assert huge.cells == 1 << 38 and huge.words == 1 << 32 and not huge.fits(1 << 60)
    edge = S.Lattice((0, 0, 0), (8192, 8192, 2048), 1, 1)
    assert edge.words == 1 << 31 and not edge.fits(1 << 60)
    below = S.Lattice((0, 0, 0), (8192, 8192, 2047), 1, 1)
    assert below.words == (1 << 31) - (1 << 20) and below.fits(1 << 60)


# ---- the one header decoder of the native side (pcc_lattice_from_host / pcc_grid_from_host in csrc/pcc_common.h) ------------
# Every entry point that takes the 8-int header refuses a bad one with PCC_EINVAL and an error that names the entry point and the
# lattice -- on the host, before any HIP call (this suite has no device: a HIP call would return PCC_EHIP).  Dummy pointers stand
# for the device arrays, as in tests/test_cpu_abi.py; nothing reads them.
GOOD_H = [-8, -16, 8, 3, 5, 7, 4, 2]
BAD_HEADERS = {
    "pitch 3": [-8, -16, 8, 3, 5, 7, 3, 2],
    "pitch 0": [-8, -16, 8, 3, 5, 7, 0, 2],
    "zero dim": [-8, -16, 8, 3, 0, 7, 4, 2],
    "zero batches": [-8, -16, 8, 3, 5, 7, 4, 0],
    "NULL header": None,
}


def _header_calls(L, p, h):
    """entry point -> call with header h (None: NULL), dummy pointer p for every array, sizes that pass the other checks"""
    big = 1 << 40
    return {
        "pcc_grid_build": lambda: L.pcc_grid_build(p, 10, h, p, p, p, big, None),
        "pcc_coords_stride_grid": lambda: L.pcc_coords_stride_grid(p, 10, None, h, p, p, p, p, p, big, None),
        "pcc_keys_canonicalize_grid": lambda: L.pcc_keys_canonicalize_grid(p, 10, h, p, p, p, p, p, p, big, None),
        "pcc_coords_expand_grid": lambda: L.pcc_coords_expand_grid(p, 10, 3, h, p, p, p, p, p, big, None),
        "pcc_coords_expand_grid_csr": lambda: L.pcc_coords_expand_grid_csr(p, 10, 3, 2, p, p, h, 10, p, p, p, p, big, None),
        "pcc_coords_expand_grid_csr_zk": lambda: L.pcc_coords_expand_grid_csr_zk(p, 10, 3, 2, p, p, h, 10, p, p, p, p, big, None),
        "pcc_coords_expand_grid_csr_slots": lambda: L.pcc_coords_expand_grid_csr_slots(p, 10, 5, 2, p, p, h, 10, p, p, p, p, 0, None),
        "pcc_coords_expand_csr": lambda: L.pcc_coords_expand_csr(p, 10, 3, 4, h, p, p, p, p, p, big, None),
        "pcc_kernel_map_build": lambda: L.pcc_kernel_map_build(p, 10, p, 10, 3, 4, 1, 0, p, p, None, None, p, p, h, p, big, None),
        "pcc_convt_fwd_csr_grid": lambda: L.pcc_convt_fwd_csr_grid(p, 10, 32, p, p, 8, 32, p, p, 10, p, p, 0, 0.0, p, p, p, h, p, None,
                                                                    0, None, None),
        "pcc_conv_thin_grid_fwd": lambda: L.pcc_conv_thin_grid_fwd(p, 10, 16, p, p, 1, p, p, p, h, p, p, big, None),
        "pcc_chconv_fwd": lambda: L.pcc_chconv_fwd(p, 10, p, 4, p, p, h, 4, p, 9, p, 27, 3, p, 4, p, 10, p, None),
        "pcc_chconv_wgrad": lambda: L.pcc_chconv_wgrad(p, 10, p, 4, p, p, h, 4, p, 9, p, 27, 3, p, 10, p, p, 4, p, big, None),
        "pcc_geom_occ_ctx": lambda: L.pcc_geom_occ_ctx(p, 10, 4, p, p, h, None, 0, None, None, None, None, p, None),
        "pcc_normals_grid": lambda: L.pcc_normals_grid(p, 10, p, h, 4, p, p, None),
        "pcc_curvature_grid": lambda: L.pcc_curvature_grid(p, 10, p, p, h, 4, p, None),
        "pcc_pcqm_features": lambda: L.pcc_pcqm_features(p, 10, p, p, h, 4, 0.5, p, p, None),
    }


@pytest.mark.parametrize("what", sorted(BAD_HEADERS))
def test_every_entry_point_refuses_a_bad_header_on_the_host(what):
    import ctypes
    from unified_point_cloud_compression_amd import lib
    L = lib.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    values = BAD_HEADERS[what]
    h = (ctypes.c_int32 * 8)(*values) if values is not None else None
    calls = _header_calls(L, p, h)
    assert len(calls) == 17
    for name, call in sorted(calls.items()):
        rc = call()
        err = L.pcc_last_error().decode()
        assert rc == -1, (name, what, rc, err)                                  # PCC_EINVAL
        assert err.startswith(name + ":") and "lattice" in err, (name, what, err)
    # the size query has no status to return: a refused header has no words
    assert L.pcc_grid_words(h) == 0 and L.pcc_last_error().decode().startswith("pcc_grid_words:")
    assert L.pcc_grid_words((ctypes.c_int32 * 8)(*GOOD_H)) == 4                  # 2 * 105 cells = 210 bits -> 4 words


def test_grid_index_is_a_three_tuple_and_grid_args_of_none():
    S, _ = _S()
    lat = S.Lattice((0, 0, 0), (4, 4, 4), 1, 1)
    bits, rank = torch.zeros(lat.words, dtype=torch.int64), torch.zeros(lat.words, dtype=torch.int32)
    g = S.GridIndex(bits, rank, lat.h)
    a, b, c = g
    assert a is bits and b is rank and c is lat.h
    assert g[0] is bits and g[1] is rank and g[2] is lat.h and len(g) == 3
    assert (g.bits, g.rank, g.h) == (bits, rank, lat.h) and bool(g)
    assert S.grid_args(None) == (None, None, None)


def test_the_package_builds_the_header_once_and_never_indexes_a_grid_index():
    pkg = os.path.join(ROOT, "unified_point_cloud_compression_amd")
    headers, indexed = [], []
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(d, f)
                for no, line in enumerate(open(path), 1):
                    if "(C.c_int32 * 8)(" in line:
                        headers.append((path, no))
                    if re.search(r"\b(g|grid|_grid)\[[012]\]", line):
                        indexed.append((path, no))
    assert [os.path.basename(p) for p, _ in headers] == ["sparse.py"], headers
    assert not indexed, indexed
