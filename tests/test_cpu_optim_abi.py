"""The host side of `csrc/pcc_optim.hip`: the chunk table, the workspace query, and the refusals both entry points make before
any launch (no GPU needed: nothing here reaches a kernel)."""
import ctypes

import numpy as np

EINVAL, EWS = -1, -3     # include/pcc_hip.h


def _lib():
    from unified_point_cloud_compression_amd import lib
    return lib, lib.load()


def test_status_codes_are_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcc_hip.h")).read()
    assert int(re.search(r"#define PCC_EINVAL \((-?\d+)\)", src).group(1)) == EINVAL
    assert int(re.search(r"#define PCC_EWS \((-?\d+)\)", src).group(1)) == EWS


def test_chunk_table():
    lib, L = _lib()
    c = L.pcc_optim_chunk_elems()
    assert c == 16384
    sizes = np.array([1, 0, c - 1, c, c + 1, 3 * c + 5], dtype=np.int64)
    want = [(0, 0), (2, 0), (3, 0), (4, 0), (4, 1), (5, 0), (5, 1), (5, 2), (5, 3)]
    assert L.pcc_optim_build_chunks(lib.nptr(sizes), len(sizes), None, 0) == len(want)
    table = np.full((len(want) + 2, 2), -7, dtype=np.int32)
    assert L.pcc_optim_build_chunks(lib.nptr(sizes), len(sizes), lib.nptr(table), len(want)) == len(want)
    assert [tuple(r) for r in table[:len(want)]] == want and (table[len(want):] == -7).all()
    short = np.full((4, 2), -7, dtype=np.int32)                       # cap below the count: the first `cap` entries only
    assert L.pcc_optim_build_chunks(lib.nptr(sizes), len(sizes), lib.nptr(short), 3) == len(want)
    assert [tuple(r) for r in short[:3]] == want[:3] and (short[3:] == -7).all()
    assert L.pcc_optim_build_chunks(None, 0, None, 0) == 0
    assert L.pcc_optim_build_chunks(lib.nptr(np.array([4, -1], dtype=np.int64)), 2, None, 0) == -1
    assert L.pcc_optim_build_chunks(lib.nptr(sizes), -1, None, 0) == -1
    assert L.pcc_optim_build_chunks(lib.nptr(np.array([c * (1 << 31)], dtype=np.int64)), 1, None, 0) == -1
    assert L.pcc_optim_ws_bytes(0) == 0 and L.pcc_optim_ws_bytes(-3) == 0
    assert L.pcc_optim_ws_bytes(9) >= 72 and L.pcc_optim_ws_bytes(9) % 256 == 0


def test_refusals_before_any_launch():
    lib, L = _lib()
    dummy = (ctypes.c_double * 64)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    ok_ws = L.pcc_optim_ws_bytes(5)
    for call in (lambda *a: L.pcc_optim_sqnorm(*a, None),
                 lambda *a: L.pcc_optim_step(*a, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None)):
        assert call(p, -1, p, 5, p, ok_ws) == EINVAL                  # n_segs < 0
        assert call(p, 3, p, -1, p, ok_ws) == EINVAL                  # n_chunks < 0
        assert call(p, 3, p, 1 << 31, p, 1 << 40) == EINVAL
        assert call(None, 3, p, 5, p, ok_ws) == EINVAL                # no segment table
        assert call(p, 0, p, 5, p, ok_ws) == EINVAL
        assert call(p, 3, None, 5, p, ok_ws) == EINVAL                # no chunk table
        assert call(p, 3, p, 5, p, 5 * 8 - 1) == EWS                  # short workspace
        assert call(p, 3, p, 5, None, ok_ws) == EWS
        assert call(p, 3, p, 0, None, 0) == 0                         # nothing to do is not an error
    assert L.pcc_optim_step(p, 3, p, 5, p, ok_ws, 2, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == EINVAL        # unknown mode
    assert L.pcc_optim_step(p, 3, p, 5, p, ok_ws, 0, 1e-3, 0.9, 0.999, 1e-8, float("nan"), None, None) == EINVAL
