"""Reference of the pair-list planner (numpy only) and the synthetic map tables its tests run on.

The planner is restated from the header comment of the pair-list form in include/pcc_hip.h, not from its kernels: the pairs of
each offset are compacted and padded to 128-pair tiles; `pos[k, o]` is the row of pair (k, o) in the padded list, `pair_in` the
input row of every padded pair (-1 = padding), `tile_k` the offset of every tile, info = (padded pairs, tiles, pairs).  Within
an offset the pairs stand in ascending output row, so every output is fully determined and the GPU comparison is bit for bit.
"""
import functools

import numpy as np

PAIR_TILE = 128        # pairs per tile of the gathered pair GEMM


def synthetic_table(K, n_in, n_out, counts, seed):
    """nbr [K, n_out] int32 (-1 = hole): offset k has exactly counts[k] pairs, on output rows drawn without replacement, with
    input rows that are distinct within the offset (as a real map's are).  A conv map in the layout `nbr[k * n_out + o]`."""
    counts = [int(c) for c in counts]
    assert len(counts) == K and all(0 <= c <= min(n_in, n_out) for c in counts), (K, n_in, n_out, counts)
    rng = np.random.default_rng(seed)
    nbr = np.full((K, n_out), -1, np.int32)
    for k, c in enumerate(counts):
        o = np.sort(rng.choice(n_out, c, replace=False))
        nbr[k, o] = rng.permutation(n_in)[:c]
    return nbr


def plan_ref(nbr):
    """The pair plan of a [K, n_out] table: dict of pos [K, n_out] int32, pstart [K + 1] int32, pair_in [padded] int32,
    tile_k [tiles] int32 and info = (padded, tiles, pairs)."""
    nbr = np.asarray(nbr)
    K, n_out = nbr.shape
    pos = np.full((K, n_out), -1, np.int32)
    pstart = np.zeros(K + 1, np.int32)
    pair_in, tile_k = [], []
    run = 0
    for k in range(K):
        pstart[k] = run
        rows = np.nonzero(nbr[k] >= 0)[0]                              # ascending output row
        tiles = -(-len(rows) // PAIR_TILE)
        pos[k, rows] = run + np.arange(len(rows))
        padded = np.full(tiles * PAIR_TILE, -1, np.int32)
        padded[:len(rows)] = nbr[k, rows]
        pair_in.append(padded)
        tile_k.extend([k] * tiles)
        run += tiles * PAIR_TILE
    pstart[K] = run
    pair_in = np.concatenate(pair_in) if pair_in else np.zeros(0, np.int32)
    assert len(pair_in) == run and len(tile_k) * PAIR_TILE == run
    return {"pos": pos, "pstart": pstart, "pair_in": pair_in.astype(np.int32),
            "tile_k": np.asarray(tile_k, np.int32).reshape(-1), "info": (run, run // PAIR_TILE, int((nbr >= 0).sum()))}


def pairs_of(nbr):
    """[(in_rows, out_rows)] per offset (int64 numpy): the list `tests.util.conv_sums64` takes."""
    out = []
    for row in np.asarray(nbr):
        o = np.nonzero(row >= 0)[0].astype(np.int64)
        out.append((row[o].astype(np.int64), o))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables of the pair-list tests
# ---------------------------------------------------------------------------------------------------------------------------------
T125_PATTERN = (0, 1, 127, 128, 129, 255, 256, 257, 401, 0, 0, 64)
T27_PATTERN = (0, 1, 127, 128, 129, 256, 300, 0, 0, 5)


def _cycle(pattern, K):
    return [pattern[k % len(pattern)] for k in range(K)]


def _single(K, n_out, k, o, row):
    nbr = np.full((K, n_out), -1, np.int32)
    nbr[k, o] = row
    return nbr


def _t125():
    counts = _cycle(T125_PATTERN, 125)
    counts[0] = counts[-1] = 0                  # leading and trailing empty offsets (the pattern has runs of two inside)
    return synthetic_table(125, 523, 401, counts, 3)


# name -> () -> nbr.  n_in of a table: TABLE_N_IN.
_BUILDERS = {
    "T125": _t125,
    "T27": lambda: synthetic_table(27, 311, 300, _cycle(T27_PATTERN, 27), 5),
    "T8full": lambda: synthetic_table(8, 140, 129, [129] * 8, 7),
    "empty": lambda: np.full((27, 300), -1, np.int32),
    "first_slot": lambda: _single(27, 300, 0, 0, 17),
    "last_slot": lambda: _single(27, 300, 26, 299, 17),                # the last-slot term of the pair total
    "full128": lambda: synthetic_table(5, 128, 128, [128] * 5, 11),    # padded == pairs
    "full129": lambda: synthetic_table(5, 131, 129, [129] * 5, 13),
    "N1": lambda: synthetic_table(125, 70, 1, [1 - k % 2 for k in range(125)], 17),     # one output row, every second offset
    "K1_2047": lambda: synthetic_table(1, 2100, 2047, [1023], 19),     # around the 2048-element block of the scan
    "K1_2048": lambda: synthetic_table(1, 2100, 2048, [1024], 23),
    "K1_2049": lambda: synthetic_table(1, 2100, 2049, [1024], 29),
    "K27_76": lambda: synthetic_table(27, 90, 76, _cycle((76, 0, 1, 75, 38, 0, 0, 2), 27), 31),
}
TABLE_N_IN = {"T125": 523, "T27": 311, "T8full": 140, "empty": 311, "first_slot": 311, "last_slot": 311, "full128": 128,
              "full129": 131, "N1": 70, "K1_2047": 2100, "K1_2048": 2100, "K1_2049": 2100, "K27_76": 90}
TABLES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def table(name):
    """The named table (read-only, shared by the tests)."""
    nbr = _BUILDERS[name]()
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def table_plan(name):
    return plan_ref(table(name))
