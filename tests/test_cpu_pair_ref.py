"""The numpy reference of the pair-list planner (tests/pair_ref.py) checked by brute force on the tables the GPU tests of the
pair-list convolution run on (tests/test_gpu_pair_conv_float64.py): the reference has to be right before the kernels are held
against it bit for bit."""
import numpy as np
import pytest
import torch

from tests import pair_ref as PR
from tests.util import conv_sums64


def _requested_counts(name):
    return {"T125": [0] + PR._cycle(PR.T125_PATTERN, 125)[1:-1] + [0], "T27": PR._cycle(PR.T27_PATTERN, 27),
            "T8full": [129] * 8, "empty": [0] * 27, "first_slot": [1] + [0] * 26, "last_slot": [0] * 26 + [1],
            "full128": [128] * 5, "full129": [129] * 5, "N1": [1 - k % 2 for k in range(125)], "K1_2047": [1023],
            "K1_2048": [1024], "K1_2049": [1024], "K27_76": PR._cycle((76, 0, 1, 75, 38, 0, 0, 2), 27)}[name]


@pytest.mark.parametrize("name", PR.TABLES)
def test_tables_hold_the_requested_counts(name):
    """Every offset has exactly the requested number of pairs, its input rows are distinct and inside [0, n_in), and the
    tables reach the counts the planner can get wrong: 0, 1, 127, 128, 129, leading, trailing and runs of empty offsets."""
    nbr = PR.table(name)
    want = _requested_counts(name)
    assert nbr.dtype == np.int32 and nbr.shape[0] == len(want)
    for k, row in enumerate(nbr):
        rows_in = [int(v) for v in row if v >= 0]
        assert len(rows_in) == want[k], (name, k)
        assert len(set(rows_in)) == len(rows_in) and all(0 <= v < PR.TABLE_N_IN[name] for v in rows_in)
        assert all(v == -1 for v in row if v < 0)


def test_t125_has_the_sizes_the_gpu_cases_are_planned_for():
    nbr = PR.table("T125")
    plan = PR.table_plan("T125")
    assert nbr.shape == (125, 401) and plan["info"] == (22144, 173, 16436)
    assert round(16436 / (125 * 401), 2) == 0.33
    counts = (nbr >= 0).sum(1)
    assert counts[0] == 0 and counts[-1] == 0 and {0, 1, 127, 128, 129, 255, 256, 257, 401, 64} == set(counts.tolist())
    assert any(counts[k] > 0 and counts[k + 1] == 0 and counts[k + 2] == 0 and counts[k + 3] > 0 for k in range(122))   # a run inside
    assert all(PR.table_plan(t)["info"][0] <= 65000 for t in PR.TABLES)


@pytest.mark.parametrize("name", PR.TABLES)
def test_plan_ref_by_brute_force(name):
    """Slot by slot: every pair occurs once in the padded list, `pos` and `pair_in` invert each other, every tile holds pairs
    of one offset only and names it, the pairs of an offset stand in ascending output row from `pstart[k]`, `pstart` is the
    running sum of the counts rounded up to 128, and info = (padded, tiles, pairs)."""
    nbr = PR.table(name)
    plan = PR.plan_ref(nbr)
    K, n_out = nbr.shape
    pos, pstart, pair_in, tile_k = plan["pos"], plan["pstart"], plan["pair_in"], plan["tile_k"]
    padded, tiles, pairs = plan["info"]
    assert pos.shape == (K, n_out) and pstart.shape == (K + 1,) and pair_in.shape == (padded,) and tile_k.shape == (tiles,)
    assert all(a.dtype == np.int32 for a in (pos, pstart, pair_in, tile_k))
    owner = {}                                  # padded slot -> (k, o)
    run = 0
    for k in range(K):
        assert pstart[k] == run
        last = -1
        cnt = 0
        for o in range(n_out):
            p = int(pos[k, o])
            if nbr[k, o] < 0:
                assert p == -1
                continue
            assert p == run + cnt, (k, o)                        # ascending output row, densely from pstart[k]
            assert p not in owner and p > last
            owner[p] = (k, o)
            assert pair_in[p] == nbr[k, o]
            last = p
            cnt += 1
        run += (cnt + 127) // 128 * 128
    assert pstart[K] == run == padded and tiles * 128 == padded and pairs == len(owner) == int((nbr >= 0).sum())
    for p in range(padded):
        if p in owner:
            assert tile_k[p // 128] == owner[p][0]
        else:
            assert pair_in[p] == -1
    for t in range(tiles):                                       # no tile is padding only, and none mixes offsets
        ks = {owner[p][0] for p in range(t * 128, t * 128 + 128) if p in owner}
        assert ks == {int(tile_k[t])}, (t, ks)


@pytest.mark.parametrize("name", PR.TABLES)
def test_pairs_of_lists_every_pair_once(name):
    nbr = PR.table(name)
    pairs = PR.pairs_of(nbr)
    assert len(pairs) == nbr.shape[0]
    seen = set()
    for k, (i, o) in enumerate(pairs):
        assert i.dtype == np.int64 and o.dtype == np.int64 and len(i) == len(o)
        assert np.all(np.diff(o) > 0)
        for ii, oo in zip(i.tolist(), o.tolist()):
            assert nbr[k, oo] == ii
            seen.add((k, oo))
    assert len(seen) == int((nbr >= 0).sum())


@pytest.mark.parametrize("name", ["T125", "T27", "T8full", "empty", "last_slot", "N1", "K1_2049"])
def test_dense_loop_sum_equals_the_pair_list_sum_in_float64(name):
    """out[o] = b + sum_k x[nbr[k, o]] @ W[k] by a loop over every slot of the table against `conv_sums64` over `pairs_of`
    (float64, on the CPU), and the same for the sum of squared terms."""
    nbr = PR.table(name)
    K, n_out = nbr.shape
    cin, cout = 6, 8
    rng = np.random.default_rng(41)
    x = rng.standard_normal((PR.TABLE_N_IN[name], cin))
    W = rng.standard_normal((K, cin, cout))
    b = rng.standard_normal(cout)
    want = np.tile(b, (n_out, 1))
    sq = np.tile(b * b, (n_out, 1))
    for k in range(K):
        for o in range(n_out):
            if nbr[k, o] >= 0:
                want[o] += x[nbr[k, o]] @ W[k]
                sq[o] += (x[nbr[k, o]] ** 2) @ (W[k] ** 2)
    ref, s2 = conv_sums64(torch.from_numpy(x), torch.from_numpy(W), torch.from_numpy(b), PR.pairs_of(nbr), n_out)
    s = np.sqrt(sq)
    assert np.all(np.abs(ref.numpy() - want) <= 1e-13 * s)
    assert np.all(np.abs(s2.numpy() - sq) <= 1e-13 * sq)
