"""Training batches assembled on the GPU (unified_point_cloud_compression_amd/data.py, csrc/pcc_data.hip) against the CPU
restatements of tests/data_ref.py: cube slicing, exact rotation, colour jitter, whole batches, determinism, and a batch fed
through the training step.  Every test here fails without the feature (the module does not exist before it)."""
import copy
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from tests import data_ref as R
from tests.util import dev, t, n, load_params

pytestmark = pytest.mark.gpu

TRANSFORMS_CFG = {"1_ColorJitter": {"key": "ColorJitter"}, "2_Rotate": {"key": "RandomRotate", "block_size": 128}}
Q_MAP = {"lambda_A_min": 0, "lambda_A_max": 12800, "lambda_G_min": 0, "lambda_G_max": 200, "mode": "quadratic"}
F64_CAP = 1e-4          # share of rows that may floor differently from the float64 rotation


@functools.lru_cache(maxsize=None)
def _frame():
    from unified_point_cloud_compression_amd import synth
    return synth.surface_cloud(0, 10)


@functools.lru_cache(maxsize=None)
def _table(cube_size=128, offset=0.0):
    from unified_point_cloud_compression_amd import data as D
    pc = _frame()
    return D.slice_into_cubes(t(pc[:, :3] + np.float32(offset)), t(pc[:, 3:]), cube_size)


def _cube_np(table, i):
    c = table.cube(i)
    return n(c["points"]), n(c["colors"])


# ---- the jitter test's inputs and its tolerance ------------------------------------------------------------------------
def jitter_colors():
    """Exact greys, 8-bit levels, saturated primaries and secondaries, all 0/1 corners, near-greys, uniform draws."""
    rng = np.random.default_rng(7)
    lv = np.arange(256, dtype=np.float32) / np.float32(255)
    greys = np.repeat(lv[:, None], 3, axis=1)
    eight = rng.integers(0, 256, (6000, 3)).astype(np.float32) / np.float32(255)
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=3)), dtype=np.float32)
    prim = np.concatenate([corners * np.float32(s) for s in (0.25, 0.5, 0.75)])
    near = np.clip(greys[::4] + rng.uniform(-1e-3, 1e-3, (64, 3)).astype(np.float32), 0, 1).astype(np.float32)
    two_equal = eight[:600].copy()
    two_equal[:200, 1] = two_equal[:200, 0]; two_equal[200:400, 2] = two_equal[200:400, 1]; two_equal[400:, 2] = two_equal[400:, 0]
    uni = rng.random((5000, 3), dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([greys, eight, corners, prim, near, two_equal, uni]))


def jitter_cases():
    """All 24 step orders x factors at the ends of their ranges and inside them: (steps, (b, c, s, hue))."""
    g = torch.Generator().manual_seed(99)
    f32 = lambda v: float(np.float32(v))
    sets = [(0.7, 0.7, 0.7, -0.3), (1.3, 1.3, 1.3, 0.3), (0.7, 1.3, 0.7, 0.3), (1.3, 0.7, 1.3, -0.3)]
    from unified_point_cloud_compression_amd import data as D
    sets += [D.ColorJitter().draw(g)["factors"] for _ in range(4)]
    return [(list(o), tuple(f32(v) for v in f)) for o in itertools.permutations(range(4)) for f in sets]


def jitter_e_ref():
    """The reference arithmetic's own noise on the test's inputs: largest |fp32 CPU restatement - float64 restatement|."""
    col, e = jitter_colors(), 0.0
    for steps, fac in jitter_cases():
        e = max(e, float(np.abs(R.jitter(col, steps, fac, np.float32).astype(np.float64) - R.jitter(col, steps, fac, np.float64)).max()))
    return e


def _colour_table(colors):
    """A table of one cube that holds the given colours (the points do not matter to the colour steps)."""
    from unified_point_cloud_compression_amd import data as D
    m = len(colors)
    pts = np.stack([np.arange(m) % 128, (np.arange(m) // 128) % 128, np.arange(m) // (128 * 128)], axis=1).astype(np.float32)
    return D.CubeTable(t(pts), t(colors), [0, m], [[0, 0, 0]], 128)


# ---- 1. slicing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube_size", [128, 64, 100])
def test_slicing_matches_the_reference_loop(cube_size):
    pc = _frame()
    tb = _table(cube_size)
    ref = R.slice_into_cubes(torch.from_numpy(pc[:, :3].copy()), torch.from_numpy(pc[:, 3:].copy()), cube_size)
    assert len(tb) == len(ref)
    assert np.array_equal(tb.h_origin, np.stack([c["offset"].numpy() for c in ref]))
    assert np.array_equal(n(tb.origin), tb.h_origin) and np.array_equal(n(tb.offsets), tb.h_offsets)
    assert int(tb.num_points.sum()) == len(pc) == int(tb.h_offsets[-1])
    P, C = n(tb.points), n(tb.colors)
    for i, c in enumerate(ref):
        a, b = tb.h_offsets[i], tb.h_offsets[i + 1]
        assert b - a == int(c["num_points"])
        assert np.array_equal(P[a:b], c["points"].numpy()) and np.array_equal(C[a:b], c["colors"].numpy()), i
    got = tb.cube(3)
    assert np.array_equal(n(got["points"]), ref[3]["points"].numpy()) and int(got["num_points"]) == int(ref[3]["num_points"])
    assert np.array_equal(n(got["offset"]), ref[3]["offset"].numpy())
    assert tb.indices(300) == [i for i, c in enumerate(ref) if c["num_points"] > 300]


def test_tables_concatenate_and_remember_their_frame():
    from unified_point_cloud_compression_amd import data as D
    a, b = _table(128), _table(128, 0.5)
    tb = D.CubeTable.concat([a, b])
    assert len(tb) == len(a) + len(b) and tb.frame.tolist() == [0] * len(a) + [1] * len(b)
    i = len(a) + 5
    assert np.array_equal(n(tb.cube(i)["points"]), n(b.cube(5)["points"])) and np.array_equal(tb.h_origin[i], b.h_origin[5])


# ---- 2. rotation ----------------------------------------------------------------------------------------------------
def _angle_params(rr):
    g = torch.Generator().manual_seed(1234)
    pairs = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (3, 2), (2, 3), (0, 3)]            # multiples of pi / 2
    f = lambda k: torch.tensor([k * math.pi / 2], dtype=torch.float32)
    return [rr.params(f(a), f(b)) for a, b in pairs] + [rr.draw(g) for _ in range(24)]


@pytest.mark.parametrize("offset", [0.5, 0.0])
def test_rotation_is_exact(offset):
    """32 angle pairs (24 drawn, (0, 0) and 7 pairs of multiples of pi/2) on the four largest 128^3 cubes of the frame,
    732 384 rows: the int32 voxels equal the ordered-fp32 restatement bit for bit -- on integer voxel corners (offset 0) and on
    voxel centres (offset 0.5).  Against the same rotation in float64 at most 1e-4 of the rows may floor differently; that
    comparison runs on the voxel centres.  Measured on the CPU for this input (restatement against float64): 7 of 732 384
    rows, 9.6e-6 (drawn pairs 1.3e-5, special pairs 0).  Integer corners are NOT a usable input for it: cos(fp32(pi/2)) =
    -4.4e-8, so a quarter turn of integer points lands within 3e-6 of voxel faces and 62 % of those rows floor differently
    in float64 whatever arithmetic the fp32 side uses.  The 24 drawn pairs (549 288 rows) are held to the same cap on both
    inputs, integer corners included -- the input training rotates (CPU: 5 rows, 9.1e-6, on corners; 7 rows on centres)."""
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128, offset)
    rr = D.RandomRotate(128)
    params = _angle_params(rr)
    big = np.argsort(-tb.num_points, kind="stable")[:4]
    cubes = [int(big[k % 4]) for k in range(len(params))]
    batcher = D.TrainBatcher(tb, len(cubes))
    coords, feats, info = batcher.assemble(cubes, [{"rotate": p} for p in params], deduplicate=False)
    C = n(coords)
    assert len(params) >= 20 and len(C) >= 300000 and len(C) == info["rows"] and int(info["outside"]) == 0
    at = diff64 = diff64_drawn = rows_drawn = 0
    for s, (ci, p) in enumerate(zip(cubes, params)):
        pts, col = _cube_np(tb, ci)
        want = R.rotate_ordered(pts, p["matrix"].numpy(), p["centre"])
        got = C[at:at + len(pts)]
        assert np.array_equal(got[:, 0], np.full(len(pts), s)) and np.array_equal(got[:, 1:], want), s
        d = int((got[:, 1:] != R.rotate_f64(pts, p["matrix"].numpy(), p["centre"])).any(axis=1).sum())
        diff64 += d
        if s >= 8:                                       # the 24 drawn pairs
            diff64_drawn, rows_drawn = diff64_drawn + d, rows_drawn + len(pts)
        at += len(pts)
    assert at == len(C)
    first = _cube_np(tb, cubes[0])[1]
    assert np.array_equal(n(feats)[:len(first)], first)                                  # colours untouched
    print(f"offset {offset}: {diff64} of {len(C)} rows floor differently from float64 ({diff64 / len(C):.2e})")
    print(f"   drawn pairs alone: {diff64_drawn} of {rows_drawn} ({diff64_drawn / rows_drawn:.2e})")
    assert rows_drawn >= 300000 and diff64_drawn <= F64_CAP * rows_drawn      # on integer points too: what training rotates
    if offset == 0.5:
        assert diff64 <= F64_CAP * len(C)


def test_rotation_matrix_matches_the_reference_construction():
    from unified_point_cloud_compression_amd import data as D
    phi, theta = torch.tensor([0.7]), torch.tensor([2.1])
    r_x = torch.tensor([[1, 0, 0], [0, torch.cos(phi), -torch.sin(phi)], [0, torch.sin(phi), torch.cos(phi)]])
    r_y = torch.tensor([[torch.cos(theta), 0, torch.sin(theta)], [0, 1, 0], [-torch.sin(theta), 0, torch.cos(theta)]])
    assert torch.equal(D.RandomRotate.rotation_matrix_3d(phi, theta), torch.mm(r_y, r_x))


# ---- 3. colour jitter -------------------------------------------------------------------------------------------------
def test_colour_jitter_matches_float64():
    """All 24 step orders x 8 factor sets (four at the ends of the ranges, four drawn inside) on 11 952 colours (exact greys,
    8-bit levels, primaries and secondaries at four levels, the 0/1 corners, near-greys, two equal channels, uniform draws)
    against the float64 restatement.  Tolerance 4 x e_ref, e_ref = largest |fp32 CPU restatement - float64 restatement| on
    these inputs, computed here from the two CPU restatements alone: measured e_ref = 1.864e-06, bound 7.456e-06; the
    kernel measured 1.862e-06 against float64 on an MI355X (profiles/data_pipeline_tolerances.txt)."""
    from unified_point_cloud_compression_amd import data as D
    col, cases = jitter_colors(), jitter_cases()
    assert len(cases) == 24 * 8
    e_ref = jitter_e_ref()
    tol = 4 * e_ref
    tb = _colour_table(col)
    batcher = D.TrainBatcher(tb, len(cases))
    params = [{"jitter": {"steps": s, "factors": f}} for s, f in cases]
    coords, feats, _ = batcher.assemble([0] * len(cases), params, deduplicate=False)
    F = n(feats).reshape(len(cases), len(col), 3)
    worst = 0.0
    for k, (s, f) in enumerate(cases):
        worst = max(worst, float(np.abs(F[k].astype(np.float64) - R.jitter(col, s, f, np.float64)).max()))
    print(f"e_ref {e_ref:.3e}, bound {tol:.3e}, kernel against float64 {worst:.3e}")
    assert 1e-8 < e_ref < 1e-5
    assert worst <= tol
    assert np.array_equal(n(coords)[:, 0], np.repeat(np.arange(len(cases)), len(col)))


def test_colour_jitter_with_unit_factors_is_the_identity():
    """b = c = s = 1 without a hue step: blend(x, y, 1) = 1 x + 0 y, the colours come back bit for bit."""
    from unified_point_cloud_compression_amd import data as D
    col = jitter_colors()
    tb = _colour_table(col)
    orders = [list(o) for o in itertools.permutations((0, 1, 2))] + [[1], [2, 0], []]
    params = [{"jitter": {"steps": o, "factors": (1.0, 1.0, 1.0, 0.25)}} for o in orders]
    _, feats, _ = D.TrainBatcher(tb, len(orders)).assemble([0] * len(orders), params, deduplicate=False)
    F = n(feats).reshape(len(orders), len(col), 3)
    for k in range(len(orders)):
        assert np.array_equal(F[k], col), orders[k]


def test_contrast_mean_is_reproducible():
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128)
    cubes = tb.indices(300)[:8]
    g = torch.Generator().manual_seed(5)
    params = [{"jitter": D.ColorJitter().draw(g)} for _ in cubes]
    a = D.TrainBatcher(tb, 8).assemble(cubes, params)
    b = D.TrainBatcher(tb, 8).assemble(cubes, params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. whole batches -------------------------------------------------------------------------------------------------
def _check_batch(tb, cubes, params, tol):
    from unified_point_cloud_compression_amd import data as D
    coords, feats, info = D.TrainBatcher(tb, len(cubes)).assemble(cubes, params)
    want_c, want_f = R.batch([_cube_np(tb, i) for i in cubes], params, np.float64)
    C, F = n(coords), n(feats)
    assert coords.dtype == torch.int32 and feats.dtype == torch.float32
    assert C.shape == want_c.shape and np.array_equal(C, want_c)
    assert len(np.unique(C, axis=0)) == len(C)
    err = float(np.abs(F.astype(np.float64) - want_f).max())
    assert err <= tol, (err, tol)
    assert info["cubes"] == list(cubes) and info["rows"] == sum(int(tb.num_points[i]) for i in cubes)
    assert int(info["outside"]) == 0
    return len(C), info["rows"]


def test_whole_batch_matches_the_cpu_pipeline():
    """8 cubes (more than 300 points) of the frame under ColorJitter + RandomRotate(128): coordinates row for row, colours
    within the jitter tolerance, first-wins de-duplication exercised (about a tenth of the rotated rows are duplicates)."""
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128)
    tol = 4 * jitter_e_ref()
    transforms = D.build_transforms(TRANSFORMS_CFG)
    b = D.TrainBatcher(tb, 8, min_points=300, transforms=transforms, generator=torch.Generator().manual_seed(11))
    cubes = b.eligible[10:18]
    params = [b.draw() for _ in cubes]
    kept, rows = _check_batch(tb, cubes, params, tol)
    print(f"{rows} rows, {kept} after de-duplication ({1 - kept / rows:.1%} duplicates)")
    assert kept < 0.99 * rows
    _check_batch(tb, cubes, [{"rotate": p["rotate"]} for p in params], 0.0)               # rotation only: colours bit-equal
    _check_batch(tb, cubes, [{"jitter": p["jitter"]} for p in params], tol)               # jitter only
    _check_batch(tb, cubes[:1], params[:1], tol)                                          # one cube
    _check_batch(tb, cubes, [{} for _ in cubes], 0.0)                                     # no transform at all


def test_last_partial_batch():
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128)
    ne = len(tb.indices(300))
    b = D.TrainBatcher(tb, 32, min_points=300, transforms=D.build_transforms(TRANSFORMS_CFG),
                       generator=torch.Generator().manual_seed(2))
    assert ne % 32 != 0 and len(b) == -(-ne // 32)
    items = list(b)
    assert [len(i[2]["cubes"]) for i in items] == [32] * (ne // 32) + [ne % 32]
    last = items[-1]
    assert int(last[0][:, 0].max()) == ne % 32 - 1
    want_c, _ = R.batch([_cube_np(tb, i) for i in last[2]["cubes"]], last[2]["params"], np.float32)
    assert np.array_equal(n(last[0]), want_c)


def test_a_wrong_extent_is_contained_and_reported():
    """The de-duplication's lattice is sized from the table's extent on the host.  A table whose extent understates its
    points (here: given by hand, too small) cannot write outside that lattice: the rows are moved onto the box and
    `info["outside"]` says so."""
    from unified_point_cloud_compression_amd import data as D
    good = _table(128)
    i = good.indices(300)[0]
    c = good.cube(i)
    m = int(c["num_points"])
    tb = D.CubeTable(c["points"].clone(), c["colors"].clone(), [0, m], [[0, 0, 0]], 128, extent=[[0, 0, 0], [10, 10, 10]])
    coords, feats, info = D.TrainBatcher(tb, 1).assemble([0], [{}])
    assert int(info["outside"]) == 1
    C = n(coords)
    assert C[:, 1:].min() >= -12 and C[:, 1:].max() <= 12 and len(np.unique(C, axis=0)) == len(C)   # reach 10 (1 + 1e-5) + 1
    ok = D.CubeTable(c["points"].clone(), c["colors"].clone(), [0, m], [[0, 0, 0]], 128)
    assert (ok.extent[0] >= 0).all() and (ok.extent[1] < 128).all()
    assert int(D.TrainBatcher(ok, 1).assemble([0], [{}])[2]["outside"]) == 0


def test_an_epoch_over_a_table_with_a_wrong_extent_raises():
    """Iterating reads the `outside` flags of an epoch once, at its end: moved points do not go unnoticed."""
    from unified_point_cloud_compression_amd import data as D
    from unified_point_cloud_compression_amd.lib import PccError
    c = _table(128).cube(_table(128).indices(300)[0])
    m = int(c["num_points"])
    tb = D.CubeTable(c["points"].clone(), c["colors"].clone(), [0, m], [[0, 0, 0]], 128, extent=[[0, 0, 0], [10, 10, 10]])
    it = iter(D.TrainBatcher(tb, 1))
    assert int(next(it)[2]["outside"]) == 1
    with pytest.raises(PccError):
        next(it)


def test_descriptor_uploads_do_not_overtake_each_other():
    """Four batches of different cubes queued back to back with deduplicate=False -- no host read anywhere -- behind matrix
    products that keep the stream busy while the host runs ahead: every batch is the restatement of ITS cubes, i.e. the
    kernels of a step read the tables of that step, not of a later one (the pinned staging buffers are rewritten only after
    the event behind their last copy)."""
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128)
    el = tb.indices(300)
    rr, g = D.RandomRotate(128), torch.Generator().manual_seed(77)
    sets = [el[0:3], el[20:28], el[40:42], el[50:57]]
    params = [[{"rotate": rr.draw(g)} for _ in cs] for cs in sets]
    b = D.TrainBatcher(tb, 8)
    b.assemble(sets[0], params[0], deduplicate=False)                    # staging buffers allocated, code loaded
    a = torch.randn((8192, 8192), device=dev())
    torch.cuda.synchronize()
    for _ in range(6):
        a = torch.mm(a, a) * 1e-4                                        # some tens of ms of queued work
    out = [b.assemble(cs, ps, deduplicate=False) for cs, ps in zip(sets, params)]
    torch.cuda.synchronize()
    for (coords, feats, info), cs, ps in zip(out, sets, params):
        want_c, want_f = R.batch([_cube_np(tb, i) for i in cs], ps, np.float32, deduplicate=False)
        assert np.array_equal(n(coords), want_c) and np.array_equal(n(feats), want_f) and int(info["outside"]) == 0


# ---- 5. determinism -----------------------------------------------------------------------------------------------------
def test_epochs_are_a_pure_function_of_the_seed():
    from unified_point_cloud_compression_amd import data as D
    tb = _table(128)
    mk = lambda seed: D.TrainBatcher(tb, 8, min_points=300, transforms=D.build_transforms(TRANSFORMS_CFG),
                                     generator=torch.Generator().manual_seed(seed))
    state = torch.random.get_rng_state()
    a, b = list(mk(3)), list(mk(3))
    assert torch.equal(state, torch.random.get_rng_state())                               # the global generator is not touched
    assert len(a) == len(b) == len(mk(3)) == -(-len(tb.indices(300)) // 8)
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2]["cubes"] == y[2]["cubes"]
    assert sorted(i for x in a for i in x[2]["cubes"]) == tb.indices(300)
    c = next(iter(mk(4)))
    assert not (c[0].shape == a[0][0].shape and torch.equal(c[0], a[0][0]) and torch.equal(c[1], a[0][1]))
    u = D.TrainBatcher(tb, 8, min_points=300, shuffle=False)
    assert [i for x in u for i in x[2]["cubes"]] == tb.indices(300)


# ---- 6. it feeds the step -------------------------------------------------------------------------------------------------
LOSS_CFG = {"Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
            "ColorLoss": {"type": "ColorLoss", "loss": "L2"},
            "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0},
            "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0}}


def _shape_noise(*args):
    """U(-.5, .5) noise that depends on the tag and the shape alone, so two evaluations of one batch see the same draw."""
    tag, like = args[0], args[-1]
    g = torch.Generator().manual_seed(1000003 * like.shape[0] + 31 * like.shape[-1] + sum(map(ord, tag)))
    return (torch.rand(tuple(like.shape), generator=g) - 0.5).to(like.device)


def test_batches_feed_the_training_step():
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    from oracle import codec
    from unified_point_cloud_compression_amd import data as D
    from unified_point_cloud_compression_amd.loss import Loss
    from unified_point_cloud_compression_amd.model import UnifiedModel
    cfg = codec.small_config(adaptive=True, offsets=True, inverse=True)
    model = load_params(UnifiedModel(copy.deepcopy(cfg)), codec.random_params(cfg, 3, gain=4.0)).to(dev()).train()
    model.entropy_model.noise_fn = _shape_noise
    loss_fn = Loss(copy.deepcopy(LOSS_CFG))
    tb = _table(128)
    g = torch.Generator().manual_seed(21)
    q_func = D.Q_Func(Q_MAP)
    batcher = D.TrainBatcher(tb, 4, min_points=300, transforms=D.build_transforms(TRANSFORMS_CFG), generator=g)
    shapes = []
    for k, (coords, feats, info) in zip(range(3), batcher):
        x = ME.SparseTensor(features=feats, coordinates=coords)
        q, lam = q_func(len(info["cubes"]), generator=g, device=dev())
        model.zero_grad(set_to_none=True)
        total, parts = loss_fn(x, model(x, q, lam))
        assert all(math.isfinite(float(v.detach())) for v in parts.values()) and math.isfinite(float(total.detach()))
        total.backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert len(grads) >= 40 and all(bool(torch.isfinite(gr).all()) for gr in grads)
        shapes.append(tuple(coords.shape))
    assert len(set(shapes)) == 3                         # differently shaped batches, one after the other

    # a rotation-only batch against the same model on the CPU-restated batch uploaded by hand
    cubes = batcher.eligible[:4]
    params = [{"rotate": D.RandomRotate(128).draw(g)} for _ in cubes]
    coords, feats, _ = batcher.assemble(cubes, params)
    want_c, want_f = R.batch([_cube_np(tb, i) for i in cubes], params, np.float32)
    assert np.array_equal(n(coords), want_c) and np.array_equal(n(feats), want_f)
    q, lam = q_func(4, generator=g, device=dev())

    def parts_of(c, f):
        x = ME.SparseTensor(features=f, coordinates=c)
        with torch.no_grad():
            return loss_fn(x, model(x, q, lam))[1]

    got, ref = parts_of(coords, feats), parts_of(t(want_c), t(want_f))
    assert set(got) == set(ref) and len(ref) >= 4
    for name in ref:
        a, b = float(got[name]), float(ref[name])
        assert abs(a - b) <= 1e-4 + 1e-4 * abs(b), (name, a, b)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch():
    from unified_point_cloud_compression_amd import data as D
    from unified_point_cloud_compression_amd.lib import PccError
    pc = _frame()[:1000]
    with pytest.raises(PccError):
        D.slice_into_cubes(torch.from_numpy(pc[:, :3].copy()), torch.from_numpy(pc[:, 3:].copy()), 64)
    with pytest.raises(PccError):
        D.slice_into_cubes(t(pc[:, :3]), t(pc[:, 3:5]), 64)
    with pytest.raises(PccError):
        D.RandomRotate(128, crop=True)
    with pytest.raises(ValueError):
        D.build_transforms({"1": {"key": "RandomFlip"}})
    tb = _table(128)
    with pytest.raises(ValueError):
        D.TrainBatcher(tb, 0)
    with pytest.raises(PccError):
        D.TrainBatcher(D.CubeTable(tb.points.cpu(), tb.colors.cpu(), tb.h_offsets, tb.h_origin, 128), 4)
    b = D.TrainBatcher(tb, 4)
    for bad in ([len(tb)], [-1], []):
        with pytest.raises(ValueError):
            b.assemble(bad, [{} for _ in bad])
    with pytest.raises(ValueError):
        b.assemble([0, 1], [{}])
    with pytest.raises(ValueError):
        b.assemble([0], [{"jitter": {"steps": [1, 1], "factors": (1.0, 1.0, 1.0, 0.0)}}])
    with pytest.raises(ValueError):
        tb.cube(len(tb))
