"""Hole fill on the GPU: dm_fill_holes (engine.fill_holes) against the numpy restatement of the
definition (tests/test_fill_host.py: fill_restate) bit for bit, over the shapes, iteration
counts and hole patterns that reach every path of the three kernels -- the whole pyramid in
one workgroup (up to 4096 cells), the 64-cell tile edge, the halo clamp at the map border, a
hole larger than a tile, a short last launch (iters > 16) -- then batches, in place, the hole
mask, a side stream, and the ImageCutSolver keyword."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import fill_restate, holed_plane, plane, raw_bits, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (65, 130), (129, 67), (150, 150)]
ALL_ITERS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33]
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def random_holes(H, W, seed=0, share=0.3):
    rng = np.random.default_rng(1000 * H + W + seed)
    x = rng.normal(0, 5, (H, W))
    x[rng.uniform(size=x.shape) < share] = np.nan
    return x


def check(x, iters):
    want, holes = fill_restate(x, iters)
    got, mask = engine.fill_holes(dev(x), iters, return_holes=True)
    assert got.dtype == torch.float64 and mask.dtype == torch.uint8
    assert same_bits(host(got), want)
    assert np.array_equal(host(mask), holes)
    return host(got)


# ---------------------------------------------------------------------------------------------
# 1. bitwise against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', [0, 3, 17])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_holes(shape, iters):
    x = random_holes(*shape)
    if shape == (1, 1):
        x[0, 0] = 2.5
    out = check(x, iters)
    assert np.isfinite(out).all()


@pytest.mark.parametrize('iters', [i for i in ALL_ITERS if i not in (0, 3, 17)])
@pytest.mark.parametrize('shape', [(65, 130), (129, 67)], ids=lambda s: '%dx%d' % s)
def test_every_launch_split(shape, iters):
    check(random_holes(*shape, seed=iters), iters)


def test_seven_tiled_levels():
    """1 x 270000: the smallest map whose first level of <= 4096 cells is level 7, so the pulls
    take two launches (six levels, then one from a pulled level) and seven levels are tiled."""
    x = random_holes(1, 270000, share=0.07)
    x[0, 1000:1200] = np.nan
    assert np.isfinite(check(x, 2)).all()
    t = dev(np.stack([x, x[:, ::-1]]))
    engine.fill_holes(t, 17, out=t)
    assert same_bits(host(t[0]), fill_restate(x, 17)[0])


@pytest.mark.parametrize('shape', [(5, 7), (33, 31), (65, 130), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_border_holes(shape):
    H, W = shape
    x = random_holes(H, W, seed=3, share=0.05)
    b = min(3, (min(H, W) - 1) // 2)
    x[:b], x[-b:], x[:, :b], x[:, -b:] = np.nan, np.nan, np.nan, np.nan
    assert np.isfinite(x).any()
    for iters in (0, 3, 17):
        assert np.isfinite(check(x, iters)).all()


def test_hole_larger_than_a_tile():
    x = plane(150, 150)
    x[25:125, 25:125] = np.nan
    for iters in (0, 16, 17):
        out = check(x, iters)
        assert out.min() >= np.nanmin(x) - 1e-9 and out.max() <= np.nanmax(x) + 1e-9


def test_quality_case():
    """The host test's plane with 30 % holes and a 40 x 40 hole: same bits, so the same error."""
    x = holed_plane(150, 150)
    out = check(x, 16)
    assert np.abs(out - plane(150, 150)).max() <= 0.125


@pytest.mark.parametrize('shape', [(5, 7), (65, 130), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_single_finite_cell(shape):
    x = np.full(shape, np.nan)
    x[shape[0] // 3, shape[1] - 2] = -7.25
    for iters in (0, 3, 17):
        assert raw_bits(check(x, iters), np.full(shape, -7.25))


@pytest.mark.parametrize('shape', [(1, 1), (33, 31), (129, 67), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_no_holes_is_a_copy(shape):
    x = np.random.default_rng(4).normal(size=shape)
    x.flat[x.size // 2] = -0.0
    for iters in (0, 17):
        assert raw_bits(check(x, iters), x)


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (65, 130), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_all_holes_is_a_copy(shape):
    x = np.full(shape, np.nan)
    x.flat[::3] = np.inf
    x.flat[1::5] = -np.inf
    x.flat[-1] = -np.nan
    for iters in (0, 3, 17):
        got, mask = engine.fill_holes(dev(x), iters, return_holes=True)
        assert raw_bits(host(got), x) and host(mask).all()
        t = dev(x)
        assert engine.fill_holes(t, iters, out=t) is t and raw_bits(host(t), x)


@pytest.mark.parametrize('shape', [(1, 9), (33, 31), (65, 130)], ids=lambda s: '%dx%d' % s)
def test_infinite_cells_are_holes(shape):
    x = random_holes(*shape, seed=9, share=0.1)
    rng = np.random.default_rng(2)
    x[rng.uniform(size=shape) < 0.1] = np.inf
    x[rng.uniform(size=shape) < 0.1] = -np.inf
    x.flat[0] = 1.0
    for iters in (0, 3, 17):
        assert np.isfinite(check(x, iters)).all()
    row = np.array([[np.inf, 1.0, -np.inf, 3.0, np.nan]])
    assert raw_bits(check(row, 0), np.array([[1.0, 1.0, 2.5, 3.0, 2.25]]))


# ---------------------------------------------------------------------------------------------
# 2. batch, in place, mask, stream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(33, 31), (65, 130)], ids=lambda s: '%dx%d' % s)
def test_batch_equals_single_calls(shape):
    x = np.stack([random_holes(*shape, seed=1), np.full(shape, np.nan), random_holes(*shape, seed=2, share=0.8)])
    for iters in (3, 17):
        got, mask = engine.fill_holes(dev(x), iters, return_holes=True)
        assert tuple(got.shape) == x.shape
        for m in range(3):
            one, m1 = engine.fill_holes(dev(x[m]), iters, return_holes=True)
            assert tuple(one.shape) == shape
            assert raw_bits(host(got[m]), host(one)) and np.array_equal(host(mask[m]), host(m1))
        assert same_bits(host(got), fill_restate(x, iters)[0])


@pytest.mark.parametrize('shape', [(33, 31), (65, 130), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_in_place(shape):
    x = random_holes(*shape, seed=5)
    for iters in (0, 3, 16, 17, 33):       # one, two and three launches per tiled level
        want = host(engine.fill_holes(dev(x), iters))
        t = dev(x)
        got, mask = engine.fill_holes(t, iters, out=t, return_holes=True)
        assert got is t
        assert raw_bits(host(t), want)
        assert np.array_equal(host(mask).astype(bool), np.isnan(x))
        o = torch.empty_like(t)
        src = dev(x)
        assert engine.fill_holes(src, iters, out=o) is o
        assert raw_bits(host(o), want) and same_bits(host(src), x)     # the input is untouched


def test_hole_mask():
    x = random_holes(129, 67, seed=6)
    x[5, 5], x[6, 6] = np.inf, -np.inf
    _, mask = engine.fill_holes(dev(x), 2, return_holes=True)
    assert np.array_equal(host(mask).astype(bool), ~np.isfinite(x))


def test_side_stream():
    x = random_holes(65, 130, seed=7)
    want = fill_restate(x, 17)[0]
    s = torch.cuda.Stream()
    t = dev(x)
    torch.cuda.synchronize()
    got = engine.fill_holes(t, 17, stream=s)
    with torch.cuda.stream(s):
        h = got.cpu()          # a read on that stream
    assert same_bits(h.numpy(), want)


@pytest.mark.parametrize('per', ['1', '5', '8', '16'])
def test_steps_per_launch_is_invisible(per, monkeypatch):
    """DM_FILL_STEPS (Jacobi steps per k_fill_tile launch; 1 = the plain relaxation) changes the
    launch split only: 17 steps as 17 x 1, 5 + 5 + 5 + 2, 8 + 8 + 1 and 16 + 1."""
    x = holed_plane(150, 150)
    want = fill_restate(x, 17)[0]
    monkeypatch.setenv('DM_FILL_STEPS', per)
    assert same_bits(host(engine.fill_holes(dev(x), 17)), want)
    t = dev(x)
    engine.fill_holes(t, 17, out=t)
    assert same_bits(host(t), want)


def test_arguments():
    t = dev(random_holes(5, 7))
    with pytest.raises(ValueError):
        engine.fill_holes(t.float())
    with pytest.raises(ValueError):
        engine.fill_holes(t.cpu())
    with pytest.raises(ValueError):
        engine.fill_holes(t[None, None])
    with pytest.raises(ValueError):
        engine.fill_holes(t, -1)
    with pytest.raises(ValueError):
        engine.fill_holes(t, 4097)
    with pytest.raises(ValueError):
        engine.fill_holes(t, out=torch.empty((7, 5), dtype=torch.float64, device='cuda'))


# ---------------------------------------------------------------------------------------------
# 3. ImageCutSolver(fill=)
# ---------------------------------------------------------------------------------------------
PAIR = dict(shape=(52, 100), seed=7, dx=2, h0=16, w0=32, ws=5)
MODES = ['elevation', 'elevation2', 'distance']


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(*PAIR['shape'], seed=PAIR['seed'], dx=PAIR['dx'])


@pytest.mark.parametrize('consistency', [None, 1.0])
@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_fill(pair, stride, consistency):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    from deepmatching_stereo_matching_amd.misc.optimize_loop import optimize_loop
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES),
              consistency=consistency)
    plain = ImageCutSolver(a, b, **kw)
    d0, o0 = plain()
    assert plain.fill is None and plain.hole_map is None
    solver = ImageCutSolver(a, b, fill=16, **kw)
    d1, o1 = solver()
    assert solver.fill == 16 and d1 is solver.d_map
    want, holes = engine.fill_holes(dev(d0), 16, return_holes=True)
    assert same_bits(d1, host(want))
    assert solver.hole_map.dtype == bool and solver.hole_map.shape == d0.shape
    assert np.array_equal(solver.hole_map, np.isnan(d0)) and np.array_equal(solver.hole_map, host(holes).astype(bool))
    assert same_bits(o1, o0)
    if consistency is None:
        assert solver.consistency_map is None
    else:
        assert same_bits(solver.consistency_map, plain.consistency_map)
        assert 0.0 < solver.hole_map.mean() < 0.5
    assert np.isfinite(d1).all()
    H, W = d1.shape[1:]
    out, err = optimize_loop(d1[0], np.ones((H, W)), 0.5, 1, [H - 1, W - 1])
    assert not np.isnan(out).any() and np.isfinite(err)


@pytest.mark.parametrize('consistency', [None, 1.0])
def test_solve_image_sharded_fill_on_device(pair, consistency):
    """shard.solve_image_sharded's own filler (engine.fill_holes on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = pair
    args = (a, b, [16, 32], [12, 24], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=consistency)
    got = shard.solve_image_sharded(*args, consistency=consistency, fill=16)
    assert len(got) == len(ref) + 1 and got[-1].dtype == torch.uint8
    want, holes = engine.fill_holes(ref[0], 16, return_holes=True)
    assert same_bits(host(got[0]), host(want)) and torch.equal(got[-1], holes)
    assert np.array_equal(host(holes).astype(bool), np.isnan(host(ref[0])))
    for g, r in zip(got[1:-1], ref[1:]):
        assert same_bits(host(g), host(r))


@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_fill_none(pair, stride):
    """fill=None: the bits of the path as it was (solve_tiles + stitch, or the bidir solve)."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES))
    n, org = engine.cut_grid(a.shape, [16, 32], stride, 5)
    s = ImageCutSolver(a, b, fill=None, **kw)
    d, o = s()
    match = engine.solve_tiles(a, b, org, 16, 32, 5, NCC, True, False, 3, 3, 'average')
    wd, wo = engine.stitch(match, n, 16, 32, stride, MODES)
    assert same_bits(d, host(wd)) and same_bits(o, host(wo)) and s.hole_map is None and s.consistency_map is None
    s = ImageCutSolver(a, b, fill=None, consistency=1.0, **kw)
    d, o = s()
    fwd, bwd = engine.solve_tiles_bidir(a, b, org, 16, 32, 5, NCC, True, False, 3, 3, 'average')
    wd, wo, we = engine.stitch_fb(fwd, bwd, n, 16, 32, stride, MODES, 1.0)
    assert same_bits(d, host(wd)) and same_bits(o, host(wo)) and same_bits(s.consistency_map, host(we))
    assert s.hole_map is None
