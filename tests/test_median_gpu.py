"""Weighted median filter on the GPU: dm_median_filter (engine.median_filter) against the
restatement of the definition (tests/test_median_host.py: median_fast, pinned there to the
plain-loop median_restate) bit for bit -- over shapes smaller than a window, on the tile sides
and across them, the unweighted, shared-weight and per-map-weight forms, ties and special
values, holes on tile seams and in the halo corner, min_count, the fill flag and the changed
mask, unit weights against the unweighted path, several passes out of place and in place,
batches, a side stream, run-to-run and tile-side independence, the argument errors, and the
ImageCutSolver / solve_image_sharded keyword."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import raw_bits, same_bits
from test_median_host import INF, NAN, median_fast, median_restate, noise, pool_map, pool_weight

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (64, 64), (65, 130)]
CASES = [(s, r) for s in SHAPES for r in (1, 2, 3)] + [(s, 7) for s in SHAPES[:5]]
WEIGHTS = ['none', 'shared', 'per-map']
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def weights(shape, seed=0):
    """Positive weights over six decades, a twentieth of them unusable."""
    rng = np.random.default_rng(17 + seed + 3 * int(np.prod(shape)))
    w = 10.0 ** rng.uniform(-3, 3, shape)
    u = rng.uniform(size=shape)
    for k, bad in enumerate([0.0, -2.0, NAN, INF]):
        w[(u >= 0.0125 * k) & (u < 0.0125 * (k + 1))] = bad
    return w


def run(x, w, r, **kw):
    got = engine.median_filter(x if torch.is_tensor(x) else dev(x), r, weight=w if torch.is_tensor(w) else dev(w),
                               return_changed=True, **kw)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.uint8
    return host(got[0]), host(got[1])


def equal(got, want):
    return raw_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def check(x, w, r, iters=1, min_count=1, fill=False):
    want = median_fast(x, w, r, iters, min_count, fill)
    got = run(x, w, r, iters=iters, min_count=min_count, fill=fill)
    assert equal(got, want)
    if not fill:
        assert np.array_equal(~np.isfinite(got[0]), ~np.isfinite(x))
    return want


# ---------------------------------------------------------------------------------------------
# 1. random maps against the restatement
# ---------------------------------------------------------------------------------------------
_REF = {}


def random_case(shape, r, kind):
    """(maps, weight, the restatement's outputs), computed once per case."""
    key = (shape, r, kind)
    if key not in _REF:
        x = np.stack([noise(*shape), noise(*shape, seed=1)]) if kind == 'per-map' else noise(*shape)
        if shape == (1, 1):
            x[..., 0, 0] = 2.5
        w = None if kind == 'none' else weights(shape) if kind == 'shared' else \
            np.stack([weights(shape, 1), weights(shape, 2)])
        _REF[key] = (x, w, median_fast(x, w, r))
    return _REF[key]


@pytest.mark.parametrize('tile', [None, '16', '32'], ids=['tile-as-built', 'tile-16', 'tile-32'])
@pytest.mark.parametrize('kind', WEIGHTS)
@pytest.mark.parametrize('shape,r', CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else 'r%d' % v)
def test_random_maps(shape, r, kind, tile, monkeypatch):
    if tile is not None:
        monkeypatch.setenv('DM_MEDIAN_TILE', tile)
    x, w, want = random_case(shape, r, kind)
    got = run(x, w, r)
    assert equal(got, want)
    assert raw_bits(got[0][~np.isfinite(x)], x[~np.isfinite(x)])
    if shape == (65, 130) and r == 3:
        fin = np.isfinite(x)
        assert not raw_bits(want[0][fin], x[fin]) and want[1].sum() > fin.sum() // 2      # it does filter


def test_fast_restatement_is_the_literal_one_here():
    """median_fast is what this file compares with; once more against the plain loops, on a map
    that crosses a tile seam."""
    x, w = noise(18, 21, seed=3), weights((18, 21), 3)
    for wt in (None, w):
        a, b = median_restate(x, wt, 2), median_fast(x, wt, 2)
        assert raw_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert equal(run(x, wt, 2), a)


# ---------------------------------------------------------------------------------------------
# 2. ties and special values, holes on the seams
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2, 3, 5])
def test_ties_and_special_values(r):
    shape = (33, 40)
    rng = np.random.default_rng(5)
    two = np.where(rng.uniform(size=shape) < 0.5, 2.0, 6.0)                 # two distinct values only
    const = np.full(shape, -3.25)                                           # a constant map
    zeros = np.where(rng.uniform(size=shape) < 0.5, 0.0, -0.0)              # +-0.0 mixed
    infs = noise(*shape, seed=2)
    infs[rng.uniform(size=shape) < 0.1] = INF
    infs[rng.uniform(size=shape) < 0.1] = -INF
    tiny = np.where(rng.uniform(size=shape) < 0.5, 5e-324, 1e300) * np.where(rng.uniform(size=shape) < 0.3, -1, 1)
    w = weights(shape)
    for x in (two, const, zeros, infs, tiny, pool_map(*shape)):
        for wt in (None, w, np.ones(shape)):
            check(x, wt, r)
            check(x, wt, r, fill=True, iters=2)
    want = median_fast(zeros, None, r)[0]
    assert (want == 0).all() and np.signbit(want).any() and not np.signbit(want).all()
    # the output's sign follows the key order: -0.0 wherever at least half the window (lower median) is -0.0
    neg = np.signbit(zeros).astype(int)
    i, j = 16, 20
    win = neg[i - r:i + r + 1, j - r:j + r + 1]
    assert np.signbit(want[i, j]) == (win.sum() >= (win.size - 1) // 2 + 1)
    assert raw_bits(median_fast(const, w, r)[0], const)


@pytest.mark.parametrize('r', [1, 3])
def test_extreme_weights(r):
    """Weights 1e-300 / 1e300 / 0 / negative / NaN / +inf, and everything between."""
    shape = (33, 40)
    for seed in range(2):
        x = noise(*shape, seed=seed)
        check(x, pool_weight(shape, seed), r)
        check(pool_map(*shape, seed), pool_weight(shape, seed), r, fill=True)
    rng = np.random.default_rng(8)
    x = noise(*shape, seed=4)
    w = rng.choice([1e-300, 1e300, 0.0, -1.0, NAN, INF, 5e-324, 1.7976931348623157e308], size=shape)
    check(x, w, r)                      # T overflows to inf in places, and 0.5 T underflows to 0 in others
    check(x, np.full(shape, 5e-324), r)
    check(x, np.full(shape, 1.7976931348623157e308), r)
    dead = np.where(rng.uniform(size=shape) < 0.5, 0.0, NAN)
    want = check(x, dead, r)            # no usable tap anywhere: the input
    assert raw_bits(want[0], x) and not want[1].any()


def test_all_holes_and_one_finite_cell():
    allh = np.full((40, 37), NAN)
    allh[1, 1], allh[32, 33], allh[39, 36] = INF, -INF, -NAN
    for wt in (None, weights((40, 37))):
        for fill in (False, True):
            got = run(allh, wt, 3, fill=fill)
            assert raw_bits(got[0], allh) and not got[1].any()
    one = allh.copy()
    one[20, 18] = 7.5
    for r in (2, 3):
        want = check(one, None, r)
        assert want[0][20, 18] == 7.5 and not want[1].any()
        want = check(one, None, r, fill=True)
        assert want[1].sum() == (2 * r + 1) ** 2 - 1 and (want[0][20 - r:21 + r, 18 - r:19 + r] == 7.5).all()
        assert check(one, np.ones((40, 37)), r, fill=True, iters=2)[1].sum() == (4 * r + 1) ** 2 - 1


@pytest.mark.parametrize('tile', ['16', '32'])
@pytest.mark.parametrize('kind', ['none', 'shared'])
def test_holes_on_tile_seams_and_halo_corners(kind, tile, monkeypatch):
    monkeypatch.setenv('DM_MEDIAN_TILE', tile)
    x = noise(70, 100, seed=8, share=0.0)
    x[32, :] = NAN                       # the first row beyond a tile of 32 (and of 16)
    x[:, 32] = NAN
    x[16, 40:60] = NAN
    x[40:60, 64] = NAN
    for c in ((34, 34), (35, 35), (29, 29), (28, 28), (63, 67), (67, 95), (18, 18), (13, 13)):
        x[c] = NAN                       # the halo's corners at r = 3
    w = None if kind == 'none' else weights((70, 100))
    for r in (2, 3, 7):
        check(x, w, r)
        check(x, w, r, fill=True)


# ---------------------------------------------------------------------------------------------
# 3. min_count, fill, unit weights, passes, in place
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2, 4])
def test_min_count(r):
    x = noise(33, 40, seed=9, share=0.3)
    w = weights((33, 40))
    K = (2 * r + 1) ** 2
    changed = []
    for mc in (1, 5, K):
        for wt in (None, w):
            for fill in (False, True):
                want = check(x, wt, r, min_count=mc, fill=fill)
        changed.append(int(want[1].sum()))
    assert changed[0] >= changed[1] >= changed[2] and changed[0] > changed[2]
    full = median_fast(np.arange(35.0 * 44).reshape(35, 44), None, r, min_count=K)[1]
    assert not full[:r].any() and not full[:, :r].any() and not full[-r:].any() and not full[:, -r:].any()


@pytest.mark.parametrize('kind', ['none', 'shared'])
def test_fill_and_changed_mask(kind):
    x = noise(65, 70, seed=9, share=0.3)
    x[20:40, 25:45] = NAN                # wider than the window: the core survives one pass
    w = None if kind == 'none' else 10.0 ** np.random.default_rng(2).uniform(-3, 3, (65, 70))      # all usable
    want = check(x, w, 3, fill=True)
    hole = np.isnan(x)
    assert want[1][:20][hole[:20]].all()                       # a filled hole has changed
    assert np.isnan(want[0][23:37, 28:42]).all() and np.isfinite(want[0][22, 30])
    assert np.array_equal(want[1].astype(bool), want[0].view(np.int64) != x.view(np.int64))
    left = [int(np.isnan(check(x, w, 3, iters=k, fill=True)[0]).sum()) for k in (2, 3, 4)]
    assert left == [8 * 8, 2 * 2, 0]
    nofill = check(x, w, 3)
    assert not nofill[1][hole].any()


@pytest.mark.parametrize('r', [1, 2, 3, 4])
def test_unit_weights_equal_the_unweighted_path(r):
    for x in (noise(65, 70, seed=10), pool_map(65, 70), np.round(noise(65, 70, seed=11))):
        for fill in (False, True):
            a = run(x, None, r, fill=fill, iters=2)
            b = run(x, np.ones((65, 70)), r, fill=fill, iters=2)
            assert raw_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('kind', ['none', 'shared'])
@pytest.mark.parametrize('iters', [1, 2, 3])
def test_passes_out_of_place_and_in_place(kind, iters):
    x = noise(65, 70, seed=10)
    w = None if kind == 'none' else weights((65, 70))
    for fill in (False, True):
        want = check(x, w, 2, iters=iters, fill=fill)
        t = dev(x)
        got = engine.median_filter(t, 2, weight=dev(w), iters=iters, fill=fill, out=t, return_changed=True)
        assert got[0] is t and raw_bits(host(t), want[0]) and np.array_equal(host(got[1]), want[1])
        t = dev(x)
        assert engine.median_filter(t, 2, weight=dev(w), iters=iters, fill=fill, out=t) is t       # no mask asked for
        assert raw_bits(host(t), want[0])
        src, o = dev(x), torch.empty((65, 70), dtype=torch.float64, device='cuda')
        assert engine.median_filter(src, 2, weight=dev(w), iters=iters, fill=fill, out=o) is o
        assert raw_bits(host(o), want[0]) and raw_bits(host(src), x)      # the input is untouched


def test_numpy_input():
    x, w = noise(20, 37), weights((20, 37))
    got = engine.median_filter(x, 2, weight=w)
    assert torch.is_tensor(got) and got.is_cuda and raw_bits(host(got), median_fast(x, w, 2)[0])


def test_batch_equals_single_calls():
    shape = (33, 70)
    x = np.stack([noise(*shape, seed=1), np.full(shape, NAN), noise(*shape, seed=2, share=0.5)])
    shared = weights(shape)
    per_map = np.stack([weights(shape, s) for s in (0, 1, 2)])
    for w in (shared, per_map, None):
        for r in (2, 3):
            got = run(x, w, r, fill=True)
            assert got[0].shape == x.shape
            for m in range(3):
                one = run(x[m], w if w is None or w.ndim == 2 else w[m], r, fill=True)
                assert one[0].shape == shape and raw_bits(got[0][m], one[0]) and np.array_equal(got[1][m], one[1])
            assert equal(got, median_fast(x, w, r, fill=True))
            assert raw_bits(got[0][1], x[1])


def test_side_stream():
    x, w = noise(65, 130, seed=7), weights((65, 130))
    want = median_fast(x, w, 3, iters=2)
    s = torch.cuda.Stream()
    t, wt = dev(x), dev(w)
    torch.cuda.synchronize()
    got = engine.median_filter(t, 3, weight=wt, iters=2, return_changed=True, stream=s)
    with torch.cuda.stream(s):
        h = [q.cpu() for q in got]          # a read on that stream
    assert raw_bits(h[0].numpy(), want[0]) and np.array_equal(h[1].numpy(), want[1])


def test_consecutive_calls_are_bit_identical():
    x = noise(129, 67, seed=8)
    for w in (None, weights((129, 67))):
        for r in (2, 7):
            t, wt = dev(x), dev(w)
            a, b = run(t, wt, r), run(t, wt, r)
            assert raw_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('tile', ['16', '32', '48'])
def test_tile_side_is_invisible(tile, monkeypatch):
    """DM_MEDIAN_TILE (16 or 32; anything else: the side as built) moves the seams only."""
    x = noise(65, 130, seed=9)
    cases = [(w, r, it) for w in (None, weights((65, 130))) for r, it in ((1, 2), (3, 2), (7, 1))]
    ref = [run(x, w, r, iters=it, fill=True) for w, r, it in cases]
    monkeypatch.setenv('DM_MEDIAN_TILE', tile)
    for (w, r, it), want in zip(cases, ref):
        got = run(x, w, r, iters=it, fill=True)
        assert raw_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    w, r, it = cases[4]
    assert equal(run(x, w, r, iters=it), median_fast(x, w, r, iters=it))


def test_arguments():
    t = dev(noise(5, 7))
    with pytest.raises(ValueError):
        engine.median_filter(t.float(), 3)
    with pytest.raises(ValueError):
        engine.median_filter(t.cpu(), 3)
    with pytest.raises(ValueError):
        engine.median_filter(t[None, None], 3)
    with pytest.raises(ValueError):
        engine.median_filter(noise(5, 7).astype(np.float32), 3)
    for bad in [0, 8, 1.5, True, None, '1']:
        with pytest.raises(ValueError):
            engine.median_filter(t, bad)
    for bad in [0, 65, 1.5, True, None]:
        with pytest.raises(ValueError):
            engine.median_filter(t, 3, iters=bad)
    for bad in [0, 50, -1, 2.0, True, None]:
        with pytest.raises(ValueError):
            engine.median_filter(t, 3, min_count=bad)
    with pytest.raises(ValueError):
        engine.median_filter(t, 1, min_count=10)
    with pytest.raises(ValueError):
        engine.median_filter(t, 3, weight=dev(np.zeros((7, 5))))
    with pytest.raises(ValueError):
        engine.median_filter(t, 3, weight=dev(np.zeros((5, 7), np.float32)))
    with pytest.raises(ValueError):
        engine.median_filter(t, 3, weight=torch.zeros((5, 7), dtype=torch.float64))
    with pytest.raises(ValueError):
        engine.median_filter(t, 3, weight=dev(np.zeros((2, 5, 7))))              # maps is [H][W]
    with pytest.raises(ValueError):
        engine.median_filter(t, 3, out=torch.empty((7, 5), dtype=torch.float64, device='cuda'))
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    assert tuple(engine.median_filter(e, 3).shape) == (0, 7)
    out, changed = engine.median_filter(e, 3, weight=e, fill=True, return_changed=True)
    assert tuple(out.shape) == (0, 7) and changed.dtype == torch.uint8 and tuple(changed.shape) == (0, 7)


# ---------------------------------------------------------------------------------------------
# 4. ImageCutSolver(median=) and shard.solve_image_sharded(median=)
# ---------------------------------------------------------------------------------------------
PAIR = dict(shape=(52, 100), seed=7, dx=2, h0=16, w0=32, ws=5)
MODES = ['elevation', 'elevation2', 'distance']
SPECKLE = (3, 0.25)
SMOOTH = (3, 10.0, 3.0)
MEDIAN = (1, 2)
E = (PAIR['ws'] - 1) // 2


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(*PAIR['shape'], seed=PAIR['seed'], dx=PAIR['dx'])


def crop(a, d):
    H, W = d.shape[-2:]
    return np.ascontiguousarray(np.asarray(a)[E:E + H, E:E + W])


@pytest.mark.parametrize('median_weight', [None, 'correlation'])
@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_median(pair, stride, median_weight):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES))
    plain = ImageCutSolver(a, b, **kw)
    d0, o0 = plain()
    assert plain.median is None
    dn, on = ImageCutSolver(a, b, median=None, median_weight=median_weight, **kw)()
    assert same_bits(dn, d0) and same_bits(on, o0)                      # median=None: the plain solver's bits
    solver = ImageCutSolver(a, b, median=MEDIAN, median_weight=median_weight, **kw)
    d1, o1 = solver()
    assert solver.median == MEDIAN and d1.shape == d0.shape
    w = o0 if median_weight == 'correlation' else None
    assert raw_bits(d1, median_fast(d0, w, *MEDIAN)[0])                 # stitch first, then the restatement
    assert np.array_equal(np.isnan(d1), np.isnan(d0)) and not same_bits(d1, d0)
    assert same_bits(o1, o0)
    assert solver.consistency_map is None and solver.speckle_map is None and solver.hole_map is None
    d2, _ = ImageCutSolver(a, b, median=3, median_weight=median_weight, **kw)()
    assert raw_bits(d2, median_fast(d0, w, 3)[0])
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, median=0, **kw)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, median=MEDIAN, median_weight='image', **kw)


@pytest.mark.parametrize('merge', [None, 'median'])
@pytest.mark.parametrize('fill', [None, 16])
def test_image_cut_solver_chain(pair, fill, merge):
    """stitch -> median -> speckle -> fill -> smooth."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=[12, 24], window_size=5, degree_map_mode=list(MODES), consistency=1.0,
              merge=merge)
    before = ImageCutSolver(a, b, **kw)
    d0, o0 = before()
    solver = ImageCutSolver(a, b, median=MEDIAN, median_weight='correlation', speckle=SPECKLE, fill=fill,
                            smooth=SMOOTH, **kw)
    d1, o1 = solver()
    d = dev(median_fast(d0, o0, *MEDIAN)[0])
    d, removed = engine.filter_speckles(d, *SPECKLE, return_removed=True)
    if fill is not None:
        d, holes = engine.fill_holes(d, fill, return_holes=True)
    d = engine.bilateral_filter(d, *SMOOTH, guide=dev(crop(a, d0)))
    assert same_bits(d1, host(d))
    assert same_bits(o1, o0) and same_bits(solver.consistency_map, before.consistency_map)
    assert np.array_equal(solver.speckle_map, host(removed).astype(bool))
    if fill is None:
        assert solver.hole_map is None
    else:
        assert np.array_equal(solver.hole_map, host(holes).astype(bool)) and np.isfinite(d1).all()
    # without the keyword the chain is the parent's
    kw2 = dict(speckle=SPECKLE, fill=fill, smooth=SMOOTH, **kw)
    p0, _ = ImageCutSolver(a, b, **kw2)()
    p1, _ = ImageCutSolver(a, b, median=None, median_weight='correlation', **kw2)()
    assert same_bits(p0, p1) and not same_bits(p0, d1)


@pytest.mark.parametrize('median_weight', [None, 'correlation'])
@pytest.mark.parametrize('consistency', [None, 1.0])
def test_solve_image_sharded_median_on_device(pair, consistency, median_weight):
    """shard.solve_image_sharded's own medianer (engine.median_filter on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = pair
    args = (a, b, [16, 32], [12, 24], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=consistency)
    same = shard.solve_image_sharded(*args, consistency=consistency, median=None, median_weight=median_weight)
    assert len(same) == len(ref) and all(same_bits(host(s), host(r)) for s, r in zip(same, ref))
    got = shard.solve_image_sharded(*args, consistency=consistency, median=MEDIAN, median_weight=median_weight)
    assert len(got) == len(ref)
    w = host(ref[1]) if median_weight == 'correlation' else None
    want = median_fast(host(ref[0]), w, *MEDIAN)[0]
    assert raw_bits(host(got[0]), want) and not same_bits(want, host(ref[0]))
    for q, r in zip(got[1:], ref[1:]):
        assert same_bits(host(q), host(r))
    # the whole chain: the median comes before the speckle filter, the fill and the smoothing
    chain = shard.solve_image_sharded(*args, consistency=consistency, median=MEDIAN, median_weight=median_weight,
                                      speckle=SPECKLE, fill=16, smooth=SMOOTH)
    assert len(chain) == len(ref) + 2
    d, removed = engine.filter_speckles(dev(want), *SPECKLE, return_removed=True)
    d, holes = engine.fill_holes(d, 16, return_holes=True)
    d = engine.bilateral_filter(d, *SMOOTH, guide=dev(crop(a, want)))
    assert same_bits(host(chain[0]), host(d))
    assert torch.equal(chain[-2], removed) and torch.equal(chain[-1], holes)
    for q, r in zip(chain[1:-2], ref[1:]):
        assert same_bits(host(q), host(r))
