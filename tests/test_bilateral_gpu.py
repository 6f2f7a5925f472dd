"""Joint bilateral filter on the GPU: dm_bilateral_filter (engine.bilateral_filter) against the
plain-loop restatement of the definition (tests/test_bilateral_host.py: bilateral_restate) bit
for bit -- over shapes that straddle the tile sides, the three guide kinds, the uint8 path
against the float64 path, special values, holes on tile seams and in the halo corner, the fill
flag, several passes out of place and in place, batches, a side stream, run-to-run and tile-side
independence, the argument errors, and the ImageCutSolver / solve_image_sharded keyword."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import raw_bits, same_bits
from test_bilateral_host import bilateral_restate, den, image, noise

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (64, 64), (65, 130), (129, 67)]
PARAMS = [(1, 0.5, 1.0), (3, 10.0, 3.0), (7, 2.0, 5.0)]
GUIDES = ['self', 'f64', 'u8']
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']
INF = float('inf')


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def fguide(H, W, seed=0, share=0.0):
    """A float64 guide: noise on a grid of 1/16 (differences repeat), `share` of it NaN."""
    rng = np.random.default_rng(31 * H + W + seed)
    g = np.rint(rng.normal(0, 3, (H, W)) * 16) / 16
    g[rng.uniform(size=(H, W)) < share] = np.nan
    return g


def guide_of(kind, H, W, seed=0):
    return None if kind == 'self' else fguide(H, W, seed) if kind == 'f64' else image(H, W, seed)


def run(x, guide, r, sc, ss, **kw):
    got = engine.bilateral_filter(x if torch.is_tensor(x) else dev(x), r, sc, ss,
                                  guide=guide if torch.is_tensor(guide) else dev(guide), return_filled=True, **kw)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.uint8
    return host(got[0]), host(got[1])


def equal(got, want):
    return same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def check(x, guide, r, sc, ss, iters=1, fill=False):
    want = bilateral_restate(x, guide, r, den(sc), den(ss), iters=iters, fill=fill)
    got = run(x, guide, r, sc, ss, iters=iters, fill=fill)
    assert equal(got, want)
    keep = ~np.isfinite(got[0])      # holes that stayed: the input's own bits
    assert raw_bits(got[0][keep], np.asarray(x, dtype=np.float64)[keep])
    if not fill:
        assert not got[1].any() and np.array_equal(keep, ~np.isfinite(x))
    return want


# ---------------------------------------------------------------------------------------------
# 1. random maps against the restatement
# ---------------------------------------------------------------------------------------------
_REF = {}


def random_case(shape, params, kind):
    """(map, guide, the restatement's outputs), computed once per case."""
    key = (shape, params, kind)
    if key not in _REF:
        x = noise(*shape)
        if shape == (1, 1):
            x[0, 0] = 2.5
        g = guide_of(kind, *shape)
        _REF[key] = (x, g, bilateral_restate(x, g, params[0], den(params[1]), den(params[2])))
    return _REF[key]


@pytest.mark.parametrize('tile', [None, '32'], ids=['tile-as-built', 'tile-32'])
@pytest.mark.parametrize('kind', GUIDES)
@pytest.mark.parametrize('params', PARAMS, ids=lambda p: '%d-%g-%g' % p)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_maps(shape, params, kind, tile, monkeypatch):
    """Maps of this size get tiles of 16 cells as built; DM_BILATERAL_TILE=32 forces the other side."""
    if tile is not None:
        monkeypatch.setenv('DM_BILATERAL_TILE', tile)
    x, g, want = random_case(shape, params, kind)
    got = run(x, g, *params)
    assert equal(got, want) and not got[1].any()
    assert raw_bits(got[0][~np.isfinite(x)], x[~np.isfinite(x)])
    if shape == (65, 130) and params[0] == 3:
        fin = np.isfinite(x)
        assert not raw_bits(want[0][fin], x[fin])      # it does smooth


@pytest.mark.parametrize('kind', GUIDES)
def test_radius_15_flat_colour(kind):
    x = noise(20, 37)
    check(x, guide_of(kind, 20, 37), 15, INF, 4.0)
    if kind == 'u8':
        check(x, guide_of(kind, 20, 37), 15, INF, INF, fill=True)      # the window's plain mean


@pytest.mark.parametrize('params', PARAMS + [(15, INF, 4.0)], ids=lambda p: '%d-%g-%g' % p)
@pytest.mark.parametrize('shape', [(33, 31), (65, 130)], ids=lambda s: '%dx%d' % s)
def test_u8_path_equals_f64_path(shape, params):
    x, g = noise(*shape, seed=2), image(*shape, seed=2)
    for fill in (False, True):
        a = run(x, g, *params, fill=fill)
        b = run(x, g.astype(np.float64), *params, fill=fill)
        assert raw_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------
# 2. special values, holes on the seams
# ---------------------------------------------------------------------------------------------
def test_infinities_are_holes():
    x = noise(33, 31, seed=3)
    x[4, 5], x[20, 30], x[32, 0] = np.inf, -np.inf, np.inf
    for kind in GUIDES:
        check(x, guide_of(kind, 33, 31), 3, 10.0, 3.0)
    want = check(x, image(33, 31), 3, 10.0, 3.0, fill=True)
    assert want[1][4, 5] and want[1][20, 30] and want[1][32, 0]


def test_non_finite_guide():
    x = noise(33, 67, seed=4)
    g = fguide(33, 67, share=0.1)
    g[3, 3], g[32, 66], g[0, 32] = np.inf, -np.inf, np.inf
    for fill in (False, True):
        want = check(x, g, 3, 10.0, 3.0, fill=fill)
        bad = ~np.isfinite(g)
        assert raw_bits(want[0][bad], x[bad])      # copied, hole or not
    per_map = np.stack([g, fguide(33, 67, seed=1, share=0.3)])
    check(np.stack([x, noise(33, 67, seed=5)]), per_map, 2, 4.0, 2.0, fill=True)


def test_negative_zero_and_huge_values():
    x = np.full((9, 40), -0.0)
    x[4, 7] = 0.0
    x[2, 35] = np.nan
    for kind in GUIDES:
        want = check(x, guide_of(kind, 9, 40), 2, 4.0, 2.0)
        assert raw_bits(want[0][np.isfinite(x)], np.zeros(np.isfinite(x).sum()))      # +0: num starts at +0
    big = noise(33, 40, seed=6) * 2e299      # near 1e300: c * c overflows when the map guides itself
    for kind in GUIDES:
        for sc in (INF, 1e150):              # -(inf) / inf is NaN, -(inf) / den is -inf: skipped either way
            want = check(big, guide_of(kind, 33, 40), 3, sc, 3.0)
            fin = np.isfinite(big)
            assert raw_bits(want[0][fin], big[fin]) == (kind == 'self')
    huge = np.abs(noise(33, 40, seed=6)) * 3e306      # num overflows: the same inf as the restatement's
    for kind in ('f64', 'u8'):
        want = bilateral_restate(huge, guide_of(kind, 33, 40), 3, den(INF), den(3.0))
        got = run(huge, guide_of(kind, 33, 40), 3, INF, 3.0)
        assert same_bits(got[0], want[0])
        assert np.isinf(want[0]).sum() > 100 and np.isfinite(huge[np.isinf(want[0])]).all()


def test_tiny_sigma_color_returns_the_input():
    x = noise(65, 70, seed=7)
    want = check(x, None, 3, 1e-9, 3.0)
    assert raw_bits(want[0], x)
    i, j = np.mgrid[0:65, 0:70]
    g = fguide(65, 70) + 64.0 * j + 8192.0 * i     # no two cells of a window share a guide value
    assert raw_bits(check(x, g, 3, 1e-9, 3.0)[0], x)
    u = ((7 * i + j) % 256).astype(np.uint8)         # distinct within a 7 x 7 window
    assert raw_bits(check(x, u, 3, 1e-3, 3.0)[0], x)


def test_all_holes_and_one_finite_cell():
    allh = np.full((40, 37), np.nan)
    allh[1, 1], allh[32, 33], allh[39, 36] = np.inf, -np.inf, -np.nan
    for kind in GUIDES:
        for fill in ([False] if kind == 'self' else [False, True]):
            got = run(allh, guide_of(kind, 40, 37), 3, 10.0, 3.0, fill=fill)
            assert raw_bits(got[0], allh) and not got[1].any()
    one = allh.copy()
    one[31, 32] = 7.5
    for kind in GUIDES:
        want = check(one, guide_of(kind, 40, 37), 3, 10.0, 3.0)
        assert want[0][31, 32] == 7.5
    want = check(one, np.zeros((40, 37), np.uint8), 3, 10.0, 3.0, fill=True)
    assert want[1].sum() == 48 and np.abs(want[0][28:35, 29:36] - 7.5).max() <= 4 * 7.5 * 2.0 ** -53   # (w 7.5) / w


@pytest.mark.parametrize('tile', ['16', '32'])
@pytest.mark.parametrize('kind', GUIDES)
def test_holes_on_tile_seams_and_halo_corners(kind, tile, monkeypatch):
    monkeypatch.setenv('DM_BILATERAL_TILE', tile)
    x = noise(70, 100, seed=8, share=0.0)
    x[32, :] = np.nan                    # the first row beyond a tile of 32 (and of 16)
    x[:, 32] = np.nan
    x[16, 40:60] = np.nan
    x[40:60, 64] = np.nan
    for c in ((34, 34), (35, 35), (29, 29), (28, 28), (63, 67), (67, 95), (18, 18), (13, 13)):
        x[c] = np.nan                    # the halo's corners at r = 3
    check(x, guide_of(kind, 70, 100), 3, 10.0, 3.0)
    if kind != 'self':
        check(x, guide_of(kind, 70, 100), 3, 10.0, 3.0, fill=True)


# ---------------------------------------------------------------------------------------------
# 3. fill, passes, in place
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'u8'])
def test_fill(kind):
    x = noise(65, 70, seed=9, share=0.3)
    x[20:40, 25:45] = np.nan             # wider than the window: the core survives one pass
    g = guide_of(kind, 65, 70)
    want = check(x, g, 3, 10.0, 3.0, fill=True)
    hole = np.isnan(x)
    assert want[1][~hole].sum() == 0 and want[1][:20][hole[:20]].all()
    assert np.isnan(want[0][23:37, 28:42]).all() and np.isfinite(want[0][22, 30])
    left = [int(np.isnan(check(x, g, 3, 10.0, 3.0, iters=k, fill=True)[0]).sum()) for k in (2, 3, 4)]
    assert left == [8 * 8, 2 * 2, 0]


@pytest.mark.parametrize('kind', GUIDES)
@pytest.mark.parametrize('iters', [1, 2, 3])
def test_passes_out_of_place_and_in_place(kind, iters):
    x, g = noise(65, 70, seed=10), guide_of(kind, 65, 70)
    for fill in ([False] if kind == 'self' else [False, True]):
        want = check(x, g, 2, 4.0, 2.0, iters=iters, fill=fill)
        t = dev(x)
        got = engine.bilateral_filter(t, 2, 4.0, 2.0, guide=dev(g), iters=iters, fill=fill, out=t, return_filled=True)
        assert got[0] is t and same_bits(host(t), want[0]) and np.array_equal(host(got[1]), want[1])
        src, o = dev(x), torch.empty((65, 70), dtype=torch.float64, device='cuda')
        assert engine.bilateral_filter(src, 2, 4.0, 2.0, guide=dev(g), iters=iters, fill=fill, out=o) is o
        assert same_bits(host(o), want[0]) and raw_bits(host(src), x)      # the input is untouched


@pytest.mark.parametrize('kind', ['f64', 'u8'])
def test_batch_equals_single_calls(kind):
    shape = (33, 70)
    x = np.stack([noise(*shape, seed=1), np.full(shape, np.nan), noise(*shape, seed=2, share=0.5)])
    shared = guide_of(kind, *shape)
    per_map = np.stack([guide_of(kind, *shape, seed=s) for s in (0, 1, 2)])
    for g in (shared, per_map, None):
        got = run(x, g, 3, 10.0, 3.0, fill=g is not None)
        assert got[0].shape == x.shape
        for m in range(3):
            one = run(x[m], g if g is None or g.ndim == 2 else g[m], 3, 10.0, 3.0, fill=g is not None)
            assert one[0].shape == shape and raw_bits(got[0][m], one[0]) and np.array_equal(got[1][m], one[1])
        assert equal(got, bilateral_restate(x, g, 3, den(10.0), den(3.0), fill=g is not None))
        assert raw_bits(got[0][1], x[1])


def test_side_stream():
    x, g = noise(65, 130, seed=7), image(65, 130)
    want = bilateral_restate(x, g, 3, den(10.0), den(3.0), iters=2)
    s = torch.cuda.Stream()
    t, gt = dev(x), dev(g)
    torch.cuda.synchronize()
    got = engine.bilateral_filter(t, 3, 10.0, 3.0, guide=gt, iters=2, return_filled=True, stream=s)
    with torch.cuda.stream(s):
        h = [q.cpu() for q in got]          # a read on that stream
    assert same_bits(h[0].numpy(), want[0]) and np.array_equal(h[1].numpy(), want[1])


def test_consecutive_calls_are_bit_identical():
    x = noise(129, 67, seed=8)
    for kind in GUIDES:
        t, g = dev(x), dev(guide_of(kind, 129, 67))
        a, b = run(t, g, 7, 2.0, 5.0), run(t, g, 7, 2.0, 5.0)
        assert raw_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('tile', ['16', '32', '48'])
def test_tile_side_is_invisible(tile, monkeypatch):
    """DM_BILATERAL_TILE (16 or 32; anything else: the side as built) moves the seams only."""
    cases = [(noise(65, 130, seed=9), kind, p, it) for kind in GUIDES
             for p, it in (((3, 10.0, 3.0), 2), ((15, 20.0, 6.0), 1))]
    ref = [run(x, guide_of(k, 65, 130), *p, iters=it, fill=k != 'self') for x, k, p, it in cases]
    monkeypatch.setenv('DM_BILATERAL_TILE', tile)
    for (x, k, p, it), r in zip(cases, ref):
        got = run(x, guide_of(k, 65, 130), *p, iters=it, fill=k != 'self')
        assert raw_bits(got[0], r[0]) and np.array_equal(got[1], r[1])
    x, k, p, it = cases[2]
    assert equal(run(x, guide_of(k, 65, 130), *p, iters=it), bilateral_restate(x, guide_of(k, 65, 130), p[0], den(p[1]),
                                                                               den(p[2]), iters=it))


def test_arguments():
    t = dev(noise(5, 7))
    with pytest.raises(ValueError):
        engine.bilateral_filter(t.float(), 3, 1.0, 1.0)
    with pytest.raises(ValueError):
        engine.bilateral_filter(t.cpu(), 3, 1.0, 1.0)
    with pytest.raises(ValueError):
        engine.bilateral_filter(t[None, None], 3, 1.0, 1.0)
    for bad in [(0, 1.0, 1.0), (16, 1.0, 1.0), (1.5, 1.0, 1.0), (True, 1.0, 1.0), (3, 0.0, 1.0), (3, 1.0, -1.0),
                (3, float('nan'), 1.0), (3, 1.0, None), (3, 1e-200, 1.0)]:
        with pytest.raises(ValueError):
            engine.bilateral_filter(t, *bad)
    for bad in [0, 65, 1.5, True, None]:
        with pytest.raises(ValueError):
            engine.bilateral_filter(t, 3, 1.0, 1.0, iters=bad)
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, fill=True)                                   # needs a guide
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, guide=dev(np.zeros((7, 5))))
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, guide=dev(np.zeros((5, 7), np.float32)))
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, guide=torch.zeros((5, 7), dtype=torch.float64))
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, guide=dev(np.zeros((2, 5, 7))))              # maps is [H][W]
    with pytest.raises(ValueError):
        engine.bilateral_filter(t, 3, 1.0, 1.0, out=torch.empty((7, 5), dtype=torch.float64, device='cuda'))
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    assert tuple(engine.bilateral_filter(e, 3, 1.0, 1.0).shape) == (0, 7)
    out, filled = engine.bilateral_filter(e, 3, 1.0, 1.0, guide=e.to(torch.uint8), fill=True, return_filled=True)
    assert tuple(out.shape) == (0, 7) and filled.dtype == torch.uint8 and tuple(filled.shape) == (0, 7)


# ---------------------------------------------------------------------------------------------
# 4. ImageCutSolver(smooth=) and shard.solve_image_sharded(smooth=)
# ---------------------------------------------------------------------------------------------
PAIR = dict(shape=(52, 100), seed=7, dx=2, h0=16, w0=32, ws=5)
MODES = ['elevation', 'elevation2', 'distance']
SPECKLE = (3, 0.25)
SMOOTH = (3, 10.0, 3.0)
E = (PAIR['ws'] - 1) // 2


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(*PAIR['shape'], seed=PAIR['seed'], dx=PAIR['dx'])


def crop(a, d):
    H, W = d.shape[-2:]
    return np.ascontiguousarray(np.asarray(a)[E:E + H, E:E + W])


@pytest.mark.parametrize('smooth_guide', ['image', 'self'])
@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_smooth(pair, stride, smooth_guide):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES))
    plain = ImageCutSolver(a, b, **kw)
    d0, o0 = plain()
    assert plain.smooth is None
    dn, on = ImageCutSolver(a, b, smooth=None, smooth_guide=smooth_guide, **kw)()
    assert same_bits(dn, d0) and same_bits(on, o0)                      # smooth=None: the plain solver's bits
    solver = ImageCutSolver(a, b, smooth=SMOOTH, smooth_guide=smooth_guide, **kw)
    d1, o1 = solver()
    assert solver.smooth == SMOOTH and d1.shape == d0.shape
    g = crop(a, d0) if smooth_guide == 'image' else None
    assert g is None or (g.dtype == np.uint8 and g.shape == d0.shape[-2:])
    assert same_bits(d1, host(engine.bilateral_filter(dev(d0), *SMOOTH, guide=dev(g))))
    assert same_bits(d1, bilateral_restate(d0, g, SMOOTH[0], den(SMOOTH[1]), den(SMOOTH[2]))[0])
    assert np.array_equal(np.isnan(d1), np.isnan(d0)) and not same_bits(d1, d0)
    assert same_bits(o1, o0)
    assert solver.consistency_map is None and solver.speckle_map is None and solver.hole_map is None
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, smooth=(0, 1.0, 1.0), **kw)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, smooth=SMOOTH, smooth_guide='img2', **kw)


@pytest.mark.parametrize('fill', [None, 16])
@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_chain(pair, stride, fill):
    """stitch -> speckle -> fill -> smooth."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES),
              consistency=1.0, speckle=SPECKLE, fill=fill)
    before = ImageCutSolver(a, b, **kw)
    d0, o0 = before()
    solver = ImageCutSolver(a, b, smooth=SMOOTH, **kw)
    d1, o1 = solver()
    g = crop(a, d0)
    assert same_bits(d1, host(engine.bilateral_filter(dev(d0), *SMOOTH, guide=dev(g))))
    assert same_bits(d1, bilateral_restate(d0, g, SMOOTH[0], den(SMOOTH[1]), den(SMOOTH[2]))[0])
    assert same_bits(o1, o0) and same_bits(solver.consistency_map, before.consistency_map)
    assert np.array_equal(solver.speckle_map, before.speckle_map)
    if fill is None:
        assert solver.hole_map is None and np.isnan(d0).any()
        assert np.array_equal(np.isnan(d1), np.isnan(d0))               # the NaN positions survive the smoothing
    else:
        assert np.array_equal(solver.hole_map, before.hole_map) and np.isfinite(d1).all()


@pytest.mark.parametrize('smooth_guide', ['image', 'self'])
@pytest.mark.parametrize('consistency', [None, 1.0])
def test_solve_image_sharded_smooth_on_device(pair, consistency, smooth_guide):
    """shard.solve_image_sharded's own smoother (engine.bilateral_filter on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = pair
    args = (a, b, [16, 32], [12, 24], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=consistency)
    same = shard.solve_image_sharded(*args, consistency=consistency, smooth=None, smooth_guide=smooth_guide)
    assert len(same) == len(ref) and all(same_bits(host(s), host(r)) for s, r in zip(same, ref))
    got = shard.solve_image_sharded(*args, consistency=consistency, smooth=SMOOTH, smooth_guide=smooth_guide)
    assert len(got) == len(ref)
    g = dev(crop(a, ref[0])) if smooth_guide == 'image' else None
    assert same_bits(host(got[0]), host(engine.bilateral_filter(ref[0], *SMOOTH, guide=g)))
    for q, r in zip(got[1:], ref[1:]):
        assert same_bits(host(q), host(r))
    # the whole chain: the smoothing comes after the fill
    chain = shard.solve_image_sharded(*args, consistency=consistency, speckle=SPECKLE, fill=16, smooth=SMOOTH,
                                      smooth_guide=smooth_guide)
    base = shard.solve_image_sharded(*args, consistency=consistency, speckle=SPECKLE, fill=16)
    assert len(chain) == len(base) == len(ref) + 2
    assert same_bits(host(chain[0]), host(engine.bilateral_filter(base[0], *SMOOTH, guide=g)))
    for q, r in zip(chain[1:], base[1:]):
        assert torch.equal(q, r) if q.dtype == torch.uint8 else same_bits(host(q), host(r))
