"""Overlap-merging stitch on the GPU: dm_stitch_merge against the plain-loop restatement of its
definition (tests/test_merge_host.py: merge_restate) on crafted maps, rule 'last' against
dm_stitch / dm_stitch_fb, the engine's own tiles merged under every rule, and the
ImageCutSolver keyword.  Every float comparison is bitwise (int64 views, NaN positions equal):
the products, sums, quotients and square roots are correctly rounded on both sides and taken in
the same order; counts are compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fb_host import same_bits
from test_merge_host import RULES, merge_restate

pytestmark = pytest.mark.gpu

MODES = ['elevation', 'elevation2', 'distance']
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']
H0, W0 = 5, 7
GEOMS = [((3, 2), (2, 3)), ((4, 3), (1, 2)), ((2, 2), (5, 7)), ((2, 3), (6, 9))]     # (n, stride)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def same_maps(got, want):
    """(d_map, out_map, err or None, spread, count) of the engine against the restatement's."""
    assert len(got) == len(want) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, k
            continue
        g = host(g)
        assert g.shape == w.shape, k
        if k == 4:
            assert g.dtype == np.uint8 and np.array_equal(g, w)
        elif not same_bits(g, w):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError('output %d differs at %s: %r != %r' % (k, bad[:4].tolist(), g[tuple(bad[0])],
                                                                        w[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------
# 1. the kernel on crafted maps
# ---------------------------------------------------------------------------------------------
def crafted(n):
    """T = n0 n1 tiles of 5 x 7 cells like test_fb_gpu.crafted(): matches near their cells with
    many round trips returning, specials (NaN, +-inf, +-1e300, off-tile, half-way cases) in rows
    and columns, B holding NaN where walks land, NaN / inf scores at valid cells, and two tiles
    whose every cell has the same elevation, distance and score (the ties of CENTER / MEDIAN)."""
    T, h, w = n[0] * n[1], H0, W0
    rng = np.random.default_rng(5 + T)
    ii, jj = np.mgrid[0:h, 0:w]
    F, B = np.empty((T, 3, h, w)), np.empty((T, 3, h, w))
    F[:, 0] = ii + rng.normal(0, 0.8, (T, h, w))
    F[:, 1] = jj + rng.normal(0, 0.8, (T, h, w))
    F[:, 2] = rng.uniform(0, 5, (T, h, w))
    B[:, 0] = ii + rng.normal(0, 0.4, (T, h, w))
    B[:, 1] = jj + rng.normal(0, 0.4, (T, h, w))
    B[:, 2] = rng.uniform(0, 5, (T, h, w))
    # tiles 1 and T - 2: exact integer matches one column to the left, an identity walk back,
    # equal scores -> equal values (elevation 1, distance 1) wherever the two overlap
    for t in (1, T - 2):
        F[t, 0], F[t, 1], F[t, 2] = ii, jj - 1.0, 2.5
        B[t, 0], B[t, 1] = ii, jj + 1.0
    F[T - 2, 1, :, 0] = 0.0              # (column -1 is off the tile: keep the first column on it)
    F[1, 1, :, 0] = 0.0
    sp_r = [2.5, -0.5, -0.51, h - 0.5, np.nextafter(h - 0.5, 0), np.nan, np.inf, -np.inf, 1e300, -1e300]
    sp_c = [2.5, -0.5, -0.51, w - 0.5, np.nextafter(w - 0.5, 0), np.nan, np.inf, -np.inf, 1e300, -1e300]
    for k, v in enumerate(sp_r):
        F[0, 0].flat[k] = v
        F[T - 1, 0].flat[34 - k] = v
    for k, v in enumerate(sp_c):
        F[0, 1].flat[12 + k] = v
        F[2, 1].flat[3 * k + 1] = v
    for k, (u, v) in enumerate(zip(sp_r, reversed(sp_c))):
        F[2, 0].flat[20 + k], F[2, 1].flat[20 + k] = u, v
    B[0, 0, 2, 3] = np.nan
    B[0, 1, 4, 6] = np.inf
    B[2, :, 1, 1] = np.nan
    F[0, :2, 4, 0] = (2.0, 3.0)
    F[0, :2, 4, 1] = (4.25, 5.75)
    F[2, :2, 4, 4] = (0.75, 1.25)
    F[3, 2].flat[[0, 9, 17, 30]] = (np.nan, np.inf, -np.inf, 1e300)      # scores of valid cells
    F[T - 1, 2].flat[[2, 16, 33]] = (np.nan, -np.inf, np.nan)
    return F, B


def _cases():
    yield None, None
    for tol in (0.0, 1.0, float('inf')):
        yield True, tol


@pytest.mark.parametrize('n,stride', GEOMS)
def test_stitch_merge_crafted(n, stride):
    F, B = crafted(n)
    f, b = dev(F), dev(B)
    seen = {'valid': 0, 'cut': 0, 'tie': 0}
    for bidir, tol in _cases():
        Bh, bd = (B, b) if bidir else (None, None)
        for rule in RULES:
            for mc in ((1,) if rule == 'last' else (1, 2, 3)):
                want = merge_restate(F, Bh, n, stride, MODES, tol, rule, mc)
                got = engine.stitch_merge(f, bd, n, H0, W0, stride, MODES, tol, rule, mc)
                same_maps(got, want)
                seen['valid'] += int(want[4].sum())
                seen['cut'] += int(((want[4] > 0) & (want[4] < mc)).sum())
                seen['tie'] += int((want[3][0][want[4] > 1] == 0).sum())
    assert same_bits(host(f), F) and same_bits(host(b), B)             # inputs untouched
    assert seen['valid'] > 0
    if stride in ((2, 3), (1, 2)):     # overlapping tiles: min_count cuts, equal values in two tiles
        assert seen['cut'] > 0 and seen['tie'] > 0
        assert merge_restate(F, None, n, stride, MODES, None, 'last')[4].max() >= 4
    else:
        assert merge_restate(F, None, n, stride, MODES, None, 'last')[4].max() == 1


def test_stitch_merge_optional_outputs_and_stream():
    n, stride = GEOMS[0]
    F, B = crafted(n)
    f, b = dev(F), dev(B)
    want = merge_restate(F, B, n, stride, MODES, 1.0, 'median', 2)
    Hout, Wout = want[1].shape
    arr = (ctypes.c_int32 * 3)(0, 1, 2)
    guard = 3.25

    def call(bwd, err, spread, count, stream=None):
        d = torch.full((3, Hout, Wout), guard, dtype=torch.float64, device='cuda')
        s = torch.full((Hout, Wout), guard, dtype=torch.float64, device='cuda')
        L.check(L.load().dm_stitch_merge(L.ptr(f), L.ptr(bwd), n[0], n[1], H0, W0, stride[0], stride[1], arr, 3,
                                         1.0, L.MERGE_RULES['median'], 2, L.ptr(d), L.ptr(s), L.ptr(err),
                                         L.ptr(spread), L.ptr(count), L.stream_handle(stream)), 'dm_stitch_merge')
        return d, s

    d, s = call(b, None, None, None)                       # every optional output NULL
    torch.cuda.synchronize()
    assert same_bits(host(d), want[0]) and same_bits(host(s), want[1])
    e = torch.empty((Hout, Wout), dtype=torch.float64, device='cuda')
    c = torch.empty((Hout, Wout), dtype=torch.uint8, device='cuda')
    d, s = call(b, e, None, c)
    assert same_bits(host(e), want[2]) and np.array_equal(host(c), want[4]) and same_bits(host(d), want[0])
    one = merge_restate(F, None, n, stride, MODES, None, 'median', 2)
    sp = torch.empty((3, Hout, Wout), dtype=torch.float64, device='cuda')
    d, s = call(None, None, sp, None)
    assert same_bits(host(d), one[0]) and same_bits(host(s), one[1]) and same_bits(host(sp), one[3])
    # a side stream, through the engine
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = engine.stitch_merge(f, b, n, H0, W0, stride, MODES, 1.0, 'median', 2, stream=side)
    side.synchronize()
    same_maps(got, want)
    # one mode, not the first expression
    same_maps(engine.stitch_merge(f, b, n, H0, W0, stride, ['distance'], 1.0, 'feather'),
              merge_restate(F, B, n, stride, ['distance'], 1.0, 'feather'))
    # the engine's own argument checks
    with pytest.raises(ValueError):
        engine.stitch_merge(f, b, n, H0, W0, stride, MODES, None)
    with pytest.raises(ValueError):
        engine.stitch_merge(f, None, n, H0, W0, stride, MODES, 1.0)
    with pytest.raises(ValueError):
        engine.stitch_merge(f[:-1], b[:-1], n, H0, W0, stride, MODES, 1.0)
    with pytest.raises(ValueError):
        engine.stitch_merge(f, b, n, H0, W0, stride, MODES, 1.0, 'last', 2)


# ---------------------------------------------------------------------------------------------
# 2. the parity anchor: rule 'last' is dm_stitch / dm_stitch_fb
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,stride', GEOMS + [((3, 5), (37, 19))])
def test_last_is_stitch(n, stride):
    if stride == (37, 19):         # more than one block, sides that are no multiple of anything
        h0, w0 = 45, 51
        T = n[0] * n[1]
        rng = np.random.default_rng(23)
        ii, jj = np.mgrid[0:h0, 0:w0]
        F = np.stack([np.stack([ii + rng.normal(0, 1.5, (h0, w0)), jj + rng.normal(0, 1.5, (h0, w0)),
                                rng.uniform(0, 5, (h0, w0))]) for _ in range(T)])
        B = np.stack([np.stack([ii + rng.normal(0, 0.7, (h0, w0)), jj + rng.normal(0, 0.7, (h0, w0)),
                                rng.uniform(0, 5, (h0, w0))]) for _ in range(T)])
        F[rng.uniform(size=F.shape) < 0.01] = np.nan
        B[rng.uniform(size=B.shape) < 0.01] = np.nan
    else:
        h0, w0 = H0, W0
        F, B = crafted(n)
    f, b = dev(F), dev(B)
    d0, s0 = engine.stitch(f, n, h0, w0, stride, MODES)
    d, s, e, sp, cnt = engine.stitch_merge(f, None, n, h0, w0, stride, MODES, rule='last')
    assert e is None and same_bits(host(d), host(d0)) and same_bits(host(s), host(s0))
    assert np.isinf(host(d0)).any() or stride == (37, 19)       # half-finite cells pass through as they are
    for tol in (0.0, 1.0, float('inf')):
        d0, s0, e0 = engine.stitch_fb(f, b, n, h0, w0, stride, MODES, tol)
        d, s, e, sp, cnt = engine.stitch_merge(f, b, n, h0, w0, stride, MODES, tol, 'last')
        assert same_bits(host(d), host(d0)) and same_bits(host(s), host(s0)) and same_bits(host(e), host(e0))
    if stride == (37, 19):
        assert cnt.numel() > 256 and int(cnt.max()) == 6       # 2 rows x 3 columns of tiles overlap


# ---------------------------------------------------------------------------------------------
# 3. the engine's own tiles: S = 32 at stride 16, window 5
# ---------------------------------------------------------------------------------------------
PAIR = dict(shape=(68, 84), seed=7, dx=2, S=32, stride=(16, 16), ws=5)


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(*PAIR['shape'], seed=PAIR['seed'], dx=PAIR['dx'])


@pytest.fixture(scope='module')
def solved(pair):
    a, b = pair
    S, ws = PAIR['S'], PAIR['ws']
    n, org = engine.cut_grid(a.shape, [S, S], PAIR['stride'], ws)
    assert n == [2, 3]
    fwd, bwd = engine.solve_tiles_bidir(a, b, org, S, S, ws, NCC, True, False, 3, 3, 'average')
    return n, fwd, bwd


@pytest.mark.parametrize('rule', RULES)
def test_engine_tiles_merged(solved, rule):
    n, fwd, bwd = solved
    S = PAIR['S']
    want = merge_restate(host(fwd), host(bwd), n, PAIR['stride'], MODES, 1.0, rule)
    got = engine.stitch_merge(fwd, bwd, n, S, S, PAIR['stride'], MODES, 1.0, rule)
    same_maps(got, want)
    assert want[4].max() == 4 and np.isnan(want[0]).mean() < 0.5
    if rule == 'last':
        assert np.isnan(want[0]).any()
    want = merge_restate(host(fwd), None, n, PAIR['stride'], MODES, None, rule)
    same_maps(engine.stitch_merge(fwd, None, n, S, S, PAIR['stride'], MODES, rule=rule), want)


# ---------------------------------------------------------------------------------------------
# 4. ImageCutSolver(merge=)
# ---------------------------------------------------------------------------------------------
def test_image_cut_solver_merge(pair, solved):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    n, fwd, bwd = solved
    S = PAIR['S']
    kw = dict(image_size=[S, S], stride=list(PAIR['stride']), window_size=PAIR['ws'], degree_map_mode=list(MODES))
    sol = ImageCutSolver(a, b, merge='median', consistency=1.0, fill=16, **kw)
    d, o = sol()
    H, W = 16 * (n[0] - 1) + S, 16 * (n[1] - 1) + S
    assert d.shape == (3, H, W) and d.dtype == np.float64 and o.shape == (H, W) and o.dtype == np.float64
    assert sol.coverage_map.shape == (H, W) and sol.coverage_map.dtype == np.uint8 and sol.coverage_map.max() == 4
    assert sol.spread_map.shape == (3, H, W) and sol.spread_map.dtype == np.float64
    assert sol.consistency_map.shape == (H, W) and sol.hole_map.shape == (3, H, W) and sol.hole_map.dtype == bool
    assert np.isfinite(d).all()
    dm, om, em, sm, cm = engine.stitch_merge(fwd, bwd, n, S, S, PAIR['stride'], MODES, 1.0, 'median')
    assert np.array_equal(sol.hole_map, np.isnan(host(dm))) and sol.hole_map.mean() < 0.5
    filled = engine.fill_holes(dm, 16)
    assert same_bits(d, host(filled)) and same_bits(o, host(om))
    assert same_bits(sol.consistency_map, host(em)) and same_bits(sol.spread_map, host(sm))
    assert np.array_equal(sol.coverage_map, host(cm))
    # fewer holes than the overwriting stitch leaves, none added
    last = np.isnan(host(engine.stitch_fb(fwd, bwd, n, S, S, PAIR['stride'], MODES, 1.0)[0]))
    assert not (sol.hole_map & ~last).any() and sol.hole_map.sum() < last.sum()
    # one direction, no fill: (d_map, out_map) with the spread and the count on the solver
    one = ImageCutSolver(a, b, merge='feather', merge_min_count=2, **kw)
    d1, o1 = one()
    dm, om, em, sm, cm = engine.stitch_merge(fwd, None, n, S, S, PAIR['stride'], MODES, rule='feather', min_count=2)
    assert em is None and one.consistency_map is None and one.hole_map is None
    assert same_bits(d1, host(dm)) and same_bits(o1, host(om)) and same_bits(one.spread_map, host(sm))
    assert np.array_equal(one.coverage_map, host(cm))
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, merge='mean', **kw)
    plain = ImageCutSolver(a, b, **kw)
    assert plain.merge is None and plain.coverage_map is None and plain.spread_map is None
