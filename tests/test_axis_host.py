"""Pairs displaced along both axes, both signs, host side (no GPU): the cases that tests/test_axis_gpu.py
runs on the device, and the conditions the restatements must meet on them before the kernels are asked to.

Everywhere else the truth of the post-processing stages is (0, dx): the row plane ('elevation2') is 0, and
+-0 is its own negation.  Here img2[y, x] = img1[y + dy, x + dx] (test_prior_lattice.two_axis_pair), so the
true (d_row, d_col) = ('elevation2', 'elevation') is (dy, dx), for the five SHIFTS.

  stage_case     the pair, the offset (m, m + 1) with m = r + s + 2, the true planes and the planes of the
                 truth plus a seeded integer offset in [-s, s]^2 per cell, on 20 x 37 cells (more than one
                 32 x 8 tile both ways) or their transpose.  The true candidate of every cell is scored;
                 candidates that point further out of the image than the truth are not all scored in the
                 cells at the border, and cannot win.  Where a neighbour of the winner is unscored the
                 sub-pixel parabola of that axis is skipped, so in those border cells "within 0.5 of the
                 truth" with the sub-pixel step says no more than the integer result does.
  1. truth       photo_fast scores exactly 1.0 at the true planes and below 0.95 at the swapped and the
                 negated ones; refine_fast and sgm_restate return every cell to the truth with shift == the
                 planted offset; lsm_fast meets the accuracy criterion of test_lsm_host on subpixel_pair in
                 both roles (exchanged: the truth is negative on both axes).
  2. transpose   the restatements on (a.T, b.T, d_col.T, d_row.T, offset swapped) give the transposed
                 outputs of the plain run bit for bit (lsm_fast: equal status, planes within LSM_GAP).
  3. matcher     the oracle's tiles of two_axis_pair(100, 100, dy, dx), stitched with and without the
                 forward-backward check: the measured shares (DESIGN.md quotes them).
  4. chain       the whole chain on that pair with a corrupted block, every stage as its host hook.

No restatement is new: photo_fast, refine_fast, sgm_restate, lsm_fast and the _host_* hooks are the ones
of their own files.  Everything is computed once (functools.lru_cache) and shared with the GPU file, which
leaves it unchanged.
"""
import functools

import numpy as np
import pytest

from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd.synthetic import subpixel_pair

from test_bilateral_host import _host_smooth
from test_fill_host import _host_fill, _host_stitch, _host_stitch_fb, _oracle_tiles, raw_bits
from test_lsm_host import _host_lsm, lsm_fast, rms
from test_median_host import _host_median
from test_photo_host import _host_photo, photo_fast
from test_prior_lattice import two_axis_pair
from test_refine_host import _host_refine, refine_fast
from test_sgm_host import q1024, sgm_costs, sgm_restate, sgm_solve
from test_speckle_host import _host_speckle

SHIFTS = [(3, 0), (-3, 0), (0, -2), (2, -3), (-2, 3)]
CELLS = (20, 37)                       # crosses the 32 x 8 tiles both ways
SEED = 11
PHOTO_RADII = [1, 2, 7]
PHOTO_SEARCH = 2                       # the photo cases have no search radius: their offset is that of s = 2
REFINE_CASES = [(2, 2), (1, 3), (7, 1)]
SGM_PENALTIES = [(0.0, 0.0), (0.25, 1.0)]
SGM_PATHS = [4, 8]
LSM_PHASES = [(1, 0), (0, 3), (2, 1)]
TRANSPOSED = (2, -3)                   # the shift of part 2
WRONG_BOUND = 0.95


def _freeze(d):
    for v in d.values():
        for x in (v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return d


# ---- the stage inputs ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(dy, dx, r, s, cells=CELLS):
    """-> dict(a, b, off, row, col (the true planes), planted (int64 [2][H][W], row then column), start_row,
    start_col (the truth plus the planted offset))."""
    H, W = cells
    m = r + s + 2
    oy, ox = m, m + 1
    a, b = two_axis_pair(oy + H + m + 2, ox + W + m + 2, dy, dx, seed=SEED)
    rng = np.random.default_rng([SEED, r, s, dy + 8, dx + 8, H])
    planted = rng.integers(-s, s + 1, (2, H, W))
    row, col = np.full((H, W), float(dy)), np.full((H, W), float(dx))
    return _freeze(dict(a=a, b=b, off=(oy, ox), row=row, col=col, planted=planted,
                        start_row=row + planted[0], start_col=col + planted[1]))


def assert_planted(planted):
    """The offsets are non-zero on each axis and of each sign somewhere, and zero somewhere."""
    for k in (0, 1):
        assert (planted[k] > 0).any() and (planted[k] < 0).any() and (planted[k] == 0).any()
    assert ((planted[0] != 0) & (planted[1] != 0)).any()


def wrong_variants(dy, dx):
    """The planes a sign or plane convention gone wrong would ask for, where they differ from the truth:
    name -> (row, col)."""
    v = {'swapped': (dx, dy), 'negated': (-dy, -dx), 'row negated': (-dy, dx), 'column negated': (dy, -dx)}
    return {k: p for k, p in v.items() if p != (dy, dx)}


def eighths(c, seed=3):
    """Planes in multiples of 1/8 around the truth of a stage case, for the transposition of photo."""
    rng = np.random.default_rng([SEED, seed])
    return c['row'] + rng.integers(-12, 13, c['row'].shape) / 8.0, c['col'] + rng.integers(-12, 13, c['col'].shape) / 8.0


def transpose_case(c):
    """The transposed problem of a stage case: images transposed, planes swapped and transposed, offset swapped."""
    t = lambda x: np.ascontiguousarray(x.T)
    oy, ox = c['off'] if isinstance(c['off'], tuple) else (c['off'], c['off'])
    out = dict(a=t(c['a']), b=t(c['b']), off=(ox, oy), row=t(c['col']), col=t(c['row']), start_row=t(c['start_col']),
               start_col=t(c['start_row']))
    if 'planted' in c:
        out['planted'] = np.stack([t(c['planted'][1]), t(c['planted'][0])])
    return out


def is_transposed(got, plain):
    """(row, col, score, shift) of the transposed problem against the plain run's: the row plane is the other's
    column plane transposed and the reverse, the shift components swap, bit for bit."""
    return raw_bits(got[0], plain[1].T) and raw_bits(got[1], plain[0].T) and raw_bits(got[2], plain[2].T) and \
        np.array_equal(got[3][0], plain[3][1].T) and np.array_equal(got[3][1], plain[3][0].T)


# ---- the restatements on them, computed once ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def photo_want(dy, dx, r, pr, pc, cells=CELLS):
    """photo_fast's score on the stage case (dy, dx, r) at the constant planes (pr, pc)."""
    c = stage_case(dy, dx, r, PHOTO_SEARCH, cells)
    z = np.zeros(cells)
    s = photo_fast(c['a'], c['b'], z + pr, z + pc, r, c['off'])[0]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def refine_want(dy, dx, r, s, subpix, cells=CELLS):
    c = stage_case(dy, dx, r, s, cells)
    return refine_fast(c['a'], c['b'], c['start_row'], c['start_col'], r, s, c['off'], 0.0, subpix)


@functools.lru_cache(maxsize=None)
def _sgm_costs(dy, dx, r, s, cells):
    c = stage_case(dy, dx, r, s, cells)
    return sgm_costs(c['a'], c['b'], c['start_row'], c['start_col'], r, s, c['off'])


@functools.lru_cache(maxsize=None)
def sgm_want(dy, dx, r, s, pen, paths, subpix=False, cells=CELLS):
    c = stage_case(dy, dx, r, s, cells)
    return sgm_solve(_sgm_costs(dy, dx, r, s, cells), c['start_row'], c['start_col'], q1024(pen[0]), q1024(pen[1]),
                     paths, subpix)


def returned_to_truth(res, c, what):
    """Both planes equal the truth in every cell and the shift is the planted offset, component for component."""
    assert np.array_equal(res[0], c['row']), '%s: the row plane is not the truth' % (what,)
    assert np.array_equal(res[1], c['col']), '%s: the column plane is not the truth' % (what,)
    assert np.array_equal(res[3], c['planted']), '%s: the shift is not the planted offset' % (what,)


# ---- the sub-pixel pairs, both roles ---------------------------------------------------------------------------
LSM_R, LSM_ITERS, LSM_CELLS = 3, 4, 48


@functools.lru_cache(maxsize=None)
def lsm_case(ky, kx, exchanged):
    """test_lsm_host.accuracy_case for any phase and for the exchanged pair -> dict(a, b, start_row, start_col, row,
    col, off): subpixel_pair's img2(y, x) = img1(y + ky / 4, x + kx / 4), so the truth is +(ky, kx) / 4, and with
    the two images exchanged -(ky, kx) / 4; the start is the truth plus uniform +-0.6 px per axis."""
    m = LSM_R + 5
    a, b = subpixel_pair(LSM_CELLS + 2 * m, LSM_CELLS + 2 * m, 5 + 10 * ky + kx, ky, kx)
    if exchanged:
        a, b, ky, kx = b, a, -ky, -kx
    rng = np.random.default_rng(100 + 10 * abs(ky) + abs(kx))
    row, col = np.full((LSM_CELLS, LSM_CELLS), ky / 4.0), np.full((LSM_CELLS, LSM_CELLS), kx / 4.0)
    return _freeze(dict(a=a, b=b, off=m, row=row, col=col, start_row=row + rng.uniform(-0.6, 0.6, row.shape),
                        start_col=col + rng.uniform(-0.6, 0.6, col.shape)))


@functools.lru_cache(maxsize=None)
def lsm_want(ky, kx, exchanged, transposed=False):
    c = lsm_case(ky, kx, exchanged)
    if transposed:
        c = transpose_case(c)
    return lsm_fast(c['a'], c['b'], c['start_row'], c['start_col'], LSM_R, LSM_ITERS, c['off'], 1.0)


def lsm_accurate(got, c, photo_of_start):
    """The criterion of tests/test_lsm_gpu.py::test_accuracy -> (rms after, accepted share)."""
    after, share = rms(got[0], got[1], c['row'], c['col']), float((got[3] == LSM_ITERS).mean())
    assert after <= 0.1 and share >= 0.99, (after, share)
    acc = got[3] == LSM_ITERS
    assert (got[2][acc] > photo_of_start[acc]).all() and raw_bits(got[2][~acc], photo_of_start[~acc])
    return after, share


# the largest difference between lsm_fast's planes on a case of part 1 and on its transposed problem
# (test_lsm_transposition measures it and holds it to this figure); the device is allowed twice as much
LSM_GAP = 2.0 ** -47                  # 7.1e-15


# ---- the matcher's pair ----------------------------------------------------------------------------------------
PAIR_SHIFTS = [(2, -3), (-2, 3)]
MATCH_MODES = ('elevation', 'elevation2', 'distance')
CHAIN_MODES = ('elevation', 'elevation2')
S, STRIDE, WS, NCC = 32, [32, 32], 5, 5
CHAIN = dict(consistency=1.0, median=1, photo=(2, 0.75), speckle=(3, 0.5), fill=16, sgm=(2, 2, 2.0, 8.0),
             sgm_where='filled', refine=(2, 1, 0.0), lsm=(2, 2, 1.0), smooth=(2, 10.0, 2.0))


def _host_sgm(img1, img2, d_row, d_col, radius, search, offset, p1, p2, paths, mask):
    """sgmer hook of solve_image_sharded (the stage runs with the sub-pixel step; p1, p2 in units of 1/1024)."""
    return sgm_restate(np.asarray(img1), np.asarray(img2), np.asarray(d_row), np.asarray(d_col), radius, search, p1, p2,
                       paths, offset, True, None if mask is None else np.asarray(mask))


HOOKS = dict(medianer=_host_median, photoer=_host_photo, speckler=_host_speckle, filler=_host_fill, sgmer=_host_sgm,
             refiner=_host_refine, lsmer=_host_lsm, smoother=_host_smooth)


def match_pair(dy, dx):
    return two_axis_pair(100, 100, dy, dx)


def corrupted_pair(dy, dx):
    """The pair with a 16 x 20 block of img2 overwritten by noise, as the `corrupted` fixtures of the stage files."""
    a, b = match_pair(dy, dx)
    b = b.copy()
    b[20:36, 24:44] = np.random.default_rng(5).integers(0, 256, (16, 20)).astype(np.uint8)
    return a, b


def pinned_tiles(*args, **kw):
    """test_fill_host._oracle_tiles in the oracle's pinned pow mode: the tiles the device computes, bit for bit."""
    from oracle import oracle as O
    O.set_pow_mode('pinned')
    try:
        return _oracle_tiles(*args, **kw)
    finally:
        O.set_pow_mode('libm')


@functools.lru_cache(maxsize=None)
def oracle_tiles(dy, dx):
    """-> (n, fwd, bwd): the oracle's tiles of match_pair in both directions, float64 [4][3][32][32]."""
    a, b = match_pair(dy, dx)
    n, org = engine.cut_grid(a.shape, [S, S], STRIDE, WS)
    fwd = pinned_tiles(a, b, org, S, S, WS, NCC, True, False, 3, 3, 'average').numpy()
    bwd = pinned_tiles(b, a, org, S, S, WS, NCC, True, False, 3, 3, 'average').numpy()
    fwd.setflags(write=False)
    bwd.setflags(write=False)
    return tuple(n), fwd, bwd


def share_within(d_map, dy, dx, where=None, tol=0.5):
    """The share of the cells (of ``where``) whose 'elevation' is within tol of dx and 'elevation2' of dy (NaN: not)."""
    with np.errstate(invalid='ignore'):
        ok = (np.abs(d_map[0] - dx) <= tol) & (np.abs(d_map[1] - dy) <= tol)
    return float(ok.mean() if where is None else ok[where].mean())


def host_chain(a, b, solver, stitcher):
    """solve_image_sharded with every stage of CHAIN replaced by its host hook -> the tuple as numpy arrays."""
    got = shard.solve_image_sharded(a, b, [S, S], STRIDE, WS, NCC, CHAIN_MODES, solver=solver, stitcher=stitcher,
                                    **CHAIN, **HOOKS)
    return [np.asarray(g) for g in got]


@functools.lru_cache(maxsize=None)
def oracle_chain(dy, dx):
    a, b = corrupted_pair(dy, dx)
    return host_chain(a, b, pinned_tiles, _host_stitch_fb)


# ---- 1. truth per stage ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cells', [CELLS, CELLS[::-1]], ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('dy,dx', SHIFTS)
def test_photo_truth(dy, dx, cells):
    worst = 0.0
    for r in PHOTO_RADII:
        s = photo_want(dy, dx, r, float(dy), float(dx), cells)
        assert s.shape == cells and (s == 1.0).all(), 'r = %d: %d cells do not score 1.0' % (r, (s != 1.0).sum())
        if r < 2:
            continue
        for name, (pr, pc) in wrong_variants(dy, dx).items():
            w = photo_want(dy, dx, r, float(pr), float(pc), cells)
            assert not np.isnan(w).all(), (r, name)
            worst = max(worst, float(np.nanmax(w)))
            assert not (w >= WRONG_BOUND).any(), 'r = %d, %s: a cell scores %.3f' % (r, name, np.nanmax(w))
    print('(%d, %d) on %d x %d cells: the best score at a wrong variant is %.3f' % (dy, dx, cells[0], cells[1], worst))


def test_wrong_variants():
    assert set(wrong_variants(2, -3)) == {'swapped', 'negated', 'row negated', 'column negated'}
    assert set(wrong_variants(3, 0)) == {'swapped', 'negated', 'row negated'}
    assert set(wrong_variants(0, -2)) == {'swapped', 'negated', 'column negated'}
    assert all(len(wrong_variants(*s)) >= 3 for s in SHIFTS)
    assert {np.sign(s[0]) for s in SHIFTS} == {np.sign(s[1]) for s in SHIFTS} == {-1, 0, 1}


@pytest.mark.parametrize('cells', [CELLS, CELLS[::-1]], ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('r,s', REFINE_CASES)
@pytest.mark.parametrize('dy,dx', SHIFTS)
def test_refine_truth(dy, dx, r, s, cells):
    c = stage_case(dy, dx, r, s, cells)
    assert_planted(c['planted'])
    returned_to_truth(refine_want(dy, dx, r, s, False, cells), c, 'refine')
    sub = refine_want(dy, dx, r, s, True, cells)
    miss = (np.abs(sub[0] - c['row']) > 0.5) | (np.abs(sub[1] - c['col']) > 0.5)
    assert not miss.any(), '%d cells are further than 0.5 from the truth' % miss.sum()
    assert np.array_equal(sub[3], c['planted'])


@pytest.mark.parametrize('cells', [CELLS, CELLS[::-1]], ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('r,s', REFINE_CASES)
@pytest.mark.parametrize('dy,dx', SHIFTS)
def test_sgm_truth(dy, dx, r, s, cells):
    c = stage_case(dy, dx, r, s, cells)
    assert_planted(c['planted'])
    for pen in SGM_PENALTIES:
        for paths in SGM_PATHS:
            returned_to_truth(sgm_want(dy, dx, r, s, pen, paths, False, cells), c, 'sgm %r, %d paths' % (pen, paths))


@pytest.mark.parametrize('exchanged', [False, True], ids=['as made', 'exchanged'])
@pytest.mark.parametrize('ky,kx', LSM_PHASES)
def test_lsm_truth(ky, kx, exchanged):
    c = lsm_case(ky, kx, exchanged)
    sign = -1 if exchanged else 1
    assert (c['row'] == sign * ky / 4.0).all() and (c['col'] == sign * kx / 4.0).all()
    before = rms(c['start_row'], c['start_col'], c['row'], c['col'])
    ps = photo_fast(c['a'], c['b'], c['start_row'], c['start_col'], LSM_R, c['off'])[0]
    after, share = lsm_accurate(lsm_want(ky, kx, exchanged), c, ps)
    print('phase (%d, %d) / 4 %s: rms before %.3f, after %.3f, accepted %.2f %%'
          % (ky, kx, 'exchanged' if exchanged else 'as made', before, after, 100 * share))
    assert 0.45 < before < 0.53


# ---- 2. transposition ----------------------------------------------------------------------------------------------
def test_photo_transposition():
    dy, dx = TRANSPOSED
    for r in PHOTO_RADII:
        c = stage_case(dy, dx, r, PHOTO_SEARCH)
        t = transpose_case(c)
        for row, col in ((c['row'], c['col']), eighths(c)):
            plain = photo_fast(c['a'], c['b'], row, col, r, c['off'])
            got = photo_fast(t['a'], t['b'], np.ascontiguousarray(col.T), np.ascontiguousarray(row.T), r, t['off'])
            assert raw_bits(got[0], plain[0].T) and raw_bits(got[1], plain[1].T), r
        assert np.isfinite(plain[0]).mean() > 0.9 and (plain[0] < 0.9).any()      # the fractions are scored, and not 1.0


@pytest.mark.parametrize('r,s', REFINE_CASES)
def test_refine_and_sgm_transposition(r, s):
    dy, dx = TRANSPOSED
    t = transpose_case(stage_case(dy, dx, r, s))
    for subpix in (False, True):
        got = refine_fast(t['a'], t['b'], t['start_row'], t['start_col'], r, s, t['off'], 0.0, subpix)
        assert is_transposed(got, refine_want(dy, dx, r, s, subpix)), ('refine', subpix)
    costs = sgm_costs(t['a'], t['b'], t['start_row'], t['start_col'], r, s, t['off'])
    for paths in SGM_PATHS:
        for subpix in (False, True):
            got = sgm_solve(costs, t['start_row'], t['start_col'], q1024(0.25), q1024(1.0), paths, subpix)
            assert is_transposed(got, sgm_want(dy, dx, r, s, (0.25, 1.0), paths, subpix)), ('sgm', paths, subpix)


def test_lsm_transposition():
    gap = 0.0
    for ky, kx in LSM_PHASES:
        for exchanged in (False, True):
            plain, got = lsm_want(ky, kx, exchanged), lsm_want(ky, kx, exchanged, True)
            assert np.array_equal(got[3], plain[3].T)
            gap = max(gap, float(np.abs(got[0] - plain[1].T).max()), float(np.abs(got[1] - plain[0].T).max()))
    print('lsm_fast, plain against transposed: the planes differ by at most %.3g' % gap)
    assert LSM_GAP / 2 <= gap <= LSM_GAP      # the device's bound is 2 LSM_GAP: a gap that shrinks must shrink it too


# ---- 3. the matcher's tiles and the consistency check --------------------------------------------------------
@pytest.mark.parametrize('dy,dx', PAIR_SHIFTS)
def test_consistency_shares(dy, dx):
    n, fwd, bwd = oracle_tiles(dy, dx)
    assert n == (2, 2)
    plain = _host_stitch(fwd, n, S, S, STRIDE, MATCH_MODES)[0]
    checked = _host_stitch_fb(fwd, bwd, n, S, S, STRIDE, MATCH_MODES, 1.0)[0]
    kept = ~np.isnan(checked[0])
    assert not np.isnan(plain).any() and np.array_equal(kept, ~np.isnan(checked[1]))
    unchecked, among, of_all = share_within(plain, dy, dx), share_within(checked, dy, dx, kept), share_within(checked, dy, dx)
    print('(%d, %d): within 0.5 of the truth %.4f unchecked, %.4f of the kept cells (%.4f of all cells); kept %.4f'
          % (dy, dx, unchecked, among, of_all, kept.mean()))
    assert kept.mean() > 0.5
    assert among >= unchecked


# ---- 4. the whole chain in its host hooks ------------------------------------------------------------------------
@pytest.mark.parametrize('dy,dx', PAIR_SHIFTS)
def test_chain_of_host_hooks(dy, dx):
    from deepmatching_stereo_matching_amd import chain
    names = chain.Chain(CHAIN_MODES, **{k: v for k, v in CHAIN.items() if k != 'consistency'}).names(1.0, None)
    assert names == ['d_map', 'out_map', 'err', 'speckles', 'holes', 'sgm_score', 'sgm_shift', 'refine_score',
                     'refine_shift', 'lsm_score', 'lsm_status', 'rejected', 'score']
    got = dict(zip(names, oracle_chain(dy, dx)))
    assert len(oracle_chain(dy, dx)) == len(names)
    filled = (got['holes'][0] | got['holes'][1]).astype(bool)
    assert got['sgm_shift'].any() and not got['sgm_shift'][:, ~filled].any()
    assert got['rejected'].any() and np.isfinite(got['d_map']).all()
    print('(%d, %d): %d cells filled, %d moved by sgm; the final d_map is within 0.5 of the truth in %.4f of the cells'
          % (dy, dx, filled.sum(), got['sgm_shift'].any(axis=0).sum(), share_within(got['d_map'], dy, dx)))
