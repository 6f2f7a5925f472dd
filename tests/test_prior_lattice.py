"""Disparity priors where the product uses them, host side (no GPU): the cases that
tests/test_prior_lattice_gpu.py runs on the device, and what can be said of them without one.

  LATTICE        ten (h0, w0, ws) MFMA tile shapes whose dispatch keys (test_shape_lattice.dispatch_key)
                 cover every branch of the level launcher (c2, c3, c5, mq_y, mq) and every volume
                 kernel ('ls', 'mfq' with and without LS_): a packed pair feeds each of them tile origins
                 at multiples of the crop size, crops that touch, and zero filler after the last crop --
                 the level kernels through the solve, the volume kernels, which the solve never
                 launches, through dm_corr_volume_ex (both in the GPU file).
  prior_case     the image pair, the tile origins (odd offsets among them, the first and the last in two
                 opposite corners) and one seeded two-axis prior per tile of a lattice entry; the priors
                 are non-zero in both components, of both signs, and clamp on each axis at some tile.
  two_axis_pair  a pair displaced along both axes: img2[y, x] = img1[y + dy, x + dx], so the true
                 ('elevation2', 'elevation') is (dy, dx).
  restated       the coarse-to-fine procedure of test_prior.coarse_to_fine_np on such pairs with the
                 CPU oracle, computed once per case and shared with the GPU tests.

No restatement is new: pack_np, shift_np, coarse_to_fine_np, ... are test_prior.py's.

The grid of a packed pair is the library's own (engine.pack_grid calls dm_pack_plan, a host function),
so these cases need the built library, as test_prior.test_pack_grid does; none needs a device.
"""
import functools

import numpy as np
import pytest

from deepmatching_stereo_matching_amd import engine, synthetic

from test_fb_host import place
from test_prior import coarse_to_fine_np, oracle_solve, pack_np, solve_level_np, stitch_planes_np
from test_shape_lattice import dispatch_key

# (h0, w0, ws)
LATTICE = [(8, 32, 3), (8, 32, 5), (4, 64, 5), (8, 64, 7), (8, 128, 3), (8, 128, 13), (8, 256, 5), (8, 256, 15),
           (96, 32, 5), (16, 32, 5)]
CONSISTENCY_CASES = [(8, 32, 5), (4, 64, 5), (8, 128, 3), (8, 256, 5)]

# tile origins inside an image of (crop + MARGIN): odd offsets among them (test_shape_lattice.ORIGINS'
# first three), the first in the top-left and the fourth in the bottom-right corner
MARGIN = (12, 14)
ORIGINS = [(0, 0), (3, 7), (2, 5), (12, 14)]
ORIGINS += [(y, x) for y, x in (((5 * k + 7) % 13, (4 * k + 1) % 15) for k in range(24)) if (y, x) not in ORIGINS]
assert len(set(ORIGINS)) == len(ORIGINS) >= 24      # a flat, wide crop needs up to 23 tiles for a ragged grid
TRUE_SHIFT = (1, -2)      # img2[y, x] = img1[y + 1, x - 2]: the matches mean something, so a check keeps some


def pack_rows(T, h0, w0, ws):
    """(crop rows, crops in the last row, crops per full row) of pack_tiles' grid for T tiles."""
    org = engine.pack_grid(T, h0, w0, ws)[0]
    rows = org[:, 0] // (h0 + ws - 1)
    return int(rows.max()) + 1, int((rows == rows.max()).sum()), int((rows == 0).sum())


def lattice_T(h0, w0, ws):
    """5, or the smallest larger T whose packed grid has at least two crop rows and a last row that is not
    full: then the zero filler lies to the right of and below the last crop."""
    for T in range(5, len(ORIGINS) + 1):
        rows, last, full = pack_rows(T, h0, w0, ws)
        if rows >= 2 and last < full:
            return T
    raise AssertionError('no T <= %d packs %r into a ragged grid' % (len(ORIGINS), (h0, w0, ws)))


def prior_case(h0, w0, ws, T=None):
    """-> (img1, img2, origins int64 [T][2], prior int64 [T][2]) of one lattice entry: random uint8
    images, img2 the same field displaced by TRUE_SHIFT, and one seeded prior per tile with both
    components drawn from +-{1, 2, 3} (the tile at (3, 7) is then never clamped)."""
    T = lattice_T(h0, w0, ws) if T is None else T
    H, W = h0 + ws - 1 + MARGIN[0], w0 + ws - 1 + MARGIN[1]
    rng = np.random.default_rng(1000 * h0 + 10 * w0 + ws)
    base = rng.integers(0, 256, size=(H + 16, W + 16)).astype(np.uint8)
    dy, dx = TRUE_SHIFT
    img1, img2 = base[8:8 + H, 8:8 + W].copy(), base[8 + dy:8 + dy + H, 8 + dx:8 + dx + W].copy()
    sign = rng.choice([-1, 1], size=(T, 2))
    sign[0], sign[3] = 1, -1      # the crops of the two corner tiles point out of the image, on both axes
    prior = rng.integers(1, 4, size=(T, 2)) * sign
    return img1, img2, np.array(ORIGINS[:T], dtype=np.int64), prior.astype(np.int64)


def assert_two_axis_clamps(prior, q_eff):
    """The priors are non-zero and of both signs in both components; on each axis a crop is clamped at each
    border of the image (the effective prior then differs from the prior, one way and the other), and at
    least one tile is not clamped at all (test_prior_gpu.test_pack_tiles' rule)."""
    prior = np.asarray(prior)
    assert (prior != 0).all() and (prior > 0).any(axis=0).all() and (prior < 0).any(axis=0).all()
    d = np.asarray(q_eff) - prior
    assert (d[:, 0] > 0).any() and (d[:, 0] < 0).any() and (d[:, 1] > 0).any() and (d[:, 1] < 0).any()
    assert (d == 0).all(axis=1).any()


# ---- the pair of two axes and its measure ------------------------------------------------------------
def two_axis_pair(h, w, dy, dx, seed=7):
    tex = synthetic.texture(h + 64, w + 64, seed)
    return tex[32:32 + h, 32:32 + w].copy(), tex[32 + dy:32 + dy + h, 32 + dx:32 + dx + w].copy()


def owner_map(n, stride, h0, w0):
    """The tile whose cell the overwriting stitch keeps, per map cell."""
    T = n[0] * n[1]
    return place(np.broadcast_to(np.arange(T, dtype=np.float64)[:, None, None], (T, h0, w0)), n, stride).astype(np.int64)


def free_share(d2, d1, free, n, stride, h0, w0, dy, dx, tol=0.5):
    """The share of the cells of the free tiles (``free``: bool [T]) within tol of (dy, dx) in both planes of
    a stitched map (NaN: not); a cell belongs to the tile the stitch took it from."""
    with np.errstate(invalid='ignore'):
        ok = (np.abs(d2 - dy) <= tol) & (np.abs(d1 - dx) <= tol)
    return float(ok[np.asarray(free)[owner_map(n, stride, h0, w0)]].mean())


def tile_share(match, free, dy, dx, tol=0.5):
    """The same share counted on the tiles themselves: every cell of every free tile."""
    h0, w0 = match.shape[2:]
    ii, jj = (x.astype(np.float64) for x in np.mgrid[0:h0, 0:w0])
    with np.errstate(invalid='ignore'):
        ok = (np.abs(ii - match[:, 0] - dy) <= tol) & (np.abs(jj - match[:, 1] - dx) <= tol)
    return float(ok[np.asarray(free)].mean())


# pair shape, (dy, dx), coarse levels, image_size, stride -- and what the restatement measured with the
# CPU oracle, seed 7, ws 5, tol 1.0: tiles, priors exactly (dy, dx), free tiles.  (Row 3: the crops of the
# first two of its 31 tile columns are clamped, 16 j - 20 < 0, so at most 93.5 % of its tiles are free.)
ROWS = {
    1: ((200, 260), (-6, 10), 1, [16, 16], [16, 16], 165, 0.970, 0.921),
    2: ((200, 260), (-6, 10), 1, [16, 32], [16, 16], 154, 1.000, 0.929),
    3: ((280, 520), (-12, 20), 2, [16, 16], [16, 16], 496, 0.954, 0.907),
}


@functools.lru_cache(maxsize=None)
def restated(row):
    """The restated procedure on one row of ROWS -> dict(img1, img2, n, origins, match, q_eff, priors,
    free, d (the stitched ('elevation2', 'elevation') planes), plain_match, plain_d).  Computed once; the
    GPU tests read it and leave it unchanged.  The oracle runs in its 'libm' pow mode, set here, whichever
    tests ran before: the mode every fixture of the suite restores, so nothing else is affected."""
    from oracle import oracle as O
    O.set_pow_mode('libm')
    shape, (dy, dx), k, size, stride = ROWS[row][:5]
    a, b = two_axis_pair(shape[0], shape[1], dy, dx)
    solve = oracle_solve()
    m, q_eff, _, valid, n, org, priors = coarse_to_fine_np(a, b, size, stride, 5, k, 1.0, solve)
    m0 = solve_level_np(a, b, org, np.zeros((len(org), 2), np.int32), size[0], size[1], 5, None, solve)[0]
    out = dict(img1=a, img2=b, n=n, origins=org, match=m, q_eff=q_eff, priors=priors, valid=valid,
               free=(q_eff == (dy, dx)).all(axis=1), d=stitch_planes_np(m, n, stride), plain_match=m0,
               plain_d=stitch_planes_np(m0, n, stride))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- 1. the lattice -------------------------------------------------------------------------------------
def test_lattice_reaches_every_kernel_class():
    keys = [dispatch_key(*c) for c in LATTICE]
    assert {lev[0] for lev, _ in keys} == {'c2', 'c3', 'c5', 'mq_y', 'mq'}
    vol = {(v[0], v[2]) for _, v in keys}
    assert ('ls', None) in vol and ('mfq', True) in vol and ('mfq', False) in vol
    for c, k in zip(LATTICE, keys):
        print(c, '-> level', k[0], 'volume', k[1])
    assert set(CONSISTENCY_CASES) <= set(LATTICE)
    assert {dispatch_key(*c)[0][0] for c in CONSISTENCY_CASES} == {'mq_y', 'c2', 'c3', 'c5'}


@pytest.mark.parametrize('h0,w0,ws', LATTICE, ids=str)
def test_lattice_case(h0, w0, ws):
    """The packed grid of every entry is ragged (two crop rows or more, the last one not full), its tile
    origins are multiples of the crop size, and the seeded priors clamp as the device test needs them to."""
    T = lattice_T(h0, w0, ws)
    rows, last, full = pack_rows(T, h0, w0, ws)
    assert rows >= 2 and last < full
    if T != 5:      # T = 5 is the issue's choice; a larger one only where 5 does not give the ragged grid
        r5 = pack_rows(5, h0, w0, ws)
        assert not (r5[0] >= 2 and r5[1] < r5[2])
    grid, Hp, Wp = engine.pack_grid(T, h0, w0, ws)
    ch, cw = h0 + ws - 1, w0 + ws - 1
    assert (grid[:, 0] % ch == 0).all() and (grid[:, 1] % cw == 0).all() and grid.max() > 0
    assert Hp == rows * ch and full * cw <= Wp < full * cw + 16
    img1, img2, org, prior = prior_case(h0, w0, ws)
    assert len(org) == T and len({tuple(o) for o in org}) == T and (org % 2 == 1).any()
    assert img1.shape == img2.shape == (ch + MARGIN[0], cw + MARGIN[1])
    assert (org[:, 0] + ch <= img1.shape[0]).all() and (org[:, 1] + cw <= img1.shape[1]).all()
    dy, dx = TRUE_SHIFT
    assert np.array_equal(img2[8:-8, 8:-8], img1[8 + dy:-8 + dy, 8 + dx:-8 + dx])
    assert_two_axis_clamps(prior, pack_np(img1, img2, org, prior, h0, w0, ws)[2])


def test_chunked_case_splits_into_three():
    """T = 7 tiles of (16, 32) under a budget of three tiles: chunks of 3, 3 and 1, each packed on its own
    grid, and with consistency= the 2 x 3 tiles of a chunk's bidirectional solve chunk again."""
    budget = 3 * engine.tile_bytes(16, 32)
    chunk = max(1, min(7, budget // engine.tile_bytes(16, 32)))
    assert chunk == 3 and [len(range(s, min(s + chunk, 7))) for s in range(0, 7, chunk)] == [3, 3, 1]
    img1, img2, org, prior = prior_case(16, 32, 5, T=7)
    assert_two_axis_clamps(prior, pack_np(img1, img2, org, prior, 16, 32, 5)[2])
    # a tile's place in the packed pair of its chunk differs from its place in the unchunked one
    whole = engine.pack_grid(7, 16, 32, 5)[0]
    assert not np.array_equal(whole[3:6], engine.pack_grid(3, 16, 32, 5)[0])


# ---- 4. the procedure on pairs displaced along both axes -----------------------------------------------
@pytest.mark.parametrize('row', sorted(ROWS))
def test_two_axis_restatement(row):
    """Measured shares are printed before they are asserted.  Free tiles: those whose effective prior is
    (dy, dx).  With the coarse levels every cell of a free tile is within 0.5 px of (dy, dx) in both planes;
    without a prior fewer than 0.4 are."""
    shape, (dy, dx), k, size, stride, tiles, exact, free_want = ROWS[row]
    r = restated(row)
    T = len(r['origins'])
    free = r['free']
    got_exact = float((r['priors'][0] == (dy, dx)).all(axis=1).mean())
    share, share0 = tile_share(r['match'], free, dy, dx), tile_share(r['plain_match'], free, dy, dx)
    on_map = free_share(r['d'][0], r['d'][1], free, r['n'], stride, size[0], size[1], dy, dx)
    on_map0 = free_share(r['plain_d'][0], r['plain_d'][1], free, r['n'], stride, size[0], size[1], dy, dx)
    print('row %d: %d tiles, priors exact %.3f, free %.3f, share coarse %.4f (stitched %.4f), no prior %.4f '
          '(stitched %.4f)' % (row, T, got_exact, free.mean(), share, on_map, share0, on_map0))
    assert T == tiles and len(r['priors']) == k + 1
    assert abs(got_exact - exact) < 0.001 and abs(free.mean() - free_want) < 0.001
    assert free.mean() > 0.9
    assert share == 1.0 and on_map == 1.0
    assert share0 < 0.4 and on_map0 < 0.4
