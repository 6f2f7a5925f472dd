"""Pairs displaced along both axes, both signs, on the device: every stage of the chain on the cases of
tests/test_axis_host.py, where the true ('elevation2', 'elevation') is (dy, dx) with dy != 0.

  1. truth       engine.photo_score, photo_refine, sgm_refine and lsm_refine against the truth of the pair (a
                 condition the restatement meets in the host file) and against their restatements byte for byte.
  2. transpose   the run on (a.T, b.T, d_col.T, d_row.T, offset swapped) against the transposed outputs of the
                 plain run, byte for byte: 32 x 8 cell tiles, rows read as dwords along x and the scan lines of
                 each direction take other paths to what must be the same answer.  No restatement is involved.
  3. matcher     engine.solve_tiles + stitch against the oracle's cut_solve, and solve_tiles_bidir + stitch_fb
                 against the restated check over the oracle's tiles.
  4. chain       every stage at once through ImageCutSolver, through shard.solve_image_sharded, and through
                 solve_image_sharded with every stage replaced by its host hook: three equal tuples.  (Also the
                 on-device test of the sharded sgm= stage.)
  5. views       d_row and d_col handed over as views that are not contiguous: every entry that takes the two
                 planes gives what it gives for contiguous ones.  This is the regression test of the one defect
                 these cases exposed (engine.py freed its contiguous copies before the launch).
"""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import engine, shard

import test_axis_host as A
from test_fill_host import _host_stitch_fb, raw_bits, same_bits
from test_lsm_host import all_bits as lsm_bits
from test_refine_host import all_bits

pytestmark = pytest.mark.gpu

BOTH = [A.CELLS, A.CELLS[::-1]]
EVERY = dict(return_score=True, return_shift=True)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()      # a copy: the shared cases are read-only


def host(t):
    return [x.cpu().numpy() for x in t] if isinstance(t, (tuple, list)) else t.cpu().numpy()


def photo(c, row, col, r, warped=False):
    return host(engine.photo_score(dev(c['a']), dev(c['b']), dev(row), dev(col), r, offset=c['off'], return_warped=warped))


def refine(c, r, s, subpix):
    return host(engine.photo_refine(dev(c['a']), dev(c['b']), dev(c['start_row']), dev(c['start_col']), r, s,
                                    offset=c['off'], subpix=subpix, **EVERY))


def sgm(c, r, s, pen, paths, subpix):
    return host(engine.sgm_refine(dev(c['a']), dev(c['b']), dev(c['start_row']), dev(c['start_col']), r, s, pen[0], pen[1],
                                  paths=paths, offset=c['off'], subpix=subpix, **EVERY))


def lsm(c):
    return host(engine.lsm_refine(dev(c['a']), dev(c['b']), dev(c['start_row']), dev(c['start_col']), A.LSM_R, A.LSM_ITERS,
                                  offset=c['off'], max_move=1.0, return_score=True, return_status=True))


# ---- 1. truth per stage ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cells', BOTH, ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('dy,dx', A.SHIFTS)
def test_photo_truth(dy, dx, cells):
    z = np.zeros(cells)
    for r in A.PHOTO_RADII:
        c = A.stage_case(dy, dx, r, A.PHOTO_SEARCH, cells)
        got = photo(c, c['row'], c['col'], r)
        assert raw_bits(got, A.photo_want(dy, dx, r, float(dy), float(dx), cells)), r
        assert (got == 1.0).all(), 'r = %d: %d cells do not score 1.0' % (r, (got != 1.0).sum())
        if r < 2:
            continue
        for name, (pr, pc) in A.wrong_variants(dy, dx).items():
            got = photo(c, z + pr, z + pc, r)
            assert raw_bits(got, A.photo_want(dy, dx, r, float(pr), float(pc), cells)), (r, name)
            assert not (got >= A.WRONG_BOUND).any(), 'r = %d, %s: a cell scores %.3f' % (r, name, np.nanmax(got))


@pytest.mark.parametrize('cells', BOTH, ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('r,s', A.REFINE_CASES)
@pytest.mark.parametrize('dy,dx', A.SHIFTS)
def test_refine_truth(dy, dx, r, s, cells):
    c = A.stage_case(dy, dx, r, s, cells)
    A.assert_planted(c['planted'])
    got = refine(c, r, s, False)
    assert all_bits(got, A.refine_want(dy, dx, r, s, False, cells))
    A.returned_to_truth(got, c, 'refine')
    sub = refine(c, r, s, True)
    assert all_bits(sub, A.refine_want(dy, dx, r, s, True, cells))
    miss = (np.abs(sub[0] - c['row']) > 0.5) | (np.abs(sub[1] - c['col']) > 0.5)
    assert not miss.any(), '%d cells are further than 0.5 from the truth' % miss.sum()


@pytest.mark.parametrize('cells', BOTH, ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('r,s', A.REFINE_CASES)
@pytest.mark.parametrize('dy,dx', A.SHIFTS)
def test_sgm_truth(dy, dx, r, s, cells):
    c = A.stage_case(dy, dx, r, s, cells)
    A.assert_planted(c['planted'])
    for pen in A.SGM_PENALTIES:
        for paths in A.SGM_PATHS:
            got = sgm(c, r, s, pen, paths, False)
            assert all_bits(got, A.sgm_want(dy, dx, r, s, pen, paths, False, cells)), (pen, paths)
            A.returned_to_truth(got, c, 'sgm %r, %d paths' % (pen, paths))


@pytest.mark.parametrize('exchanged', [False, True], ids=['as made', 'exchanged'])
@pytest.mark.parametrize('ky,kx', A.LSM_PHASES)
def test_lsm_truth(ky, kx, exchanged):
    c = A.lsm_case(ky, kx, exchanged)
    got = lsm(c)
    assert lsm_bits(got, A.lsm_want(ky, kx, exchanged))
    ps = photo(c, c['start_row'], c['start_col'], A.LSM_R)
    after, share = A.lsm_accurate(got, c, ps)
    print('phase (%d, %d) / 4 %s: rms after %.3f, accepted %.2f %%' % (ky, kx, 'exchanged' if exchanged else 'as made',
                                                                     after, 100 * share))


# ---- 2. transposition, no restatement involved ----------------------------------------------------------------------
def test_photo_transposition():
    dy, dx = A.TRANSPOSED
    for r in A.PHOTO_RADII:
        c = A.stage_case(dy, dx, r, A.PHOTO_SEARCH)
        t = A.transpose_case(c)
        for row, col in ((c['row'], c['col']), A.eighths(c)):
            plain = photo(c, row, col, r, True)
            got = photo(t, col.T, row.T, r, True)
            assert raw_bits(got[0], plain[0].T), 'r = %d: the score differs' % r
            assert raw_bits(got[1], plain[1].T), 'r = %d: the warped plane differs' % r
        assert np.isfinite(plain[0]).mean() > 0.9 and (plain[0] < 0.9).any()


@pytest.mark.parametrize('r,s', A.REFINE_CASES)
def test_refine_transposition(r, s):
    c = A.stage_case(*A.TRANSPOSED, r, s)
    t = A.transpose_case(c)
    for subpix in (False, True):
        plain = refine(c, r, s, subpix)
        assert plain[3].any()
        assert A.is_transposed(refine(t, r, s, subpix), plain), subpix


@pytest.mark.parametrize('r,s', A.REFINE_CASES)
def test_sgm_transposition(r, s):
    c = A.stage_case(*A.TRANSPOSED, r, s)
    t = A.transpose_case(c)
    for paths in A.SGM_PATHS:
        for subpix in (False, True):
            plain = sgm(c, r, s, (0.25, 1.0), paths, subpix)
            assert plain[3].any()
            assert A.is_transposed(sgm(t, r, s, (0.25, 1.0), paths, subpix), plain), (paths, subpix)


def test_lsm_transposition():
    """Equal status; the planes within twice the largest difference lsm_fast shows between the two orientations on
    these inputs (test_axis_host.LSM_GAP: the sums of a window are taken in another order)."""
    for ky, kx in A.LSM_PHASES:
        for exchanged in (False, True):
            c = A.lsm_case(ky, kx, exchanged)
            plain, got = lsm(c), lsm(A.transpose_case(c))
            assert np.array_equal(got[3], plain[3].T), (ky, kx, exchanged)
            gap = max(np.abs(got[0] - plain[1].T).max(), np.abs(got[1] - plain[0].T).max())
            assert gap <= 2 * A.LSM_GAP, (ky, kx, exchanged, gap)


# ---- 3. the matcher and the consistency check ---------------------------------------------------------------------
@pytest.mark.parametrize('dy,dx', A.PAIR_SHIFTS)
def test_matcher_and_consistency(dy, dx):
    from oracle import oracle as O
    a, b = A.match_pair(dy, dx)
    S, STRIDE, WS, MODES = A.S, A.STRIDE, A.WS, list(A.MATCH_MODES)
    n, org = engine.cut_grid(a.shape, [S, S], STRIDE, WS)
    d, s = engine.stitch(engine.solve_tiles(a, b, org, S, S, WS, A.NCC), n, S, S, STRIDE, MODES)
    O.set_pow_mode('pinned')
    try:
        od, os_ = O.cut_solve(a, b, image_size=[S, S], stride=STRIDE, window_size=WS, degree_map_mode=A.MATCH_MODES)
    finally:
        O.set_pow_mode('libm')
    assert same_bits(host(d), od) and same_bits(host(s), os_)
    _, ofwd, obwd = A.oracle_tiles(dy, dx)
    fwd, bwd = engine.solve_tiles_bidir(a, b, org, S, S, WS, A.NCC)
    assert same_bits(host(fwd), ofwd) and same_bits(host(bwd), obwd)
    got = host(engine.stitch_fb(fwd, bwd, n, S, S, STRIDE, MODES, 1.0))
    want = _host_stitch_fb(ofwd, obwd, n, S, S, STRIDE, A.MATCH_MODES, 1.0)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    kept = ~np.isnan(got[0][0])
    assert kept.mean() > 0.5 and A.share_within(got[0], dy, dx, kept) >= A.share_within(host(d), dy, dx)


# ---- 4. the whole chain ------------------------------------------------------------------------------------------
def _device_stitch_fb(*args):
    """engine.stitch_fb as the stitcher of a run whose stages are host hooks: the device's maps as numpy arrays."""
    return tuple(host(engine.stitch_fb(*args)))


@pytest.mark.parametrize('dy,dx', A.PAIR_SHIFTS)
def test_chain_three_ways(dy, dx):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = A.corrupted_pair(dy, dx)
    S, STRIDE, WS = A.S, A.STRIDE, A.WS
    solver = ImageCutSolver(a, b, image_size=[S, S], stride=STRIDE, window_size=WS, degree_map_mode=list(A.CHAIN_MODES),
                            **A.CHAIN)
    solver.log_flg = False
    names = solver.chain.names(1.0, None)
    lay = solver.chain.layout(64, 64, 1.0, None)
    cut = solver._execute_matching_device()
    sharded = shard.solve_image_sharded(a, b, [S, S], STRIDE, WS, A.NCC, A.CHAIN_MODES, **A.CHAIN)
    hooks = A.host_chain(a, b, None, _device_stitch_fb)
    assert len(cut) == len(sharded) == len(hooks) == len(names) == 13
    for (name, shape, dtype), p, q, h in zip(lay, cut, sharded, hooks):
        assert p.dtype == q.dtype == dtype and tuple(p.shape) == tuple(q.shape) == h.shape == shape, name
        assert h.dtype == host(p).dtype, name
        assert raw_bits(host(p.double()), host(q.double())), '%s: ImageCutSolver and solve_image_sharded differ' % name
        assert raw_bits(host(p.double()), h.astype(np.float64)), '%s: the device stages and the host hooks differ' % name
    got = dict(zip(names, hooks))
    filled = (got['holes'][0] | got['holes'][1]).astype(bool)
    shift = host(sharded[names.index('sgm_shift')])
    assert shift.any() and not shift[:, ~filled].any()      # the sharded sgm stage moves cells, and only filled ones
    # the matcher equals the oracle (part 3), so the host chain over the oracle's tiles is this one: its share is DESIGN.md's
    full = dict(zip(names, A.oracle_chain(dy, dx)))
    share, want = A.share_within(host(cut[0]), dy, dx), A.share_within(got['d_map'], dy, dx)
    print('(%d, %d): the final d_map is within 0.5 of the truth in %.4f of the cells (host hooks %.4f)' % (dy, dx, share, want))
    assert share >= want and raw_bits(got['d_map'], full['d_map'])


# ---- 5. planes that are views: the regression test of the defect these cases exposed ---------------------------
def view(x):
    """The plane on the device as a view that is not contiguous (column-major memory, the same values)."""
    t = dev(np.ascontiguousarray(x.T)).T
    assert not t.is_contiguous() and tuple(t.shape) == x.shape
    return t


def test_planes_that_are_views():
    """d_row and d_col as views that are not contiguous: the entry copies them, and each copy has to live until
    the launch.  (The copies were temporaries, freed at once: the block of d_row's copy was handed to d_col's, and
    the kernel read d_col twice -- seen only where the two planes differ.)"""
    dy, dx = A.TRANSPOSED
    r, s = 2, 2
    c = A.stage_case(dy, dx, r, s)
    a, b, off = dev(c['a']), dev(c['b']), c['off']
    row, col = c['start_row'], c['start_col']
    calls = {
        'photo_score': lambda p, q: engine.photo_score(a, b, p, q, r, offset=off, return_warped=True),
        'photo_refine': lambda p, q: engine.photo_refine(a, b, p, q, r, s, offset=off, **EVERY),
        'sgm_refine': lambda p, q: engine.sgm_refine(a, b, p, q, r, s, 0.25, 1.0, offset=off, **EVERY),
        'lsm_refine': lambda p, q: engine.lsm_refine(a, b, p + 0.25, q - 0.25, r, 2, offset=off, return_score=True,
                                                     return_status=True),
        'tile_prior': lambda p, q: engine.tile_prior(p, q, [(0, 0), (5, 9), (8, 20)], 8, 8, 2, scale=1),
    }
    for name, call in calls.items():
        want, got = host(call(dev(row), dev(col))), host(call(view(row), view(col)))
        for w, g in zip(want, got):
            assert w.dtype == g.dtype and raw_bits(w.astype(np.float64), g.astype(np.float64)), name
    assert host(calls['tile_prior'](view(c['row']), view(c['col'])))[0].tolist() == [[dy, dx]] * 3
