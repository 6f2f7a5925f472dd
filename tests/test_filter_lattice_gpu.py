"""Matching._filter on the GPU (k_filter and the ``filt`` hook of dm_match), where it acts.

Everything here is compared bit for bit with ``oracle.match`` under the pinned pow (the one the
kernels evaluate), and with the reference's own results (tests/golden/filter_*.npz) at the
tolerances of test_oracle_golden.py.  The pairs, the restatement and the premises -- which
passes run, which act, which cases must differ from the unfiltered match -- are the ones of
test_filter_lattice.py, where they are established on the CPU; a case whose premise says the
filter acts is checked to differ from the unfiltered match here too, so a k_filter that copies
its input fails it.  Shapes are S = 8, 16 and 32.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_filter_lattice import (FMODES, GOLD, PAIRS, WINDOWS, filter_restate, held_to_fixture, key,
                                 lattice_counts, load, pass_plan, quiet_levels, acting_levels, sides, stored)

pytestmark = pytest.mark.gpu

METHOD = {'cv2.TM_CCOEFF_NORMED': 5, 'cv2.TM_CCOEFF': 4}
# (pair, levels kept): the first pass lands on an 8 x 8 or a 16 x 16 top map and acts there
CUTS = (('filter_s16_noise', 2), ('filter_s16_ccoeff', 2), ('filter_s32_roll', 2), ('filter_s32_sin', 2),
        ('filter_s32_sin', 3))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=True), 'max |d| = %r' % np.nanmax(np.abs(a - b))


@pytest.fixture(scope='module', autouse=True)
def device():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'


class Lists:
    """What Matching reads of a Correlation_map: co_map_list (cut to its first k levels) and N_map."""

    def __init__(self, co_map_list, k):
        self.co_map_list = co_map_list[:k]
        self.N_map = 2 ** (k - 1)


@functools.lru_cache(maxsize=None)
def sources(name, k=None):
    """The three level sources of one pair: the mirror's Correlation_map (levels 0 and 1 on demand
    where the fused level kernel takes the shape), a pyramid that stores level 1, plain numpy.
    ``k``: a set of its own for the matches cut to k levels (a 2-level match stores level 1 for good)."""
    from deepmatching_stereo_matching_amd import engine
    from deepmatching_stereo_matching_amd.misc.Correlation_map import Correlation_map
    g, levels = load(name, 'pinned')
    ws, feat = int(g['ws']), str(g['feature'])
    co = Correlation_map(g['img1'], g['img2'], window_size=ws, feature_name=feat)
    co()
    h0, w0 = levels[0].shape[:2]
    batch = engine.TileBatch(g['img1'], g['img2'], [(0, 0)], h0, w0, ws, METHOD[feat])
    kept = engine.DevicePyramid(batch, fuse_level2=0)
    assert kept.levels[1] is not None
    # the S = 32 pairs are the ones whose level 1 the default configuration derives on demand
    assert engine.level12_fused(32, 32, 5) and not engine.level12_fused(16, 16, 5)
    if 'DM_FUSE_L2' not in os.environ:
        assert engine.FUSE_DEFAULT == 2 and not engine.level1_stored()
    if engine.level12_fused(h0, w0, ws) and not engine.level1_stored():
        assert co.co_map_list.pyramid.levels[1] is None      # k_match_step_l1 derives it
    return co, kept, levels


@functools.lru_cache(maxsize=None)
def want(name, k, w, mode, n, sub):
    """oracle.match on the first k levels; n == 0: unfiltered."""
    levels = load(name, 'pinned')[1][:k]
    if n == 0:
        return O.match(levels, sub_pix=sub)
    return O.match(levels, sub_pix=sub, filtering=True, filter_window_size=w, filtering_num=n, filtering_mode=mode)


def on_all_sources(name, k, w, mode, n, sub):
    from deepmatching_stereo_matching_amd.misc.Matching import Matching
    co, kept, levels = sources(name, None if k == len(load(name)[1]) else k)
    ref = want(name, k, w, mode, n, sub)
    kw = dict(filter_window_size=w, filtering=True, filtering_num=n, filtering_mode=mode, sub_pix=sub)
    _same(Matching(Lists(co.co_map_list, k), **kw)(), ref)
    _same(kept.match(sub, True, w, n, mode, nlev=k)[0].cpu().numpy(), ref)
    _same(Matching(Lists(levels, k), **kw)(), ref)
    return ref


def swaps(name, k, w, n):
    """Buffer swaps of dm_match: one per step of the descent and one per pass that runs."""
    levels = load(name)[1][:k]
    return k - 1 + sum(pass_plan(sides(levels), w, n))


# ---- the lattice ------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', FMODES)
@pytest.mark.parametrize('w', WINDOWS)
@pytest.mark.parametrize('name', PAIRS)
def test_lattice(name, w, mode):
    g, levels = load(name, 'pinned')
    k = len(levels)
    for n in lattice_counts(g, w, mode):
        act = [x for x in acting_levels(levels, w, n) if x not in quiet_levels(name, levels, w)]
        for sub in (False, True):
            ref = on_all_sources(name, k, w, mode, n, sub)
            held_to_fixture(ref, stored(g, key(w, mode, n), sub), sub)
            if act:
                assert not np.array_equal(ref[:2], want(name, k, w, mode, 0, sub)[:2])
            else:
                _same(ref, want(name, k, w, mode, 0, sub))
    from deepmatching_stereo_matching_amd import engine
    if engine.level12_fused(*levels[0].shape[:2], int(g['ws'])) and not engine.level1_stored():
        assert sources(name)[0].co_map_list.pyramid.levels[1] is None     # still derived on demand


@pytest.mark.parametrize('mode', FMODES)
@pytest.mark.parametrize('w', WINDOWS)
@pytest.mark.parametrize('name,k', CUTS)
def test_lattice_on_cut_pyramids(name, k, w, mode):
    """A co_map_list cut to k levels: the descent starts on an 8 x 8 or 16 x 16 map and the first
    pass filters that map (k_match_top's output), where every window up to 7 fits."""
    for n in (1, 2, k, k + 2):
        for sub in (False, True):
            ref = on_all_sources(name, k, w, mode, n, sub)
            if w >= 3:
                assert not np.array_equal(ref[:2], want(name, k, w, mode, 0, sub)[:2])
            else:
                _same(ref, want(name, k, w, mode, 0, sub))


def test_both_buffer_parities():
    """dm_match picks its first buffer so that the last phase writes d_out: the number of swaps,
    K steps plus the passes that run, comes out odd and even in the lattice above.  The parity
    here is worked out on the host from (levels, window, count)."""
    odd = [('filter_s16_noise', 5, 3, 3), ('filter_s16_noise', 2, 3, 2), ('filter_s32_roll', 6, 3, 4),
           ('filter_s32_roll', 6, 3, 8)]
    even = [('filter_s16_noise', 5, 3, 4), ('filter_s16_noise', 2, 3, 1), ('filter_s16_noise', 5, 5, 3),
            ('filter_s32_roll', 6, 7, 6)]
    assert [swaps(*c) for c in odd] == [5, 3, 7, 9]      # (pair, levels, window, count)
    assert [swaps(*c) for c in even] == [6, 2, 4, 8]
    for name, k, w, n in odd + even:
        for mode in FMODES:
            on_all_sources(name, k, w, mode, n, True)


# ---- batches ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def canvas():
    """Four S = 16, ws 5 tiles side by side in one image pair: two on which the filter acts from
    the 4 x 4 map on, the suite's older pair (quiet: no median pass changes it before the last two
    levels), and independent noise."""
    from deepmatching_stereo_matching_amd.synthetic import stereo_pair
    r = np.load(os.path.join(GOLD, 'filter_s32_roll.npz'))
    n = np.load(os.path.join(GOLD, 'filter_s16_noise.npz'))
    tiles = [(r['img1'][:20, :20], r['img2'][:20, :20]), stereo_pair(20, 20, seed=1, dx=2),
             (n['img1'], n['img2']), (r['img1'][8:28, 8:28], r['img2'][8:28, 8:28])]
    a = np.ascontiguousarray(np.hstack([t[0] for t in tiles]))
    b = np.ascontiguousarray(np.hstack([t[1] for t in tiles]))
    org = np.array([(0, 20 * t) for t in range(len(tiles))], dtype=np.int64)
    O.set_pow_mode('pinned')
    try:
        levels = [O.pyramid(O.corr_l0(x, y, 5))[0] for x, y in tiles]
        back = [O.pyramid(O.corr_l0(y, x, 5))[0] for x, y in tiles]
    finally:
        O.set_pow_mode('libm')
    return a, b, org, tiles, levels, back


@functools.lru_cache(maxsize=None)
def tile_want(t, w, mode, n, sub, backward=False):
    lv = canvas()[5 if backward else 4][t]
    if n == 0:
        return O.match(lv, sub_pix=sub)
    return O.match(lv, sub_pix=sub, filtering=True, filter_window_size=w, filtering_num=n, filtering_mode=mode)


BATCH_CASES = [(3, 'median', 3), (3, 'median', 4), (3, 'average', 4), (4, 'average', 5), (5, 'median', 4),
               (5, 'average', 5), (7, 'median', 5), (7, 'average', 7)]


def test_batched_tiles_equal_single_tiles():
    """T = 4 different tiles in one DevicePyramid: tile t's filtered match is the single-tile one
    (the t * 3 * P offsets of k_filter), the acting tiles next to the quiet one."""
    from deepmatching_stereo_matching_amd import engine
    a, b, org, tiles, levels, _ = canvas()
    pyr = engine.DevicePyramid(engine.TileBatch(a, b, org, 16, 16, 5, 5))
    single = [engine.DevicePyramid(engine.TileBatch(x, y, [(0, 0)], 16, 16, 5, 5)) for x, y in tiles]
    for w, mode, n in BATCH_CASES:
        for sub in (False, True):
            out = pyr.match(sub, True, w, n, mode).cpu().numpy()
            for t in range(len(tiles)):
                _same(out[t], single[t].match(sub, True, w, n, mode)[0].cpu().numpy())
                _same(out[t], tile_want(t, w, mode, n, sub))
        for t in (0, 2, 3):          # the filter acts on these tiles, each in its own way
            assert not np.array_equal(tile_want(t, w, mode, n, False)[:2], tile_want(t, w, mode, 0, False)[:2])
    for n in (3, 4):                 # ... and leaves the quiet tile alone while it moves its neighbours
        _same(tile_want(1, 3, 'median', n, True), tile_want(1, 3, 'median', 0, True))
    assert len({tile_want(t, 3, 'median', 4, False)[:2].tobytes() for t in range(4)}) == 4


def test_score_plane_is_copied():
    """The last pass (count = nlev, on the h0 x w0 map) moves rows and columns and copies the score
    plane: the scores of count nlev are those of count nlev - 1 bit for bit, in every tile."""
    from deepmatching_stereo_matching_amd import engine
    a, b, org, tiles, _, _ = canvas()
    pyr = engine.DevicePyramid(engine.TileBatch(a, b, org, 16, 16, 5, 5))
    for w in (3, 5, 7):
        for mode in FMODES:
            last = pyr.match(False, True, w, 5, mode).cpu().numpy()
            prev = pyr.match(False, True, w, 4, mode).cpu().numpy()
            _same(last[:, 2], prev[:, 2])
            for t in range(len(tiles)):
                _same(last[t], tile_want(t, w, mode, 5, False))
            for t in (0, 2, 3):
                assert not np.array_equal(last[t, :2], prev[t, :2])


@pytest.mark.parametrize('w,mode,n', [(3, 'median', 4), (5, 'average', 5)])
def test_tiled_paths(w, mode, n):
    """solve_tiles in one chunk and one tile per chunk, solve_tiles_bidir against the two one-way
    solves, solve_tiles_prior with a zero prior: all the filtered per-tile oracle results."""
    from deepmatching_stereo_matching_amd import engine
    a, b, org, tiles, _, _ = canvas()
    opts = (True, True, w, n, mode)
    fwd_want = np.stack([tile_want(t, w, mode, n, True) for t in range(len(tiles))])
    bwd_want = np.stack([tile_want(t, w, mode, n, True, backward=True) for t in range(len(tiles))])
    assert not np.array_equal(fwd_want, np.stack([tile_want(t, w, mode, 0, True) for t in range(len(tiles))]))
    one = engine.solve_tiles(a, b, org, 16, 16, 5, 5, *opts).cpu().numpy()
    _same(one, fwd_want)
    _same(engine.solve_tiles(a, b, org, 16, 16, 5, 5, *opts, mem_budget=1).cpu().numpy(), one)
    fwd, bwd = engine.solve_tiles_bidir(a, b, org, 16, 16, 5, 5, *opts)
    _same(fwd.cpu().numpy(), one)
    _same(bwd.cpu().numpy(), engine.solve_tiles(b, a, org, 16, 16, 5, 5, *opts).cpu().numpy())
    _same(bwd.cpu().numpy(), bwd_want)
    fwd, bwd = engine.solve_tiles_bidir(a, b, org, 16, 16, 5, 5, *opts, mem_budget=1)
    _same(fwd.cpu().numpy(), one)
    _same(bwd.cpu().numpy(), bwd_want)
    out, q_eff = engine.solve_tiles_prior(a, b, org, np.zeros((len(org), 2), dtype=np.int64), 16, 16, 5, 5, *opts)
    assert not q_eff.cpu().numpy().any()
    _same(out.cpu().numpy(), one)


CUT_VARIANTS = {'w3_average': {}, 'w3_median': {'filtering_mode': 'median'},
                'w5_median': {'filtering_mode': 'median', 'filtering_window_size': 5}}


@pytest.mark.parametrize('variant', sorted(CUT_VARIANTS))
def test_image_cut_solver(variant):
    """ImageCutSolver(filtering=True, filtering_num=4): the reference's stitched maps, the per-tile
    oracle results stitched by oracle.cut_solve, and the same keywords through the shard path."""
    from deepmatching_stereo_matching_amd import shard
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    g = np.load(os.path.join(GOLD, 'filter_cut_64_s16_st12.npz'))
    modes = [str(m) for m in g['modes']]
    extra = CUT_VARIANTS[variant]
    kw = dict(image_size=[16, 16], stride=[12, 12], window_size=5, degree_map_mode=modes, filtering=True,
              filtering_num=4, **extra)
    assert not np.array_equal(g['d_map_' + variant], g['d_map_off'])      # the filter acts on this image
    d_map, score = ImageCutSolver(g['img1'], g['img2'], **kw)()
    O.set_pow_mode('pinned')
    try:
        od, os_ = O.cut_solve(g['img1'], g['img2'], **kw)
    finally:
        O.set_pow_mode('libm')
    _same(d_map, od)
    _same(score, os_)
    assert np.max(np.abs(d_map - g['d_map_' + variant])) <= 1e-9
    assert np.max(np.abs(score - g['score_' + variant])) <= 1e-12
    sd, ss = shard.solve_image_sharded(g['img1'], g['img2'], [16, 16], [12, 12], 5, 5, modes, True, True,
                                       extra.get('filtering_window_size', 3), 4,
                                       extra.get('filtering_mode', 'average'))
    _same(sd.cpu().numpy(), od)
    _same(ss.cpu().numpy(), os_)


# ---- bookkeeping and refusals ---------------------------------------------------------------------------

def test_counter_of_one_matching_object():
    """One Matching object, filtering_num = nlev + 2, called three times: nlev passes, then the 2
    left are used up on the skipped 1 x 1 and 2 x 2 maps, then none (Matching.py:91-93, :136-138)."""
    from deepmatching_stereo_matching_amd.misc.Matching import Matching
    name = 'filter_s16_noise'
    co, _, levels = sources(name)
    nlev = len(levels)
    m = Matching(co, filtering=True, filtering_num=nlev + 2)
    left = nlev + 2
    for call in range(3):
        assert m.filtering_num == left == (nlev + 2, 2, 0)[call]
        _same(m(), want(name, nlev, 3, 'median', left, True))
        left = max(0, left - nlev)
    assert m.filtering_num == 0
    _same(m.map, want(name, nlev, 3, 'median', 0, True))
    assert not np.array_equal(want(name, nlev, 3, 'median', nlev + 2, True), m.map)


def test_non_square_tiles_and_window_range():
    from deepmatching_stereo_matching_amd.misc.Correlation_map import Correlation_map
    from deepmatching_stereo_matching_amd.misc.Matching import Matching
    g = np.load(os.path.join(GOLD, 'filter_edges.npz'))
    co = Correlation_map(g['nonsquare_img1'], g['nonsquare_img2'], window_size=5)
    co()
    plain = Matching(co)()
    held_to_fixture(plain, g['nonsquare_plain'], True)
    for n in (1, 2):     # used up on the 1 x 2 and 2 x 4 maps: no pass, no refusal
        _same(Matching(co, filtering=True, filtering_num=n)(), plain)
    with pytest.raises(NotImplementedError, match='Matching.py:235-236'):
        Matching(co, filtering=True, filtering_num=3)()
    assert str(g['nonsquare_n3_raises']).startswith('ValueError')    # what the reference does there
    sq, _, _ = sources('filter_s16_noise')
    want_plain = want('filter_s16_noise', 5, 3, 'median', 0, True)
    for w in (0, 8, 9):
        with pytest.raises(NotImplementedError, match='not in'):
            Matching(sq, filter_window_size=w, filtering=True)()
        _same(Matching(sq, filter_window_size=w, filtering=False)(), want_plain)
    for w in (-3, 100):
        _same(Matching(sq, filter_window_size=w)(), want_plain)


def test_steered_levels():
    """Hand-made levels through engine.match_levels: every position against a border, the filter
    acting on the seam; held to the restatement and to the reference's own maps."""
    from deepmatching_stereo_matching_amd import engine
    g = np.load(os.path.join(GOLD, 'filter_edges.npz'))
    levels = [g['steered_level%d' % k] for k in range(3)]
    _same(engine.match_levels(levels, False).cpu().numpy(), g['steered_plain'])
    for w, mode in ((3, 'median'), (3, 'average'), (5, 'median'), (5, 'average'), (7, 'average')):
        for sub in (False, True):
            m = engine.match_levels(levels, sub, True, w, 3, mode).cpu().numpy()
            ref, left = filter_restate(levels, sub, True, w, 3, mode)
            assert not left
            _same(m, ref)
            held_to_fixture(m, g['steered_w%d_%s_%s' % (w, mode, 'sub' if sub else 'nosub')], sub)
            if not sub:
                assert not np.array_equal(m[:2], g['steered_plain'][:2])
