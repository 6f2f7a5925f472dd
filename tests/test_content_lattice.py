"""Content lattice: images at the ends of the value range, with exact ties, and flat, on every
kernel path -- the content axis next to test_shape_lattice.py's shape axis.

The hot path rests on value-range arguments ("Value ranges"): the int32
MFMA accumulator read as the float 1.5 * 2^23 + acc, n * acc and num below 2^24 in y_of_acc,
the 24-bit multiplies of num_of, the signed-byte conversions in front of the dot products, the
a_p = 0 rule, the NaN writes of the fused kernel, and the first-NaN / first-maximum rule of the
window argmax.  The smooth texture of synthetic.stereo_pair stays in the lower third of every
one of these ranges and has unique maxima; synthetic.content_pair's kinds do not.

CPU part:
  * the ledger: for every (kind, case) the GPU tests below run, the int64 extremes the kind is
    there for are reached (conditions, not measurements: a kind edited so that it misses its
    extreme fails here);
  * the oracle's level 0 against a plain numpy restatement (int64 sums, float64 division and
    min-max): same NaN pattern, |d| <= 2^-21, the bound test_oracle_stream.py asserts for the
    float32 rounding of level 0;
  * the oracle's streamed mode against its materialising mode on every kind, bit for bit.
GPU part: DESIGN.md section 2's rule -- with the pinned pow every output equals the oracle bit
for bit, the binary16 volume equals np.float16 of the oracle's level 0.  No tolerance.
"""
import functools

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from oracle import oracle as O
from deepmatching_stereo_matching_amd.synthetic import CONTENT_KINDS, content_pair
from test_shape_lattice import ORIGINS, _crop, _feat, _same, check_levels_and_match, oracle_tile

SEED = 12
KINDS = list(CONTENT_KINDS)
TOL_L0 = 2.0 ** -21

# (h0, w0, ws): the level kernels -- mq_y, c2, c3, c5; GW = 4 with the runtime window side; the
# non-YF branch at KS = 1 .. 4 (ws = 15: the largest n)
LEVEL_CASES = [(8, 32, 5), (4, 64, 5), (8, 128, 5), (4, 256, 5), (8, 64, 3),
               (8, 64, 7), (8, 128, 9), (8, 32, 13), (8, 32, 15)]
VOLUME_CASES = [(4, 64, 5), (8, 128, 5), (8, 64, 7), (8, 32, 15)]     # ls, ls, mfq, mfq
GENERIC_CASES = [(16, 48, 5), (8, 24, 3)]                             # w0 not a power of two
FILTER_CASE, FILTER_KINDS = (32, 32, 5), ['dark', 'checker', 'edge']
STITCH_SHAPE, STITCH_TILE, STITCH_STRIDE, STITCH_WS = (100, 164), [32, 32], [16, 32], 5
STITCH_KINDS = ['dark', 'checker']
RESTATEMENT_CASES = [(8, 32, 5), (4, 64, 5), (4, 256, 5), (8, 64, 7), (8, 32, 15)]
STREAM_CASES = [(8, 32, 5), (8, 64, 7)]


# both methods on every (kind, case): a run takes about 0.05 s, and alternating the method
# would leave the flat-patch kinds (NaN writes: NORMED only) off half of the paths
LEVEL_RUNS = [(k, c, m) for c in LEVEL_CASES for k in KINDS for m in (5, 4)]
VOLUME_RUNS = [(k, c, m) for c in VOLUME_CASES for k in KINDS for m in (5, 4)]
GENERIC_RUNS = [(k, c, m) for c in GENERIC_CASES for k in KINDS for m in (5, 4)]
FILTER_RUNS = [(k, fuse) for k in FILTER_KINDS for fuse in (0, 2)]


def stitch_origins():
    """The cut grid of the stitch case, restated (image_cut_solver.py:62, :103-113: j outer, i
    inner); the GPU test asserts engine.cut_grid gives the same."""
    ex = (STITCH_WS - 1) // 2
    n = [(STITCH_SHAPE[i] - STITCH_TILE[i] - 2 * ex) // STITCH_STRIDE[i] for i in range(2)]
    return n, [(STITCH_STRIDE[0] * i, STITCH_STRIDE[1] * j) for j in range(n[1]) for i in range(n[0])]


def images(layout, kind, h0, w0, ws):
    """(img1, img2, tile origins) of one run.  'lattice': the shape lattice's padding, one tile
    plus 3 rows and 7 columns (odd pitch, odd origins); 'single': one tile, as the mirror takes
    it; 'stitch': the 100 x 164 image and its cut grid."""
    if layout == 'lattice':
        a, b = content_pair(kind, h0 + ws - 1 + 3, w0 + ws - 1 + 7, SEED)
        return a, b, ORIGINS
    if layout == 'single':
        a, b = content_pair(kind, h0 + ws - 1, w0 + ws - 1, SEED)
        return a, b, [(0, 0)]
    assert layout == 'stitch' and [h0, w0] == STITCH_TILE and ws == STITCH_WS
    a, b = content_pair(kind, STITCH_SHAPE[0], STITCH_SHAPE[1], SEED)
    return a, b, stitch_origins()[1]


def ledger_pairs():
    """Every (layout, kind, case) a GPU test of this file runs, once."""
    pairs = [('lattice', k, c) for k, c, _ in LEVEL_RUNS + VOLUME_RUNS]
    pairs += [('single', k, c) for k, c, _ in GENERIC_RUNS]
    pairs += [('lattice', k, FILTER_CASE) for k, _ in FILTER_RUNS]
    pairs += [('stitch', k, tuple(STITCH_TILE) + (STITCH_WS,)) for k in STITCH_KINDS]
    return list(dict.fromkeys(pairs))


# ----------------------------------------------------------------------------------------
# the restatement: plain numpy, independent of dm_oracle.c
# ----------------------------------------------------------------------------------------
def numpy_sums(ca, cb, ws):
    """int64 (acc', num, sT, dT, dI) of one tile crop, acc' = sum (a - 128)(b - 128) over the
    window, [P][P] with patches down and windows across.  (The P x P products go through a
    float64 matrix product: every partial sum is an integer below 225 * 128^2 < 2^53, so it is
    exact, and BLAS does it in milliseconds; everything after it is int64.)"""
    n = ws * ws
    T = sliding_window_view(ca.astype(np.int64) - 128, (ws, ws)).reshape(-1, n)
    I = sliding_window_view(cb.astype(np.int64) - 128, (ws, ws)).reshape(-1, n)
    acc = (T.astype(np.float64) @ I.astype(np.float64).T).astype(np.int64)
    sT, sI = T.sum(1), I.sum(1)
    num = n * acc - sT[:, None] * sI[None, :]
    dT = n * (T * T).sum(1) - sT * sT
    dI = n * (I * I).sum(1) - sI * sI
    return acc, num, sT, dT, dI


def numpy_l0(num, dT, dI, n, method):
    """float64 level 0 [P][P] (before the rectification): NORMED r = num / sqrt(dT dI), 0 where
    dI == 0, the row NaN where dT == 0; CCOEFF r = num / n; then the per-row min-max (a constant
    row is 0 / 0 = NaN)."""
    with np.errstate(all='ignore'):
        if method == 5:
            r = num / np.sqrt(dT.astype(np.float64)[:, None] * dI.astype(np.float64)[None, :])
            r[:, dI == 0] = 0.0
            r[dT == 0, :] = np.nan
        else:
            r = num / np.float64(n)
        lo, hi = r.min(1, keepdims=True), r.max(1, keepdims=True)
        return (r - lo) / (hi - lo)


def attainable_num(n):
    """The largest |num| two ws x ws uint8 patches can reach: k of the n taps at 255 and the
    rest at 0 in both, num = 255^2 k (n - k), k = n // 2.  (n^2 255^2 / 4 is its real-valued
    bound; n is odd.)"""
    return 255 * 255 * (n // 2) * (n - n // 2)


@functools.lru_cache(maxsize=None)
def ledger(layout, kind, case):
    """The figures of one (kind, case) over its tile crops: int64 extremes as fractions of the
    bounds the kernels' comments claim, and the shares of level-0 rows (NORMED) that are NaN /
    whose maximum is attained more than once (a NaN row counts: the argmax's first-NaN rule
    chooses among equals there too)."""
    h0, w0, ws = case
    n = ws * ws
    a, b, origins = images(layout, kind, h0, w0, ws)
    acc_hi = acc_lo = num_abs = st_abs = 0
    rows = nan_rows = tied_rows = 0
    for r, c in origins:
        acc, num, sT, dT, dI = numpy_sums(_crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws), ws)
        acc_hi, acc_lo = max(acc_hi, int(acc.max())), min(acc_lo, int(acc.min()))
        num_abs, st_abs = max(num_abs, int(np.abs(num).max())), max(st_abs, int(np.abs(sT).max()))
        x = numpy_l0(num, dT, dI, n, 5)
        nan = np.isnan(x).all(1)
        assert np.array_equal(nan, np.isnan(x).any(1))           # a row is NaN or NaN-free
        tied = nan.copy()
        tied[~nan] = (x[~nan] == x[~nan].max(1, keepdims=True)).sum(1) > 1
        rows, nan_rows, tied_rows = rows + len(nan), nan_rows + int(nan.sum()), tied_rows + int(tied.sum())
    return dict(n=n, acc_hi=acc_hi, acc_lo=acc_lo, num_abs=num_abs, st_abs=st_abs,
                f_acc_hi=acc_hi / (n * 128 * 128), f_acc_lo=-acc_lo / (n * 128 * 128),
                f_num=num_abs / (n * n * 255 * 255 / 4), f_st=st_abs / (128 * n),
                nan_share=nan_rows / rows, tied_share=tied_rows / rows)


@pytest.mark.parametrize('layout,kind,case', ledger_pairs(), ids=lambda v: str(v).replace(' ', ''))
def test_ledger_kind_reaches_what_it_is_there_for(layout, kind, case):
    """Non-vacuity: the comparison of a GPU test on this (kind, case) exercises the range
    argument the kind stands for.  |num|: 0.99 of n^2 255^2 / 4 where two patches can reach it
    (n >= 25); at n = 9 the attainable extreme 255^2 * 20 is 0.9877 of that bound, and the
    condition there is the attainable extreme itself."""
    h0, w0, ws = case
    n = ws * ws
    g = ledger(layout, kind, case)
    print(kind, case, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in g.items()})
    if kind in ('dark', 'edge'):
        assert g['acc_hi'] == n * 128 * 128
        assert g['st_abs'] == 128 * n
    if kind in ('dark_bright', 'edge', 'checker'):
        assert g['acc_lo'] <= -0.99 * n * 128 * 128
    if kind in ('binary', 'checker'):
        assert g['num_abs'] >= min(0.99 * n * n * 255 * 255 / 4, attainable_num(n))
    if kind in ('checker', 'stripes'):
        assert g['tied_share'] == 1.0
    if kind == 'dark' and ws == 5:
        assert 0.0 < g['nan_share'] < 1.0
        a, b, origins = images(layout, kind, h0, w0, ws)
        for r, c in origins:        # every tile: level 2 with some NaN, not all NaN
            lev, _, _ = O.pyramid(O.corr_l0(_crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws), ws))
            assert np.isnan(lev[2]).any() and not np.isnan(lev[2]).all(), (r, c)
    if kind == 'const':
        assert g['nan_share'] == 1.0


def test_ledger_fails_on_a_tamed_kind(monkeypatch):
    """The ledger is a condition on the generator: with `dark`'s background at 1 instead of 0,
    max acc' is n 127^2, not n 128^2, and the ledger's assertion fails."""
    import sys
    import deepmatching_stereo_matching_amd.synthetic as S

    def tamed(kind, h, w, seed):
        a, b = S.content_pair(kind, h, w, seed)
        return np.maximum(a, 1), np.maximum(b, 1)
    monkeypatch.setattr(sys.modules[__name__], 'content_pair', tamed)
    ledger.cache_clear()
    try:
        with pytest.raises(AssertionError):
            test_ledger_kind_reaches_what_it_is_there_for('lattice', 'dark', (8, 32, 5))
    finally:
        ledger.cache_clear()


@pytest.mark.parametrize('case', RESTATEMENT_CASES, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('kind', KINDS)
def test_oracle_l0_vs_numpy_restatement(kind, case):
    """O.corr_l0 (dm_oracle.c: the kernels' pinned float32 formula) against the restatement, on
    every tile crop, both methods: identical NaN pattern, |d| <= 2^-21; and the oracle's own
    two formulas (pinned against the f64 division) within the same bound, no NaN moved."""
    h0, w0, ws = case
    a, b, origins = images('lattice', kind, h0, w0, ws)
    worst = 0.0
    for r, c in origins:
        ca, cb = _crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws)
        _, num, _, dT, dI = numpy_sums(ca, cb, ws)
        for method in (5, 4):
            want = numpy_l0(num, dT, dI, ws * ws, method)
            got = O.corr_l0(ca, cb, ws, _feat(method)).reshape(want.shape).astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (kind, case, method)
            if not np.isnan(want).all():
                worst = max(worst, float(np.nanmax(np.abs(got - want))))
            d = O.zncc_formula_diff(ca, cb, ws, _feat(method))
            assert d['nan_mismatch'] == 0 and d['max_abs'] <= TOL_L0, (kind, case, method, d)
    print('oracle vs numpy', kind, case, 'max |d| = %.3e' % worst)
    assert worst <= TOL_L0


@pytest.mark.parametrize('pow_mode', ['libm', 'pinned'])
@pytest.mark.parametrize('case', STREAM_CASES, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('kind', KINDS)
def test_oracle_stream_equals_materialised(kind, case, pow_mode):
    """pyramid_stream / match_stream (what checks the large tiles) == pyramid / match, bit for
    bit, on every kind, both methods."""
    h0, w0, ws = case
    a, b, _ = images('single', kind, h0, w0, ws)
    O.set_pow_mode(pow_mode)
    try:
        for method in (5, 4):
            lev, it, nm = O.pyramid(O.corr_l0(a, b, ws, _feat(method)))
            slev, sit, snm = O.pyramid_stream(a, b, ws, _feat(method))
            assert (it, nm, len(lev)) == (sit, snm, len(slev))
            for k in range(1, len(lev)):
                _same(slev[k], lev[k])
            for sp in (False, True):
                _same(O.match_stream(a, b, ws, slev, sub_pix=sp, feature=_feat(method)), O.match(lev, sub_pix=sp))
    finally:
        O.set_pow_mode('libm')


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pinned_pow():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    O.set_pow_mode('pinned')
    yield
    O.set_pow_mode('libm')


def _ids(v):
    return str(v).replace(' ', '')


@pytest.mark.gpu
@pytest.mark.parametrize('kind,case,method', LEVEL_RUNS, ids=_ids)
def test_content_levels_vs_oracle(kind, case, method, pinned_pow):
    """Every kind on every level-kernel path: fuse_level2 = 0 / 1 / 2 (mode 2: the on-demand
    l0_value / l1_value and sub-pixel step of the matching), the direct two-output
    dm_corr_level12 call, every level >= 1 and match(sub_pix=True), bit for bit."""
    h0, w0, ws = case
    a, b, _ = images('lattice', kind, h0, w0, ws)
    check_levels_and_match(a, b, h0, w0, ws, method)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,case,method', VOLUME_RUNS, ids=_ids)
def test_content_volume_vs_oracle(kind, case, method, pinned_pow):
    """The level-0 volume kernels (k_volume_ls, k_volume_mfq) on every kind: float32 == oracle,
    binary16 == np.float16(oracle), and the min/max-known calls after a mode-2 pyramid == the
    standalone calls (test_volume_lattice_vs_oracle's form)."""
    import torch
    from deepmatching_stereo_matching_amd import _lib as L
    from deepmatching_stereo_matching_amd import engine
    h0, w0, ws = case
    a, b, origins = images('lattice', kind, h0, w0, ws)
    P, T = h0 * w0, len(origins)
    batch = engine.TileBatch(a, b, origins, h0, w0, ws, method)
    lib = L.load()
    fresh = engine.DevicePyramid(batch, build=False).compute_stats()
    v32 = torch.empty((T, P, P), dtype=torch.float32, device='cuda')
    v16 = torch.empty((T, P, P), dtype=torch.float16, device='cuda')
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh.stats), 0, L.ptr(v32), L.stream_handle()))
    fresh16 = engine.DevicePyramid(batch, build=False).compute_stats()
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh16.stats), L.DM_VOLUME_F16, L.ptr(v16),
                                  L.stream_handle()))
    r32, r16 = v32.cpu().numpy(), v16.cpu().numpy()
    assert r16.dtype == np.float16
    for t, (r, c) in enumerate(origins):
        l0 = O.corr_l0(_crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws), ws, _feat(method)).reshape(P, P)
        _same(r32[t], l0)
        _same(r16[t], l0.astype(np.float16))
    pyr = engine.DevicePyramid(batch, fuse_level2=2)
    assert pyr._have_minmax
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN, L.ptr(v32),
                                  L.stream_handle()))
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN | L.DM_VOLUME_F16,
                                  L.ptr(v16), L.stream_handle()))
    _same(v32.cpu().numpy(), r32)
    _same(v16.cpu().numpy(), r16)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,case,method', GENERIC_RUNS, ids=_ids)
def test_content_generic_path_and_mirror(kind, case, method, pinned_pow):
    """The generic kernels (w0 = 48, 24) through Correlation_map / Matching, as
    test_shapes_vs_oracle does: every level and the matching, bit for bit."""
    from deepmatching_stereo_matching_amd.misc import Correlation_map, Matching
    h0, w0, ws = case
    a, b, _ = images('single', kind, h0, w0, ws)
    co = Correlation_map.Correlation_map(a, b, window_size=ws, feature_name=_feat(method))
    co()
    ol0 = O.corr_l0(a, b, ws, _feat(method))
    olev, it, n_map = O.pyramid(ol0)
    assert co.iteration == it and co.N_map == n_map
    _same(co.co_map.astype(np.float32), ol0)
    for k in range(len(olev)):
        _same(co.co_map_list[k], olev[k])
    _same(Matching.Matching(co, sub_pix=False)(), O.match(olev, sub_pix=False))
    _same(Matching.Matching(co)(), O.match(olev, sub_pix=True))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,fuse', FILTER_RUNS, ids=_ids)
def test_content_match_filter(kind, fuse, pinned_pow):
    """Matching._filter (the median / average of the disparities between the levels of the
    descent) on maps with NaN scores and tied maxima, level 1 stored and on demand."""
    from deepmatching_stereo_matching_amd import engine
    h0, w0, ws = FILTER_CASE
    a, b, origins = images('lattice', kind, h0, w0, ws)
    levs = [oracle_tile(a, b, r, c, h0, w0, ws, 5)[0] for r, c in origins]
    pyr = engine.DevicePyramid(engine.TileBatch(a, b, origins, h0, w0, ws, 5), fuse_level2=fuse)
    assert (pyr.levels[1] is None) == (fuse == 2)
    for mode in ('median', 'average'):
        got = pyr.match(sub_pix=True, filtering=True, filtering_mode=mode).cpu().numpy()
        for t, lev in enumerate(levs):
            _same(got[t], O.match(lev, sub_pix=True, filtering=True, filtering_mode=mode))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', STITCH_KINDS)
def test_content_batched_engine_and_stitch(kind, pinned_pow):
    """engine.solve_tiles on the overlapping cut grid of a 100 x 164 image == the per-tile
    oracle, and ImageCutSolver == O.cut_solve (tiling, stitching, cal_map)."""
    from deepmatching_stereo_matching_amd import engine
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    h0, w0 = STITCH_TILE
    ws = STITCH_WS
    a, b, origins = images('stitch', kind, h0, w0, ws)
    n, org = engine.cut_grid(a.shape, STITCH_TILE, STITCH_STRIDE, ws)
    assert list(n) == stitch_origins()[0] and [tuple(o) for o in org.tolist()] == origins
    got = engine.solve_tiles(a, b, org, h0, w0, ws, 5).cpu().numpy()
    for t, (r, c) in enumerate(origins):
        _same(got[t], oracle_tile(a, b, r, c, h0, w0, ws, 5)[1])
    kw = dict(image_size=STITCH_TILE, stride=STITCH_STRIDE, window_size=ws,
              degree_map_mode=['elevation', 'elevation2', 'distance'])
    d_map, score = ImageCutSolver(a, b, **kw)()
    od, os_ = O.cut_solve(a, b, **kw)
    _same(d_map, od)
    _same(score, os_)
