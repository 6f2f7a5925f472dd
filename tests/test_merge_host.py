"""Overlap-merging stitch (dm_stitch_merge), host side (no GPU): merge_restate, a plain-loop
numpy statement of the definition in include/dmstereo.h; the entry's argument validation (it
returns before any HIP call); fixed points of the restatement; the theorem that merging never
adds a hole; and the sharded path with the oracle as tile solver and the restatement as the
merger -- one process and gloo world size 2 -- against a direct computation.

Comparisons are bitwise (int64 views, NaN positions equal)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard

from test_fb_host import _case, _free_port, _host_stitch, _host_stitch_fb, _oracle_tiles, fb_restate, place, same_bits
from test_fill_host import fill_restate

RULES = ('last', 'center', 'feather', 'median')


# ---------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------
def _values(ly, lx, r, q):
    """dm_stitch's three cal_map expressions, by dm_cal_mode."""
    a, b = np.float64(ly) - r, np.float64(lx) - q
    return (b, a, np.sqrt(a * a + b * b))


def _fb_err(F, B, t, ly, lx):
    h, w = F.shape[2:]
    qi, qj = np.floor(F[t, 0, ly, lx] + 0.5), np.floor(F[t, 1, ly, lx] + 0.5)
    if not (qi >= 0 and qi < h and qj >= 0 and qj < w):      # on the doubles, before any cast
        return np.float64(np.nan)
    dr, dc = B[t, 0, int(qi), int(qj)] - np.float64(ly), B[t, 1, int(qi), int(qj)] - np.float64(lx)
    return np.sqrt(dr * dr + dc * dc)


def _median(vals):
    """The definition's median by ranks of a list of float64 in candidate order."""
    m = len(vals)
    lo, hi = (m - 1) // 2, m // 2
    a = b = np.float64(np.nan)
    for c, v in enumerate(vals):
        rank = sum(1 for c2, v2 in enumerate(vals) if v2 < v or (v2 == v and c2 < c))
        if rank == lo:
            a = v
        if rank == hi:
            b = v
    return a if m % 2 else (a + b) * np.float64(0.5)


def merge_restate(F, B, n, stride, modes, tol=None, rule='feather', min_count=1):
    """dm_stitch_merge on host arrays: F, B (or None) float64 [T][3][h0][w0], modes a list of
    names -> (dmap [nmodes][H][W], score [H][W], err [H][W] or None, spread [nmodes][H][W],
    count [H][W] uint8).  One Python loop per pixel and candidate, float64 in the order written."""
    F = np.asarray(F, dtype=np.float64)
    B = None if B is None else np.asarray(B, dtype=np.float64)
    ids = [L.CAL_MODES[m] for m in modes]
    T, _, h0, w0 = F.shape
    assert T == n[0] * n[1] and rule in RULES and (rule != 'last' or min_count == 1)
    H, W = stride[0] * (n[0] - 1) + h0, stride[1] * (n[1] - 1) + w0
    nan = np.float64(np.nan)
    dmap, spread = np.full((len(ids), H, W), nan), np.full((len(ids), H, W), nan)
    score, err = np.full((H, W), nan), np.full((H, W), nan)
    count = np.zeros((H, W), np.uint8)
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                cands = []          # (v[3], s, e, g, valid) in the order j outer, i inner
                for j in range(n[1]):
                    for i in range(n[0]):
                        ly, lx = y - i * stride[0], x - j * stride[1]
                        if not (0 <= ly < h0 and 0 <= lx < w0):
                            continue
                        t = j * n[0] + i
                        r, q, s = F[t, 0, ly, lx], F[t, 1, ly, lx], F[t, 2, ly, lx]
                        e = _fb_err(F, B, t, ly, lx) if B is not None else nan
                        valid = bool(np.isfinite(r) and np.isfinite(q) and (B is None or e <= tol))
                        g = np.float64(min(ly + 1, h0 - ly)) * np.float64(min(lx + 1, w0 - lx))
                        cands.append((_values(ly, lx, r, q), s, e, g, valid))
                if not cands:
                    continue
                ok = [c for c in cands if c[4]]
                m = len(ok)
                count[y, x] = m
                for k, mode in enumerate(ids):
                    if m:
                        vs = [c[0][mode] for c in ok]
                        mx = mn = vs[0]
                        for v in vs[1:]:
                            mn, mx = (v if v < mn else mn), (v if v > mx else mx)
                        spread[k, y, x] = mx - mn
                last = cands[-1]
                if rule == 'last':
                    keep = B is None or last[2] <= tol
                    for k, mode in enumerate(ids):
                        dmap[k, y, x] = last[0][mode] if keep else nan
                    score[y, x], err[y, x] = last[1], last[2]
                    continue
                if m == 0:
                    score[y, x], err[y, x] = last[1], last[2]
                    continue
                out = [nan, nan, nan]
                if rule == 'center':
                    best = ok[0]
                    for c in ok[1:]:
                        if c[3] >= best[3]:
                            best = c
                    out, score[y, x], err[y, x] = list(best[0]), best[1], best[2]
                else:
                    emin = ok[0][2]
                    for c in ok[1:]:
                        emin = c[2] if c[2] < emin else emin
                    err[y, x] = emin
                    if rule == 'feather':
                        num, snum, den = [np.float64(0)] * 3, np.float64(0), np.float64(0)
                        for c in ok:
                            num = [num[e_] + c[3] * c[0][e_] for e_ in range(3)]
                            snum = snum + c[3] * c[1]
                            den = den + c[3]
                        out, score[y, x] = [v / den for v in num], snum / den
                    else:
                        out = [_median([c[0][e_] for c in ok]) for e_ in range(3)]
                        score[y, x] = _median([c[1] for c in ok])
                if m >= min_count:
                    for k, mode in enumerate(ids):
                        dmap[k, y, x] = out[mode]
    return dmap, score, (err if B is not None else None), spread, count


def _host_merge(fwd, bwd, n, h0, w0, stride, modes, tol, rule, min_count):
    """merger hook of solve_image_sharded."""
    return merge_restate(np.asarray(fwd), None if bwd is None else np.asarray(bwd), n, stride, modes, tol,
                         rule, min_count)


# ---------------------------------------------------------------------------------------------
# 2. validation through the library (never-dereferenced pointers)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)


def _merge_args(**kw):
    a = dict(f=P8, b=P8, n0=2, n1=2, h0=4, w0=4, s0=2, s1=2, modes=(ctypes.c_int32 * 1)(0), nm=1, tol=1.0,
             rule=2, mc=1, d=P8, s=P8, e=P8, sp=P8, c=P8)
    a.update(kw)
    return (a['f'], a['b'], a['n0'], a['n1'], a['h0'], a['w0'], a['s0'], a['s1'], a['modes'], a['nm'], a['tol'],
            a['rule'], a['mc'], a['d'], a['s'], a['e'], a['sp'], a['c'], None)


def test_abi_version_unchanged(lib):
    assert lib.dm_abi_version() == 110
    assert 'dm_stitch_merge' in L.header_symbols() and 'dm_stitch_merge' in L.SIGNATURES
    assert L.MERGE_RULES == {'last': 0, 'center': 1, 'feather': 2, 'median': 3}


@pytest.mark.parametrize('kw,needle', [
    (dict(f=None), 'stitch'), (dict(d=None), 'stitch'), (dict(s=None), 'stitch'), (dict(n0=0), 'stitch'),
    (dict(n1=0), 'stitch'), (dict(s0=0), 'stitch'), (dict(s1=-3), 'stitch'), (dict(h0=0), 'stitch'),
    (dict(w0=0), 'stitch'), (dict(modes=None), 'stitch'), (dict(nm=9), 'stitch'),
    (dict(modes=(ctypes.c_int32 * 1)(9)), 'please input valid mode! (9)'),
    (dict(rule=-1), 'rule'), (dict(rule=4), 'rule'),
    (dict(mc=0), 'min_count'), (dict(mc=256), 'min_count'), (dict(rule=0, mc=2), 'min_count must be 1'),
    (dict(b=None), 'backward'),                                  # d_err without d_bwd
    (dict(tol=-1.0), 'tolerance'), (dict(tol=float('nan')), 'tolerance'),
])
def test_stitch_merge_validation(lib, kw, needle):
    assert lib.dm_stitch_merge(*_merge_args(**kw)) == L.DM_ERR_ARG
    assert needle in L.last_error()


def test_stitch_merge_candidate_bound(lib):
    # 9 x 8 tiles of 9 x 8 cells at stride 1: 72 tiles over the middle pixel
    kw = dict(n0=9, n1=8, h0=9, w0=8, s0=1, s1=1)
    assert lib.dm_stitch_merge(*_merge_args(**kw)) == L.DM_ERR_UNSUPPORTED
    assert '72' in L.last_error() and str(L.DM_MERGE_MAX_CAND) in L.last_error()
    with pytest.raises(NotImplementedError):
        L.check(lib.dm_stitch_merge(*_merge_args(**kw)))
    # larger tiles: the tile counts bound the candidates, min(9, 100) * min(8, 50)
    kw = dict(n0=9, n1=8, h0=100, w0=100, s0=1, s1=2)
    assert lib.dm_stitch_merge(*_merge_args(**kw)) == L.DM_ERR_UNSUPPORTED
    assert '72' in L.last_error()
    # and it is checked after the arguments
    assert lib.dm_stitch_merge(*_merge_args(rule=7, **kw)) == L.DM_ERR_ARG


def test_engine_stitch_merge_argument_checks():
    f = torch.zeros((4, 3, 4, 4), dtype=torch.float64)
    with pytest.raises(ValueError):
        engine.stitch_merge(f, f, (2, 2), 4, 4, (2, 2), ['elevation'], 1.0)          # host tensors
    with pytest.raises(ValueError):
        engine.stitch_merge(f, None, (2, 2), 4, 4, (2, 2), ['elevation'], rule='mean')
    with pytest.raises(ValueError):
        engine.merge_rule('mean')
    assert engine.merge_rule('median') == 3


# ---------------------------------------------------------------------------------------------
# 3. fixed points of the restatement
# ---------------------------------------------------------------------------------------------
MODES3 = ['elevation', 'elevation2', 'distance']


def _cal(tiles, mode):
    """cal_map of [T][3][h][w] tiles, vectorised: the same three expressions."""
    T, _, h, w = tiles.shape
    ii, jj = (x.astype(np.float64) for x in np.mgrid[0:h, 0:w])
    with np.errstate(all='ignore'):
        a, b = ii - tiles[:, 0], jj - tiles[:, 1]
        return {'elevation': b, 'elevation2': a, 'distance': np.sqrt(a * a + b * b)}[mode]


def _random_tiles(n, h0, w0, seed, nan_share=0.05, cells=False):
    """Matches near their cell, a share of NaN entries (``cells``: NaN in rows 0 and 1 at once)."""
    T = n[0] * n[1]
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:h0, 0:w0]
    F = np.stack([np.stack([ii + rng.normal(0, 1.0, (h0, w0)), jj + rng.normal(0, 1.0, (h0, w0)),
                            rng.uniform(0, 5, (h0, w0))]) for _ in range(T)])
    B = np.stack([np.stack([ii + rng.normal(0, 0.5, (h0, w0)), jj + rng.normal(0, 0.5, (h0, w0)),
                            rng.uniform(0, 5, (h0, w0))]) for _ in range(T)])
    if cells:
        F[:, :2][np.broadcast_to(rng.uniform(size=(T, 1, h0, w0)) < nan_share, (T, 2, h0, w0))] = np.nan
    else:
        F[rng.uniform(size=F.shape) < nan_share] = np.nan
    return F, B


@pytest.mark.parametrize('stride', [(3, 4), (6, 8), (7, 10)])
def test_last_is_place(stride):
    n, h0, w0 = (3, 2), 6, 8
    F, B = _random_tiles(n, h0, w0, 3)
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, MODES3, rule='last')
    assert e is None
    for k, mode in enumerate(MODES3):
        assert same_bits(d[k], place(_cal(F, mode), n, stride))
    assert same_bits(s, place(F[:, 2], n, stride))
    if stride == (3, 4):
        assert cnt.max() == 4
    d, s, e, sp, cnt = merge_restate(F, B, n, stride, MODES3, 1.0, 'last')
    err, masked = fb_restate(F, B, 1.0)
    for k, mode in enumerate(MODES3):
        assert same_bits(d[k], place(_cal(masked, mode), n, stride))
    assert same_bits(s, place(F[:, 2], n, stride)) and same_bits(e, place(err, n, stride))
    assert 0 < np.isnan(d).mean() < 1
    covered = ~np.isnan(place(np.zeros((n[0] * n[1], h0, w0)), n, stride))
    assert (cnt[~covered] == 0).all() and np.isnan(sp[:, ~covered]).all()
    if stride == (7, 10):        # a stride larger than the tile leaves gaps
        assert (~covered).any() and np.isnan(s[~covered]).all() and np.isnan(e[~covered]).all()


@pytest.mark.parametrize('bidir', [False, True])
def test_stride_equal_to_tile_makes_every_rule_last(bidir):
    """One candidate per pixel: every rule returns it.  (With one direction LAST passes a cell
    with one finite coordinate through, as dm_stitch does, and the other rules reject it: the
    NaN cells here are NaN in both coordinates.)  CENTER and MEDIAN return it bit for bit; FEATHER
    returns (g v) / g, two roundings of relative error 2^-53 each, so within 2 ulp of v."""
    n, h0, w0 = (2, 3), 5, 7
    F, B = _random_tiles(n, h0, w0, 8, cells=True)
    args = (F, B if bidir else None, n, (h0, w0), MODES3, 1.0 if bidir else None)
    want = merge_restate(*args, 'last')
    assert want[4].max() == 1 and want[4].min() == 0
    for rule in RULES[1:]:
        got = merge_restate(*args, rule)
        for k, (g, w) in enumerate(zip(got, want)):
            if rule == 'feather' and k < 2:
                assert np.array_equal(np.isnan(g), np.isnan(w))
                ok = ~np.isnan(w)
                assert (np.abs(g[ok] - w[ok]) <= 2 * np.spacing(np.abs(w[ok]))).all()
            else:
                assert (g is None and w is None) or same_bits(g, w), rule
        assert got[4].dtype == np.uint8 and np.array_equal(got[4], want[4])
        assert (got[3][:, got[4] == 1] == 0).all() and np.isnan(got[3][:, got[4] == 0]).all()


def _two_by_two(vals, scores=None, h0=4, w0=4):
    """2 x 2 tiles of h0 x w0 at stride (h0/2, w0/2); tile t's every cell has elevation
    vals[t] (q = lx - vals[t], r = ly) and score scores[t]."""
    T = 4
    ii, jj = np.mgrid[0:h0, 0:w0]
    F = np.zeros((T, 3, h0, w0))
    for t in range(T):
        F[t, 0], F[t, 1] = ii, jj - np.float64(vals[t])
        F[t, 2] = (scores or vals)[t]
    return F, (2, 2), (h0 // 2, w0 // 2)


def test_median_even_and_odd():
    F, n, stride = _two_by_two([4.0, 1.0, 3.0, 2.0], [7.0, 5.0, 5.0, 9.0])
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='median')
    assert cnt[2, 2] == 4 and d[0, 2, 2] == 2.5 and s[2, 2] == 6.0 and sp[0, 2, 2] == 3.0
    assert cnt[0, 2] == 2 and d[0, 0, 2] == (4.0 + 3.0) * 0.5        # tiles 0 and 2 (j = 0, 1; i = 0)
    assert cnt[0, 0] == 1 and d[0, 0, 0] == 4.0
    F[1, 0, 0, 2] = np.nan                   # tile 1 (i = 1, j = 0) loses its cell over pixel (2, 2)
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='median')
    assert cnt[2, 2] == 3 and d[0, 2, 2] == 3.0 and s[2, 2] == 7.0 and sp[0, 2, 2] == 2.0
    assert _median([np.float64(v) for v in (2.0, 1.0, 2.0, 1.0)]) == 1.5
    assert np.isnan(_median([np.float64(np.nan), np.float64(1.0)]))


def test_center_ties_go_to_the_later_candidate():
    F, n, stride = _two_by_two([4.0, 1.0, 3.0, 2.0])
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='center')
    # pixel (2, 2): local cells (2,2), (0,2), (2,0), (0,0) of tiles 0..3, weights 4, 2, 2, 1
    assert d[0, 2, 2] == 4.0 and s[2, 2] == 4.0
    # pixel (3, 3): local (3,3), (1,3), (3,1), (1,1): weights 1, 2, 2, 4 -> tile 3
    assert d[0, 3, 3] == 2.0
    # pixel (2, 3): local (2,3), (0,3), (2,1), (0,1): weights 2, 1, 4, 2 -> tile 2
    assert d[0, 2, 3] == 3.0
    # a tie: 5 x 4 tiles at stride (2, 2), pixel (3, 0) is covered by tiles 0 (local (3,0):
    # min(4, 2) * 1 = 2) and 1 (local (1,0): min(2, 4) * 1 = 2)
    F, n, stride = _two_by_two([4.0, 1.0, 3.0, 2.0], h0=5, w0=4)
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='center')
    assert cnt[3, 0] == 2 and d[0, 3, 0] == 1.0          # the later of the two tied candidates
    F[1, 1, 1, 0] = np.inf                                # ... unless it is not valid
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='center')
    assert cnt[3, 0] == 1 and d[0, 3, 0] == 4.0


def test_feather_weights_and_min_count_cut():
    F, n, stride = _two_by_two([4.0, 1.0, 3.0, 2.0])
    d, s, e, sp, cnt = merge_restate(F, None, n, stride, ['elevation'], rule='feather')
    assert d[0, 2, 2] == (4 * 4.0 + 2 * 1.0 + 2 * 3.0 + 1 * 2.0) / 9.0
    assert d[0, 0, 0] == 4.0 and d[0, 5, 5] == 2.0
    for rule in RULES[1:]:
        full = merge_restate(F, None, n, stride, ['elevation'], rule=rule)
        for mc in (2, 3, 4, 5):
            cut = merge_restate(F, None, n, stride, ['elevation'], rule=rule, min_count=mc)
            keep = full[4] >= mc
            assert np.isnan(cut[0][0][~keep]).all() and same_bits(cut[0][0][keep], full[0][0][keep])
            for a, b in zip(cut[1:], full[1:]):          # only d_map is cut
                assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
        assert np.isnan(merge_restate(F, None, n, stride, ['elevation'], rule=rule, min_count=5)[0]).all()


def test_nothing_valid_keeps_last_score_and_err():
    n, h0, w0, stride = (2, 2), 4, 4, (2, 2)
    F, B = _random_tiles(n, h0, w0, 21, nan_share=0.0)
    F[:, 0, :, :] += 40.0                   # every match off its tile: err NaN everywhere
    last = merge_restate(F, B, n, stride, ['elevation'], 1.0, 'last')
    for rule in RULES[1:]:
        got = merge_restate(F, B, n, stride, ['elevation'], 1.0, rule)
        assert np.isnan(got[0]).all() and (got[4] == 0).all() and np.isnan(got[3]).all()
        assert same_bits(got[1], last[1]) and same_bits(got[2], last[2])


# ---------------------------------------------------------------------------------------------
# 4. the theorem: rules 1..3 with min_count = 1 never add a hole to LAST's map
# ---------------------------------------------------------------------------------------------
MODES = ('elevation', 'distance')
GEOM = dict(image_size=[16, 16], stride=[8, 8], ws=5)


@pytest.fixture(scope='module')
def tiles():
    """The oracle's forward and backward tiles of test_fb_host's pair at stride 8."""
    a, b = _case()
    n, org = engine.cut_grid(a.shape, GEOM['image_size'], GEOM['stride'], GEOM['ws'])
    fwd = _oracle_tiles(a, b, org, 16, 16, 5, 5, True, False, 3, 3, 'average').numpy()
    bwd = _oracle_tiles(b, a, org, 16, 16, 5, 5, True, False, 3, 3, 'average').numpy()
    return n, fwd, bwd


@pytest.fixture(scope='module')
def direct(tiles):
    n, fwd, bwd = tiles
    return {rule: merge_restate(fwd, bwd, n, GEOM['stride'], MODES, 1.0, rule) for rule in RULES}


def test_merging_never_adds_a_hole(tiles, direct):
    n, fwd, bwd = tiles
    assert n == [3, 5]
    last = np.isnan(direct['last'][0])
    ref = _host_stitch_fb(fwd, bwd, n, 16, 16, GEOM['stride'], MODES, 1.0)
    for g, w in zip(direct['last'][:3], ref):
        assert same_bits(g, w)
    assert direct['last'][4].max() == 4
    for rule in RULES[1:]:
        holes = np.isnan(direct[rule][0])
        assert not (holes & ~last).any(), rule
        print('%s: %d holes, last: %d of %d cells' % (rule, holes.sum(), last.sum(), last.size))
        assert holes.sum() < last.sum(), rule           # a strict subset on this pair
        assert np.array_equal(holes[0], direct[rule][4] == 0) and np.array_equal(holes[0], holes[1])


# ---------------------------------------------------------------------------------------------
# 5. the sharded path
# ---------------------------------------------------------------------------------------------
def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


def _same_maps(got, want):
    want = [w for w in want if w is not None]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = np.asarray(g)
        assert g.dtype == w.dtype
        assert np.array_equal(g, w) if w.dtype == np.uint8 else same_bits(g, w)


@pytest.mark.parametrize('rule', RULES)
def test_sharded_merge_single_process(direct, rule):
    a, b = _case()
    got = _sharded(a, b, consistency=1.0, merge=rule, merger=_host_merge)
    assert len(got) == 5
    _same_maps(got, direct[rule])


def test_sharded_merge_one_direction(tiles):
    a, b = _case()
    n, fwd, _ = tiles
    got = _sharded(a, b, merge='feather', merge_min_count=2, merger=_host_merge)
    assert len(got) == 4
    _same_maps(got, merge_restate(fwd, None, n, GEOM['stride'], MODES, None, 'feather', 2))
    with pytest.raises(ValueError):
        _sharded(a, b, merge='mean', merger=_host_merge)


def test_sharded_merge_none_is_unchanged():
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, merge=None, merger=_host_merge)
    ref = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)
    assert len(got) == 3 and len(ref) == 3
    for g, r in zip(got, ref):
        assert same_bits(g, r)
    got, ref = _sharded(a, b, stitcher=_host_stitch, merge=None), _sharded(a, b, stitcher=_host_stitch)
    assert len(got) == 2 and len(ref) == 2
    for g, r in zip(got, ref):
        assert same_bits(g, r)


def _host_fill(maps, iters):
    return fill_restate(np.asarray(maps), iters)


def test_sharded_merge_with_fill(direct):
    a, b = _case()
    plain = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, fill=16, filler=_host_fill)
    got = _sharded(a, b, consistency=1.0, merge='median', merger=_host_merge, fill=16, filler=_host_fill)
    assert len(plain) == 4 and len(got) == 6
    want_d, want_holes = fill_restate(direct['median'][0], 16)
    assert same_bits(got[0], want_d) and np.array_equal(np.asarray(got[5]), want_holes)
    _same_maps(got[1:5], direct['median'][1:])
    assert np.isfinite(np.asarray(got[0])).all()
    holes, plain_holes = np.asarray(got[5]).astype(bool), np.asarray(plain[3]).astype(bool)
    assert not (holes & ~plain_holes).any() and holes.sum() < plain_holes.sum()


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        kw = dict(consistency=1.0, merge='feather', merger=_host_merge)
        all_ = _sharded(a, b, **kw)
        root = _sharded(a, b, result='root', fill=16, filler=_host_fill, **kw)
        one = _sharded(a, b, merge='center', merger=_host_merge)
        none = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, merge=None)
        q.put((rank, [np.asarray(x) for x in all_], [None if x is None else np.asarray(x) for x in root],
               [np.asarray(x) for x in one], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_merge_gloo_world_2(tiles, direct):
    n, fwd, bwd = tiles
    want_one = merge_restate(fwd, None, n, GEOM['stride'], MODES, None, 'center')
    want_none = _host_stitch_fb(fwd, bwd, n, 16, 16, GEOM['stride'], MODES, 1.0)
    want_fill = fill_restate(direct['feather'][0], 16)
    size = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, size, port, q)) for r in range(size)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(size)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, all_, root, one, none in res:
        _same_maps(all_, direct['feather'])
        if rank == 0:
            assert same_bits(root[0], want_fill[0]) and np.array_equal(root[5], want_fill[1])
            _same_maps(root[1:5], direct['feather'][1:])
        else:
            assert root == [None] * 6
        _same_maps(one, want_one)
        _same_maps(none, want_none)
