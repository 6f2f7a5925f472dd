"""Weighted median filter, host side (no GPU): the plain-loop restatement of the definition
(median_restate: what dm_median_filter must equal bit for bit), a faster vectorised restatement
pinned to it (median_fast: the one the GPU tests use), properties of the definition, the two
planted cases the filter exists for, argument validation of the two C entries (it returns before
any HIP call) and of the keywords, and the sharded path with the oracle as tile solver, a host
stitcher and the restatement injected as the medianer -- single process and gloo world size 2.

Comparisons with the restatement are bitwise (int64 views)."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard

from test_fill_host import (GEOM, MODES, _case, _free_port, _host_fill, _host_stitch, _host_stitch_fb,
                            _oracle_tiles, fill_restate, raw_bits, same_bits)
from test_speckle_host import _host_speckle, speckle_restate


@pytest.fixture(scope='module', autouse=True)
def entries():
    """What this file restates and checks is the pair of C entries: without them nothing here holds."""
    lib = L.load()
    assert hasattr(lib, 'dm_median_filter') and hasattr(lib, 'dm_median_bytes')
    assert callable(getattr(engine, 'median_filter', None)) and callable(getattr(engine, 'median_params', None))


# ---------------------------------------------------------------------------------------------
# the definition in plain loops; Python floats are IEEE doubles, one rounding per addition
# ---------------------------------------------------------------------------------------------
SIGN = 1 << 63
ALL = (1 << 64) - 1
INF, NAN = float('inf'), float('nan')


def key_of(v):
    """The order-preserving 64-bit integer of a double."""
    b = struct.unpack('<Q', struct.pack('<d', v))[0]
    return (b ^ ALL) if b & SIGN else (b | SIGN)


def _finite(v):
    return -1.7976931348623157e308 <= v <= 1.7976931348623157e308      # (NaN fails both)


def _pass(x, w, r, min_count, fill):
    H, W = x.shape
    X = x.tolist()
    Wt = None if w is None else w.tolist()
    out = x.copy()
    for i in range(H):
        for j in range(W):
            if not _finite(X[i][j]) and not fill:
                continue
            taps = []                       # (key, weight, row, column) in window order
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    y, t = i + dy, j + dx
                    if not (0 <= y < H and 0 <= t < W) or not _finite(X[y][t]):
                        continue
                    wt = 1.0
                    if Wt is not None:
                        wt = Wt[y][t]
                        if not (wt > 0 and wt < INF):
                            continue
                    taps.append((key_of(X[y][t]), wt, y, t))
            n = len(taps)
            if n < min_count:
                continue
            if Wt is None:
                best = sorted(taps, key=lambda t: t[0])[(n - 1) // 2]
            else:
                T = 0.0
                for t in taps:
                    T = T + t[1]
                best = None
                for cand in taps:           # the candidate loop of the definition
                    S = 0.0
                    for t in taps:
                        if t[0] <= cand[0]:
                            S = S + t[1]
                    if S >= 0.5 * T and (best is None or cand[0] < best[0]):
                        best = cand
            out[i, j] = x[best[2], best[3]]  # equal keys are equal bits: any tap of that key will do
    return out


def _maps(x, weight):
    x = np.ascontiguousarray(x, dtype=np.float64)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    xs = x[None] if x.ndim == 2 else x
    ws = [None if w is None else (w if w.ndim == 2 else w[k]) for k in range(len(xs))]
    return x, xs, ws


def _changed(out, x):
    return (out.view(np.int64) != x.view(np.int64)).astype(np.uint8)


def median_restate(x, weight, r, iters=1, min_count=1, fill=False):
    """The definition on [H][W] or [M][H][W] float64 maps; weight None, [H][W] or of x's shape ->
    (out, uint8 changed)."""
    x, xs, ws = _maps(x, weight)
    outs = []
    for m, w in zip(xs, ws):
        cur = m
        for _ in range(iters):
            cur = _pass(cur, w, r, min_count, fill)
        outs.append(cur)
    out = np.ascontiguousarray(np.stack(outs).reshape(x.shape))
    return out, _changed(out, x)


# ---------------------------------------------------------------------------------------------
# the fast restatement: the window as a stack of planes, sorted by key; the weighted form bisects
# over the sorted taps, S summed in window order over the whole map at once (a tap that does not
# take part adds +0, which changes no bit of a sum of terms >= +0 that starts at +0)
# ---------------------------------------------------------------------------------------------
_S = np.uint64(SIGN)
_SENT = np.uint64(ALL)


def _fast_pass(x, w, r, min_count, fill):
    H, W = x.shape
    bits = x.view(np.uint64)
    keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits | _S)
    fin = np.isfinite(x)
    use = fin if w is None else fin & (w > 0) & (w < INF)
    kp = np.full((H + 2 * r, W + 2 * r), _SENT, dtype=np.uint64)
    kp[r:r + H, r:r + W] = np.where(use, keys, _SENT)
    wp = np.zeros((H + 2 * r, W + 2 * r))
    if w is not None:
        wp[r:r + H, r:r + W] = np.where(use, w, 0.0)
    D = 2 * r + 1
    K = np.stack([kp[dy:dy + H, dx:dx + W] for dy in range(D) for dx in range(D)])       # window order
    Wk = np.stack([wp[dy:dy + H, dx:dx + W] for dy in range(D) for dx in range(D)])
    n = (K != _SENT).sum(axis=0)
    srt = np.sort(K, axis=0)                                                             # sentinels last
    if w is None:
        sel = np.take_along_axis(srt, np.maximum((n - 1) // 2, 0)[None], axis=0)[0]
    else:
        T = np.zeros((H, W))
        for k in range(D * D):
            T = T + Wk[k]
        half = 0.5 * T
        lo, hi = np.zeros((H, W), dtype=np.int64), np.maximum(n - 1, 0)                   # the answer is in [lo, hi]
        while (lo < hi).any():
            mid = (lo + hi) // 2
            cand = np.take_along_axis(srt, mid[None], axis=0)[0]
            S = np.zeros((H, W))
            for k in range(D * D):
                S = S + np.where(K[k] <= cand, Wk[k], 0.0)
            ok = S >= half
            hi = np.where(ok, mid, hi)
            lo = np.where(ok, lo, np.minimum(mid + 1, hi))
        sel = np.take_along_axis(srt, lo[None], axis=0)[0]
    val = np.where(sel >> np.uint64(63) != 0, sel ^ _S, ~sel)
    take = (fin | fill) & (n >= min_count)
    return np.where(take, val, bits).view(np.float64)


def median_fast(x, weight, r, iters=1, min_count=1, fill=False):
    """median_restate, vectorised -> (out, uint8 changed)."""
    x, xs, ws = _maps(x, weight)
    outs = []
    for m, w in zip(xs, ws):
        cur = np.ascontiguousarray(m)
        for _ in range(iters):
            cur = np.ascontiguousarray(_fast_pass(cur, w, r, min_count, fill))
        outs.append(cur)
    out = np.ascontiguousarray(np.stack(outs).reshape(x.shape))
    return out, _changed(out, x)


POOL = np.array([0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, 1.5, -2.25, 3.0, 3.0000000000000004, 7.0, 1e-3,
                 NAN, -NAN, INF, -INF])


def pool_map(H, W, seed=0):
    rng = np.random.default_rng(4000 * H + 7 * W + seed)
    return np.ascontiguousarray(POOL[rng.integers(0, len(POOL), (H, W))])


def pool_weight(shape, seed=0):
    """Weights spanning 1e-300 .. 1e300, a quarter of them ones, some zero, negative, NaN and +inf."""
    rng = np.random.default_rng(91 + seed + 13 * int(np.prod(shape)))
    w = 10.0 ** rng.uniform(-300, 300, shape)
    u = rng.uniform(size=shape)
    w[u < 0.25] = 1.0
    for k, bad in enumerate([0.0, -0.0, -1.0, NAN, INF, -INF]):
        w[(u >= 0.25 + 0.03 * k) & (u < 0.28 + 0.03 * k)] = bad
    return w


def noise(H, W, seed=0, share=0.1):
    rng = np.random.default_rng(1000 * H + W + seed)
    x = rng.normal(0, 5, (H, W))
    x[rng.uniform(size=x.shape) < share] = np.nan
    return x


# ---------------------------------------------------------------------------------------------
# 1. the restatements and the properties of the definition
# ---------------------------------------------------------------------------------------------
def test_key_order():
    vals = [-INF, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, 1e300, INF]
    keys = [key_of(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert key_of(-0.0) + 1 == key_of(0.0)
    assert key_of(NAN) > key_of(INF)


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (5, 7), (12, 12), (11, 8)])
@pytest.mark.parametrize('r', [1, 2, 3])
def test_fast_equals_literal(shape, r):
    K = (2 * r + 1) ** 2
    for seed, x in enumerate([pool_map(*shape), noise(*shape, share=0.2), np.round(noise(*shape), 0)]):
        w1 = pool_weight(shape, seed)
        for w in (None, w1, np.ones(shape), np.abs(noise(*shape, seed=5, share=0)) + 0.1):
            for min_count, fill, iters in [(1, False, 1), (1, True, 2), (min(5, K), False, 1), (K, True, 1)]:
                a, ca = median_restate(x, w, r, iters, min_count, fill)
                b, cb = median_fast(x, w, r, iters, min_count, fill)
                assert raw_bits(a, b) and np.array_equal(ca, cb), (shape, r, seed, min_count, fill, iters)
    # a batch is its maps, with a shared and with a per-map weight
    xs = np.stack([pool_map(*shape, seed=s) for s in range(3)])
    wm = np.stack([pool_weight(shape, s) for s in range(3)])
    for w in (None, wm[0], wm):
        a, ca = median_restate(xs, w, r)
        b, cb = median_fast(xs, w, r)
        assert raw_bits(a, b) and np.array_equal(ca, cb)
        for k in range(3):
            assert raw_bits(a[k], median_restate(xs[k], w if w is None or w.ndim == 2 else w[k], r)[0])


@pytest.mark.parametrize('shape,r', [((7, 9), 1), ((10, 12), 2), ((12, 10), 3), ((24, 31), 7)])
def test_properties(shape, r):
    H, W = shape
    for seed in range(3):
        x = pool_map(H, W, seed)
        w = pool_weight(shape, seed)
        for fill in (False, True):
            un, _ = median_fast(x, None, r, fill=fill)
            # weights of 1.0 equal the unweighted form bit for bit
            assert raw_bits(median_fast(x, np.ones(shape), r, fill=fill)[0], un)
            for out, wt in ((un, None), (median_fast(x, w, r, fill=fill)[0], w)):
                hole_in, hole_out = ~np.isfinite(x), ~np.isfinite(out)
                if not fill:        # the holes are where they were, bit for bit
                    assert np.array_equal(hole_in, hole_out) and raw_bits(out[hole_in], x[hole_in])
                else:               # a hole that stays is the input's
                    assert not (hole_out & ~hole_in).any() and raw_bits(out[hole_out], x[hole_out])
                ob, xb = out.view(np.int64), x.view(np.int64)
                for i, j in zip(*np.nonzero(~hole_out)):     # every finite output's bits occur in its window
                    win = xb[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1]
                    assert (win == ob[i, j]).any(), (i, j)
    # two passes are the pass applied twice; an all-hole map comes out as it went in
    x, w = pool_map(H, W, 9), pool_weight(shape, 9)
    once = median_fast(x, w, r)[0]
    assert raw_bits(median_fast(x, w, r, iters=2)[0], median_fast(once, w, r)[0])
    allh = np.full(shape, NAN)
    allh[0, 0], allh[-1, -1], allh[H // 2, W // 2] = INF, -INF, -NAN
    for fill in (False, True):
        out, ch = median_fast(allh, None, r, fill=fill)
        assert raw_bits(out, allh) and not ch.any()


def test_small_cases():
    # the lower median of an even window; -0.0 sorts before +0.0
    x = np.array([[1.0, 2.0, 3.0, 4.0]])
    assert median_restate(x, None, 1)[0].tolist() == [[1.0, 2.0, 3.0, 3.0]]
    z = np.array([[0.0, -0.0]])
    out = median_restate(z, None, 1)[0]
    assert raw_bits(out, np.array([[-0.0, -0.0]]))
    # +-inf are holes: kept, never read; FILL gives them the median of their window
    x = np.array([[1.0, INF, 3.0, -INF, 5.0]])
    assert raw_bits(median_restate(x, None, 1)[0], np.array([[1.0, INF, 3.0, -INF, 5.0]]))
    out, ch = median_restate(x, None, 1, fill=True)
    assert out.tolist() == [[1.0, 1.0, 3.0, 3.0, 5.0]] and ch.tolist() == [[0, 1, 0, 1, 0]]
    # a heavy tap wins; a tap with an unusable weight is not read, but its own cell is filtered
    x = np.array([[1.0, 2.0, 9.0]])
    assert median_restate(x, np.array([[1.0, 1.0, 5.0]]), 1)[0].tolist() == [[1.0, 9.0, 9.0]]
    assert median_restate(x, np.array([[1.0, 1.0, NAN]]), 1)[0].tolist() == [[1.0, 1.0, 2.0]]
    assert median_restate(x, np.array([[0.0, -1.0, INF]]), 1)[0].tolist() == [[1.0, 2.0, 9.0]]    # n = 0 < min_count
    # min_count: the corner of a 3 x 3 map has 4 taps, the edge 6, the centre 9
    x = np.arange(9.0).reshape(3, 3)
    _, ch = median_restate(x, None, 1, min_count=5)
    # (the lower medians of the edges' six taps are 2, 3, 4 and 5: only the edge cell 3 is its own; corners are copied)
    assert ch.tolist() == [[0, 1, 0], [0, 0, 1], [0, 1, 0]]
    _, ch = median_restate(x, None, 1, min_count=9)
    assert not ch.any()


def clean_map(H=24, W=40, step=19):
    return np.where(np.arange(W)[None, :] >= step, 6.0, 2.0) * np.ones((H, 1))


def test_planted_impulses():
    """Isolated +-40 impulses on the two-plane step map: one radius-1 pass restores every interior cell."""
    clean = clean_map()
    x = clean.copy()
    ii, jj = np.mgrid[1:24:3, 2:40:3]
    x[ii, jj] = np.where((ii + jj) % 2 == 0, 40.0, -40.0)
    assert (x != clean).sum() == 8 * 13
    for fn in (median_restate, median_fast):
        out, ch = fn(x, None, 1)
        assert raw_bits(out[1:-1, 1:-1], clean[1:-1, 1:-1])
        assert raw_bits(fn(x, np.ones_like(x), 1)[0], out)


def test_planted_blobs():
    """2 x 3 blobs of wrong values with weight 0.05: the unweighted radius-1 median leaves 8 wrong cells,
    the weighted one none."""
    clean = clean_map()
    x, w = clean.copy(), np.ones_like(clean)
    for i, j in [(5, 8), (12, 18), (17, 30)]:
        x[i:i + 2, j:j + 3] = 30.0
        w[i:i + 2, j:j + 3] = 0.05
    for fn in (median_restate, median_fast):
        assert (fn(x, None, 1)[0] != clean).sum() == 8
        assert (fn(x, w, 1)[0] != clean).sum() == 0


# ---------------------------------------------------------------------------------------------
# 2. validation of the C entries and of the keywords
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_header_declares_median(lib):
    syms = L.header_symbols()
    assert 'dm_median_filter' in syms and 'dm_median_bytes' in syms
    assert 'dm_median_filter' in L.SIGNATURES and 'dm_median_bytes' in L.SIGNATURES
    assert lib.dm_abi_version() == 110
    assert L.DM_MEDIAN_FILL == 1


def _args(d_in=P8, weight=None, wmaps=1, M=1, H=4, W=4, r=3, min_count=1, iters=1, flags=0, out=P8, changed=None,
          work=P8):
    return (d_in, weight, wmaps, M, H, W, r, min_count, iters, flags, out, changed, work, None)


@pytest.mark.parametrize('kw,code,needle', [
    (dict(d_in=None), L.DM_ERR_ARG, 'null'),
    (dict(out=None), L.DM_ERR_ARG, 'null'),
    (dict(work=None), L.DM_ERR_ARG, 'null'),
    (dict(M=0), L.DM_ERR_ARG, 'shape'),
    (dict(H=0), L.DM_ERR_ARG, 'shape'),
    (dict(W=-1), L.DM_ERR_ARG, 'shape'),
    (dict(M=-2), L.DM_ERR_ARG, 'shape'),
    (dict(r=0), L.DM_ERR_ARG, 'radius'),
    (dict(r=8), L.DM_ERR_ARG, 'radius'),
    (dict(r=-3), L.DM_ERR_ARG, 'radius'),
    (dict(iters=0), L.DM_ERR_ARG, 'iters'),
    (dict(iters=65), L.DM_ERR_ARG, 'iters'),
    (dict(min_count=0), L.DM_ERR_ARG, 'min_count'),
    (dict(min_count=-1), L.DM_ERR_ARG, 'min_count'),
    (dict(r=1, min_count=10), L.DM_ERR_ARG, 'min_count'),
    (dict(r=7, min_count=226), L.DM_ERR_ARG, 'min_count'),
    (dict(flags=2), L.DM_ERR_ARG, 'flags'),
    (dict(flags=-1), L.DM_ERR_ARG, 'flags'),
    (dict(weight=P8, wmaps=2, M=3), L.DM_ERR_ARG, 'weight_maps'),
    (dict(weight=P8, wmaps=0), L.DM_ERR_ARG, 'weight_maps'),
    (dict(H=65536, W=32768), L.DM_ERR_UNSUPPORTED, 'cells'),                       # H W = 2^31
    (dict(M=65536), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=64 * 65535 + 1, W=1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=1, W=64 * 65535 + 1, weight=P8, flags=1, r=7, min_count=225, iters=64, changed=P8),
     L.DM_ERR_UNSUPPORTED, 'cells'),                                             # every argument valid but the shape
    (dict(M=65536, wmaps=7), L.DM_ERR_UNSUPPORTED, 'cells'),                       # weight_maps is not read without weights
])
def test_median_filter_validation(lib, kw, code, needle):
    assert lib.dm_median_filter(*_args(**kw)) == code
    assert needle in L.last_error()


def test_median_bytes(lib):
    refused = [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 65536, 32768), (65536, 4, 4),
               (1, 64 * 65535 + 1, 1), (1, 1, 64 * 65535 + 1)]
    for bad in refused:
        assert lib.dm_median_bytes(*bad) == 0, bad
        assert lib.dm_fill_bytes(*bad) == 0, bad                                   # the same limits
    for H, W in [(1, 1), (1, 9), (5, 7), (64, 64), (65, 130), (1024, 1024), (46341, 46340), (64 * 65535, 1),
                 (1, 64 * 65535)]:
        prev = 0
        for M in (1, 2, 3, 7, 65535):
            b = lib.dm_median_bytes(M, H, W)
            assert b >= 8 * M * H * W and b % 16 == 0 and b >= prev and lib.dm_fill_bytes(M, H, W) > 0, (M, H, W)
            prev = b


def test_median_params():
    assert engine.median_params(1) == (1, 1)
    assert engine.median_params((2,)) == (2, 1)
    assert engine.median_params([3, 4]) == (3, 4)
    assert engine.median_params((np.int64(7), np.int32(64))) == (7, 64)
    got = engine.median_params((np.int64(2), np.int64(2)))
    assert type(got[0]) is int and type(got[1]) is int
    for bad in [None, 0, 8, -1, 1.0, True, '3', (), (1, 2, 3), (0,), (8, 1), (1, 0), (1, 65), (1.5, 1), (1, 1.0),
                (True, 1), (1, True), ('1', 1), (1, None), ((1,), 1)]:
        with pytest.raises(ValueError):
            engine.median_params(bad)


def test_median_weight_keyword():
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = _case()
    s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 16], median=(2, 3), median_weight='correlation')
    assert s.median == (2, 3) and s.median_weight == 'correlation'
    s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 16])
    assert s.median is None and s.median_weight is None
    assert ImageCutSolver(a, b, median=1).median == (1, 1)
    for bad in ('score', 'image', 1, True, 'Correlation', ''):
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, median=1, median_weight=bad)
        with pytest.raises(ValueError):
            _sharded(a, b, stitcher=_host_stitch, median=1, median_weight=bad, medianer=_host_median)
    for bad in (0, 8, (1, 0), 1.0, (1, 2, 3), True):
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, median=bad)
        with pytest.raises(ValueError):
            _sharded(a, b, stitcher=_host_stitch, median=bad, medianer=_host_median)


# ---------------------------------------------------------------------------------------------
# 3. the sharded path: oracle tile solver, host stitcher, the restatement as the medianer
# ---------------------------------------------------------------------------------------------
MEDIAN = (1, 2)
SPECKLE = (3, 0.25)


def _host_median(maps, weight, radius, iters):
    """medianer hook of solve_image_sharded: the filtered maps."""
    return median_fast(np.asarray(maps), None if weight is None else np.asarray(weight), radius, iters)[0]


def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map, err) of the consistency-checked solve: today's call."""
    a, b = _case()
    return [np.asarray(x) for x in _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)]


@pytest.fixture(scope='module')
def chain(plain):
    """The chain after the stitch in the restatements: median (by correlation) -> speckle -> fill."""
    med = median_restate(plain[0], plain[1], *MEDIAN)[0]
    spk = speckle_restate(med, *SPECKLE)
    fil = fill_restate(spk[0], 16)
    return med, spk, fil


def _check_chain(got, plain, chain):
    med, spk, fil = chain
    assert len(got) == 5
    assert same_bits(got[0], fil[0]) and np.isfinite(np.asarray(got[0])).all()
    assert same_bits(got[1], plain[1]) and same_bits(got[2], plain[2])      # never touched
    assert np.array_equal(np.asarray(got[3]), spk[1]) and np.array_equal(np.asarray(got[4]), fil[1])


def _check_median_only(got, plain, weighted):
    assert len(got) == 3
    want = median_restate(plain[0], plain[1] if weighted else None, *MEDIAN)[0]
    assert raw_bits(np.asarray(got[0]), want)
    assert np.array_equal(np.isnan(np.asarray(got[0])), np.isnan(plain[0]))  # holes stay holes
    assert not same_bits(got[0], plain[0])
    assert same_bits(got[1], plain[1]) and same_bits(got[2], plain[2])


def test_sharded_median_single_process(plain, chain):
    a, b = _case()
    kw = dict(stitcher=_host_stitch_fb, consistency=1.0, median=MEDIAN, medianer=_host_median)
    _check_median_only(_sharded(a, b, **kw), plain, False)
    _check_median_only(_sharded(a, b, median_weight='correlation', **kw), plain, True)
    _check_chain(_sharded(a, b, median_weight='correlation', speckle=SPECKLE, speckler=_host_speckle, fill=16,
                          filler=_host_fill, **kw), plain, chain)
    assert np.isnan(plain[0]).any()
    # the order of the stages shows: the median after the speckle filter and the fill gives another map
    med, spk, fil = chain
    late = median_restate(fill_restate(speckle_restate(plain[0], *SPECKLE)[0], 16)[0], plain[1], *MEDIAN)[0]
    assert not same_bits(late, fil[0])


def test_sharded_median_without_consistency():
    a, b = _case()
    ref = _sharded(a, b, stitcher=_host_stitch)
    assert len(ref) == 2
    for mw in (None, 'correlation'):
        got = _sharded(a, b, stitcher=_host_stitch, median=MEDIAN[0], median_weight=mw, medianer=_host_median)
        assert len(got) == 2
        want = median_restate(np.asarray(ref[0]), None if mw is None else np.asarray(ref[1]), MEDIAN[0])[0]
        assert raw_bits(np.asarray(got[0]), want) and same_bits(got[1], ref[1])


def test_sharded_median_none_is_unchanged(plain):
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, median=None, median_weight='correlation',
                   medianer=_host_median)
    assert len(got) == 3
    for g, r in zip(got, plain):
        assert same_bits(g, r)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        kw = dict(stitcher=_host_stitch_fb, consistency=1.0, medianer=_host_median)
        only = _sharded(a, b, median=MEDIAN, **kw)
        corr = _sharded(a, b, median=MEDIAN, median_weight='correlation', **kw)
        all_ = _sharded(a, b, median=MEDIAN, median_weight='correlation', speckle=SPECKLE, speckler=_host_speckle,
                        fill=16, filler=_host_fill, **kw)
        root = _sharded(a, b, median=MEDIAN, result='root', **kw)
        none = _sharded(a, b, median=None, **kw)
        q.put((rank, [np.asarray(x) for x in only], [np.asarray(x) for x in corr], [np.asarray(x) for x in all_],
               [None if x is None else np.asarray(x) for x in root], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_median_gloo_world_2(plain, chain):
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
    for rank, only, corr, all_, root, none in res:
        _check_median_only(only, plain, False)
        _check_median_only(corr, plain, True)
        _check_chain(all_, plain, chain)
        if rank == 0:
            _check_median_only(root, plain, False)
        else:
            assert root == [None, None, None]
        assert len(none) == 3
        for g, r in zip(none, plain):
            assert same_bits(g, r), rank
