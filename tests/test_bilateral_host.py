"""Joint bilateral filter, host side (no GPU): the plain-loop restatement of the definition
(bilateral_restate: what dm_bilateral_filter must equal bit for bit) against an independent
vectorised numpy version, the planted two-plane case the guided form exists for, special values,
argument validation of the two C entries (it returns before any HIP call) and of the keyword,
and the sharded path with the oracle as tile solver, a host stitcher and the restatement
injected as the smoother -- single process and gloo world size 2.

Comparisons with the restatement are bitwise (int64 views, NaN positions equal)."""
import ctypes
import os

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
    assert hasattr(lib, 'dm_bilateral_filter') and hasattr(lib, 'dm_bilateral_bytes')
    assert callable(getattr(engine, 'bilateral_filter', None)) and callable(getattr(engine, 'smooth_params', None))


# ---------------------------------------------------------------------------------------------
# the definition in plain loops; Python floats are IEEE doubles, one rounding per operation
# ---------------------------------------------------------------------------------------------
_EXP = {}


def _exp(a):
    """The pinned dm_exp (the oracle's dmo_exp), memoised by argument."""
    from oracle import oracle as O
    if a != a:
        return O.exp(a)
    v = _EXP.get(a)
    if v is None:
        if len(_EXP) >= 1 << 20:      # (a float64 guide of noise repeats no argument)
            _EXP.clear()
        v = _EXP[a] = O.exp(a)
    return v


def den(sigma):
    """2.0 * sigma**2 as the caller's Python evaluates it."""
    return engine.bilateral_den(sigma)


def _pass(x, g, r, den_color, den_space, fill):
    H, W = x.shape
    X, G = x.tolist(), g.tolist()
    xfin, gfin = np.isfinite(x), np.isfinite(g)
    ok = (xfin & gfin).tolist()
    xfin, gfin = xfin.tolist(), gfin.tolist()
    ws = [[_exp(-float(dy * dy + dx * dx) / den_space) for dx in range(-r, r + 1)] for dy in range(-r, r + 1)]
    out = x.copy()
    for i in range(H):
        for j in range(W):
            if not gfin[i][j] or not (xfin[i][j] or fill):
                continue
            g0 = G[i][j]
            num = 0.0
            den_ = 0.0
            for dy in range(max(-r, -i), min(r, H - 1 - i) + 1):
                okr, Gr, Xr, wr = ok[i + dy], G[i + dy], X[i + dy], ws[dy + r]
                for dx in range(max(-r, -j), min(r, W - 1 - j) + 1):
                    t = j + dx
                    if not okr[t]:
                        continue
                    c = g0 - Gr[t]
                    wc = _exp(-(c * c) / den_color)
                    w = wr[dx + r] * wc
                    if not w > 0:
                        continue
                    num = num + w * Xr[t]
                    den_ = den_ + w
            if den_ > 0:
                out[i, j] = num / den_
    return out


def _one(x, guide, r, den_color, den_space, iters, fill):
    cur = x
    for _ in range(iters):
        cur = _pass(cur, cur if guide is None else guide, r, den_color, den_space, fill)
    return cur


def bilateral_restate(x, guide, radius, den_color, den_space, iters=1, fill=False):
    """The definition on [H][W] or [M][H][W] float64 maps; guide None, [H][W] or of x's shape,
    float64 or uint8 -> (out, uint8 filled)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = None if guide is None else np.ascontiguousarray(guide).astype(np.float64)
    assert not (fill and g is None)
    den_color, den_space = float(den_color), float(den_space)
    if x.ndim == 2:
        out = _one(x, g, radius, den_color, den_space, iters, fill)
    else:
        out = np.stack([_one(m, g if g is None or g.ndim == 2 else g[k], radius, den_color, den_space, iters, fill)
                        for k, m in enumerate(x)])
    filled = (~np.isfinite(x) & np.isfinite(out)).astype(np.uint8)
    return out, filled


def bilateral_numpy(x, guide, r, den_color, den_space, fill=False):
    """One pass, independently: shifted slices of NaN-padded planes, np.exp, masked sums."""
    H, W = x.shape
    g = x if guide is None else np.asarray(guide, dtype=np.float64)
    xp = np.pad(x, r, constant_values=np.nan)
    gp = np.pad(g, r, constant_values=np.nan)
    num, den_ = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(all='ignore'):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xt = xp[r + dy:r + dy + H, r + dx:r + dx + W]
                gt = gp[r + dy:r + dy + H, r + dx:r + dx + W]
                w = np.exp(-(dy * dy + dx * dx) / den_space) * np.exp(-((g - gt) ** 2) / den_color)
                m = np.isfinite(xt) & np.isfinite(gt) & (w > 0)
                num += np.where(m, w * np.where(m, xt, 0.0), 0.0)
                den_ += np.where(m, w, 0.0)
        take = np.isfinite(g) & (np.isfinite(x) | fill) & (den_ > 0)
        return np.where(take, num / np.where(den_ > 0, den_, 1.0), x)


def noise(H, W, seed=0, share=0.1):
    rng = np.random.default_rng(1000 * H + W + seed)
    x = rng.normal(0, 5, (H, W))
    x[rng.uniform(size=x.shape) < share] = np.nan
    return x


def image(H, W, seed=0):
    """A uint8 guide: two flat regions with a slanted edge, plus noise."""
    rng = np.random.default_rng(77 * H + W + seed)
    i, j = np.mgrid[0:H, 0:W]
    g = np.where(2 * j + i > W, 170.0, 70.0) + rng.normal(0, 6, (H, W))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,r,sc,ss', [((5, 7), 7, 2.0, 5.0), ((33, 31), 3, 10.0, 3.0), ((20, 37), 1, 0.5, 1.0),
                                            ((9, 1), 2, 4.0, 2.0)])
def test_restatement_against_numpy(shape, r, sc, ss):
    x = noise(*shape)
    rng = np.random.default_rng(3)
    fg = rng.normal(0, 3, shape)
    fg[rng.uniform(size=shape) < 0.05] = np.nan
    for guide, fill in [(None, False), (fg, False), (image(*shape), False), (image(*shape), True), (fg, True)]:
        got, filled = bilateral_restate(x, guide, r, den(sc), den(ss), fill=fill)
        want = bilateral_numpy(x, guide, r, den(sc), den(ss), fill=fill)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max() <= 1e-12
        assert np.array_equal(filled.astype(bool), np.isnan(x) & np.isfinite(got))
        if not fill:
            assert not filled.any() and raw_bits(got[np.isnan(x)], x[np.isnan(x)])
    # two passes are the pass applied twice; a self-guided pass is guided by its own input
    once = bilateral_restate(x, None, r, den(sc), den(ss))[0]
    assert raw_bits(bilateral_restate(x, None, r, den(sc), den(ss), iters=2)[0],
                    bilateral_restate(once, None, r, den(sc), den(ss))[0])
    assert raw_bits(once, bilateral_restate(x, x, r, den(sc), den(ss))[0])


def planted(H=48, W=64, seed=4864, step=29):
    """Two planes 4 px apart, the step at column `step` -> (truth, noisy map with 8 % NaN, uint8
    guide with 60 / 180 either side of the step, the band within 3 columns of the step)."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W]
    truth = 0.02 * i + 0.01 * j + np.where(j >= step, 4.0, 0.0)
    x = truth + rng.normal(0, 0.3, (H, W))
    x[rng.uniform(size=(H, W)) < 0.08] = np.nan
    g = np.where(j >= step, 180.0, 60.0) + rng.normal(0, 2, (H, W))
    band = (j >= step - 3) & (j < step + 3)
    return truth, x, np.clip(np.rint(g), 0, 255).astype(np.uint8), band


def rms(a, b, m):
    return float(np.sqrt(np.mean((a[m] - b[m]) ** 2)))


def test_planted_step():
    """Measured with this seed: 0.303 -> 0.046 over the finite cells; in the band 0.054 guided against
    1.124 with the same Gaussian and no guide (the figures are printed)."""
    truth, x, g, band = planted()
    fin = np.isfinite(x)
    out, filled = bilateral_restate(x, g, 3, den(10.0), den(3.0))
    flat, _ = bilateral_restate(x, np.zeros_like(g), 3, den(10.0), den(3.0))
    before, after = rms(x, truth, fin), rms(out, truth, fin)
    edge, edge_flat = rms(out, truth, fin & band), rms(flat, truth, fin & band)
    print('rms %.3f -> %.3f; band: guided %.3f, unguided %.3f' % (before, after, edge, edge_flat))
    assert after <= before / 3
    assert edge <= edge_flat / 3
    assert np.array_equal(np.isnan(out), np.isnan(x)) and raw_bits(out[~fin], x[~fin]) and not filled.any()
    out, filled = bilateral_restate(x, g, 3, den(10.0), den(3.0), fill=True)
    assert np.isfinite(out).all() and np.array_equal(filled.astype(bool), ~fin)
    assert rms(out, truth, ~fin) <= before / 3


def test_special_values():
    inf = float('inf')
    # +-inf in the map are holes: not smoothed, not read
    x = np.array([[1.0, np.inf, 3.0, -np.inf, 5.0]])
    out, _ = bilateral_restate(x, None, 1, inf, inf)
    assert raw_bits(out, x)
    out, filled = bilateral_restate(x, np.zeros((1, 5)), 1, inf, inf, fill=True)
    assert out.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]] and filled.tolist() == [[0, 1, 0, 1, 0]]
    # a non-finite guide cell is copied and skipped as a tap
    g = np.array([[0.0, np.nan, 0.0, np.inf, 0.0]])
    out, _ = bilateral_restate(np.array([[1.0, 2.0, 3.0, 4.0, 5.0]]), g, 1, inf, inf)
    assert out.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]]
    out, _ = bilateral_restate(np.array([[1.0, 2.0, 3.0, 4.0, 6.0]]), g, 2, inf, inf)
    assert out.tolist() == [[2.0, 2.0, 10.0 / 3, 4.0, 4.5]]
    # a sigma_color so small that every off-centre wc underflows: the input's bits
    x = noise(9, 11, share=0.2)
    assert raw_bits(bilateral_restate(x, None, 2, den(1e-9), den(2.0))[0], x)
    # an all-hole map, and a map with one finite cell
    allh = np.full((6, 5), np.nan)
    allh[1, 1], allh[2, 3], allh[5, 4] = np.inf, -np.inf, -np.nan
    assert raw_bits(bilateral_restate(allh, None, 3, 8.0, 8.0)[0], allh)
    out, filled = bilateral_restate(allh, np.zeros((6, 5), np.uint8), 3, 8.0, 8.0, fill=True)
    assert raw_bits(out, allh) and not filled.any()
    allh[2, 2] = 7.5
    out, filled = bilateral_restate(allh, np.zeros((6, 5), np.uint8), 1, 8.0, 8.0, fill=True)
    assert (out[1:4, 1:4] == 7.5).all() and filled.sum() == 8 and raw_bits(out[0], allh[0])
    # a hole block wider than the window keeps its core for one pass and loses it at the next
    x = np.ones((9, 9))
    x[2:7, 2:7] = np.nan
    z = np.zeros((9, 9), np.uint8)
    assert bilateral_restate(x, z, 1, 8.0, 8.0, fill=True)[1].sum() == 16
    assert bilateral_restate(x, z, 1, 8.0, 8.0, iters=2, fill=True)[1].sum() == 24
    assert bilateral_restate(x, z, 1, 8.0, 8.0, iters=3, fill=True)[1].sum() == 25
    # overflow of w * X: the cell is not finite any more, as the header says
    big = np.full((1, 3), 1.7e308)
    assert np.isinf(bilateral_restate(big, None, 1, inf, inf)[0]).all()


# ---------------------------------------------------------------------------------------------
# 2. validation of the C entries and of the keyword
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences
NAN, INF = float('nan'), float('inf')


def test_header_declares_bilateral(lib):
    syms = L.header_symbols()
    assert 'dm_bilateral_filter' in syms and 'dm_bilateral_bytes' in syms
    assert 'dm_bilateral_filter' in L.SIGNATURES and 'dm_bilateral_bytes' in L.SIGNATURES
    assert lib.dm_abi_version() == 110
    assert (L.DM_BILAT_FILL, L.DM_BILAT_GUIDE_U8) == (1, 2)


def _args(d_in=P8, guide=None, gmaps=1, M=1, H=4, W=4, r=3, dc=2.0, ds=2.0, iters=1, flags=0, out=P8, filled=None,
          work=P8):
    return (d_in, guide, gmaps, M, H, W, r, dc, ds, iters, flags, out, filled, work, None)


@pytest.mark.parametrize('kw,code,needle', [
    (dict(d_in=None), L.DM_ERR_ARG, 'null'),
    (dict(out=None), L.DM_ERR_ARG, 'null'),
    (dict(work=None), L.DM_ERR_ARG, 'null'),
    (dict(M=0), L.DM_ERR_ARG, 'shape'),
    (dict(H=0), L.DM_ERR_ARG, 'shape'),
    (dict(W=-1), L.DM_ERR_ARG, 'shape'),
    (dict(M=-2), L.DM_ERR_ARG, 'shape'),
    (dict(r=0), L.DM_ERR_ARG, 'radius'),
    (dict(r=16), L.DM_ERR_ARG, 'radius'),
    (dict(r=-3), L.DM_ERR_ARG, 'radius'),
    (dict(iters=0), L.DM_ERR_ARG, 'iters'),
    (dict(iters=65), L.DM_ERR_ARG, 'iters'),
    (dict(dc=0.0), L.DM_ERR_ARG, 'den_color'),
    (dict(dc=-1.0), L.DM_ERR_ARG, 'den_color'),
    (dict(dc=NAN), L.DM_ERR_ARG, 'den_color'),
    (dict(ds=0.0), L.DM_ERR_ARG, 'den_space'),
    (dict(ds=-INF), L.DM_ERR_ARG, 'den_space'),
    (dict(ds=NAN), L.DM_ERR_ARG, 'den_space'),
    (dict(flags=4), L.DM_ERR_ARG, 'flags'),
    (dict(flags=-1, guide=P8), L.DM_ERR_ARG, 'flags'),
    (dict(guide=P8, gmaps=2, M=3), L.DM_ERR_ARG, 'guide_maps'),
    (dict(guide=P8, gmaps=0), L.DM_ERR_ARG, 'guide_maps'),
    (dict(flags=1), L.DM_ERR_ARG, 'need a guide'),
    (dict(flags=2), L.DM_ERR_ARG, 'need a guide'),
    (dict(flags=3), L.DM_ERR_ARG, 'need a guide'),
    (dict(H=65536, W=32768), L.DM_ERR_UNSUPPORTED, 'cells'),                       # H W = 2^31
    (dict(M=65536), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=64 * 65535 + 1, W=1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=1, W=64 * 65535 + 1, guide=P8, flags=3, dc=INF, ds=INF, r=15, iters=64, filled=P8),
     L.DM_ERR_UNSUPPORTED, 'cells'),                                             # every argument valid but the shape
])
def test_bilateral_filter_validation(lib, kw, code, needle):
    assert lib.dm_bilateral_filter(*_args(**kw)) == code
    assert needle in L.last_error()


def test_bilateral_bytes(lib):
    refused = [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 65536, 32768), (65536, 4, 4),
               (1, 64 * 65535 + 1, 1), (1, 1, 64 * 65535 + 1)]
    for bad in refused:
        assert lib.dm_bilateral_bytes(*bad) == 0, bad
        assert lib.dm_fill_bytes(*bad) == 0, bad                                   # the same limits
    for H, W in [(1, 1), (1, 9), (5, 7), (64, 64), (65, 130), (1024, 1024), (46341, 46340), (64 * 65535, 1),
                 (1, 64 * 65535)]:
        prev = 0
        for M in (1, 2, 3, 7, 65535):
            b = lib.dm_bilateral_bytes(M, H, W)
            assert b >= 8 * M * H * W and b % 16 == 0 and b >= prev and lib.dm_fill_bytes(M, H, W) > 0, (M, H, W)
            prev = b


def test_smooth_params():
    assert engine.smooth_params((3, 10.0, 3.0)) == (3, 10.0, 3.0)
    assert engine.smooth_params([1, 1, 1]) == (1, 1.0, 1.0)
    assert engine.smooth_params((np.int64(15), np.float32(0.5), INF)) == (15, 0.5, INF)
    got = engine.smooth_params((7, 2, 5))
    assert type(got[0]) is int and type(got[1]) is float and type(got[2]) is float
    for bad in [None, 3, (3,), (3, 1.0), (3, 1.0, 1.0, 1.0), (0, 1.0, 1.0), (16, 1.0, 1.0), (-1, 1.0, 1.0),
                (1.5, 1.0, 1.0), (True, 1.0, 1.0), ('3', 1.0, 1.0), (3, 0.0, 1.0), (3, 1.0, 0), (3, -1.0, 1.0),
                (3, NAN, 1.0), (3, 1.0, NAN), (3, '1', 1.0), (3, None, 1.0), (3, 1.0, True), (3, -INF, 1.0), '313']:
        with pytest.raises(ValueError):
            engine.smooth_params(bad)
    assert engine.bilateral_den(3.0) == 18.0 and engine.bilateral_den(INF) == INF and engine.bilateral_den(1e200) == INF


# ---------------------------------------------------------------------------------------------
# 3. the sharded path: oracle tile solver, host stitcher, the restatement as the smoother
# ---------------------------------------------------------------------------------------------
SMOOTH = (3, 10.0, 3.0)
SPECKLE = (3, 0.25)


def _host_smooth(maps, guide, radius, sigma_color, sigma_space):
    """smoother hook of solve_image_sharded: the smoothed maps."""
    return bilateral_restate(np.asarray(maps), guide, radius, den(sigma_color), den(sigma_space))[0]


def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


def _guide(a, d_map):
    e = (GEOM['ws'] - 1) // 2
    H, W = np.shape(d_map)[-2:]
    return np.asarray(a)[e:e + H, e:e + W]


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map, err) of the consistency-checked solve: today's call."""
    a, b = _case()
    return [np.asarray(x) for x in _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)]


@pytest.fixture(scope='module')
def chain(plain):
    """The chain after the stitch in the restatements: speckle -> fill -> smooth (image guide)."""
    a, _ = _case()
    spk = speckle_restate(plain[0], *SPECKLE)
    fil = fill_restate(spk[0], 16)
    smo = bilateral_restate(fil[0], _guide(a, plain[0]), SMOOTH[0], den(SMOOTH[1]), den(SMOOTH[2]))[0]
    return spk, fil, smo


def _check_chain(got, plain, chain):
    spk, fil, smo = chain
    assert len(got) == 5
    assert same_bits(got[0], smo) and np.isfinite(np.asarray(got[0])).all()
    assert same_bits(got[1], plain[1]) and same_bits(got[2], plain[2])      # never touched
    assert np.array_equal(np.asarray(got[3]), spk[1]) and np.array_equal(np.asarray(got[4]), fil[1])


def _check_smooth_only(got, plain, a, guided=True):
    assert len(got) == 3
    want = bilateral_restate(plain[0], _guide(a, plain[0]) if guided else None, SMOOTH[0], den(SMOOTH[1]),
                             den(SMOOTH[2]))[0]
    assert same_bits(got[0], want)
    assert np.array_equal(np.isnan(np.asarray(got[0])), np.isnan(plain[0]))  # holes stay holes
    assert not same_bits(got[0], plain[0])
    assert same_bits(got[1], plain[1]) and same_bits(got[2], plain[2])


def test_sharded_smooth_single_process(plain, chain):
    a, b = _case()
    kw = dict(stitcher=_host_stitch_fb, consistency=1.0, smooth=SMOOTH, smoother=_host_smooth)
    _check_smooth_only(_sharded(a, b, **kw), plain, a)
    _check_smooth_only(_sharded(a, b, smooth_guide='self', **kw), plain, a, guided=False)
    _check_chain(_sharded(a, b, speckle=SPECKLE, speckler=_host_speckle, fill=16, filler=_host_fill, **kw),
                 plain, chain)
    assert np.isnan(plain[0]).any()


def test_sharded_smooth_without_consistency():
    a, b = _case()
    ref = _sharded(a, b, stitcher=_host_stitch)
    got = _sharded(a, b, stitcher=_host_stitch, smooth=SMOOTH, smoother=_host_smooth)
    assert len(ref) == 2 and len(got) == 2
    g = _guide(a, ref[0])
    assert g.dtype == np.uint8 and g.shape == np.shape(ref[0])[-2:]
    want = bilateral_restate(np.asarray(ref[0]), g, SMOOTH[0], den(SMOOTH[1]), den(SMOOTH[2]))[0]
    assert same_bits(got[0], want) and same_bits(got[1], ref[1])


def test_sharded_smooth_none_is_unchanged(plain):
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, smooth=None, smoother=_host_smooth)
    assert len(got) == 3
    for g, r in zip(got, plain):
        assert same_bits(g, r)


def test_sharded_smooth_bad_keyword():
    a, b = _case()
    for bad in ((0, 1.0, 1.0), (3, -1.0, 1.0), 3, (True, 1.0, 1.0), (3, 1.0, NAN), (3, 1.0)):
        with pytest.raises(ValueError):
            _sharded(a, b, stitcher=_host_stitch, smooth=bad, smoother=_host_smooth)
    with pytest.raises(ValueError):
        _sharded(a, b, stitcher=_host_stitch, smooth=SMOOTH, smooth_guide='img2', smoother=_host_smooth)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        kw = dict(stitcher=_host_stitch_fb, consistency=1.0, smoother=_host_smooth)
        only = _sharded(a, b, smooth=SMOOTH, **kw)
        all_ = _sharded(a, b, smooth=SMOOTH, speckle=SPECKLE, speckler=_host_speckle, fill=16, filler=_host_fill, **kw)
        root = _sharded(a, b, smooth=SMOOTH, result='root', **kw)
        none = _sharded(a, b, smooth=None, **kw)
        q.put((rank, [np.asarray(x) for x in only], [np.asarray(x) for x in all_],
               [None if x is None else np.asarray(x) for x in root], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_smooth_gloo_world_2(plain, chain):
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
    a, _ = _case()
    for rank, only, all_, root, none in res:
        _check_smooth_only(only, plain, a)
        _check_chain(all_, plain, chain)
        if rank == 0:
            _check_smooth_only(root, plain, a)
        else:
            assert root == [None, None, None]
        assert len(none) == 3
        for g, r in zip(none, plain):
            assert same_bits(g, r), rank
