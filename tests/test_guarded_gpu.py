"""Every entry point under guards (helpers: tests/test_guarded_host.py).

Each case calls the public API on small inputs three times: once with ordinary allocations (the
reference run: these results are pinned to the oracle or the restatements by the other GPU files,
which this one does not repeat), then with poison 0xFF and with poison 0x00.  In the guarded runs
every allocation of the package comes from the guarded allocator -- exact sizes, 16-byte aligned
and no more, contents the poison -- and every input and ``out=`` tensor the case passes is a
guarded buffer at its natural alignment (images at odd addresses whose last byte is the last byte
a tile may read).  After a synchronize every guard must still hold the poison, every input the API
does not document as written must hold the bytes put in, every returned tensor must equal the
reference run's byte for byte (NaN payloads and -0.0 count, optional outputs too), and the
library must have been entered through every entry the case declares.  Nothing is measured and
there is no tolerance.

Two poisons, so that one that happens to equal a sentinel (the -1 hole label of the speckle
filter, an all-zero counter) cannot hide a dependence.  The ledger test of the host file holds
the declared entries against the header."""
import ctypes

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import holed_plane
from test_guarded_host import POISONS, _site, install, record
from test_photo_host import planes as disparity_planes

pytestmark = pytest.mark.gpu

NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']
F64, U8, I32, I8 = torch.float64, torch.uint8, torch.int32, torch.int8


# ---------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------
class Ctx:
    """What a case allocates through: guarded buffers in a guarded run (``g`` the allocator),
    ordinary tensors in the reference run (``g`` None)."""

    def __init__(self, g):
        self.g = g
        self.results = []

    def inp(self, array, dtype=None, misalign=None, label=None):
        """An input of the call."""
        if self.g is not None:
            return self.g.guarded(array, dtype, misalign, device='cuda', label=label or _site(2))
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        return (t.to(dtype) if dtype is not None else t).cuda().clone()

    def inout(self, array, dtype=None, misalign=None, label=None):
        """A buffer the API documents as written (an in-place map)."""
        t = self.inp(array, dtype, misalign, label=label or _site(2))
        if self.g is not None:
            self.g.written(t)
        return t

    def out(self, shape, dtype=F64, misalign=None, label=None):
        """An ``out=`` tensor: pre-filled with the poison in a guarded run."""
        if self.g is not None:
            return self.g.out(shape, dtype, device='cuda', misalign=misalign, label=label or _site(2))
        return torch.empty(tuple(shape), dtype=dtype, device='cuda')

    def work(self, nbytes):
        """A workspace for a direct call of the C ABI: exact size, 16-byte aligned and no more."""
        if self.g is not None:
            return self.g.alloc((int(nbytes),), U8, 'cuda', label=_site(2))
        return torch.empty(int(nbytes), dtype=U8, device='cuda')

    def add(self, tag, value):
        """One or more results (a tensor, an array, None, or a tuple / list of them)."""
        if isinstance(value, (tuple, list)):
            for k, v in enumerate(value):
                self.add('%s[%d]' % (tag, k), v)
        else:
            self.results.append((tag, value))


class Case:
    def __init__(self, name, entries, fn, env):
        self.name, self.entries, self.fn, self.env = name, tuple(entries), fn, dict(env or {})


CASES = []


def case(name, entries, env=None):
    def deco(fn):
        CASES.append(Case(name, entries, fn, env))
        return fn
    return deco


def _bytes(v):
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.detach().contiguous().reshape(-1).view(U8)


def _compare(tag, got, want, what):
    if want is None or got is None:
        assert got is None and want is None, (tag, what)
        return
    if not isinstance(want, (torch.Tensor, np.ndarray)):
        assert got == want, (tag, what)
        return
    assert type(got) is type(want) and got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (tag, what)
    a, b = _bytes(got), _bytes(want)
    if not torch.equal(a, b):
        at = int((a != b).nonzero()[0, 0])
        raise AssertionError('%s: %s differs from the reference run, first at byte %d of %d' % (what, tag, at, a.numel()))


def _run(c, g):
    x = Ctx(g)
    c.fn(x)
    torch.cuda.synchronize()
    return x.results


def run_case(c, monkeypatch):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    ref = _run(c, None)
    assert ref, 'a case returns something'
    for poison in POISONS:
        what = '%s, poison 0x%02X' % (c.name, poison)
        with monkeypatch.context() as mp:
            g = install(mp, poison)
            rec = record(mp)
            got = _run(c, g)
            g.check()
            g.check_inputs()
            assert [t for t, _ in got] == [t for t, _ in ref], what
            for (tag, gv), (_, rv) in zip(got, ref):
                _compare(tag, gv, rv, what)
            missing = sorted(set(c.entries) - set(rec.calls))
            assert not missing, '%s: declared but not called: %s' % (what, missing)
            assert g.arenas, what


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def tile_images(h0, w0, ws, seed):
    """(img1, img2, origins): T = 3 tiles at (0, 0), (3, 7) and one that ends on the image's last
    row, last column and so last byte; the pitch (= the width: the images are contiguous) is odd."""
    ch, cw = h0 + ws - 1, w0 + ws - 1
    H, W = ch + 5, cw + 9 + (cw % 2)
    assert W % 2 == 1
    a, b = stereo_pair(H, W, seed=seed, dx=2)
    return a, b, [(0, 0), (3, 7), (H - ch, W - cw)]


def holed_maps(H, W):
    """M = 2 maps with about a fifth of the cells holes: the fill tests' plane with random holes and
    one block of them, rippled so that the speckle filter finds segments of every size, and noise
    with NaN, +-inf, -0.0 and a NaN payload among its holes."""
    rng = np.random.default_rng(31 * H + W)
    p = holed_plane(H, W, seed=H + W, share=0.18, big=min(H, W) // 5)
    p = p + np.where(rng.uniform(size=p.shape) < 0.3, rng.normal(0, 0.4, p.shape), 0.0)
    q = rng.normal(0, 2, (H, W))
    hole = rng.uniform(size=q.shape) < 0.2
    q[hole] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(hole.sum()))
    q[0, 0], q[H - 1, W - 1] = -0.0, 1.5
    q.view(np.uint64)[H // 2, W // 2] = 0x7ff8000000000123
    x = np.stack([p, q])
    assert 0.1 < np.mean(~np.isfinite(x)) < 0.3
    return x


MAP_SHAPES = [(33, 31), (65, 130), (150, 150)]
SID = '%dx%d'


def photo_inputs(H, W, r):
    """Images cut so that the outermost windows touch all four borders (the 'tight' margin of the
    photo tests) and disparities of both signs up to 3 pixels with specials among them: some
    windows lie partly outside."""
    m = r + 1
    a, b = stereo_pair(H + 2 * m, W + 2 * m + 2, seed=H + W + r, dx=1)
    dr, dc = disparity_planes(H, W, r, 'mixed')
    mask = (np.random.default_rng(H + r).uniform(size=(H, W)) < 0.7).astype(np.uint8)
    return a, b, dr, dc, (m, m + 1), mask


# ---------------------------------------------------------------------------------------------
# the tile pipeline
# ---------------------------------------------------------------------------------------------
def pipeline(h0, w0, ws, full, filt=False):
    def fn(x):
        a, b, org = tile_images(h0, w0, ws, seed=h0 + w0 + ws)
        ta, tb = x.inp(a), x.inp(b)
        assert not x.g or (ta.data_ptr() % 2 == 1 and ta.stride(0) % 2 == 1)
        batch = engine.TileBatch(ta, tb, org, h0, w0, ws, NCC)
        pyr = engine.DevicePyramid(batch)
        m = pyr.match()
        x.add('match', m)
        x.add('match nlev 2', pyr.match(nlev=2))
        flat = pyr.match(sub_pix=False)
        x.add('match no sub_pix', flat)
        if filt:
            x.add('match median filter', pyr.match(filtering=True, filtering_mode='median'))
            x.add('match average filter', pyr.match(filtering=True, filtering_mode='average', nlev=pyr.nlev - 1))
        for mode in ('elevation', 'elevation2', 'distance'):
            x.add('cal_map ' + mode, engine.cal_map(m, mode))
        x.add('subpix_map_tiles', engine.subpix_map_tiles(pyr, x.inout(flat)))
        x.add('levels', [t for t in pyr.levels if t is not None])
        if not full:
            return
        x.add('volume', pyr.volume())                                    # the min / max known
        x.add('volume f16', pyr.volume_f16())
        cold = engine.DevicePyramid(batch, build=False)
        x.add('volume f16 cold', cold.volume_f16())                      # its own min / max sweep
        x.add('volume after f16', cold.volume())
        lv = pyr.materialized_levels('f32')
        x.add('materialized f32', lv)
        x.add('materialized f16', pyr.materialized_levels('f16'))
        x.add('match on levels', pyr.match(levels=lv))
        x.add('subpix_map', engine.subpix_map(lv[0][0].reshape(h0, w0, h0, w0), x.inout(flat[0])))
    return fn


BUILD = ('dm_corr_stats', 'dm_match', 'dm_cal_map', 'dm_subpix_map_tiles', 'dm_aggregate')
FULL = ('dm_corr_volume_ex', 'dm_rectify', 'dm_rectify_f16', 'dm_subpix_map')
# the c2, c3, c5 instances, mq KS 2 and KS 4
for shp in [(4, 64, 5), (8, 128, 3), (4, 256, 5), (8, 32, 9), (8, 64, 15)]:
    case('pipeline %dx%d ws%d' % shp, BUILD + FULL + ('dm_corr_level12', 'dm_corr_level1'))(pipeline(*shp, full=True))
# a 3 x 1 top level (six levels); a square fused shape, for Matching._filter
case('pipeline 96x32 ws5', BUILD + ('dm_corr_level12', 'dm_corr_level1'))(pipeline(96, 32, 5, full=False))
case('pipeline 32x32 ws5 filter', BUILD + ('dm_corr_level12', 'dm_corr_level1'))(pipeline(32, 32, 5, False, filt=True))
# shapes mf16_eligible rejects (w0 below 32; w0 no power of two): the generic kernels
case('pipeline 16x16 ws5 generic', BUILD + FULL + ('dm_corr_level1',))(pipeline(16, 16, 5, True, filt=True))
case('pipeline 8x24 ws3 generic', BUILD + FULL + ('dm_corr_level1',))(pipeline(8, 24, 3, True))


def fuse_case(mode):
    def fn(x):
        a, b, org = tile_images(8, 128, 3, seed=11)
        pyr = engine.DevicePyramid(engine.TileBatch(x.inp(a), x.inp(b), org, 8, 128, 3, NCC))
        assert pyr.fuse_level2 == mode and (pyr.levels[1] is None) == (mode == 2)
        x.add('match', pyr.match())
        x.add('levels', [t for t in pyr.levels if t is not None])
    return fn


case('DM_FUSE_L2=0', ('dm_corr_stats', 'dm_corr_level1', 'dm_aggregate', 'dm_match'), env={'DM_FUSE_L2': '0'})(fuse_case(0))
case('DM_FUSE_L2=1', ('dm_corr_stats', 'dm_corr_level12', 'dm_aggregate', 'dm_match'), env={'DM_FUSE_L2': '1'})(fuse_case(1))
case('DM_FUSE_L2=2', ('dm_corr_stats', 'dm_corr_level12', 'dm_aggregate', 'dm_match'), env={'DM_FUSE_L2': '2'})(fuse_case(2))


@case('solve_tiles', ('dm_corr_stats', 'dm_corr_level12', 'dm_match'))
def _solve_tiles(x):
    a, b, org = tile_images(4, 64, 5, seed=3)
    x.add('tiles', engine.solve_tiles(x.inp(a), x.inp(b), org, 4, 64, 5, NCC))
    # one tile per chunk: a fresh workspace per tile
    x.add('chunked', engine.solve_tiles(x.inp(a), x.inp(b), org, 4, 64, 5, NCC, mem_budget=1))


@case('solve_tiles_bidir', ('dm_corr_stats', 'dm_corr_level12', 'dm_aggregate', 'dm_match'))
def _solve_tiles_bidir(x):
    a, b, org = tile_images(8, 32, 5, seed=5)
    x.add('bidir', engine.solve_tiles_bidir(x.inp(a), x.inp(b), org, 8, 32, 5, NCC))


@case('volume entries of the ABI', ('dm_corr_stats', 'dm_corr_volume', 'dm_corr_volume_f16'))
def _volume_abi(x):
    """dm_corr_volume and dm_corr_volume_f16 have no caller in the package (it goes through
    dm_corr_volume_ex): the C entries on a workspace of exactly dm_stats_bytes, an MFMA shape and a
    generic one."""
    lib = L.load()
    for h0, w0, ws in [(4, 64, 5), (8, 32, 9), (6, 10, 3)]:
        a, b, org = tile_images(h0, w0, ws, seed=w0)
        batch = engine.TileBatch(x.inp(a), x.inp(b), org, h0, w0, ws, NCC)
        stats = x.work(lib.dm_stats_bytes(batch.ref()))
        P = h0 * w0
        # d_l0 is 16-byte aligned, as the header asks (the MFMA volume kernels store 16 bytes per lane)
        v, vh = x.out((3, P, P), torch.float32, misalign=16), x.out((3, P, P), torch.float16, misalign=16)
        L.check(lib.dm_corr_stats(batch.ref(), L.ptr(stats), L.stream_handle()))
        # a volume at its element's alignment only is rejected by all three entries, before any launch
        off32, off16 = ctypes.c_void_p(v.data_ptr() + 4), ctypes.c_void_p(vh.data_ptr() + 2)
        for rc in (lib.dm_corr_volume(batch.ref(), L.ptr(stats), off32, L.stream_handle()),
                   lib.dm_corr_volume_f16(batch.ref(), L.ptr(stats), off16, L.stream_handle()),
                   lib.dm_corr_volume_ex(batch.ref(), L.ptr(stats), 0, off32, L.stream_handle()),
                   lib.dm_corr_volume_ex(batch.ref(), L.ptr(stats), L.DM_VOLUME_F16, off16, L.stream_handle())):
            assert rc == L.DM_ERR_ARG and '16-byte aligned' in L.last_error()
        with pytest.raises(ValueError, match='16-byte aligned'):
            L.check(lib.dm_corr_volume(batch.ref(), L.ptr(stats), off32, L.stream_handle()))
        L.check(lib.dm_corr_volume_f16(batch.ref(), L.ptr(stats), L.ptr(vh), L.stream_handle()))
        L.check(lib.dm_corr_volume(batch.ref(), L.ptr(stats), L.ptr(v), L.stream_handle()))
        x.add('volume %dx%d' % (h0, w0), (v, vh))


@case('reference mirrors', ('dm_rectify64', 'dm_rectify', 'dm_aggregate', 'dm_sub_pix_cal'))
def _mirrors(x):
    from deepmatching_stereo_matching_amd.misc.Correlation_map import Correlation_map
    from deepmatching_stereo_matching_amd.misc.sub_pix_cal import sub_pix_cal
    rng = np.random.default_rng(2)
    a, b = stereo_pair(12, 14, seed=1, dx=1)
    co = Correlation_map(a, b, window_size=3)
    m = rng.uniform(0, 1, (6, 10, 6, 10))
    m[1, 2, 3, 4] = np.nan
    x.add('rectify64', co._rectification(m))
    x.add('rectify32', co._rectification(m.astype(np.float32)))
    x.add('aggregation', co._aggregation(m))
    arr, score = rng.uniform(-4, 4, (33, 31)), rng.uniform(0, 1, (33, 31))
    for direction in (0, 1):
        x.add('sub_pix_cal %d' % direction, sub_pix_cal(arr, score, direction))


# ---------------------------------------------------------------------------------------------
# stitching
# ---------------------------------------------------------------------------------------------
def stitch_case(n, stride):
    def fn(x):
        from test_merge_gpu import H0, W0, MODES, crafted
        F, B = crafted(n)
        f, b = x.inp(F), x.inp(B)
        x.add('stitch', engine.stitch(f, n, H0, W0, stride, MODES))
        x.add('stitch_fb', engine.stitch_fb(f, b, n, H0, W0, stride, MODES, 1.0))
        for rule in ('last', 'center', 'feather', 'median'):
            x.add('merge ' + rule, engine.stitch_merge(f, None, n, H0, W0, stride, MODES, None, rule, 1))
            x.add('merge fb ' + rule, engine.stitch_merge(f, b, n, H0, W0, stride, MODES, 1.0, rule,
                                                          1 if rule == 'last' else 2))
        x.add('fb_check', engine.fb_check(f, b, 1.0))
        x.add('fb_check unmasked', engine.fb_check(f, b, 0.0, masked=False))
        x.add('fb_check one tile', engine.fb_check(f[2], b[2], float('inf')))
    return fn


# test_merge_gpu.GEOMS, and a grid whose output has cells no tile covers
for n, stride in [((3, 2), (2, 3)), ((4, 3), (1, 2)), ((2, 2), (5, 7)), ((2, 3), (6, 9)), ((3, 5), (37, 19))]:
    case('stitch n%dx%d stride %dx%d' % (n + stride), ('dm_stitch', 'dm_stitch_fb', 'dm_stitch_merge', 'dm_fb_check'))(
        stitch_case(n, stride))


# ---------------------------------------------------------------------------------------------
# map stages: out of place, out= a guarded tensor, in place
# ---------------------------------------------------------------------------------------------
def three_ways(x, tag, maps, call):
    """``call(src, out)`` -> the stage's results, with out None, a guarded ``out=`` and in place."""
    at = _site(2)      # the case's own line names the buffers
    src = x.inp(maps, label=at + ' (%s, source)' % tag)
    x.add(tag + ' new', call(src, None))
    x.add(tag + ' out=', call(src, x.out(maps.shape, label=at + ' (%s, out=)' % tag)))
    t = x.inout(maps, label=at + ' (%s, in place)' % tag)
    x.add(tag + ' in place', call(t, t))


def fill_case(H, W):
    def fn(x):
        maps = holed_maps(H, W)
        for iters in (0, 3, 17):
            three_ways(x, 'fill %d' % iters, maps, lambda s, o: engine.fill_holes(s, iters, out=o, return_holes=True))
        x.add('no mask', engine.fill_holes(x.inp(maps), 3))
        x.add('one map', engine.fill_holes(x.inp(maps[1]), 17, return_holes=True))
        allh = np.full((2, H, W), np.nan)
        allh[1] = maps[0]
        x.add('a map of holes', engine.fill_holes(x.inp(allh), 3))
    return fn


def speckle_case(H, W):
    def fn(x):
        maps = holed_maps(H, W)
        every = dict(return_removed=True, return_sizes=True, return_labels=True)
        three_ways(x, 'speckle', maps, lambda s, o: engine.filter_speckles(s, 6, 0.5, out=o, **every))
        for k in every:      # each optional output omitted in turn
            x.add('without ' + k, engine.filter_speckles(x.inp(maps), 6, 0.5, **dict(every, **{k: False})))
        x.add('none', engine.filter_speckles(x.inp(maps), 50, float('inf')))
        x.add('size 0', engine.filter_speckles(x.inp(maps[0]), 0, 0.0, return_sizes=True, return_labels=True))
    return fn


def bilateral_case(H, W):
    def fn(x):
        maps = holed_maps(H, W)
        rng = np.random.default_rng(H)
        g8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
        g64 = rng.normal(0, 3, (2, H, W))
        g64[0, 1, 1], g64[1, H - 1, 0] = np.nan, np.inf
        for r in (2, 15):
            for iters in (1, 2):
                tag = 'r%d i%d' % (r, iters)
                three_ways(x, tag + ' self', maps,
                           lambda s, o: engine.bilateral_filter(s, r, 1.5, 3.0, iters=iters, out=o, return_filled=True))
                three_ways(x, tag + ' u8 fill', maps,
                           lambda s, o: engine.bilateral_filter(s, r, 20.0, 3.0, guide=x.inp(g8), iters=iters, fill=True,
                                                                out=o, return_filled=True))
            x.add('r%d f64 guide' % r, engine.bilateral_filter(x.inp(maps), r, 2.0, float('inf'), guide=x.inp(g64)))
            x.add('r%d f64 guide fill' % r, engine.bilateral_filter(x.inp(maps), r, 2.0, 4.0, guide=x.inp(g64[0]),
                                                                    iters=2, fill=True, return_filled=True))
    return fn


def median_case(H, W):
    def fn(x):
        maps = holed_maps(H, W)
        rng = np.random.default_rng(W)
        w1 = rng.uniform(0, 2, (H, W))
        w1[rng.uniform(size=w1.shape) < 0.1] = 0.0
        w1[0, 0], w1[H - 1, W - 1] = np.nan, np.inf
        w2 = rng.uniform(0.5, 1.5, (2, H, W))
        for r, iters in [(1, 1), (1, 2), (3, 3), (7, 1), (7, 2)]:
            tag = 'r%d i%d' % (r, iters)
            three_ways(x, tag, maps, lambda s, o: engine.median_filter(s, r, iters=iters, out=o, return_changed=True))
            three_ways(x, tag + ' weighted', maps,
                       lambda s, o: engine.median_filter(s, r, weight=x.inp(w2 if r == 3 else w1), iters=iters,
                                                         min_count=2, fill=True, out=o, return_changed=True))
        x.add('r3 no mask', engine.median_filter(x.inp(maps), 3, iters=2))
    return fn


for shape in MAP_SHAPES:
    case('fill ' + SID % shape, ('dm_fill_holes',))(fill_case(*shape))
    case('speckle ' + SID % shape, ('dm_filter_speckles',))(speckle_case(*shape))
    case('bilateral ' + SID % shape, ('dm_bilateral_filter',))(bilateral_case(*shape))
    case('median ' + SID % shape, ('dm_median_filter',))(median_case(*shape))

# another tile side changes which stores are ragged; a short last launch of the relaxation.  (The
# library reads these variables, and DM_SEQ_SUM below, with getenv on every call, so setting them
# for the test takes effect; tests/test_speckle_gpu.py, test_fill_gpu.py and test_seq_sum_gpu.py
# show that the results do not depend on them.)
case('DM_SPECKLE_TILE=16', ('dm_filter_speckles',), env={'DM_SPECKLE_TILE': '16'})(speckle_case(65, 130))
case('DM_FILL_STEPS=5', ('dm_fill_holes',), env={'DM_FILL_STEPS': '5'})(fill_case(150, 150))


# ---------------------------------------------------------------------------------------------
# the stages that read the images
# ---------------------------------------------------------------------------------------------
def photo_case(H, W, r):
    def fn(x):
        a, b, dr, dc, off, _ = photo_inputs(H, W, r)
        ta, tb = x.inp(a), x.inp(b)
        assert not x.g or ta.data_ptr() % 2 == 1
        maps = np.stack([dc, dr, dr - dc])
        x.add('score', engine.photo_score(ta, tb, x.inp(dr), x.inp(dc), r, offset=off, return_warped=True))
        three_ways(x, 'reject', maps, lambda s, o: engine.photo_score(ta, tb, x.inp(dr), x.inp(dc), r, offset=off,
                                                                      min_score=0.5, maps=s, out=o,
                                                                      return_warped=True, return_rejected=True))
        x.add('reject, no masks', engine.photo_score(ta, tb, x.inp(dr), x.inp(dc), r, offset=off, min_score=-0.25,
                                                     maps=x.inp(maps[0])))
        t = x.inout(maps)      # the planes are planes of the map that is rejected in place
        x.add('aliased', engine.photo_score(ta, tb, t[1], t[0], r, offset=off, min_score=0.5, maps=t, out=t,
                                            return_rejected=True))
    return fn


def refine_case(H, W, r):
    def fn(x):
        a, b, dr, dc, off, mask = photo_inputs(H, W, r)
        ta, tb = x.inp(a), x.inp(b)
        every = dict(return_score=True, return_shift=True)
        for s in (1, 3):
            x.add('s%d' % s, engine.photo_refine(ta, tb, x.inp(dr), x.inp(dc), r, s, offset=off, **every))
            x.add('s%d mask' % s, engine.photo_refine(ta, tb, x.inp(dr), x.inp(dc), r, s, offset=off, min_gain=0.05,
                                                      subpix=False, mask=x.inp(mask), out=(x.out(dr.shape), x.out(dr.shape)),
                                                      **every))
            tr, tc = x.inout(dr), x.inout(dc)      # the outputs are the inputs
            x.add('s%d aliased' % s, engine.photo_refine(ta, tb, tr, tc, r, s, offset=off, mask=x.inp(mask),
                                                         out=(tr, tc), **every))
        x.add('no outputs', engine.photo_refine(ta, tb, x.inp(dr), x.inp(dc), r, 1, offset=off))
    return fn


def lsm_case(H, W, r):
    def fn(x):
        a, b, dr, dc, off, mask = photo_inputs(H, W, r)
        ta, tb = x.inp(a), x.inp(b)
        every = dict(return_score=True, return_status=True)
        for iters in (1, 4):
            x.add('i%d' % iters, engine.lsm_refine(ta, tb, x.inp(dr), x.inp(dc), r, iters, offset=off, **every))
            x.add('i%d mask' % iters, engine.lsm_refine(ta, tb, x.inp(dr), x.inp(dc), r, iters, offset=off, max_move=0.5,
                                                        mask=x.inp(mask), out=(x.out(dr.shape), x.out(dr.shape)), **every))
            tr, tc = x.inout(dr), x.inout(dc)
            x.add('i%d aliased' % iters, engine.lsm_refine(ta, tb, tr, tc, r, iters, offset=off, mask=x.inp(mask),
                                                           out=(tr, tc), **every))
        x.add('no outputs', engine.lsm_refine(ta, tb, x.inp(dr), x.inp(dc), r, 1, offset=off))
    return fn


for shape in MAP_SHAPES[:2]:
    for r in (1, 3, 7):
        case('photo_score %s r%d' % (SID % shape, r), ('dm_photo_score',))(photo_case(*shape, r))
        case('photo_refine %s r%d' % (SID % shape, r), ('dm_photo_refine',))(refine_case(*shape, r))
        case('lsm_refine %s r%d' % (SID % shape, r), ('dm_lsm_refine',))(lsm_case(*shape, r))


# ---------------------------------------------------------------------------------------------
# priors
# ---------------------------------------------------------------------------------------------
@case('downsample2', ('dm_downsample2',))
def _downsample2(x):
    rng = np.random.default_rng(4)
    wide = rng.integers(0, 256, (10, 64)).astype(np.uint8)
    x.add('vector path', engine.downsample2(x.inp(wide, misalign=16)))      # aligned rows of 32 bytes: the uint4 path
    x.add('same rows, odd address', engine.downsample2(x.inp(wide)))        # the byte path
    x.add('odd sides', engine.downsample2(x.inp(rng.integers(0, 256, (11, 67)).astype(np.uint8))))
    x.add('two rows', engine.downsample2(x.inp(rng.integers(0, 256, (2, 3)).astype(np.uint8))))


@case('tile_prior', ('dm_tile_prior',))
def _tile_prior(x):
    maps = holed_maps(65, 130) * 3.0
    maps[:, 40:, 100:] = np.nan            # a tile without a finite cell takes the others' median
    org = np.array([(0, 0), (3, 7), (60, 90), (100, 200), (20, 230), (90, 215)])
    for scale in (1, 2):
        x.add('scale %d' % scale, engine.tile_prior(x.inp(maps[0]), x.inp(maps[1]), org, 32, 32, 2, scale=scale))
    x.add('device origins', engine.tile_prior(x.inp(maps[1]), x.inp(maps[0]), x.inp(org, dtype=I32), 9, 5, 0))


def pack_inputs():
    """T = 5 tiles on a grid of 2 columns (a ragged last grid row) and priors that push crops of
    img2 over every border."""
    h0, w0, ws = 8, 32, 5
    a, b = stereo_pair(47, 91, seed=9, dx=3)
    org = np.array([(0, 0), (3, 7), (35, 55), (20, 30), (35, 0)])
    assert (org[:, 0] + h0 + ws - 1).max() == 47 and (org[:, 1] + w0 + ws - 1).max() == 91
    prior = np.array([(2, -3), (-50, 70), (9, 9), (0, 1), (-1, -2)])
    return a, b, org, prior, h0, w0, ws


@case('pack_tiles and shift_matches', ('dm_pack_tiles', 'dm_shift_matches'))
def _pack(x):
    a, b, org, prior, h0, w0, ws = pack_inputs()
    assert engine.pack_grid(len(org), h0, w0, ws)[1:] == (36, 80)      # 3 x 2 crops of 12 x 36
    res = engine.pack_tiles(x.inp(a), x.inp(b), org, prior, h0, w0, ws)
    x.add('pack', res)
    x.add('pack, device prior', engine.pack_tiles(x.inp(a), x.inp(b), org, x.inp(prior, dtype=I32), h0, w0, ws))
    rng = np.random.default_rng(6)
    m = rng.normal(0, 4, (5, 3, h0, w0))
    m[1, 0, 2, 3], m[4, 1, 7, 31] = np.nan, -0.0
    q = x.inp(np.asarray(prior), dtype=I32)
    x.add('shift', engine.shift_matches(x.inout(m), q))                     # float64 at 8 mod 16: the scalar path
    x.add('shift aligned', engine.shift_matches(x.inout(m, misalign=16), q))      # the double2 path
    odd = rng.normal(0, 4, (2, 3, 3, 5))
    x.add('shift odd cells', engine.shift_matches(x.inout(odd, misalign=16), x.inp(prior[:2], dtype=I32)))


@case('solve_tiles_prior', ('dm_pack_tiles', 'dm_shift_matches', 'dm_corr_stats', 'dm_corr_level12', 'dm_match',
                            'dm_fb_check'))
def _solve_tiles_prior(x):
    a, b, org, prior, h0, w0, ws = pack_inputs()
    x.add('prior', engine.solve_tiles_prior(x.inp(a), x.inp(b), org, prior, h0, w0, ws, NCC))
    x.add('prior, checked', engine.solve_tiles_prior(x.inp(a), x.inp(b), org, x.inp(prior, dtype=I32), h0, w0, ws, NCC,
                                                     consistency=1.0, mem_budget=1))


@case('solve_coarse_to_fine', ('dm_downsample2', 'dm_tile_prior', 'dm_pack_tiles', 'dm_shift_matches', 'dm_stitch',
                               'dm_fb_check', 'dm_corr_stats', 'dm_match'))
def _coarse_to_fine(x):
    a, b = stereo_pair(100, 100, seed=7, dx=6)
    match, q_eff, err, valid, n, org = engine.solve_coarse_to_fine(x.inp(a), x.inp(b), [32, 32], [8, 8], 5, NCC, 1)
    assert err is None and list(n) == [8, 8]
    x.add('coarse to fine', (match, q_eff, valid, org))


# ---------------------------------------------------------------------------------------------
# the Gauss-Seidel post-processing
# ---------------------------------------------------------------------------------------------
@case('optimize_loop', ('dm_image_threshold', 'dm_optimize_loop'))
def _optimize_loop(x):
    from deepmatching_stereo_matching_amd.misc.optimize_loop import image_threshold, optimize_loop
    rng = np.random.default_rng(8)
    h, w = 64, 80
    img, coef = rng.uniform(-2, 12, (h, w)), rng.uniform(0.5, 2, (h, w))
    x.add('threshold', image_threshold(x.inp(img), [1, 9]))
    x.add('e 0', optimize_loop(x.inp(img), x.inp(coef), 0.008, 0, (h - 1, w - 1)))
    x.add('e 2', optimize_loop(x.inp(img), x.inp(coef), 0.008, 2, (h, w)))
    x.add('numpy', optimize_loop(img[:20, :30], coef[:20, :30], 0.008, 1, (20, 30)))


@case('bilateral loop', ('dm_make_weight', 'dm_opt_loop_bilateral'))
def _bilateral_loop(x):
    from deepmatching_stereo_matching_amd.misc import opt_loop
    rng = np.random.default_rng(9)
    h, w, e = 97, 120, 2
    img, guide = rng.uniform(0, 10, (h, w)), rng.uniform(0, 255, (h, w))
    coef = rng.uniform(0.5, 2, (h, w))
    g, c = opt_loop.make_weight(x.inp(guide), e, (h, w), [5.0, 3.0])
    x.add('weights', (g, c))
    t = x.inout(img)
    x.add('horizon', opt_loop.optimize_loop_bilateral_horizon(t, c, g, x.inp(coef), 0.0, e, (h, w)))
    x.add('vertical', opt_loop.optimize_loop_bilateral_vertical(t, c, g, x.inp(coef), 0.0, e, (h, w)))


def seq_sum_case(x):
    lib = L.load()
    rng = np.random.default_rng(10)
    for n in (1, 63, 64, 1000, 4097):
        v, out = x.inp(rng.uniform(0, 3, n) * 10.0 ** rng.integers(-3, 4, n)), x.out((), F64)
        L.check(lib.dm_seq_sum(L.ptr(v), n, L.ptr(out), L.stream_handle()), 'dm_seq_sum')
        x.add('sum of %d' % n, out)


case('dm_seq_sum', ('dm_seq_sum',))(seq_sum_case)
case('DM_SEQ_SUM=chain', ('dm_seq_sum',), env={'DM_SEQ_SUM': 'chain'})(seq_sum_case)


# ---------------------------------------------------------------------------------------------
# the chain: every stage at once, each handing its map over in place
# ---------------------------------------------------------------------------------------------
CHAIN = dict(image_size=[32, 32], stride=[32, 32], window_size=5, degree_map_mode=['elevation', 'elevation2'])
STAGES = dict(median=(1, 2), median_weight='correlation', photo=(2, 0.75), speckle=(4, 1.0), fill=16,
              refine=(2, 2, 0.05), refine_where='filled', lsm=(2, 3), lsm_where='filled', smooth=(2, 10.0, 2.0))
CHAIN_ENTRIES = ('dm_corr_stats', 'dm_corr_level12', 'dm_aggregate', 'dm_match', 'dm_median_filter', 'dm_photo_score',
                 'dm_filter_speckles', 'dm_fill_holes', 'dm_photo_refine', 'dm_lsm_refine', 'dm_bilateral_filter')


def corrupted_pair():
    """tests/test_lsm_gpu.py's: dx = 2, a 2 x 2 grid of 32 x 32 tiles, a block of img2 overwritten."""
    a, b = stereo_pair(100, 100, seed=7, dx=2)
    b = b.copy()
    b[20:36, 24:44] = np.random.default_rng(5).integers(0, 256, (16, 20)).astype(np.uint8)
    return a, b


@case('ImageCutSolver chain', CHAIN_ENTRIES + ('dm_stitch',))
def _chain(x):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = corrupted_pair()
    solver = ImageCutSolver(x.inp(a), x.inp(b), **STAGES, **CHAIN)
    solver.log_flg = False
    res = solver._execute_matching_device()
    assert len(res) == 10 and tuple(res[0].shape) == (2, 64, 64)
    x.add('chain', res)


@case('ImageCutSolver chain, checked and merged', CHAIN_ENTRIES + ('dm_stitch_merge',))
def _chain_merged(x):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = corrupted_pair()
    solver = ImageCutSolver(x.inp(a), x.inp(b), consistency=1.0, merge='feather', **STAGES,
                            **dict(CHAIN, stride=[16, 16]))
    solver.log_flg = False
    x.add('chain', solver._execute_matching_device())


@case('solve_image_sharded', ('dm_corr_stats', 'dm_match', 'dm_stitch_fb', 'dm_fill_holes', 'dm_lsm_refine',
                              'dm_photo_score'))
def _sharded(x):
    from deepmatching_stereo_matching_amd import shard
    a, b = corrupted_pair()
    x.add('sharded', shard.solve_image_sharded(x.inp(a), x.inp(b), [32, 32], [32, 32], 5, NCC,
                                               ['elevation', 'elevation2'], consistency=1.0, fill=16, lsm=(2, 3, 1.0),
                                               lsm_where='filled', photo=2))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name.replace(' ', '_'))
def test_guarded(c, monkeypatch):
    run_case(c, monkeypatch)
