"""Geometry and content lattice of the Gauss-Seidel post-processing (dm_optimize_loop,
dm_make_weight, dm_opt_loop_bilateral; csrc/dm_postproc.hip, csrc/dm_gs_pf.h), on top of
tests/test_postproc.py.  DESIGN.md section 4d′ maps every gap to the test that closes it.

The comparisons are test_postproc.py's own: maps, errors and weights bit for bit against the
oracle (same pinned exp) and against the reference-made goldens when sweeping on the golden
weights.  No tolerance is introduced here.

  geometry   sweeps narrower than the map in both axes (the colour weights' pitch is
             size[1] - e, the map's is w), coefficients wider / taller / smaller than the map
             (pitch wc), every depth of numpy's pairwise sum (e = 4 ... 15), sweeps of one
             update, one row, one column, 1 / 2 / 3 levels -- every case on the pipelined
             kernels (DM_GS_PF=1) and on the one-lane-per-update kernels (DM_GS_PF=0), from
             numpy arrays and from device tensors
  widths     one case per pipelined bilateral instance (e = 1 ... 5) whose widest level
             exceeds the R * NTHR / LPU updates the instance prefetches; the premise is
             asserted on the host schedule
  content    NaN / +-inf in map, guide and coefficient, a == 4 alpha, K == 0/0; placed so
             that the Gauss-Seidel flood stays small and the comparison still says something
"""
import os

import numpy as np
import pytest

from oracle import oracle as O

from test_postproc import _cell, gold, same, same_err, sigma_of

ALPHA = 0.008
FAR = 1e6      # coefficient cells no update addresses
PFS = ('1', '0')   # DM_GS_PF: pipelined level walks / one lane per update


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def loop_mask(h, w, s0, s1, e):
    """cells some update of optimize_loop writes (forward and backward sweep)"""
    m = np.zeros((h, w), dtype=bool)
    n = max(0, s0 - 2 * e - 1) * max(0, s1 - 2 * e - 1)
    for kind in (0, 1):
        for s in range(n):
            m[_cell(kind, s, s0, s1, e)] = True
    return m


def bilat_mask(h, w, s0, s1, e):
    m = np.zeros((h, w), dtype=bool)
    m[e:max(e, s0 - e - 1), e:max(e, s1 - e - 1)] = True
    return m


def assert_untouched(out, before, mask):
    """cells no update addresses keep their bits (NaN payloads included)"""
    assert np.array_equal(bits(out)[~mask], bits(before)[~mask])


def field(h, w, seed, size=None):
    """(guide, map, coefficient of the map's shape); cells outside `size` unlike their neighbours"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    guide = 5 + 4 * np.sin(x / 13.0) * np.cos(y / 7.0) + rng.normal(0, 0.7, (h, w))
    img = guide + rng.normal(0, 0.3, (h, w))
    coef = rng.uniform(0.2, 1.5, (h, w))
    if size is not None:
        out = np.ones((h, w), dtype=bool)
        out[:size[0], :size[1]] = False
        guide[out] = rng.uniform(40, 60, int(out.sum()))
        img[out] = rng.uniform(-60, -40, int(out.sum()))
    return guide, img, coef


def device():
    import torch
    return torch.device('cuda', 0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device())


# ---------------------------------------------------------------------------------------
# CPU: the premises of the GPU cases, on the host-only dm_gs_schedule
# ---------------------------------------------------------------------------------------
# updates prefetched per level by k_bilateral_pf<E, LPU, R, NTHR>: R * NTHR / LPU, and one
# round NTHR / LPU, as dm_opt_loop_bilateral dispatches them (the DM_BILAT_PF lines of
# csrc/dm_postproc.hip): e -> (LPU, R, NTHR)
PF_INST = {1: (4, 1, 1024), 2: (4, 1, 1024), 3: (4, 2, 512), 4: (8, 2, 512), 5: (8, 1, 512)}
# (swept rows, swept columns, e): the sweep is size (rows, cols) of a (rows + 3, cols + 5) map,
# so the weights' pitch differs from the map's in every instance.  The last is the first one
# transposed: tall and narrow, every level short
WIDE = [(263, 523, 1), (265, 780, 2), (267, 1037, 3), (141, 659, 4), (79, 407, 5), (523, 263, 1)]
PAD = (3, 5)


def pf_limit(e):
    lpu, r, nthr = PF_INST[e]
    return r * nthr // lpu, nthr // lpu


def widths(h, w, s0, s1, e):
    from deepmatching_stereo_matching_amd import postproc
    _, off = postproc.host_schedule(2, h, w, s0, s1, e)
    return np.diff(off)


def test_wide_level_premises():
    assert [pf_limit(e)[0] for e in (1, 2, 3, 4, 5)] == [256, 256, 256, 128, 64]
    widest, parity = {}, set()
    for s0, s1, e in WIDE:
        d = widths(s0 + PAD[0], s1 + PAD[1], s0, s1, e)
        widest[(s0, s1, e)] = int(d.max())
        parity.add(len(d) & 1)
    for s0, s1, e in WIDE[:5]:
        lim, rnd = pf_limit(e)
        assert widest[(s0, s1, e)] > lim > 0      # the loop "levels wider than R*NG updates" runs
        assert widest[(s0, s1, e)] > rnd          # R = 2: the second prefetch round holds updates
    assert widest == {(263, 523, 1): 260, (265, 780, 2): 259, (267, 1037, 3): 258, (141, 659, 4): 130,
                      (79, 407, 5): 66, (523, 263, 1): 130}
    assert widest[WIDE[5]] <= pf_limit(1)[0]      # the contrast: never leaves the prefetch
    assert parity == {0, 1}                       # the ping-pong ends on either buffer
    # why these cases exist: three instances of test_postproc.test_gpu_bilateral_pipelined stay
    # inside their first prefetch round, and e = 3 inside its first round of two
    for n, e in ((300, 1), (150, 3), (70, 5)):
        assert int(widths(n, n, n, n, e).max()) <= pf_limit(e)[1]
    for n, e in ((800, 2), (700, 4)):
        assert int(widths(n, n, n, n, e).max()) > pf_limit(e)[0]


# sweeps of 1, 2 and 3 levels, one row and one column, for every pipelined instance and the
# fall-back (e = 0, 6): (rows, columns) of updates
TINY = [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (2, 2), (1, 7), (6, 1)]


def tiny_geo(e, ni, nj):
    s0, s1 = 2 * e + 1 + ni, 2 * e + 1 + nj
    return s0 + 2, s1 + 3, s0, s1


def test_tiny_level_counts():
    from deepmatching_stereo_matching_amd import postproc
    seen = set()
    for e in range(0, 7):
        for ni, nj in TINY:
            h, w, s0, s1 = tiny_geo(e, ni, nj)
            for kind in (0, 1, 2):
                order, off = postproc.host_schedule(kind, h, w, s0, s1, e)
                assert len(order) == ni * nj
                if kind == 2:
                    seen.add(len(off) - 1)
                    if e and (ni == 1 or nj == 1):      # a row or a column of windows is a chain
                        assert len(off) - 1 == ni * nj
    assert {1, 2, 3} <= seen


def test_bilateral_rejects_wide_color_before_launch():
    """postproc.bilateral: a colour matrix whose second dimension is not size[1] - e would be
    read at the wrong pitch; ValueError before anything touches a device (host tensors here)"""
    import torch
    from deepmatching_stereo_matching_amd import postproc
    e, size = 1, (9, 10)
    img = torch.zeros((10, 12), dtype=torch.float64)
    gauss = torch.ones((3, 3), dtype=torch.float64)
    coef = torch.ones((10, 12), dtype=torch.float64)
    for cols in (size[1] - e + 1, size[1] - e - 1, 12 - e):
        color = torch.ones((size[0] - e, cols, 3, 3), dtype=torch.float64)
        with pytest.raises(ValueError):
            postproc.bilateral(img, color, gauss, coef, e, size, False)
    assert float(img.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------
# GPU: geometry lattice
# ---------------------------------------------------------------------------------------
def run_loop(img, coef, alpha, e, size, on_device):
    """the mirror from numpy arrays or from device tensors -> (map, error) as numpy / float"""
    from deepmatching_stereo_matching_amd.misc.optimize_loop import optimize_loop
    if not on_device:
        keep = img.copy()
        out, err = optimize_loop(img, coef, alpha, e, size)
        assert isinstance(out, np.ndarray) and np.array_equal(bits(img), bits(keep))
        return out, err
    import torch
    t, tc = dev(img), dev(coef)
    out, err = optimize_loop(t, tc, alpha, e, size)
    assert isinstance(out, torch.Tensor) and out is not t
    assert np.array_equal(bits(t.cpu().numpy()), bits(img))      # the sweep runs on a thresholded copy
    return out.cpu().numpy(), float(err)


def run_bilat(img, color, gauss, coef, e, size, vert, on_device):
    """in place, as the reference: the swept map is the object handed in"""
    from deepmatching_stereo_matching_amd.misc import opt_loop as M
    fn = M.optimize_loop_bilateral_vertical if vert else M.optimize_loop_bilateral_horizon
    if not on_device:
        a = img.copy()
        out, err = fn(a, color, gauss, coef, ALPHA, e, size)
        assert out is a
        return a, err
    t = dev(img)
    out, err = fn(t, color if not isinstance(color, np.ndarray) else dev(color),
                  gauss if not isinstance(gauss, np.ndarray) else dev(gauss), dev(coef), ALPHA, e, size)
    assert out is t
    return t.cpu().numpy(), float(err)


@pytest.mark.gpu
@pytest.mark.parametrize('pf', PFS)
@pytest.mark.parametrize('path', gold('loop'), ids=os.path.basename)
def test_gpu_lattice_loop_golden(path, pf, monkeypatch):
    monkeypatch.setenv('DM_GS_PF', pf)
    z = np.load(path)
    e, size, alpha = int(z['exclusion']), list(z['size']), float(z['alpha'])
    ref, rerr = O.optimize_loop(z['img'], z['coef'], alpha, e, size)
    assert same(ref, z['out']) and same_err(rerr, z['error'])
    mask = loop_mask(*z['img'].shape, size[0], size[1], e)
    for on_device in (False, True):
        out, err = run_loop(z['img'].copy(), z['coef'], alpha, e, size, on_device)
        assert same(out, z['out']) and same_err(err, z['error']), on_device
        assert_untouched(out, O.image_threshold(z['img']), mask)


@pytest.mark.gpu
@pytest.mark.parametrize('pf', PFS)
@pytest.mark.parametrize('path', gold('bilat'), ids=os.path.basename)
def test_gpu_lattice_bilateral_golden(path, pf, monkeypatch):
    from deepmatching_stereo_matching_amd.misc import opt_loop as M
    monkeypatch.setenv('DM_GS_PF', pf)
    z = np.load(path)
    e, size = int(z['exclusion']), list(z['size'])
    og, oc = O.make_weight(z['guide'], e, size, sigma_of(z))
    tg, tc = M.make_weight(dev(z['guide']), e, size, sigma_of(z))    # device-resident weights
    assert same(tg.cpu().numpy(), og) and same(tc.cpu().numpy(), oc)
    mask = bilat_mask(*z['img'].shape, size[0], size[1], e)
    for vert, key in ((False, 'h'), (True, 'v')):
        ref, rerr = O.opt_loop_bilateral(z['img'], oc, og, z['coef'], e, size, vert)
        for on_device in (False, True):
            out, err = run_bilat(z['img'], z['color'], z['gauss'], z['coef'], e, size, vert, on_device)
            assert same(out, z['out_' + key]) and err == z['error_' + key], (key, on_device)
            assert_untouched(out, z['img'], mask)
            out, err = run_bilat(z['img'], tc if on_device else oc, tg if on_device else og, z['coef'], e, size,
                                 vert, on_device)
            assert same(out, ref) and err == rerr, (key, on_device)
            assert_untouched(out, z['img'], mask)


def loop_case(h, w, e, size, coef_shape, seed):
    """a map with a few cells beyond the [0, 10] clamp and a coefficient of its own shape that
    is FAR wherever no update reads it"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-2, 12, (h, w))
    coef = rng.uniform(0.05, 2, coef_shape)
    keep = np.zeros(coef_shape, dtype=bool)
    mask = loop_mask(h, w, size[0], size[1], e)
    hh, ww = min(h, coef_shape[0]), min(w, coef_shape[1])
    keep[:hh, :ww] = mask[:hh, :ww]
    assert keep.sum() == mask.sum()         # the coefficient covers every swept cell
    coef[~keep] = FAR
    return img, coef, mask


# (h, w, e, size, coefficient shape): wider and taller, the minimum (s0 - e, s1 - e), shorter
# and wider, narrower than the map but not minimal
LOOP_GEO = [(67, 83, 1, (60, 71), (70, 90)), (67, 83, 2, (67, 83), (65, 81)), (40, 45, 0, (39, 44), (39, 50)),
            (31, 29, 3, (25, 27), (22, 31)), (90, 37, 1, (88, 30), (100, 33))]


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,e,size,cshape', LOOP_GEO)
def test_gpu_loop_coefficient_pitch(h, w, e, size, cshape, monkeypatch):
    img, coef, mask = loop_case(h, w, e, size, cshape, h * w + e)
    ref, rerr = O.optimize_loop(img, coef, ALPHA, e, size)
    assert np.isfinite(ref).all()
    for pf in PFS:
        monkeypatch.setenv('DM_GS_PF', pf)
        for on_device in (False, True):
            out, err = run_loop(img, coef, ALPHA, e, size, on_device)
            assert same(out, ref) and same_err(err, rerr), (pf, on_device)
            assert_untouched(out, O.image_threshold(img), mask)


@pytest.mark.gpu
@pytest.mark.parametrize('e', [0, 1, 2, 4])
def test_gpu_loop_tiny(e, monkeypatch):
    for ni, nj in TINY:
        h, w, s0, s1 = tiny_geo(e, ni, nj)
        img, coef, mask = loop_case(h, w, e, (s0, s1), (s0 - e + 1, s1 - e + 2), 100 * e + 10 * ni + nj)
        ref, rerr = O.optimize_loop(img, coef, ALPHA, e, (s0, s1))
        assert mask.sum() >= ni * nj and np.isfinite(ref).all()
        for pf in PFS:
            monkeypatch.setenv('DM_GS_PF', pf)
            out, err = run_loop(img, coef, ALPHA, e, (s0, s1), False)
            assert same(out, ref) and same_err(err, rerr), (ni, nj, pf)
            assert_untouched(out, O.image_threshold(img), mask)


@pytest.mark.gpu
@pytest.mark.parametrize('e', [0, 1, 2, 3, 4, 5, 6])
def test_gpu_bilateral_tiny(e, monkeypatch):
    """1, 2 and 3 levels, a row and a column of updates on every pipelined instance: the
    look-ahead of two levels and the ping-pong pair have nothing to look at"""
    for ni, nj in TINY:
        h, w, s0, s1 = tiny_geo(e, ni, nj)
        guide, img, coef = field(h, w, 100 * e + 10 * ni + nj, (s0, s1))
        coef = coef[:e + 3, :e + 2] if (ni + nj) & 1 else coef
        og, oc = O.make_weight(guide, e, (s0, s1), [4, 6])
        mask = bilat_mask(h, w, s0, s1, e)
        assert mask.sum() == ni * nj
        for vert in (False, True):
            ref, rerr = O.opt_loop_bilateral(img, oc, og, coef, e, (s0, s1), vert)
            assert np.isfinite(ref).all()
            for pf in PFS:
                monkeypatch.setenv('DM_GS_PF', pf)
                out, err = run_bilat(img, oc, og, coef, e, (s0, s1), vert, True)
                assert same(out, ref) and err == rerr, (ni, nj, vert, pf)
                assert_untouched(out, img, mask)


# ---------------------------------------------------------------------------------------
# GPU: levels wider than the prefetch of every pipelined bilateral instance
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('s0,s1,e', WIDE)
def test_gpu_bilateral_wide_levels(s0, s1, e, monkeypatch):
    from deepmatching_stereo_matching_amd.misc import opt_loop as M
    h, w = s0 + PAD[0], s1 + PAD[1]
    guide, img, coef = field(h, w, s0 + s1 + e, (s0, s1))
    og, oc = O.make_weight(guide, e, (s0, s1), [5, 5])
    tg, tc = M.make_weight(dev(guide), e, (s0, s1), [5, 5])     # k_make_weight over many blocks
    assert same(tg.cpu().numpy(), og) and same(tc.cpu().numpy(), oc)
    mask = bilat_mask(h, w, s0, s1, e)
    for vert in (False, True):
        ref, rerr = O.opt_loop_bilateral(img, oc, og, coef, e, (s0, s1), vert)
        assert np.isfinite(ref).all()
        for pf in PFS:
            monkeypatch.setenv('DM_GS_PF', pf)
            out, err = run_bilat(img, tc, tg, coef, e, (s0, s1), vert, True)
            assert same(out, ref) and err == rerr, (vert, pf)
            assert_untouched(out, img, mask)


# ---------------------------------------------------------------------------------------
# GPU: non-finite content.  A Gauss-Seidel sweep carries a non-finite value into every cell
# it visits afterwards, and a flooded map compares NaN with NaN; the sources sit where the
# oracle's output keeps at least 8 and at most a quarter of its cells non-finite (asserted)
# ---------------------------------------------------------------------------------------
NAN, INF = float('nan'), float('inf')


def assert_informative(ref):
    bad = int((~np.isfinite(ref)).sum())
    assert 8 <= bad <= ref.size // 4, bad


# 18 x 20 map, e = 1: (cells of the map, cells of the coefficient).  +-inf in the map are
# clamped by image_threshold before the sweep; a == 4 alpha divides by zero
LOOP_NONFINITE = {
    'map': ({(11, 19): NAN, (3, 4): INF, (7, 9): -INF}, {}),
    'coef_nan': ({}, {(10, 18): NAN}),
    'coef_inf': ({}, {(12, 18): INF}),
    'coef_4alpha': ({}, {(9, 18): 4 * ALPHA}),
    'all': ({(9, 19): NAN, (2, 2): INF, (5, 11): -INF}, {(3, 18): NAN, (5, 18): INF, (7, 18): 4 * ALPHA}),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(LOOP_NONFINITE))
def test_gpu_loop_nonfinite(name, monkeypatch):
    h, w, e = 18, 20, 1
    rng = np.random.default_rng(5)
    img = rng.uniform(-2, 12, (h, w))
    coef = rng.uniform(0.1, 2, (h, w))
    for pos, v in LOOP_NONFINITE[name][0].items():
        img[pos] = v
    for pos, v in LOOP_NONFINITE[name][1].items():
        coef[pos] = v
    ref, rerr = O.optimize_loop(img, coef, ALPHA, e, (h, w))
    assert_informative(ref)
    mask = loop_mask(h, w, h, w, e)
    for pf in PFS:
        monkeypatch.setenv('DM_GS_PF', pf)
        for on_device in (False, True):
            out, err = run_loop(img, coef, ALPHA, e, (h, w), on_device)
            assert same(out, ref) and same_err(err, rerr), (pf, on_device)
            assert_untouched(out, O.image_threshold(img), mask)


# (h, w, e, cells of the map, cells of the guide); the guide's NaN gives NaN colour weights,
# its +inf gives weights of exactly 0 around it and one NaN (inf - inf) at its own cell
BILAT_NONFINITE = {
    'e1_map_nan': (18, 20, 1, {(12, 18): NAN}, {}),
    'e1_map_inf': (18, 20, 1, {(13, 17): INF}, {}),
    'e1_guide': (18, 20, 1, {}, {(13, 18): NAN, (15, 9): INF}),
    'e2_map_nan': (20, 22, 2, {(16, 20): NAN, (17, 17): NAN}, {}),
    'e2_map_inf_guide_nan': (20, 22, 2, {(17, 16): INF}, {(16, 20): NAN}),
    'e2_guide_inf': (20, 22, 2, {}, {(13, 18): INF}),
    'e3_map': (22, 24, 3, {(18, 12): NAN, (17, 19): -INF}, {}),
    'e3_guide': (22, 24, 3, {}, {(18, 20): NAN, (15, 12): INF}),
    'e4_map': (16, 18, 4, {(13, 14): NAN, (14, 3): INF}, {}),
    'e4_guide': (16, 18, 4, {}, {(13, 13): NAN, (9, 10): INF}),
    'e5_map': (19, 21, 5, {(16, 10): NAN, (15, 17): INF}, {}),
    'e5_guide': (19, 21, 5, {}, {(15, 15): NAN, (11, 12): INF}),
    'e6_map_guide': (21, 23, 6, {(18, 11): NAN}, {(16, 19): NAN}),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(BILAT_NONFINITE))
def test_gpu_bilateral_nonfinite(name, monkeypatch):
    from deepmatching_stereo_matching_amd.misc import opt_loop as M
    h, w, e, in_map, in_guide = BILAT_NONFINITE[name]
    guide, img, coef = field(h, w, h + w + e)
    for pos, v in in_map.items():
        img[pos] = v
    clean = O.make_weight(guide, e, (h, w), [5, 5])[1]
    for pos, v in in_guide.items():
        guide[pos] = v
    og, oc = O.make_weight(guide, e, (h, w), [5, 5])
    if in_guide:
        assert np.isnan(oc).any()
    if INF in in_guide.values():
        assert (oc == 0).sum() > (clean == 0).sum()
    g, c = M.make_weight(guide, e, (h, w), [5, 5])
    assert same(g, og) and same(c, oc)
    mask = bilat_mask(h, w, h, w, e)
    for vert in (False, True):
        ref, rerr = O.opt_loop_bilateral(img, oc, og, coef, e, (h, w), vert)
        assert_informative(ref)
        for pf in PFS:
            monkeypatch.setenv('DM_GS_PF', pf)
            for on_device in (False, True):
                out, err = run_bilat(img, oc, og, coef, e, (h, w), vert, on_device)
                assert same(out, ref) and same_err(err, rerr), (vert, pf, on_device)
                assert_untouched(out, img, mask)


@pytest.mark.gpu
@pytest.mark.parametrize('e', [1, 4, 6])
def test_gpu_bilateral_constant_coefficient(e, monkeypatch):
    """coefficient[e, e] == its neighbours: a == 0 and K == 0/0, so every swept cell becomes
    NaN and every other cell keeps its bits"""
    h, w = 2 * e + 9, 2 * e + 11
    size = (h - 1, w - 2)
    guide, img, _ = field(h, w, 7 + e, size)
    coef = np.full((h, w), 0.7)
    og, oc = O.make_weight(guide, e, size, [5, 5])
    mask = bilat_mask(h, w, size[0], size[1], e)
    for vert in (False, True):
        ref, rerr = O.opt_loop_bilateral(img, oc, og, coef, e, size, vert)
        assert np.isnan(ref[mask]).all() and np.isnan(rerr)
        assert_untouched(ref, img, mask)
        for pf in PFS:
            monkeypatch.setenv('DM_GS_PF', pf)
            for on_device in (False, True):
                out, err = run_bilat(img, oc, og, coef, e, size, vert, on_device)
                assert np.isnan(out[mask]).all() and np.isnan(err), (vert, pf, on_device)
                assert_untouched(out, img, mask)


# ---------------------------------------------------------------------------------------
# GPU: the colour matrix the mirrors accept
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('e', [1, 3])
def test_gpu_bilateral_color_shape(e, monkeypatch):
    from deepmatching_stereo_matching_amd.misc import opt_loop as M
    h, w = 2 * e + 14, 2 * e + 13
    size = (h - 5, w - 3)
    guide, img, coef = field(h, w, 31 + e, size)
    og, oc = O.make_weight(guide, e, size, [5, 5])
    # made for a larger size[0]: more rows than the sweep needs, the same pitch
    tg, tall = O.make_weight(guide, e, (h - 1, size[1]), [5, 5])
    assert tall.shape[0] > oc.shape[0] and tall.shape[1:] == oc.shape[1:]
    # made for a larger size[1]: another pitch
    _, wide = O.make_weight(guide, e, (size[0], w), [5, 5])
    assert wide.shape[0] == oc.shape[0] and wide.shape[1] != oc.shape[1]
    for vert in (False, True):
        ref, rerr = O.opt_loop_bilateral(img, oc, og, coef, e, size, vert)
        for pf in PFS:
            monkeypatch.setenv('DM_GS_PF', pf)
            for on_device in (False, True):
                out, err = run_bilat(img, tall, tg, coef, e, size, vert, on_device)
                assert same(out, ref) and err == rerr, (vert, pf, on_device)
        fn = M.optimize_loop_bilateral_vertical if vert else M.optimize_loop_bilateral_horizon
        a = img.copy()
        with pytest.raises(ValueError):
            fn(a, wide, og, coef, ALPHA, e, size)
        t = dev(img)
        with pytest.raises(ValueError):
            fn(t, dev(wide), dev(og), dev(coef), ALPHA, e, size)
        assert np.array_equal(bits(a), bits(img)) and np.array_equal(bits(t.cpu().numpy()), bits(img))
