"""Disparity priors and the coarse-to-fine solve, host side (no GPU): the keyword and argument
validation, and a numpy restatement of the four library entries (include/dmstereo.h, "Disparity
priors") and of the whole procedure, which tests/test_prior_gpu.py compares the device with.

The restatement:
  downsample2_np   dst[y][x] = (a + b + c + d + 2) >> 2 over each 2 x 2 block, an odd end dropped.
  footprint        image rows first = o + e .. last = o + e + size - 1 -> map rows first // s - e ..
                   last // s - e, each end clamped into [0, n - 1].
  tile_prior_np    over a tile's footprint cells where both planes are finite: the element
                   (n - 1) // 2 of each plane in the order of the order-preserving key of the
                   double; q = rint(s * median) as int32.  A tile without such a cell takes the lower
                   median of the other tiles' q per component, 0 if there is none.
  pack_np          crop t of img1 at o_t, of img2 at o_t - q_t clamped into the image; q_eff = o_t -
                   the clamped origin.
  shift_np         rows 0 and 1 of tile t minus q_eff[t].
  coarse_to_fine_np  engine.solve_coarse_to_fine's docstring with a per-crop-pair solver (the
                   oracle) in place of the device.
"""
import ctypes

import numpy as np
import pytest

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fb_host import fb_restate, place

SIGN = np.uint64(0x8000000000000000)


# ---- the restatement -----------------------------------------------------------------------------
def downsample2_np(img):
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape
    a = img[:H // 2 * 2, :W // 2 * 2].astype(np.uint32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def footprint(o, size, e, s, n):
    """(lo, hi), inclusive, of the map cells under image pixels o + e .. o + e + size - 1."""
    first, last = o + e, o + e + size - 1
    return min(max(first // s - e, 0), n - 1), min(max(last // s - e, 0), n - 1)


def key(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b & SIGN != 0, ~b, b | SIGN)


def lower_median(v):
    """The element (n - 1) // 2 of the finite doubles v in the order of their keys."""
    return v[np.argsort(key(v), kind='stable')[(len(v) - 1) // 2]]


def tile_prior_np(d_row, d_col, origins, h0, w0, e, scale):
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    Hc, Wc = d_row.shape
    org = np.asarray(origins).reshape(-1, 2)
    q = np.zeros((len(org), 2), dtype=np.int32)
    valid = np.zeros(len(org), dtype=np.uint8)
    for t, (oy, ox) in enumerate(org):
        y0, y1 = footprint(int(oy), h0, e, scale, Hc)
        x0, x1 = footprint(int(ox), w0, e, scale, Wc)
        r, c = d_row[y0:y1 + 1, x0:x1 + 1].ravel(), d_col[y0:y1 + 1, x0:x1 + 1].ravel()
        ok = np.isfinite(r) & np.isfinite(c)
        if ok.any():
            for k, v in enumerate((r[ok], c[ok])):
                q[t, k] = np.int32(np.clip(np.rint(float(scale) * lower_median(v)), -2.0 ** 30, 2.0 ** 30))
            valid[t] = 1
    if valid.any() and not valid.all():
        for k in range(2):
            v = np.sort(q[valid == 1, k])
            q[valid == 0, k] = v[(len(v) - 1) // 2]
    return q, valid


def pack_np(img1, img2, origins, prior, h0, w0, ws):
    """(crops of img1 [T][ch][cw], crops of img2, q_eff int32 [T][2])."""
    H, W = img1.shape
    ch, cw = h0 + ws - 1, w0 + ws - 1
    c1, c2, q_eff = [], [], []
    for (oy, ox), (qy, qx) in zip(np.asarray(origins).reshape(-1, 2), np.asarray(prior).reshape(-1, 2)):
        sy, sx = min(max(int(oy) - int(qy), 0), H - ch), min(max(int(ox) - int(qx), 0), W - cw)
        c1.append(img1[oy:oy + ch, ox:ox + cw])
        c2.append(img2[sy:sy + ch, sx:sx + cw])
        q_eff.append((int(oy) - sy, int(ox) - sx))
    return np.stack(c1), np.stack(c2), np.array(q_eff, dtype=np.int32)


def shift_np(match, q_eff):
    m = np.array(match, dtype=np.float64)
    m[:, 0] -= q_eff[:, 0, None, None].astype(np.float64)
    m[:, 1] -= q_eff[:, 1, None, None].astype(np.float64)
    return m


def stitch_planes_np(match, n, stride):
    """The overwriting stitch of [T][3][h0][w0] matches in modes ('elevation2', 'elevation')."""
    h0, w0 = match.shape[2:]
    ii, jj = (x.astype(np.float64) for x in np.mgrid[0:h0, 0:w0])
    return np.stack([place(ii - match[:, 0], n, stride), place(jj - match[:, 1], n, stride)])


def solve_level_np(img1, img2, origins, prior, h0, w0, ws, tol, solve):
    """engine.solve_tiles_prior with ``solve(crop1, crop2) -> match [3][h0][w0]`` -> (match, q_eff, err)."""
    c1, c2, q_eff = pack_np(img1, img2, origins, prior, h0, w0, ws)
    m = np.stack([solve(a, b) for a, b in zip(c1, c2)])
    err = None
    if tol is not None:
        err, m = fb_restate(m, np.stack([solve(b, a) for a, b in zip(c1, c2)]), tol)
    return shift_np(m, q_eff), q_eff, err


def coarse_to_fine_np(img1, img2, image_size, stride, ws, k, tol, solve, consistency=None):
    """-> (match, q_eff, err, valid, n, origins, priors per level) of level 0."""
    h0, w0 = image_size
    e = (ws - 1) // 2
    imgs = [(img1, img2)]
    for _ in range(k):
        imgs.append((downsample2_np(imgs[-1][0]), downsample2_np(imgs[-1][1])))
    grids = [engine.cut_grid(a.shape, image_size, stride, ws) for a, _ in imgs]
    prior, valid, priors = np.zeros((len(grids[k][1]), 2), dtype=np.int32), None, {}
    for j in range(k, -1, -1):
        n, org = grids[j]
        priors[j] = prior
        m, q_eff, err = solve_level_np(imgs[j][0], imgs[j][1], org, prior, h0, w0, ws, tol if j else consistency, solve)
        if j:
            d = stitch_planes_np(m, n, stride)
            prior, valid = tile_prior_np(d[0], d[1], grids[j - 1][1], h0, w0, e, 2)
    return m, q_eff, err, valid, n, org, priors


def oracle_solve(ws=5):
    from oracle import oracle as O
    return lambda a, b: O.solve_pair(a, b, ws, 'cv2.TM_CCOEFF_NORMED', True)[0]


def share_within(d_elev, d_elev2, dx, col0, tol=0.5):
    """The share of the cells of map columns >= col0 within tol of (0, dx) in both planes (NaN: not)."""
    with np.errstate(invalid='ignore'):
        ok = (np.abs(d_elev[:, col0:] - dx) <= tol) & (np.abs(d_elev2[:, col0:]) <= tol)
    return float(ok.mean())


# ---- the restatement on hand-worked cases ----------------------------------------------------------
def test_downsample2_np_by_hand():
    a = np.array([[0, 1, 255, 255, 9], [2, 3, 255, 254, 9], [7, 7, 7, 7, 9]], dtype=np.uint8)
    assert downsample2_np(a).tolist() == [[2, 255]]      # (6 + 2) >> 2 = 2; (1019 + 2) >> 2 = 255
    assert downsample2_np(np.zeros((2, 2), np.uint8)).shape == (1, 1)


def test_footprint_first_and_last_tile_of_100x260():
    # S 16, stride 16, ws 5 (e 2), scale 2: the 100 x 260 image holds 5 x 15 tiles, its half 1 x 6
    n, org = engine.cut_grid((100, 260), [16, 16], [16, 16], 5)
    nc, _ = engine.cut_grid((50, 130), [16, 16], [16, 16], 5)
    assert (n, nc) == ([5, 15], [1, 6])
    Hc, Wc = 16 * nc[0], 16 * nc[1]
    assert (Hc, Wc) == (16, 96)
    # first tile, origin (0, 0): pixels 2 .. 17 -> 1 .. 8 at half size -> cells -1 .. 6, clamped 0 .. 6
    assert tuple(org[0]) == (0, 0)
    assert footprint(0, 16, 2, 2, Hc) == (0, 6) and footprint(0, 16, 2, 2, Wc) == (0, 6)
    # last tile, origin (64, 224): rows 66 .. 81 -> 33 .. 40 -> cells 31 .. 38: below the map's 16 rows,
    # the clamp leaves its last row; columns 226 .. 241 -> 113 .. 120 -> cells 111 .. 118 -> column 95
    assert tuple(org[-1]) == (64, 224)
    assert footprint(64, 16, 2, 2, Hc) == (15, 15) and footprint(224, 16, 2, 2, Wc) == (95, 95)
    # a tile in the middle: origin 32 -> pixels 34 .. 49 -> 17 .. 24 -> cells 15 .. 22
    assert footprint(32, 16, 2, 2, Wc) == (15, 22)
    # scale 1 is the tile's own cells
    assert footprint(32, 16, 2, 1, 96) == (32, 47)


def test_footprint_wholly_outside_a_smaller_map():
    # a 4 x 5 map under a tile at origin (40, 60): every footprint cell lies beyond it; one edge row / column
    assert footprint(40, 16, 2, 2, 4) == (3, 3)
    assert footprint(60, 16, 2, 2, 5) == (4, 4)
    d_row = np.arange(20, dtype=np.float64).reshape(4, 5)
    d_col = -d_row
    q, valid = tile_prior_np(d_row, d_col, [[40, 60]], 16, 16, 2, 2)
    assert q.tolist() == [[38, -38]] and valid.tolist() == [1]      # cell (3, 4) = 19, times 2


def test_tile_prior_np_median_ties_and_fallback():
    d_row = np.full((8, 16), np.nan)
    d_col = np.full((8, 16), np.nan)
    # tile 0 (cells 0 .. 7 x 0 .. 7 at scale 1, e 0): four usable cells, the lower median is the 2nd
    d_row[0, :4] = [0.25, 0.75, 2.5, -1.0]
    d_col[0, :4] = [1.25, 1.5, 9.0, 1.0]
    d_row[1, 0] = 100.0      # usable in one plane only: left out of both
    # tile 1 (columns 8 .. 15): nothing usable
    q, valid = tile_prior_np(d_row, d_col, [[0, 0], [0, 8]], 8, 8, 0, 1)
    assert valid.tolist() == [1, 0]
    assert q.tolist() == [[0, 1], [0, 1]]      # rint(0.25) = 0, rint(1.25) = 1; tile 1 takes tile 0's
    # scale 2: rint(2 * 0.25) = rint(0.5) = 0 (ties to even), rint(2 * 1.25) = rint(2.5) = 2
    q2, _ = tile_prior_np(d_row, d_col, [[0, 0]], 16, 16, 0, 2)
    assert q2.tolist() == [[0, 2]]
    # no tile has a cell: all zeros
    q0, v0 = tile_prior_np(np.full((4, 4), np.nan), np.zeros((4, 4)), [[0, 0], [8, 8]], 4, 4, 1, 2)
    assert not q0.any() and not v0.any()
    # the fallback is the LOWER median of the measured priors, per component
    d = np.full((4, 16), np.nan)
    for j, v in enumerate((5.0, 1.0, 9.0, 3.0)):
        d[:, 4 * j] = v
    d[:, 12] = np.nan
    q3, v3 = tile_prior_np(d, -d, [[0, 0], [0, 4], [0, 8], [0, 12]], 4, 4, 0, 1)
    assert v3.tolist() == [1, 1, 1, 0] and q3[3].tolist() == [5, -5]
    assert key(np.array([-0.0]))[0] < key(np.array([0.0]))[0] < key(np.array([5e-324]))[0]


def test_pack_np_clamps_at_every_border():
    img = np.arange(30 * 40, dtype=np.uint32).reshape(30, 40).astype(np.uint8)
    org = [[0, 0], [10, 20], [10, 20], [10, 20]]
    prior = [[5, 7], [-100, -100], [3, 2], [1, -2]]
    img2 = img[::-1].copy()
    c1, c2, q_eff = pack_np(img, img2, org, prior, 16, 16, 5)
    assert c1.shape == (4, 20, 20) and np.array_equal(c1[1], img[10:30, 20:40])
    # (0, 0) is the first and (10, 20) the last origin that fits: a prior that points outside has no effect
    assert q_eff.tolist() == [[0, 0], [0, 0], [3, 2], [1, 0]]
    assert np.array_equal(c2[2], img2[7:27, 18:38]) and np.array_equal(c2[3], img2[9:29, 20:40])
    _, _, q2 = pack_np(img, img, [[5, 10]], [[-100, 100]], 16, 16, 5)
    assert q2.tolist() == [[-5, 10]]      # img2's crop at (10, 0)


def test_restated_procedure_on_pair_a():
    """The procedure itself does what it is for (CPU oracle, pair A of the GPU tests): without a prior
    few cells are right; with one coarse level every tile's prior is (0, 12) and every cell of the
    tiles whose crop was not clamped (map columns >= 16) is within 0.5 px in both planes."""
    a, b = stereo_pair(100, 260, seed=7, dx=12, max_disp=12)
    solve = oracle_solve()
    n, org = engine.cut_grid(a.shape, [16, 16], [16, 16], 5)
    m0, _, _ = solve_level_np(a, b, org, np.zeros((len(org), 2), np.int32), 16, 16, 5, None, solve)
    d0 = stitch_planes_np(m0, n, [16, 16])
    assert share_within(d0[1], d0[0], 12, 0) < 0.3
    m, q_eff, _, valid, n, org, priors = coarse_to_fine_np(a, b, [16, 16], [16, 16], 5, 1, 1.0, solve)
    assert np.array_equal(priors[0], np.tile([[0, 12]], (len(org), 1)))
    assert np.array_equal(q_eff[:, 1], np.minimum(org[:, 1], 12))
    d = stitch_planes_np(m, n, [16, 16])
    assert share_within(d[1], d[0], 12, 16) == 1.0


# ---- the library's argument checks (they return before any HIP call) -------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(16)


def test_entry_validation(lib):
    assert lib.dm_downsample2(None, 8, 4, 8, P8, 4, None) == L.DM_ERR_ARG
    assert lib.dm_downsample2(P8, 8, 1, 8, P8, 4, None) == L.DM_ERR_ARG
    assert '2 x 2' in L.last_error()
    assert lib.dm_downsample2(P8, 7, 4, 8, P8, 4, None) == L.DM_ERR_ARG
    assert lib.dm_tile_prior(P8, P8, 4, 4, P8, 1, 4, 4, 1, 3, P8, P8, None) == L.DM_ERR_ARG
    assert 'scale' in L.last_error()
    assert lib.dm_tile_prior(P8, None, 4, 4, P8, 1, 4, 4, 1, 2, P8, P8, None) == L.DM_ERR_ARG
    assert lib.dm_tile_prior(P8, P8, 0, 4, P8, 1, 4, 4, 1, 2, P8, P8, None) == L.DM_ERR_ARG
    assert lib.dm_tile_prior(P8, P8, 4, 4, P8, 1, 4, 4, -1, 2, P8, P8, None) == L.DM_ERR_ARG
    assert lib.dm_pack_tiles(P8, 40, P8, 40, 10, 40, P8, P8, 1, 16, 16, 5, P8, P8, P8, P8, None) == L.DM_ERR_ARG
    assert 'holds no crop' in L.last_error()
    assert lib.dm_pack_tiles(P8, 40, P8, 39, 30, 40, P8, P8, 1, 16, 16, 5, P8, P8, P8, P8, None) == L.DM_ERR_ARG
    assert lib.dm_pack_tiles(P8, 40, P8, 40, 30, 40, P8, P8, 1, 16, 16, 5, ctypes.c_void_p(8), P8, P8, P8,
                             None) == L.DM_ERR_ARG
    assert 'aligned' in L.last_error()
    assert lib.dm_pack_tiles(P8, 40, P8, 40, 30, 40, P8, P8, 0, 16, 16, 5, P8, P8, P8, P8, None) == L.DM_ERR_UNSUPPORTED
    assert lib.dm_shift_matches(P8, None, 1, 4, 4, None) == L.DM_ERR_ARG
    assert lib.dm_shift_matches(P8, P8, 1, 0, 4, None) == L.DM_ERR_ARG
    assert lib.dm_abi_version() == 110      # additive entries


@pytest.mark.parametrize('T,h0,w0,ws', [(1, 16, 16, 5), (12, 16, 16, 5), (48, 16, 16, 5), (7, 3, 50, 1), (64, 128, 128, 5)])
def test_pack_grid(T, h0, w0, ws):
    org, Hp, Wp = engine.pack_grid(T, h0, w0, ws)
    ch, cw = h0 + ws - 1, w0 + ws - 1
    assert org.shape == (T, 2) and Wp % 16 == 0
    assert len({tuple(o) for o in org}) == T and (org[:, 0] % ch == 0).all() and (org[:, 1] % cw == 0).all()
    assert (org[:, 0] + ch).max() == Hp and (org[:, 1] + cw).max() <= Wp < (org[:, 1] + cw).max() + 16
    if (T, h0) == (12, 16):
        assert (Hp, Wp) == (60, 80)      # 4 crops of 20 columns a row, 3 rows


# ---- the keywords ------------------------------------------------------------------------------------
def _pair():
    return stereo_pair(72, 120, seed=3, dx=2)


def test_keywords_default_to_none():
    a, b = _pair()
    s = ImageCutSolver(a, b, [16, 16], [16, 16])
    assert s.prior is None and s.coarse is None and s.prior_map is None and s.prior_valid_map is None


@pytest.mark.parametrize('kw,needle', [
    (dict(prior=(0, 0), coarse=1), 'cannot be combined'),
    (dict(prior=(0, 0), padding=True), 'padding'),
    (dict(coarse=1, padding=True), 'padding'),
    (dict(coarse=0), 'coarse'),
    (dict(coarse=5), 'coarse'),
    (dict(coarse=True), 'coarse'),
    (dict(coarse=1.0), 'coarse'),
    (dict(coarse=(1, -1.0)), 'tol'),
    (dict(coarse=(1, 1.0, 2)), 'coarse'),
    (dict(prior=(0.5, 0)), 'prior'),
    (dict(prior=(0, 0, 0)), 'prior'),
    (dict(prior=np.zeros((5, 2), np.int64)), 'tile order'),
    (dict(prior=np.zeros((3, 4, 4))), 'prior'),
    (dict(prior=(0, 2 ** 31)), 'prior'),
    (dict(prior=(0, 0), merge='feather', consistency=1.0), 'merge'),
    (dict(coarse=1, merge='feather', consistency=1.0), 'merge'),
])
def test_keyword_validation(kw, needle):
    a, b = _pair()
    with pytest.raises(ValueError, match=needle):
        ImageCutSolver(a, b, [16, 16], [16, 16], **kw)


def test_keyword_forms():
    a, b = _pair()      # 3 x 6 tiles
    s = ImageCutSolver(a, b, [16, 16], [16, 16], prior=(1, -2))
    assert s.prior[0] == 'tiles' and s.prior[1].shape == (18, 2) and (s.prior[1] == [1, -2]).all()
    q = np.arange(36).reshape(18, 2)
    s = ImageCutSolver(a, b, [16, 16], [16, 16], prior=q)
    assert s.prior[0] == 'tiles' and np.array_equal(s.prior[1], q)
    s = ImageCutSolver(a, b, [16, 16], [16, 16], prior=np.zeros((2, 48, 96), np.float32))
    assert s.prior[0] == 'dense' and s.prior[1].dtype == np.float64
    assert ImageCutSolver(a, b, [16, 16], [16, 16], coarse=2).coarse == (2, 1.0)
    assert ImageCutSolver(a, b, [16, 16], [16, 16], coarse=(3, 0.5)).coarse == (3, 0.5)


def test_coarse_grids():
    grids = engine.coarse_grids((200, 520), [16, 16], [16, 16], 5, 2)
    assert [g[0] for g in grids] == [[11, 31], [5, 15], [1, 6]]
    with pytest.raises(ValueError, match='no tile at the coarsest level'):
        engine.coarse_grids((100, 260), [16, 16], [16, 16], 5, 3)
    assert len(engine.coarse_grids((100, 260), [16, 16], [16, 16], 5, 1)) == 2


def test_sharding_refuses_the_keywords(monkeypatch):
    a, b = _pair()
    for kw in (dict(prior=(0, 0)), dict(coarse=1)):
        with pytest.raises(ValueError, match='not supported with tile sharding'):
            shard.solve_image_sharded(a, b, [16, 16], [16, 16], 5, L.DM_TM_CCOEFF_NORMED, **kw)
    monkeypatch.setattr(shard, 'tile_sharding_enabled', lambda: True)
    for kw in (dict(prior=(0, 0)), dict(coarse=1)):
        s = ImageCutSolver(a, b, [16, 16], [16, 16], **kw)
        s.log_flg = False
        with pytest.raises(ValueError, match='not supported with tile sharding'):
            s()
