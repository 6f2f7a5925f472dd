"""Disparity priors on the device where the product uses them (tests/test_prior_lattice.py has the cases
and the host side; every restatement is test_prior.py's, test_fb_host.py's or test_merge_host.py's):

  1. a two-axis prior per tile through every level kernel class of the solve (LATTICE), against the
     CPU oracle of the packed crop pairs by test_shape_lattice's rule (pinned pow, bit for bit), with
     consistency= against fb_restate of the device's own two directions; the volume kernels, which the
     solve never launches, on the packed pair through dm_corr_volume_ex, one entry per volume key; a
     zero and a known prior at the production tile sizes S = 64 and 128;
  2. solve_tiles_prior's chunk loop against the unchunked call;
  3. every stitch branch of ImageCutSolver with a prior that differs from tile to tile on both axes;
  4. coarse-to-fine on pairs displaced along both axes, stage by stage and end to end;
  5. the branches of csrc/dm_prior.hip that no other test runs, and the four entries on a side stream.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import chain, engine
from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver

from test_fb_host import _host_stitch, fb_restate, place, same_bits
from test_merge_host import merge_restate
from test_prior import downsample2_np, pack_np, shift_np, stitch_planes_np, tile_prior_np
from test_prior_lattice import (CONSISTENCY_CASES, LATTICE, MARGIN, ORIGINS, ROWS, assert_two_axis_clamps, free_share,
                                lattice_T, prior_case, restated, two_axis_pair)
from test_shape_lattice import _same, dispatch_key, oracle_tile

pytestmark = pytest.mark.gpu

METHOD = L.DM_TM_CCOEFF_NORMED
MODES = ['elevation', 'elevation2']
Q30 = 2 ** 30


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.fixture
def pinned_pow():
    """test_shape_lattice's pow mode, for one test: the oracle is back on 'libm', the mode every other test
    of the suite (and test_prior_lattice.restated) computes under, when the test ends."""
    from oracle import oracle as O
    O.set_pow_mode('pinned')
    yield
    O.set_pow_mode('libm')


# ---- 1. priors through every kernel instance class -------------------------------------------------------
@pytest.mark.parametrize('h0,w0,ws', LATTICE, ids=str)
def test_solve_tiles_prior_lattice(h0, w0, ws, pinned_pow):
    img1, img2, org, prior = prior_case(h0, w0, ws)
    T = len(org)
    c1, c2, q_ref = pack_np(img1, img2, org, prior, h0, w0, ws)
    assert_two_axis_clamps(prior, q_ref)
    local = np.stack([oracle_tile(a, b, 0, 0, h0, w0, ws, METHOD)[1] for a, b in zip(c1, c2)])
    match, q_eff = engine.solve_tiles_prior(img1, img2, org, prior, h0, w0, ws, METHOD)
    assert np.array_equal(host(q_eff), q_ref)
    _same(host(match), shift_np(local, q_ref))
    if (h0, w0, ws) not in CONSISTENCY_CASES:
        return
    m, qe, err = engine.solve_tiles_prior(img1, img2, org, prior, h0, w0, ws, METHOD, consistency=1.0)
    p1, p2, _, _ = engine.pack_tiles(img1, img2, org, prior, h0, w0, ws)
    fwd, bwd = engine.solve_tiles_bidir(p1, p2, engine.pack_grid(T, h0, w0, ws)[0], h0, w0, ws, METHOD)
    _same(host(fwd), local)
    e_ref, m_ref = fb_restate(host(fwd), host(bwd), 1.0)
    kept = e_ref <= 1.0
    assert kept.any() and not kept.all()      # the check keeps some cells and rejects some
    assert np.array_equal(host(qe), q_ref)
    assert same_bits(host(err), e_ref)
    assert same_bits(host(m), shift_np(m_ref, q_ref))


# The solve never launches a volume kernel (the level kernel leaves min / max behind and matching re-derives
# level 0), so the packed pair reaches them only through dm_corr_volume_ex: one entry per volume key.
VOLUME_CASES = [c for i, c in enumerate(LATTICE) if dispatch_key(*c)[1] not in [dispatch_key(*d)[1] for d in LATTICE[:i]]]


@pytest.mark.parametrize('h0,w0,ws', VOLUME_CASES, ids=str)
def test_volume_of_packed_pair_vs_oracle(h0, w0, ws, pinned_pow):
    """The level-0 volume kernels on pack_tiles' output at pack_grid's origins, as
    test_shape_lattice.test_volume_lattice_vs_oracle runs them on a plain pair: float32 == the oracle's
    level 0 of pack_np's crop pairs, binary16 == np.float16 of it, and the min/max-known calls after the
    level kernel == the standalone ones."""
    from oracle import oracle as O
    img1, img2, org, prior = prior_case(h0, w0, ws)
    T, P = len(org), h0 * w0
    c1, c2, q_ref = pack_np(img1, img2, org, prior, h0, w0, ws)
    assert_two_axis_clamps(prior, q_ref)
    p1, p2, _, _ = engine.pack_tiles(img1, img2, org, prior, h0, w0, ws)
    batch = engine.TileBatch(p1, p2, engine.pack_grid(T, h0, w0, ws)[0], h0, w0, ws, METHOD)
    lib = L.load()
    v32 = torch.empty((T, P, P), dtype=torch.float32, device='cuda')
    v16 = torch.empty((T, P, P), dtype=torch.float16, device='cuda')
    fresh = engine.DevicePyramid(batch, build=False).compute_stats()
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh.stats), 0, L.ptr(v32), L.stream_handle()))
    fresh16 = engine.DevicePyramid(batch, build=False).compute_stats()      # sweeps for its own min / max
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh16.stats), L.DM_VOLUME_F16, L.ptr(v16), L.stream_handle()))
    r32, r16 = host(v32), host(v16)
    for t in range(T):
        l0 = O.corr_l0(c1[t], c2[t], ws, 'cv2.TM_CCOEFF_NORMED').reshape(P, P)
        _same(r32[t], l0)
        _same(r16[t], l0.astype(np.float16))
    pyr = engine.DevicePyramid(batch, fuse_level2=2)
    assert pyr._have_minmax
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN, L.ptr(v32), L.stream_handle()))
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN | L.DM_VOLUME_F16, L.ptr(v16),
                                  L.stream_handle()))
    _same(host(v32), r32)
    _same(host(v16), r16)


@pytest.mark.parametrize('S', [64, 128])
def test_prior_at_production_tile_sizes(S):
    dy, dx = -6, 10
    a, b = two_axis_pair(S + 4 + 8, 2 * S + 4 + 12, dy, dx, seed=S)
    org = np.array([[1, 11], [1, 11 + S]])      # two tiles side by side whose img2 crops at o - q lie inside
    opts = (S, S, 5, METHOD)
    # (a) a zero prior
    plain = host(engine.solve_tiles(a, b, org, *opts))
    zero, q0 = engine.solve_tiles_prior(a, b, org, np.zeros((2, 2), np.int64), *opts)
    assert same_bits(host(zero), plain) and not host(q0).any()
    # (b) the true prior: the crops of img2 are those of img1, byte for byte
    q = np.tile([[dy, dx]], (2, 1))
    p1, p2, _, qe = engine.pack_tiles(a, b, org, q, S, S, 5)
    assert np.array_equal(host(qe), q) and torch.equal(p1, p2) and p1.any()
    ref = host(engine.solve_tiles(a, a, org, *opts))
    assert not same_bits(ref, plain)
    assert same_bits(host(engine.solve_tiles(p1, p2, engine.pack_grid(2, S, S, 5)[0], *opts)), ref)
    m, qe = engine.solve_tiles_prior(a, b, org, q, *opts)
    assert np.array_equal(host(qe), q) and same_bits(host(m), shift_np(ref, q))


# ---- 2. the chunk loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tol', [None, 1.0])
def test_solve_tiles_prior_chunked(tol):
    img1, img2, org, prior = prior_case(16, 32, 5, T=7)
    q_ref = pack_np(img1, img2, org, prior, 16, 32, 5)[2]
    assert_two_axis_clamps(prior, q_ref)
    whole = engine.solve_tiles_prior(img1, img2, org, prior, 16, 32, 5, METHOD, consistency=tol)
    parts = engine.solve_tiles_prior(img1, img2, org, prior, 16, 32, 5, METHOD, consistency=tol,
                                     mem_budget=3 * engine.tile_bytes(16, 32))
    assert len(whole) == len(parts) == (2 if tol is None else 3)
    assert np.array_equal(host(whole[1]), q_ref) and np.array_equal(host(parts[1]), q_ref)
    assert same_bits(host(parts[0]), host(whole[0]))
    if tol is not None:
        assert same_bits(host(parts[2]), host(whole[2]))
        kept = host(whole[2]) <= tol
        assert kept.any() and not kept.all()


# ---- 3. ImageCutSolver with a prior that differs from tile to tile ----------------------------------------
SIZE3, STRIDE3 = [16, 32], [8, 16]
GEOM3 = dict(image_size=SIZE3, stride=STRIDE3, window_size=5, degree_map_mode=MODES)


def run(a, b, **kw):
    s = ImageCutSolver(a, b, **kw)
    s.log_flg = False
    s()
    return s


@pytest.fixture(scope='module')
def case3():
    """The pair, the priors, the device's own tiles (one direction, and checked at 1 px) and the plain
    solver's maps; computed once, read by every test of this section."""
    a, b = two_axis_pair(90, 180, -6, 10)
    n, org = engine.cut_grid(a.shape, SIZE3, STRIDE3, 5)
    assert n == [8, 9]
    T = len(org)
    prior = np.array([[-6, 10]]) + np.random.default_rng(3).integers(-2, 3, size=(T, 2))
    assert len(np.unique(prior[:, 0])) > 2 and len(np.unique(prior[:, 1])) > 2
    q_ref = pack_np(a, b, org, prior, 16, 32, 5)[2]
    assert (q_ref != prior).any() and (q_ref == prior).all(axis=1).any()      # clamped tiles and free ones
    s = ImageCutSolver(a, b, **GEOM3)
    opts = (s.sub_pix, s.filtering, s.filtering_window_size, s.filtering_num, s.filtering_mode)
    tiles, q_eff = engine.solve_tiles_prior(a, b, org, prior, 16, 32, 5, METHOD, *opts)
    tiles_c, q_eff_c, err = engine.solve_tiles_prior(a, b, org, prior, 16, 32, 5, METHOD, *opts, consistency=1.0)
    assert np.array_equal(host(q_eff), q_ref) and np.array_equal(host(q_eff_c), q_ref)
    return dict(a=a, b=b, n=n, org=org, prior=prior, q_ref=q_ref, tiles=host(tiles), tiles_c=host(tiles_c),
                err=host(err), plain=run(a, b, **GEOM3, prior=prior))


def test_solver_prior_plain(case3):
    c, s = case3, case3['plain']
    d, out = _host_stitch(c['tiles'], c['n'], 16, 32, STRIDE3, MODES)
    assert s.d_map.shape == d.shape == (2, 72, 160)
    assert same_bits(s.d_map, d) and same_bits(s.out_map, out)
    n0, n1 = c['n']
    want = np.array([[c['q_ref'][j * n0 + i] for j in range(n1)] for i in range(n0)])
    assert s.prior_map.shape == (n0, n1, 2) and np.array_equal(s.prior_map, want)
    assert s.prior_valid_map.shape == (n0, n1) and s.prior_valid_map.all()
    # the prior did its work: a free tile's prior is at most 2 px off on either axis, which leaves about
    # (1 - 2/16) (1 - 2/32) = 0.82 of its cells a match inside the crop (1 - |d| / S)
    free = (c['q_ref'] == c['prior']).all(axis=1)
    assert free_share(d[1], d[0], free, c['n'], STRIDE3, 16, 32, -6, 10) > 0.5


def test_solver_prior_consistency(case3):
    c = case3
    s = run(c['a'], c['b'], **GEOM3, prior=c['prior'], consistency=1.0)
    d, out = _host_stitch(c['tiles_c'], c['n'], 16, 32, STRIDE3, MODES)
    assert same_bits(s.d_map, d) and same_bits(s.out_map, out)
    assert same_bits(s.consistency_map, place(c['err'], c['n'], STRIDE3))
    assert np.array_equal(s.prior_map, case3['plain'].prior_map)
    # every cell is covered, and the stitch keeps the last tile that covers it: a cell it rejected has an
    # error above the tolerance or none
    hole = np.isnan(s.d_map).any(axis=0)
    assert hole.any() and not hole.all()
    assert not (s.consistency_map[hole] <= 1.0).any()
    assert (s.consistency_map[~hole] <= 1.0).all()


@pytest.mark.parametrize('rule,min_count', [('last', 1), ('center', 1), ('feather', 2), ('median', 1)])
def test_solver_prior_merge(case3, rule, min_count):
    c = case3
    s = run(c['a'], c['b'], **GEOM3, prior=c['prior'], merge=rule, merge_min_count=min_count)
    d, out, err, spread, count = merge_restate(c['tiles'], None, c['n'], STRIDE3, MODES, None, rule, min_count)
    assert err is None and s.consistency_map is None and count.max() == 4
    assert same_bits(s.d_map, d) and same_bits(s.out_map, out) and same_bits(s.spread_map, spread)
    assert s.coverage_map.dtype == np.uint8 and np.array_equal(s.coverage_map, count)
    assert np.array_equal(s.prior_map, case3['plain'].prior_map)
    if rule == 'last':
        assert same_bits(s.d_map, case3['plain'].d_map)


def test_solver_prior_chain(case3):
    """The chain runs once, on the level-0 map, after the stitch of the shifted tiles."""
    c, plain = case3, case3['plain']
    s = run(c['a'], c['b'], **GEOM3, prior=c['prior'], median=1, fill=16)
    got = chain.Chain(MODES, fill=16, median=1).run((dev(plain.d_map), dev(plain.out_map)), c['a'], c['b'], 2, None, None)
    assert len(got) == 3
    assert same_bits(s.d_map, host(got[0])) and same_bits(s.out_map, host(got[1]))
    assert s.hole_map.dtype == bool and np.array_equal(s.hole_map, host(got[2]).astype(bool))
    assert not same_bits(s.d_map, plain.d_map)      # the median moved something


# ---- 4. coarse to fine along both axes --------------------------------------------------------------------
def test_two_axis_coarse_stage_by_stage():
    """Row 2 ([16, 32] tiles, an MFMA shape): every stage against the restatement applied to the device's own
    output of the stage before, as test_prior_gpu.test_coarse_one_stage_by_stage does on one axis."""
    _, (dy, dx), k, size, stride = ROWS[2][:5]
    h0, w0 = size
    r = restated(2)
    a, b = r['img1'].copy(), r['img2'].copy()      # (the shared reference is read-only)
    trace = []
    match, q_eff, err, valid, n, org = engine.solve_coarse_to_fine(a, b, size, stride, 5, METHOD, k, trace=trace)
    assert [t['level'] for t in trace] == [1, 0] and err is None and n == r['n'] and np.array_equal(org, r['origins'])
    top, fine = trace
    # the half-resolution pair and its grid
    a1, b1 = host(top['img1']), host(top['img2'])
    assert np.array_equal(a1, downsample2_np(a)) and np.array_equal(b1, downsample2_np(b))
    n1, org1 = engine.cut_grid(a1.shape, size, stride, 5)
    assert top['n'] == n1 and np.array_equal(top['origins'], org1)
    assert not host(top['prior']).any() and not host(top['q_eff']).any()
    # the coarse level: both directions of its packed pair, checked in the local frames, then shifted (by 0)
    p1, p2, _, _ = engine.pack_tiles(a1, b1, org1, top['prior'], h0, w0, 5)
    fwd, bwd = engine.solve_tiles_bidir(p1, p2, engine.pack_grid(len(org1), h0, w0, 5)[0], h0, w0, 5, METHOD)
    e_ref, m_ref = fb_restate(host(fwd), host(bwd), 1.0)
    assert same_bits(host(top['match']), shift_np(m_ref, host(top['q_eff'])))
    assert same_bits(host(top['err']), e_ref)
    # its masked matches stitched in ('elevation2', 'elevation')
    d1 = host(top['d_map'])
    assert same_bits(d1, stitch_planes_np(host(top['match']), n1, stride))
    # the coarse maps -> the priors of level 0, non-zero on both axes
    q_ref, v_ref = tile_prior_np(d1[0], d1[1], org, h0, w0, 2, 2)
    assert np.array_equal(host(fine['prior']), q_ref) and np.array_equal(host(valid), v_ref)
    assert (q_ref == (dy, dx)).all(axis=1).mean() == ROWS[2][6] == 1.0      # as in the restatement: every prior exact
    assert (q_ref[:, 0] < 0).any() and (q_ref[:, 1] > 0).any()
    # the priors -> the packed crops of level 0
    p1, p2, _, qe = engine.pack_tiles(a, b, org, fine['prior'], h0, w0, 5)
    c1, c2, qe_ref = pack_np(a, b, org, q_ref, h0, w0, 5)
    grid = engine.pack_grid(len(org), h0, w0, 5)[0]
    x1, x2 = host(p1), host(p2)
    ch, cw = h0 + 4, w0 + 4
    assert all(np.array_equal(x1[y:y + ch, x:x + cw], c1[t]) and np.array_equal(x2[y:y + ch, x:x + cw], c2[t])
               for t, (y, x) in enumerate(grid))
    assert np.array_equal(host(qe), qe_ref) and np.array_equal(host(q_eff), qe_ref)
    # the local matches of the packed pair -> the shifted matches
    local = host(engine.solve_tiles(p1, p2, grid, h0, w0, 5, METHOD))
    assert same_bits(host(match), shift_np(local, qe_ref))


@pytest.mark.parametrize('row', [2, 3])
def test_two_axis_coarse_end_to_end(row):
    """Measured shares are printed before they are asserted (DESIGN.md section 4m records them)."""
    _, (dy, dx), k, size, stride = ROWS[row][:5]
    h0, w0 = size
    r = restated(row)
    a, b, n = r['img1'].copy(), r['img2'].copy(), r['n']
    ref_share = free_share(r['d'][0], r['d'][1], r['free'], n, stride, h0, w0, dy, dx)
    geom = dict(image_size=size, stride=stride, window_size=5, degree_map_mode=MODES)
    s = run(a, b, **geom, coarse=k)
    q = s.prior_map.transpose(1, 0, 2).reshape(-1, 2)      # tile order: t = j n0 + i
    free = (q == (dy, dx)).all(axis=1)
    share = free_share(s.d_map[1], s.d_map[0], free, n, stride, h0, w0, dy, dx)
    plain = run(a, b, **geom)
    share0 = free_share(plain.d_map[1], plain.d_map[0], free, n, stride, h0, w0, dy, dx)
    print('row %d: free tiles restatement %.4f, device %.4f; share within 0.5 px over the free tiles: restatement '
          '%.4f, device %.4f, without coarse= %.4f' % (row, r['free'].mean(), free.mean(), ref_share, share, share0))
    assert share >= ref_share - 0.01
    assert share0 < 0.4
    assert (s.prior_map[..., 0].T.ravel()[r['free']] == dy).all()      # on the restatement's free tiles
    assert (q[free] == (dy, dx)).all() and free.mean() >= r['free'].mean() - 0.01


# ---- 5. kernel branches of dm_prior.hip -------------------------------------------------------------------
def fallback_case(kind):
    """600 tiles of 4 x 4 cells on planes of 80 x 120 (scale 1, e 0: a tile's footprint is its own cells).
    'even' / 'odd': about a third of the tiles have no usable cell, the number of the others is even / odd;
    'single': one tile measures."""
    rng = np.random.default_rng(17)
    org = np.array([(4 * (t // 30), 4 * (t % 30)) for t in range(600)])
    d_row = rng.integers(-160, 161, size=(80, 120)) * 0.25
    d_col = rng.integers(-160, 161, size=(80, 120)) * 0.25
    hole = rng.random(600) < 1 / 3
    hole[[3, 255, 256, 300, 511, 512, 550, 599]] = True
    hole[[0, 257, 598]] = False
    if kind == 'single':
        hole[:] = True
        hole[400] = False
    elif (600 - hole.sum()) % 2 != (0 if kind == 'even' else 1):
        hole[1] = not hole[1]
    for t in np.flatnonzero(hole):
        y, x = org[t]
        if t % 3 == 0:      # one plane only, or both: unusable either way
            d_row[y:y + 4, x:x + 4] = np.nan
        elif t % 3 == 1:
            d_col[y:y + 4, x:x + 4] = np.inf
        else:
            d_row[y:y + 4, x:x + 4] = -np.inf
            d_col[y:y + 4, x:x + 4] = np.nan
    return d_row, d_col, org, hole


@pytest.mark.parametrize('kind', ['even', 'odd', 'single'])
def test_prior_fallback_over_600_tiles(kind):
    d_row, d_col, org, hole = fallback_case(kind)
    q_ref, v_ref = tile_prior_np(d_row, d_col, org, 4, 4, 0, 1)
    assert np.array_equal(v_ref == 0, hole)
    measured = int(v_ref.sum())
    assert measured == 1 if kind == 'single' else measured % 2 == (0 if kind == 'even' else 1) and 350 < measured < 450
    assert hole[:256].any() and hole[256:512].any() and hole[512:].any()
    own = q_ref[v_ref == 1]
    if kind != 'single':
        assert (own > 0).any(axis=0).all() and (own < 0).any(axis=0).all()
    assert q_ref[3].any() and (q_ref[hole] == q_ref[3]).all()      # one fallback value, not zero
    q, valid = engine.tile_prior(dev(d_row), dev(d_col), org, 4, 4, 0, scale=1)
    assert np.array_equal(host(valid), v_ref) and np.array_equal(host(q), q_ref)


def test_tile_prior_clamp_and_pack_at_the_clamp():
    org = [[0, 0]]
    big = dev(np.full((4, 4), 1e300)), dev(np.full((4, 4), -1e300))
    for scale in (1, 2):
        q, valid = engine.tile_prior(big[0], big[1], org, 4, 4, 0, scale=scale)
        assert host(q).tolist() == [[Q30, -Q30]] and host(valid).tolist() == [1]
        assert np.array_equal(host(q), tile_prior_np(host(big[0]), host(big[1]), org, 4, 4, 0, scale)[0])
    half = np.full((4, 4), 2.0 ** 29 + 0.25)
    for scale, want in ((2, Q30), (1, 2 ** 29)):      # rint(2^30 + 0.5) = 2^30 (ties to even); rint(2^29 + 0.25) = 2^29
        q, _ = engine.tile_prior(dev(half), dev(-half), org, 4, 4, 0, scale=scale)
        assert host(q).tolist() == [[want, -want]]
        assert np.array_equal(host(q), tile_prior_np(half, -half, org, 4, 4, 0, scale)[0])
    # priors of +-2^30 on the device: every crop is clamped to a border
    rng = np.random.default_rng(4)
    img1 = rng.integers(0, 256, size=(30, 40)).astype(np.uint8)
    img2 = rng.integers(0, 256, size=(30, 40)).astype(np.uint8)
    torg = np.array([[5, 10], [5, 10], [0, 0], [10, 20], [3, 7]])
    prior = np.array([[Q30, -Q30], [-Q30, Q30], [Q30, Q30], [-Q30, -Q30], [-Q30, 3]])
    p1, p2, _, q_eff = engine.pack_tiles(img1, img2, torg, dev(prior.astype(np.int32)), 16, 16, 5)
    c1, c2, q_ref = pack_np(img1, img2, torg, prior, 16, 16, 5)
    assert q_ref.tolist() == [[5, -10], [-5, 10], [0, 0], [0, 0], [-7, 3]]
    assert np.array_equal(host(q_eff), q_ref)
    check_packed(host(p1), host(p2), c1, c2, 5, 16, 16, 5)


def check_packed(a1, a2, c1, c2, T, h0, w0, ws):
    """The packed pair against pack_np's crops: every crop in its place, everything else zero."""
    grid, Hp, Wp = engine.pack_grid(T, h0, w0, ws)
    ch, cw = h0 + ws - 1, w0 + ws - 1
    assert a1.shape == a2.shape == (Hp, Wp)
    rest1, rest2 = a1.copy(), a2.copy()
    for t, (y, x) in enumerate(grid):
        assert np.array_equal(a1[y:y + ch, x:x + cw], c1[t]), t
        assert np.array_equal(a2[y:y + ch, x:x + cw], c2[t]), t
        rest1[y:y + ch, x:x + cw] = 0
        rest2[y:y + ch, x:x + cw] = 0
    assert not rest1.any() and not rest2.any()
    return grid


def downsample_buffer():
    """A (36, 48) image with the value edges in its first blocks: saturated, and sums of 4 k + 2 (the
    rounding adds 2 and floors, so 4 k + 2 goes up)."""
    a = np.random.default_rng(6).integers(0, 256, size=(36, 48)).astype(np.uint8)
    a[0:2, 0:2] = 255                        # 1020 -> 255
    a[0:2, 2:4] = [[255, 255], [255, 253]]   # 1018 = 4 * 254 + 2 -> 255
    a[0:2, 4:6] = [[1, 1], [0, 0]]           # 2 -> 1
    a[0:2, 6:8] = [[0, 1], [2, 3]]           # 6 -> 2
    a[0:2, 8:10] = [[0, 1], [0, 0]]          # 1 -> 0
    a[2:4, 0:2] = [[255, 255], [255, 254]]   # 1019 -> 255
    a[2:4, 30:32] = 255                      # the last block of the vector path's first 32 source bytes
    a[32:34, 30:32] = [[7, 8], [9, 10]]      # 34 = 4 * 8 + 2 -> 9, in the last destination row
    return a


def vector_path(t, out_w):
    """dm_downsample2's own rule for the 16-byte path, on the source view (the destination is a fresh
    contiguous tensor of out_w columns)."""
    return out_w % 16 == 0 and t.data_ptr() % 16 == 0 and t.stride(0) % 16 == 0


def test_downsample2_paths():
    a = downsample_buffer()
    buf = dev(a)
    assert buf.data_ptr() % 16 == 0 and buf.stride(0) == 48
    assert downsample2_np(a)[0, :5].tolist() == [255, 255, 1, 2, 0] and downsample2_np(a)[1, 0] == 255
    # a view with odd H and W on the vector path: Wd = 16, base and stride multiples of 16
    view = buf[:35, :33]
    assert vector_path(view, 16) and not view.is_contiguous()
    out = engine.downsample2(view)
    assert tuple(out.shape) == (17, 16) and out.data_ptr() % 16 == 0
    assert np.array_equal(host(out), downsample2_np(a[:35, :33]))
    assert host(out)[16, 15] == 9
    # the same view one column to the right: the base is no multiple of 16, the byte path
    shifted = buf[:35, 1:34]
    assert not vector_path(shifted, 16) and shifted.stride(0) == 48
    assert np.array_equal(host(engine.downsample2(shifted)), downsample2_np(a[:35, 1:34]))
    # contiguous (10, 33): Wd = 16 but a stride of 33, the byte path
    c = np.ascontiguousarray(a[:10, 2:35])
    t = dev(c)
    assert t.stride(0) == 33 and not vector_path(t, 16)
    assert np.array_equal(host(engine.downsample2(t)), downsample2_np(c))
    # the whole buffer (Wd = 24: the byte path) and its left 32 columns as a view (the vector path)
    assert np.array_equal(host(engine.downsample2(buf)), downsample2_np(a))
    assert vector_path(buf[:, :32], 16)
    assert np.array_equal(host(engine.downsample2(buf[:, :32])), downsample2_np(a[:, :32]))


def offset_tiles(m):
    """The tiles m [T][3][h][w] as a contiguous device view that starts 8 bytes off a 16-byte boundary, with
    a guard double before and after it -> (view, the whole buffer)."""
    base = torch.full((m.size + 2,), 3.25, dtype=torch.float64, device='cuda')
    assert base.data_ptr() % 16 == 0
    view = base[1:-1].view(m.shape)
    view.copy_(dev(m))
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view, base


@pytest.mark.parametrize('shape', [(3, 3, 4, 6), (1, 3, 4, 6), (1, 3, 3, 5), (2, 3, 2, 1)])
def test_shift_matches_scalar_path_and_T1(shape):
    """An even number of cells at a pointer that is no multiple of 16 takes the scalar path; T = 1 on both."""
    rng = np.random.default_rng(sum(shape))
    m = rng.normal(size=shape) * 10
    m[0, 0, 1, 0] = np.nan
    m[-1, 1, 0, 0] = -np.inf
    q = rng.integers(-50, 51, size=(shape[0], 2)).astype(np.int32)
    q[0] = (-7, 9)
    want = shift_np(m, q)
    view, base = offset_tiles(m)
    out = engine.shift_matches(view, dev(q))
    assert out.data_ptr() == view.data_ptr()
    assert same_bits(host(out), want) and same_bits(host(out)[:, 2], m[:, 2])
    assert host(base)[[0, -1]].tolist() == [3.25, 3.25]      # nothing written outside the tiles
    assert same_bits(host(engine.shift_matches(dev(m), dev(q))), want)      # aligned: the vector path if P is even


def test_shift_matches_at_the_clamp():
    """Priors of +-2^30 on values near 1: one rounding of the difference, as numpy's."""
    rng = np.random.default_rng(12)
    m = 1.0 + rng.normal(size=(2, 3, 4, 6)) * 1e-3
    m[0, 1, 0, 0], m[1, 0, 0, 0] = 1.0 + 2.0 ** -23, 0.5 + 2.0 ** -24      # above 2^30 a double's ulp is 2^-22: a tie, and below one
    q = np.array([[Q30, -Q30], [-Q30, Q30]], dtype=np.int32)
    want = shift_np(m, q)
    for k in ((0, 1, 0, 0), (1, 0, 0, 0)):      # the exact difference is no double: it is rounded, once
        assert Fraction(float(want[k])) != Fraction(float(m[k])) + Q30
    for t in (dev(m), offset_tiles(m)[0]):
        assert same_bits(host(engine.shift_matches(t, dev(q))), want)


PACK_SHAPES = [(16, 32, 5), (32, 16, 3), (7, 50, 1), (8, 32, 15)]


@pytest.mark.parametrize('one', [True, False], ids=['T1', 'ragged'])
@pytest.mark.parametrize('h0,w0,ws', PACK_SHAPES, ids=str)
def test_pack_tiles_shapes_and_views(h0, w0, ws, one):
    """h0 != w0, ws 1 and 15, T = 1 and a grid whose last row is partly filled; the images are device views with
    different row strides that start at odd bytes; two-axis priors that clamp at all four borders."""
    T = 1 if one else lattice_T(h0, w0, ws)
    ch, cw = h0 + ws - 1, w0 + ws - 1
    H, W = ch + MARGIN[0], cw + MARGIN[1]
    rng = np.random.default_rng(100 * h0 + w0 + ws + T)
    big1 = rng.integers(1, 256, size=(H + 3, W + 9)).astype(np.uint8)      # no zero: the filler is told from a crop
    big2 = rng.integers(1, 256, size=(H + 5, W + 22)).astype(np.uint8)
    img1, img2 = big1[2:2 + H, 3:3 + W], big2[2:2 + H, 5:5 + W]
    v1, v2 = dev(big1)[2:2 + H, 3:3 + W], dev(big2)[2:2 + H, 5:5 + W]
    assert v1.stride(0) != v2.stride(0) and v1.data_ptr() % 2 == 1 and v2.data_ptr() % 2 == 1
    org = np.array(ORIGINS[1:2] if one else ORIGINS[:T], dtype=np.int64)      # T = 1: the tile at (3, 7)
    sign = rng.choice([-1, 1], size=(T, 2))
    if not one:
        sign[0], sign[3] = 1, -1
    prior = rng.integers(1, 4, size=(T, 2)) * sign
    c1, c2, q_ref = pack_np(img1, img2, org, prior, h0, w0, ws)
    if one:
        assert np.array_equal(q_ref, prior) and prior.all()      # not clamped: the crop of img2 really moves
    else:
        assert_two_axis_clamps(prior, q_ref)
    p1, p2, porg, q_eff = engine.pack_tiles(v1, v2, org, prior, h0, w0, ws)
    assert p1.is_contiguous() and p2.is_contiguous()
    assert np.array_equal(host(q_eff), q_ref)
    grid = check_packed(host(p1), host(p2), c1, c2, T, h0, w0, ws)
    assert np.array_equal(host(porg), grid)
    if not one:      # the grid is ragged: there is filler below the first row's crops
        rows = grid[:, 0] // ch
        assert rows.max() >= 1 and (rows == rows.max()).sum() < (rows == 0).sum()
    b = engine.TileBatch(p1, p2, grid, h0, w0, ws, METHOD)      # the solver's own checks accept the packed pair
    assert b.T == T and b.img1.data_ptr() == p1.data_ptr() and b.img2.data_ptr() == p2.data_ptr()


# ---- the four entries on a side stream ----------------------------------------------------------------------
@pytest.fixture
def side():
    """A side stream, with the default stream kept busy by a large copy that has nothing to do with the
    entry's data: the inputs are complete (a device-wide synchronize) before the copy is queued."""
    big = torch.empty(1 << 29, dtype=torch.uint8, device='cuda')
    other = torch.empty_like(big)
    s = torch.cuda.Stream()

    def start():
        torch.cuda.synchronize()
        other.copy_(big, non_blocking=True)
        return s
    yield start
    torch.cuda.synchronize()


def test_downsample2_side_stream(side):
    a = downsample_buffer()
    view = dev(a)[:35, :33]
    s = side()
    out = engine.downsample2(view, stream=s)
    s.synchronize()
    assert np.array_equal(host(out), downsample2_np(a[:35, :33]))


def test_tile_prior_side_stream(side):
    d_row, d_col, org, _ = fallback_case('odd')
    q_ref, v_ref = tile_prior_np(d_row, d_col, org, 4, 4, 0, 1)
    r, c, o = dev(d_row), dev(d_col), dev(org.astype(np.int32))
    s = side()
    q, valid = engine.tile_prior(r, c, o, 4, 4, 0, scale=1, stream=s)
    s.synchronize()
    assert np.array_equal(host(q), q_ref) and np.array_equal(host(valid), v_ref)


def test_pack_tiles_side_stream(side):
    img1, img2, org, prior = prior_case(16, 32, 5, T=7)
    c1, c2, q_ref = pack_np(img1, img2, org, prior, 16, 32, 5)
    a, b, q = dev(img1), dev(img2), dev(prior.astype(np.int32))
    s = side()
    p1, p2, porg, q_eff = engine.pack_tiles(a, b, org, q, 16, 32, 5, stream=s)
    s.synchronize()
    assert np.array_equal(host(q_eff), q_ref)
    assert np.array_equal(host(porg), check_packed(host(p1), host(p2), c1, c2, 7, 16, 32, 5))


def test_shift_matches_side_stream(side):
    rng = np.random.default_rng(21)
    m = rng.normal(size=(5, 3, 16, 32)) * 10
    q = rng.integers(-50, 51, size=(5, 2)).astype(np.int32)
    t, qd = dev(m), dev(q)
    s = side()
    out = engine.shift_matches(t, qd, stream=s)
    s.synchronize()
    assert same_bits(host(out), shift_np(m, q))
