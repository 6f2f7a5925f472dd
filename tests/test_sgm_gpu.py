"""dm_sgm_refine on the device against the restatement of tests/test_sgm_host.py, byte for byte:
both planes, the score and the shift.  The lattice is the smallest shapes at which each part can go
wrong: maps that cross the 32 x 8 tiles both ways and whose diagonals are shorter than a side, every
window-row width (radius 1, 2, 3, 7), every label count, both path counts, penalties from none to
the largest, with and without the sub-pixel step, on maps with rint ties, dead cells inside the
lines, anchors, candidates that are partly or wholly unscored at every image border, and on images
with exact ties and flat windows.
"""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair

import test_guarded_gpu as G
from test_fill_host import raw_bits
from test_sgm_host import (CELLS, OFF, P1, P2, R, S_, q1024, sgm_costs, sgm_restate, sgm_solve, step_scene, weak_solved,
                           wrong)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (37, 1), (9, 33), (33, 9)]
RADII = [1, 2, 3, 7]
PENALTIES = [(0.0, 0.0), (0.25, 1.0), (2.0, 8.0), (16.0, 16.0)]
KINDS = ['stereo', 'binary', 'stripes', 'checker', 'const']


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def images(kind, Hi, Wi, seed):
    if kind == 'stereo':
        return stereo_pair(Hi, Wi, seed=seed, dx=2)
    return content_pair(kind, Hi, Wi, seed)


def lattice_case(H, W, r, s, kind, seed):
    """(img1, img2, d_row, d_col, (oy, ox), mask).  The image leaves r rows above the first cell's window and one
    column more on the left (oy != ox), r + 1 below and on the right: with disparities around (0, 2) of up to 2.5
    pixels and s candidates a side, cells near each border have candidates partly and wholly unscored.  The planes:
    multiples of 1/4 (exact halves: rint ties), -0.0, a NaN with a payload, +-inf islands (dead cells inside lines),
    one row of cells so far off that none of its candidates is scored, and one cell at the limit 2^30."""
    oy, ox = r, r + 1
    Hi, Wi = H + oy + r + 1, W + ox + r + 1
    a, b = images(kind, Hi, Wi, seed)
    rng = np.random.default_rng(1000 * H + 10 * W + r + seed)
    dr = rng.integers(-10, 11, (H, W)) / 4.0
    dc = 2.0 + rng.integers(-10, 11, (H, W)) / 4.0
    u = rng.uniform(size=(H, W))
    dr[u < 0.06] = -0.0
    dc[(u > 0.06) & (u < 0.10)] = np.inf
    dr[(u > 0.10) & (u < 0.13)] = -np.inf
    dc.view(np.uint64)[(u > 0.13) & (u < 0.16)] = 0x7ff8000000000123
    dr.view(np.uint64)[(u > 0.16) & (u < 0.18)] = 0xfff8000000000001
    if H > 4:
        dr[H // 2, :] = 1000.0                 # no candidate of this row of cells is scored
        dc[H // 2 + 1, W // 2] = -1.5e9        # beyond 2^30: dead
        dc[H // 2 - 1, W // 2] = float(ox + W // 2 - 2 ** 30)      # px = 2^30 exactly: alive, unscored
    if H * W > 1:
        dr[0, W - 1], dc[0, W - 1] = 0.5, 2.5
        dr[H - 1, 0], dc[H - 1, 0] = -0.5, 1.5
    mask = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
    return a, b, np.ascontiguousarray(dr), np.ascontiguousarray(dc), (oy, ox), mask


def strided(img, pad=5):
    """The image as a device view whose row stride is above its width."""
    t = torch.zeros((img.shape[0], img.shape[1] + pad), dtype=torch.uint8, device='cuda')
    t[:, :img.shape[1]] = torch.from_numpy(img).cuda()
    return t[:, :img.shape[1]]


def device(a, b, dr, dc, r, s, p1, p2, paths, off, subpix, mask, pad=5, **kw):
    ta, tb = (strided(a, pad), strided(b, pad + 2)) if pad else (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    m = None if mask is None else torch.from_numpy(mask).cuda()
    return engine.sgm_refine(ta, tb, torch.from_numpy(dr).cuda(), torch.from_numpy(dc).cuda(), r, s, p1, p2, paths=paths,
                             offset=off, subpix=subpix, mask=m, **kw)


def host(t):
    return [x.cpu().numpy() for x in t]


def assert_equal(got, want, what):
    assert raw_bits(got[0], want[0]), '%s: the row plane differs' % (what,)
    assert raw_bits(got[1], want[1]), '%s: the column plane differs' % (what,)
    assert raw_bits(got[2], want[2]), '%s: the score differs' % (what,)
    assert got[3].dtype == np.int8 and np.array_equal(got[3], want[3]), '%s: the shift differs' % (what,)


_COSTS = {}


def costs_of(H, W, r, s, kind, seed, masked):
    """The lattice case and the restatement's costs (rules 1 and 2), computed once per key."""
    key = (H, W, r, s, kind, seed, masked)
    if key not in _COSTS:
        a, b, dr, dc, off, mask = lattice_case(H, W, r, s, kind, seed)
        mask = mask if masked else None
        _COSTS[key] = (a, b, dr, dc, off, mask, sgm_costs(a, b, dr, dc, r, s, off, mask))
    return _COSTS[key]


def check(H, W, r, s, paths, pen, subpix, kind, masked, seed=0):
    a, b, dr, dc, off, mask, costs = costs_of(H, W, r, s, kind, seed, masked)
    want = sgm_solve(costs, dr, dc, q1024(pen[0]), q1024(pen[1]), paths, subpix)
    got = host(device(a, b, dr, dc, r, s, pen[0], pen[1], paths, off, subpix, mask, return_score=True, return_shift=True))
    assert_equal(got, want, (H, W, r, s, paths, pen, subpix, kind, masked))
    return costs, want


# every shape with every radius; the other settings cycle so that each value meets each shape and each radius
SHAPE_CASES = [(shape, r, 1 + (i + j) % 3, (4, 8)[(i + j) % 2], PENALTIES[(i + 2 * j) % 4], bool((i + j // 2) % 2),
                KINDS[(i + j) % 5], bool((i + j) % 3))
               for i, shape in enumerate(SHAPES) for j, r in enumerate(RADII)]
# one shape and radius with every search, path count and penalty (the costs are shared)
SETTING_CASES = [((9, 33), 2, s, paths, pen, bool((s + k) % 2), 'stereo', True)
                 for s in (1, 2, 3) for paths in (4, 8) for k, pen in enumerate(PENALTIES)]
# every content kind with the largest label count on the shape with the longest diagonals
KIND_CASES = [((33, 9), 3, 3, 8, PENALTIES[1 + k % 3], bool(k % 2), kind, bool(k % 2)) for k, kind in enumerate(KINDS)]


def _id(c):
    return '%dx%d-r%d-s%d-p%d-%g_%g-%s-%s-%s' % (c[0] + (c[1], c[2], c[3]) + c[4] + ('sub' if c[5] else 'int', c[6],
                                                                                    'mask' if c[7] else 'all'))


@pytest.mark.parametrize('c', SHAPE_CASES + SETTING_CASES + KIND_CASES, ids=_id)
def test_kernel_equals_restatement(c):
    (H, W), r, s, paths, pen, subpix, kind, masked = c
    costs, want = check(H, W, r, s, paths, pen, subpix, kind, masked)
    if (H, W) == (9, 33) and kind == 'stereo':      # the lattice holds what its docstring says
        st = costs['state']
        assert (st == 0).any() and (st == 2).any() and (not masked or (st == 1).any())
        free = st == 2
        nsc = costs['scored'].sum(axis=2)
        assert (nsc[free] == 0).any() and ((nsc[free] > 0) & (nsc[free] < (2 * s + 1) ** 2)).any()
        assert (nsc[free] == (2 * s + 1) ** 2).any() and not costs['scored'][H // 2].any()
        if pen[0] > 0:
            assert want[3].any()


def test_lattice_covers_the_settings():
    cases = SHAPE_CASES + SETTING_CASES + KIND_CASES
    assert {c[0] for c in cases} == set(SHAPES) and {c[1] for c in cases} >= set(RADII)
    assert {(c[2], c[3]) for c in cases} == {(s, p) for s in (1, 2, 3) for p in (4, 8)}
    assert {c[4] for c in cases} == set(PENALTIES) and {c[5] for c in cases} == {True, False}
    assert {c[6] for c in cases} == set(KINDS) and {c[7] for c in cases} == {True, False}
    for shape in SHAPES:
        assert {c[1] for c in cases if c[0] == shape} >= set(RADII)


def tile_edge_case(r, s):
    """(img1, img2, d_row, d_col, (oy, ox), mask): 9 x 33 cells -- one past the 8-row and the 32-column tile -- on
    a 24 x 48 image.  The offset r - 1 puts the img1 windows of the first row and column of cells one pixel outside
    the image (a 15-pixel window leaves no room to do the same at the other end: 24 = 9 + 15, 48 = 33 + 15), so the
    last row and column of cells claim the position Hi - r - 1 / Wi - r - 1 instead: their img2 windows leave the
    image for every label but those with a negative step, and with s = 1 the last column scores one label a row
    (at radius 1 the 3-byte row).  One cell is NaN; the mask holds both values."""
    H, W, Hi, Wi = 9, 33, 24, 48
    oy = ox = r - 1
    a, b = stereo_pair(Hi, Wi, seed=10 * r + s, dx=2)
    rng = np.random.default_rng(100 * r + s)
    dr = rng.integers(-6, 7, (H, W)) / 4.0
    dc = 2.0 + rng.integers(-6, 7, (H, W)) / 4.0
    dr[H - 1, :] = float(oy + H - 1 - (Hi - r - 1))
    dc[:, W - 1] = float(ox + W - 1 - (Wi - r - 1))
    dr[4, 16] = np.nan
    mask = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
    assert mask.min() == 0 and mask.max() == 1
    return a, b, np.ascontiguousarray(dr), np.ascontiguousarray(dc), (oy, ox), mask


@pytest.mark.parametrize('s', [1, 2, 3])
@pytest.mark.parametrize('r', [1, 2, 4, 7])
def test_every_cost_kernel_instance(r, s):
    """Every (dwords per window row, label count) instance of k_sgm_cost -- radius 4 is the three-dword row, which
    RADII has not -- on a map that crosses the tile edges by one cell, from images that are views of row stride 64."""
    a, b, dr, dc, off, mask = tile_edge_case(r, s)
    costs = sgm_costs(a, b, dr, dc, r, s, off, mask)
    free, nsc = costs['state'] == 2, costs['scored'].sum(axis=2)
    assert (costs['state'] == 0).sum() == 1 and (costs['state'] == 1).any()      # the NaN cell, the anchors
    assert not costs['scored'][0].any() and not costs['scored'][:, 0].any()       # the img1 window leaves the image
    for edge in (np.s_[-1, :], np.s_[:, -1]):                                     # some labels' img2 windows do
        assert (nsc[edge][free[edge]] <= s * (2 * s + 1)).all() and (nsc[edge][free[edge]] > 0).any()
    assert (nsc[1:-1, 1:-1][free[1:-1, 1:-1]] == (2 * s + 1) ** 2).any()
    want = sgm_solve(costs, dr, dc, q1024(0.25), q1024(1.0), 8, True)
    ta, tb = strided(a, 16), strided(b, 16)
    assert ta.stride(0) == tb.stride(0) == 64 and tuple(ta.shape) == (24, 48)
    got = host(engine.sgm_refine(ta, tb, torch.from_numpy(dr).cuda(), torch.from_numpy(dc).cuda(), r, s, 0.25, 1.0, paths=8,
                                 offset=off, subpix=True, mask=torch.from_numpy(mask).cuda(), return_score=True,
                                 return_shift=True))
    assert_equal(got, want, (r, s))


# ---------------------------------------------------------------------------------------------
# cross-checks
# ---------------------------------------------------------------------------------------------
def _plain():
    H, W, r, s = 9, 33, 2, 2
    a, b, dr, dc, off, mask = lattice_case(H, W, r, s, 'stereo', 3)
    return a, b, dr, dc, off, mask, r, s


def test_zero_penalties_score_is_the_photo_score():
    """p1 = p2 = 0: the score of a moved cell is engine.photo_score at the output's integer disparity."""
    a, b, dr, dc, off, mask, r, s = _plain()
    row, col, score, shift = device(a, b, dr, dc, r, s, 0.0, 0.0, 8, off, False, None, return_score=True,
                                    return_shift=True)
    photo = engine.photo_score(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), row, col, r, offset=off)
    moved = shift.any(dim=0).cpu().numpy()
    assert moved.sum() > 20
    assert raw_bits(score.cpu().numpy()[moved], photo.cpu().numpy()[moved])
    assert (row.cpu().numpy()[moved] % 1 == 0).all() and (col.cpu().numpy()[moved] % 1 == 0).all()


def test_runs_aliasing_outputs_and_streams_agree():
    a, b, dr, dc, off, mask, r, s = _plain()
    args = (r, s, 0.25, 1.0)
    every = dict(return_score=True, return_shift=True)
    ref = host(device(a, b, dr, dc, *args, 8, off, True, mask, **every))
    assert ref[3].any()
    assert_equal(host(device(a, b, dr, dc, *args, 8, off, True, mask, **every)), ref, 'second run')
    assert_equal(host(device(a, b, dr, dc, *args, 8, off, True, mask, pad=0, **every)), ref, 'contiguous images')
    # the outputs are the inputs
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    tr, tc, tm = torch.from_numpy(dr).cuda(), torch.from_numpy(dc).cuda(), torch.from_numpy(mask).cuda()
    out = engine.sgm_refine(ta, tb, tr, tc, *args, offset=off, mask=tm, out=(tr, tc), **every)
    assert out[0].data_ptr() == tr.data_ptr() and out[1].data_ptr() == tc.data_ptr()
    assert_equal(host(out), ref, 'aliased')
    # crossed: the row output over the column input
    tr, tc = torch.from_numpy(dr).cuda(), torch.from_numpy(dc).cuda()
    out = engine.sgm_refine(ta, tb, tr, tc, *args, offset=off, mask=tm, out=(tc, tr), **every)
    assert_equal(host(out), ref, 'crossed')
    # without the optional outputs
    tr, tc = torch.from_numpy(dr).cuda(), torch.from_numpy(dc).cuda()
    two = engine.sgm_refine(ta, tb, tr, tc, *args, offset=off, mask=tm)
    assert len(two) == 2 and raw_bits(two[0].cpu().numpy(), ref[0]) and raw_bits(two[1].cpu().numpy(), ref[1])
    one = engine.sgm_refine(ta, tb, tr, tc, *args, offset=off, mask=tm, return_shift=True)
    assert len(one) == 3 and np.array_equal(one[2].cpu().numpy(), ref[3]) and raw_bits(one[0].cpu().numpy(), ref[0])
    # a bool mask, a non-default stream
    st = torch.cuda.Stream()
    got = engine.sgm_refine(ta, tb, tr, tc, *args, offset=off, mask=tm.bool(), stream=st, **every)
    st.synchronize()
    assert_equal(host(got), ref, 'stream')
    assert raw_bits(tr.cpu().numpy(), dr) and raw_bits(tc.cpu().numpy(), dc)      # the inputs are not written


def test_python_surface_rejects():
    a, b, dr, dc, off, mask, r, s = _plain()
    ta, tb, tr, tc = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(dr).cuda(), \
        torch.from_numpy(dc).cuda()
    for kw in (dict(paths=5), dict(mask=torch.ones((9, 32), dtype=torch.uint8, device='cuda')), dict(out=(tr,)),
               dict(out=(tr, tc.float())), dict(offset=(1, 2, 3))):
        with pytest.raises(ValueError):
            engine.sgm_refine(ta, tb, tr, tc, r, s, 1.0, 2.0, **kw)
    for bad in ((0, s, 1.0, 2.0), (r, 4, 1.0, 2.0), (r, s, 2.0, 1.0), (r, s, 1.0, 17.0)):
        with pytest.raises(ValueError):
            engine.sgm_refine(ta, tb, tr, tc, *bad)
    with pytest.raises(ValueError):
        engine.sgm_refine(ta, tb[:, 1:], tr, tc, r, s, 1.0, 2.0)
    e = torch.empty((0, 5), dtype=torch.float64, device='cuda')
    assert tuple(engine.sgm_refine(ta, tb, e, e, r, s, 1.0, 2.0)[0].shape) == (0, 5)


def test_weak_scene_on_the_device():
    """The weak scene of tests/test_sgm_host.py: the device equals the restatement, so its conditions hold there."""
    a, b, dr, dc, inside, single, agg = weak_solved(1)
    for (p1, p2), want in (((0.0, 0.0), single), ((2.0, 8.0), agg)):
        got = host(device(a, b, dr, dc, R, S_, p1, p2, 8, OFF, False, None, return_score=True, return_shift=True))
        assert_equal(got, want, 'weak scene %r' % ((p1, p2),))
    w1, w8 = int(wrong(single, 0.0, 2.0)[inside].sum()), int(wrong(got, 0.0, 2.0)[inside].sum())
    assert w1 >= 100 and w8 <= w1 / 10.0


def test_step_scene_on_the_device():
    a, b, dr, dc, truth, xc = step_scene(0)
    got = host(device(a, b, dr, dc, R, S_, 2.0, 8.0, 8, OFF, False, None, return_score=True, return_shift=True))
    assert_equal(got, sgm_restate(a, b, dr, dc, R, S_, P1, P2, 8, OFF, False), 'step scene')
    cols = np.arange(CELLS) + OFF
    outside = np.broadcast_to((cols < xc - R - 2) | (cols > xc + R + 5), (CELLS, CELLS))
    assert not wrong(got, 0.0, truth)[outside].any()


# ---------------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------------
GEOM = dict(image_size=[32, 32], stride=[32, 32], window_size=5, degree_map_mode=['elevation', 'elevation2'])
SGM, REFINE, LSM = (2, 2, 2.0, 8.0), (2, 1, 0.0), (2, 2, 1.0)


def test_solver_equals_the_stages_one_by_one():
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = G.corrupted_pair()
    modes = GEOM['degree_map_mode']
    base = ImageCutSolver(a, b, consistency=1.0, fill=16, **GEOM)
    base.log_flg = False
    d_map, out_map, err, holes = [t.clone() for t in base._execute_matching_device()]
    assert int(holes.sum()) > 50
    full = ImageCutSolver(a, b, consistency=1.0, fill=16, sgm=SGM, sgm_where='filled', refine=REFINE, lsm=LSM, **GEOM)
    full.log_flg = False
    res = full._execute_matching_device()
    assert full.chain.names(1.0, None) == ['d_map', 'out_map', 'err', 'holes', 'sgm_score', 'sgm_shift', 'refine_score',
                                          'refine_shift', 'lsm_score', 'lsm_status']
    d = d_map.clone()
    d, sscore, sshift = engine.sgm_stage(a, b, d, modes, engine.sgm_params(SGM), 2, holes)
    d, rscore, rshift = engine.refine_stage(a, b, d, modes, REFINE, 2, holes)
    d, lscore, lstatus = engine.lsm_stage(a, b, d, modes, LSM, 2, None)
    want = (d, out_map, err, holes, sscore, sshift, rscore, rshift, lscore, lstatus)
    assert len(res) == len(want)
    for name, g, w in zip(full.chain.names(1.0, None), res, want):
        assert g.dtype == w.dtype and raw_bits(g.double().cpu().numpy(), w.double().cpu().numpy()), name
    assert sshift.any() and not sshift[:, ~(holes[0] | holes[1]).bool()].any()      # only filled cells move
    # the attributes
    full()
    assert full.sgm_score_map.dtype == np.float64 and full.sgm_score_map.shape == (64, 64)
    assert full.sgm_shift_map.dtype == np.int8 and full.sgm_shift_map.shape == (2, 64, 64)
    assert raw_bits(full.sgm_score_map, sscore.cpu().numpy()) and np.array_equal(full.sgm_shift_map, sshift.cpu().numpy())
    assert raw_bits(full.d_map, d.cpu().numpy())
    # sgm=None: today's tuple
    none = ImageCutSolver(a, b, consistency=1.0, fill=16, sgm=None, **GEOM)
    none.log_flg = False
    got = none._execute_matching_device()
    assert len(got) == 4
    for g, w in zip(got, (d_map, out_map, err, holes)):
        assert g.dtype == w.dtype and raw_bits(g.double().cpu().numpy(), w.double().cpu().numpy())
    none()
    assert none.sgm_score_map is None and none.sgm_shift_map is None


# ---------------------------------------------------------------------------------------------
# the guarded case (tests/test_guarded_gpu.py's harness; not registered in its CASES, which are held
# against include/dmstereo.h: tests/test_sgm_host.py holds this one against include/dmstereo_sgm.h)
# ---------------------------------------------------------------------------------------------
def guarded_inputs(H, W, r):
    """Images cut so that the outermost img1 windows touch all four borders: the last byte of img1 is the last a
    window reads; img2's windows end one row and column earlier (rule 2)."""
    a, b = stereo_pair(H + 2 * r, W + 2 * r, seed=H + W + r, dx=1)
    rng = np.random.default_rng(H + r)
    dr = rng.integers(-6, 7, (H, W)) / 4.0
    dc = 1.0 + rng.integers(-6, 7, (H, W)) / 4.0
    dr[rng.uniform(size=(H, W)) < 0.05] = np.nan
    dc[rng.uniform(size=(H, W)) < 0.05] = -np.inf
    dr[0, 0] = -0.0
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    return a, b, dr, dc, (r, r), mask


def _guarded(x):
    every = dict(return_score=True, return_shift=True)
    for (H, W), r, s, paths in (((33, 31), 1, 3, 8), ((9, 40), 3, 2, 4), ((12, 35), 7, 1, 8)):
        a, b, dr, dc, off, mask = guarded_inputs(H, W, r)
        ta, tb = x.inp(a), x.inp(b)
        assert not x.g or (ta.data_ptr() % 2 == 1 and ta.stride(0) == a.shape[1])
        tag = '%dx%d r%d s%d' % (H, W, r, s)
        x.add(tag, engine.sgm_refine(ta, tb, x.inp(dr), x.inp(dc), r, s, 0.5, 2.0, paths=paths, offset=off, **every))
        x.add(tag + ' mask', engine.sgm_refine(ta, tb, x.inp(dr), x.inp(dc), r, s, 2.0, 8.0, paths=paths, offset=off,
                                               subpix=False, mask=x.inp(mask), out=(x.out(dr.shape), x.out(dr.shape)),
                                               **every))
        tr, tc = x.inout(dr), x.inout(dc)      # the outputs are the inputs
        x.add(tag + ' aliased', engine.sgm_refine(ta, tb, tr, tc, r, s, 0.5, 2.0, paths=paths, offset=off,
                                                  mask=x.inp(mask), out=(tr, tc), **every))
        x.add(tag + ' no outputs', engine.sgm_refine(ta, tb, x.inp(dr), x.inp(dc), r, s, 0.0, 0.0, paths=paths,
                                                     offset=off))


GUARDED_CASE = G.Case('sgm_refine', ('dm_sgm_refine',), _guarded, None)


def test_guarded_sgm(monkeypatch):
    """Guarded buffers, exact workspace (engine._workspace asks for dm_sgm_bytes and the guarded allocator gives
    exactly that), two poisons: nothing outside the buffers is written, no input is written, and the results equal
    the ordinary run's byte for byte."""
    G.run_case(GUARDED_CASE, monkeypatch)
