"""Affine least-squares matching on the GPU: dm_lsm_affine (engine.lsm_affine) against the restatement of
the definition (tests/test_lsm_affine_host.py: lsm_affine_fast, pinned there to the plain-loop
lsm_affine_restate) bit for bit -- both planes, the score, the status and the four affine planes -- over
maps smaller and larger than one 32 x 8 workgroup tile whose last tile row and column are partial, radius
2, 3, 5 and 7 with 1 and 8 steps, images just large enough and with a wide margin, disparities near the
truth, integers, fractions of both signs, -0.0, positions on each image border and past it, NaN, +-inf and
+-1e300; offsets of both signs that push cells out of the image; a shear bound that ends cells at -2; with
and without mask; ramps along both axes with both signs of the slope and of the disparity; row-strided
images, in place and out of place, every optional pointer omitted in turn, a side stream, run-to-run
equality, guarded buffers, the argument errors, and the ImageCutSolver / solve_image_sharded keyword end to
end."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import content_pair, ramp_pair, stereo_pair

import test_guarded_gpu as G
from test_fill_host import raw_bits, same_bits
from test_lsm_affine_host import all_bits5, central, lsm_affine_fast, lsm_affine_restate, ramp_case, rms_at
from test_lsm_gpu import border_planes
from test_photo_host import NAN

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 33), (9, 31), (17, 65)]
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']
EVERY = dict(return_score=True, return_status=True, return_affine=True)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


_REF = {}


def case(shape, r, margin):
    """(img1, img2, d_row, d_col, offset, mask), made once per case.  The largest shape has a flat block in img1
    (cells without a pivot) and one in img2 (cells whose samples have no variance)."""
    key = (shape, r, margin)
    if key not in _REF:
        H, W = shape
        m = r + 1 if margin == 'tight' else r + 9
        oy, ox = m, m + 1
        a, b = stereo_pair(H + 2 * m, W + 2 * m + 2, seed=H + W + r, dx=1)
        if shape == (17, 65):
            a, b = a.copy(), b.copy()
            a[m + 2:m + 2 + 2 * r + 5, m + 8:m + 8 + 2 * r + 6] = 9
            b[m + 1:m + 1 + 2 * r + 8, m + 40:m + 40 + 2 * r + 8] = 200
        dr, dc = border_planes(H, W, a.shape[0], a.shape[1], r, oy, ox)
        mask = (np.random.default_rng(H * W + r).uniform(size=(H, W)) < 0.6).astype(np.uint8)
        _REF[key] = (a, b, dr, dc, (oy, ox), mask)
    return _REF[key]


def want(c, r, iters, max_move=1.0, max_shear=0.5, mask=False):
    a, b, dr, dc, off, m = c
    key = ('want', id(c), r, iters, max_move, max_shear, mask)
    if key not in _REF:
        _REF[key] = lsm_affine_fast(a, b, dr, dc, r, iters, off, max_move, max_shear, m if mask else None)
    return _REF[key]


def run(a, b, dr, dc, r, iters, off, max_move=1.0, max_shear=0.5, mask=None, **kw):
    got = engine.lsm_affine(a if torch.is_tensor(a) else dev(a), b if torch.is_tensor(b) else dev(b), dev(dr), dev(dc),
                            r, iters, offset=off, max_move=max_move, max_shear=max_shear, mask=dev(mask), **EVERY, **kw)
    assert [g.dtype for g in got] == [torch.float64] * 3 + [torch.int8, torch.float64]
    assert tuple(got[4].shape) == (4,) + tuple(np.shape(dr))
    return [host(g) for g in got]


VARIANTS = [dict(), dict(max_move=0.25, mask=True), dict(max_move=2.0, max_shear=0.03)]


def check(shape, r, iters, margin, variants=VARIANTS):
    c = case(shape, r, margin)
    a, b, dr, dc, off, mask = c
    for v in variants:
        w = want(c, r, iters, **v)
        got = run(a, b, dr, dc, r, iters, off, v.get('max_move', 1.0), v.get('max_shear', 0.5),
                  mask if v.get('mask') else None)
        assert all_bits5(got, w), (shape, r, iters, margin, v)
        kept = w[3] != iters
        assert raw_bits(got[0][kept], dr[kept]) and raw_bits(got[1][kept], dc[kept])      # NaN payloads, -0.0: copied
    return c


# ---------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('margin', ['tight', 'wide'])
@pytest.mark.parametrize('iters', [1, 8])
@pytest.mark.parametrize('r', [2, 3, 5, 7])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda v: '%dx%d' % v)
def test_against_restatement(shape, r, iters, margin):
    c = check(shape, r, iters, margin, VARIANTS if r < 7 else VARIANTS[:2])
    if shape == (17, 65) and margin == 'wide':
        w = want(c, r, iters)
        seen = set(np.unique(w[3]).tolist())
        assert seen >= {-2, -1, 0, iters}, seen      # a path that is never taken must not pass silently
        assert (w[3] == iters).mean() > 0.1
        assert ((w[3] == -1) & np.isnan(w[2])).any()                   # -1 from a pivot


def test_fast_restatement_is_the_literal_one_here():
    c = case((7, 33), 2, 'tight')
    a, b, dr, dc, off, mask = c
    sl = (slice(0, 7), slice(0, 6))
    lit = lsm_affine_restate(a, b, dr[sl], dc[sl], 2, 2, off)
    w = want(c, 2, 2)
    assert all_bits5(lit, [w[0][sl], w[1][sl], w[2][sl], w[3][sl], w[4][(slice(None),) + sl]])


@pytest.mark.parametrize('off', [(-3, 2), (4, -6), (30, 3), (3, 60)], ids=str)
def test_offsets_of_both_signs(off):
    """A map that hangs over the image on one side: the cells outside and in the halo rule's border are skipped
    (status 0), cells whose start lies outside end at -2, the rest are matched."""
    H, W, r = 17, 40, 3
    a, b = stereo_pair(36, 70, seed=11, dx=1)
    rng = np.random.default_rng(5)
    dr, dc = rng.uniform(-0.6, 0.6, (H, W)), 1.0 + rng.uniform(-0.6, 0.6, (H, W))
    dr[::3, ::4] += 9.0      # starts far off: outside the image near the border
    w = lsm_affine_fast(a, b, dr, dc, r, 3, off)
    assert all_bits5(run(a, b, dr, dc, r, 3, off), w)
    assert {0, -2, 3} <= set(np.unique(w[3]).tolist())


@pytest.mark.parametrize('kind', ['binary', 'dark_bright', 'checker', 'const', 'identical'])
def test_content_classes(kind):
    """The largest moments, at radius 7, and the classes where nothing may move."""
    H, W, r = 9, 37, 7
    m = r + 4
    a, b = content_pair(kind, H + 2 * m, W + 2 * m, 3)
    rng = np.random.default_rng(1)
    shift = 1.0 if kind == 'checker' else (0.0 if kind in ('identical', 'const') else 3.0)
    for dr, dc in ((np.zeros((H, W)), np.full((H, W), shift)),
                   (rng.uniform(-0.7, 0.7, (H, W)), shift + rng.uniform(-0.7, 0.7, (H, W)))):
        w = lsm_affine_fast(a, b, dr, dc, r, 2, m)
        assert all_bits5(run(a, b, dr, dc, r, 2, m), w)
        if kind == 'const':
            assert (w[3] == -1).all() and np.isnan(w[2]).all()
    if kind == 'identical':
        z = np.zeros((H, W))
        w = lsm_affine_fast(a, b, z, z, r, 2, m)
        assert not (w[3] == 2).any() and all_bits5(run(a, b, z, z, r, 2, m), w)


@pytest.mark.parametrize('d0', [2.0, -2.0])
@pytest.mark.parametrize('axis,g', [(1, 0.2), (0, 0.2), (1, -0.15), (0, -0.15)])
def test_ramps_on_both_axes(axis, g, d0):
    """ramp_pair along the columns and along the rows, both signs of the slope and of the disparity: the
    restatement's bits, hence its accuracy; the shear bound ends the cells of the ramp at -2."""
    a, b, sr, sc, tr, tc = ramp_case(3, g, axis, d0=d0, size=44)
    w = lsm_affine_fast(a, b, sr, sc, 5, 6)
    got = run(a, b, sr, sc, 5, 6, 0)
    assert all_bits5(got, w)
    sel = central(got[3], axis)
    acc = sel & (got[3] == 6)
    stretch = float(np.median(got[4][0 if axis == 1 else 3][acc]))
    e = rms_at(got[0], got[1], tr, tc, sel)
    print('axis %d g %+.2f d0 %+.0f: rms %.4f px, accepted %.3f, stretch %+.4f (truth %+.4f)'
          % (axis, g, d0, e, acc.sum() / sel.sum(), stretch, -g / (1 + g)))
    assert acc.sum() > 0.95 * sel.sum() and e < 0.05 and abs(stretch + g / (1 + g)) < 0.01
    ps = host(engine.photo_score(a, b, dev(sr), dev(sc), 5))
    ok = got[3] == 6
    rest = ~ok & ~np.isnan(got[2])
    assert (got[2][ok] > ps[ok]).all() and raw_bits(got[2][rest], ps[rest])
    tight = run(a, b, sr, sc, 5, 6, 0, max_shear=0.05)
    assert all_bits5(tight, lsm_affine_fast(a, b, sr, sc, 5, 6, 0, 1.0, 0.05))
    assert (tight[3][acc] == -2).all() and raw_bits(tight[0][acc], sr[acc]) and raw_bits(tight[2][acc], ps[acc])


def test_identical_windows_never_move():
    c = case((9, 31), 3, 'wide')
    a, b, dr, dc, off, mask = c
    z, one = np.zeros((9, 31)), np.ones((9, 31))
    z[4, 5] = -0.0
    got = run(a, b, z, one, 3, 4, off)
    assert (got[3] == -3).all() and (got[2] == 1.0).all() and raw_bits(got[0], z) and raw_bits(got[1], one)
    assert np.isnan(got[4]).all()


# ---------------------------------------------------------------------------------------------
# 2. the calling forms
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def strided():
    """img1 and img2 as views, with different row strides, into wider device tensors."""
    a, b = case((17, 65), 2, 'wide')[:2]
    Hi, Wi = a.shape
    wa = torch.full((Hi + 2, Wi + 13), 77, dtype=torch.uint8, device='cuda')
    wb = torch.full((Hi + 3, Wi + 30), 99, dtype=torch.uint8, device='cuda')
    wa[1:1 + Hi, 5:5 + Wi] = dev(a)
    wb[2:2 + Hi, 3:3 + Wi] = dev(b)
    va, vb = wa[1:1 + Hi, 5:5 + Wi], wb[2:2 + Hi, 3:3 + Wi]
    assert va.stride(0) != vb.stride(0) and not va.is_contiguous() and not vb.is_contiguous()
    return va, vb


def test_strided_images_and_host_images(strided):
    c = case((17, 65), 2, 'wide')
    a, b, dr, dc, off, mask = c
    va, vb = strided
    w = want(c, 2, 3)
    assert all_bits5(run(va, vb, dr, dc, 2, 3, off), w)
    assert all_bits5(run(va, b, dr, dc, 2, 3, off), w)
    assert all_bits5(run(torch.from_numpy(a), dev(np.ascontiguousarray(b.T)).T, dr, dc, 2, 3, off), w)
    got = engine.lsm_affine(a, b, dev(dr), dev(dc), 2, 3, offset=off, mask=dev(mask.astype(bool)))
    wm = want(c, 2, 3, mask=True)
    assert len(got) == 2 and raw_bits(host(got[0]), wm[0]) and raw_bits(host(got[1]), wm[1])


def test_in_place_and_out_of_place(strided):
    """out=(d_row, d_col) works in place, and the planes may be planes of one d_map: the solver's call."""
    c = case((17, 65), 2, 'wide')
    a, b, dr, dc, off, mask = c
    va, vb = strided
    w = want(c, 2, 3)
    m = dev(np.stack([dc, dr]))
    res = engine.lsm_affine(va, vb, m[1], m[0], 2, 3, offset=off, out=(m[1], m[0]), return_affine=True)
    assert res[0].data_ptr() == m[1].data_ptr() and res[1].data_ptr() == m[0].data_ptr()
    assert raw_bits(host(m[1]), w[0]) and raw_bits(host(m[0]), w[1]) and raw_bits(host(res[2]), w[4])
    tr, tc = dev(dr), dev(dc)
    o = (torch.zeros((17, 65), dtype=torch.float64, device='cuda'), torch.zeros((17, 65), dtype=torch.float64, device='cuda'))
    res = engine.lsm_affine(va, vb, tr, tc, 2, 3, offset=off, out=o, return_score=True)
    assert res[0] is o[0] and res[1] is o[1] and raw_bits(host(o[0]), w[0]) and raw_bits(host(o[1]), w[1])
    assert raw_bits(host(res[2]), w[2]) and raw_bits(host(tr), dr) and raw_bits(host(tc), dc)      # the inputs are left alone
    d, score, status, aff = engine.lsm_affine_stage(a, b, dev(np.stack([dc, dr])), ['elevation', 'elevation2'],
                                                    (2, 3, 1.0, 0.5), off)
    assert raw_bits(host(d), np.stack([w[1], w[0]])) and raw_bits(host(score), w[2])
    assert np.array_equal(host(status), w[3]) and raw_bits(host(aff), w[4])


def test_side_stream_and_run_to_run():
    c = case((17, 65), 3, 'wide')
    a, b, dr, dc, off, mask = c
    w = want(c, 3, 8)
    first = run(a, b, dr, dc, 3, 8, off)
    assert all_bits5(first, w)
    for _ in range(3):
        assert all_bits5(run(a, b, dr, dc, 3, 8, off), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ta, tb, tr, tc = dev(a), dev(b), dev(dr), dev(dc)
    torch.cuda.synchronize()
    got = engine.lsm_affine(ta, tb, tr, tc, 3, 8, offset=off, stream=side, **EVERY)
    side.synchronize()
    assert all_bits5([host(g) for g in got], w)


def test_every_optional_pointer_omitted_in_turn():
    """The C entry with each NULL-able pointer NULL in turn: the others are what they were."""
    c = case((9, 31), 3, 'tight')
    a, b, dr, dc, off, mask = c
    lib = L.load()
    ta, tb, tr, tc, tm = dev(a), dev(b), dev(dr), dev(dc), dev(mask)
    work = torch.empty(lib.dm_lsm_affine_bytes(a.shape[0], a.shape[1], 9, 31, 3, 2), dtype=torch.uint8, device='cuda')
    names = ('mask', 'score', 'status', 'affine')
    for give in (names,) + tuple(tuple(n for n in names if n != drop) for drop in names) + ((),):
        o_row = torch.full((9, 31), 5.0, dtype=torch.float64, device='cuda')
        o_col = torch.full((9, 31), 5.0, dtype=torch.float64, device='cuda')
        score = torch.full((9, 31), 5.0, dtype=torch.float64, device='cuda')
        status = torch.full((9, 31), 5, dtype=torch.int8, device='cuda')
        aff = torch.full((4, 9, 31), 5.0, dtype=torch.float64, device='cuda')
        L.check(lib.dm_lsm_affine(L.ptr(ta), ta.stride(0), L.ptr(tb), tb.stride(0), a.shape[0], a.shape[1], L.ptr(tr),
                                  L.ptr(tc), 9, 31, off[0], off[1], 3, 2, 1.0, 0.5, 0,
                                  L.ptr(tm if 'mask' in give else None), L.ptr(o_row), L.ptr(o_col),
                                  L.ptr(score if 'score' in give else None), L.ptr(status if 'status' in give else None),
                                  L.ptr(aff if 'affine' in give else None), L.ptr(work), L.stream_handle()),
                'dm_lsm_affine')
        torch.cuda.synchronize()
        w = want(c, 3, 2, mask='mask' in give)
        assert raw_bits(host(o_row), w[0]) and raw_bits(host(o_col), w[1]), give
        assert raw_bits(host(score), w[2]) if 'score' in give else bool((score == 5).all()), give
        assert np.array_equal(host(status), w[3]) if 'status' in give else bool((status == 5).all()), give
        assert raw_bits(host(aff), w[4]) if 'affine' in give else bool((aff == 5).all()), give


def test_argument_errors():
    a, b = stereo_pair(20, 24, seed=1, dx=1)
    d = torch.zeros((5, 7), dtype=torch.float64, device='cuda')
    for bad in (dict(radius=1), dict(radius=8), dict(radius=2.0), dict(iters=0), dict(iters=9), dict(offset=(1, 2, 3)),
                dict(offset=1.5), dict(max_move=0.0), dict(max_move=2.5), dict(max_move=NAN), dict(max_shear=0.0),
                dict(max_shear=1.0), dict(max_shear=NAN), dict(max_shear='0.5'), dict(mask=d),
                dict(mask=torch.ones((7, 5), dtype=torch.uint8, device='cuda')), dict(out=d), dict(out=(d,)),
                dict(out=(d, d.float())), dict(out=(d, d[:4]))):
        kw = dict(radius=2, iters=1, offset=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.lsm_affine(a, b, d, d, kw.pop('radius'), kw.pop('iters'), **kw)
    for args in ((a, b, d.cpu(), d), (a, b, d, d.float()), (a, b, d, d[:4]), (a.astype(np.float64), b, d, d),
                 (a, b[:, :20], d, d)):
        with pytest.raises(ValueError):
            engine.lsm_affine(*args, 2, 1)
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    got = engine.lsm_affine(a, b, e, e, 2, 1, **EVERY)
    assert [tuple(g.shape) for g in got] == [(0, 7)] * 4 + [(4, 0, 7)] and got[3].dtype == torch.int8


# ---------------------------------------------------------------------------------------------
# 3. the guarded case (tests/test_guarded_gpu.py's harness; not registered in its CASES, which are held
# against include/dmstereo.h: tests/test_lsm_affine_host.py holds this one against include/dmstereo_lsm.h)
# ---------------------------------------------------------------------------------------------
def guarded_inputs(H, W, r):
    """Images cut so that the outermost halo windows touch all four borders: the first and the last byte of img1 are
    the first and the last a cell reads; starts up to 1.5 px off push the warps of the border cells to the image's
    edge and past it."""
    a, b = stereo_pair(H + 2 * (r + 1), W + 2 * (r + 1), seed=H + W + r, dx=1)
    rng = np.random.default_rng(H + r)
    dr = rng.integers(-6, 7, (H, W)) / 4.0
    dc = 1.0 + rng.integers(-6, 7, (H, W)) / 4.0
    dr[rng.uniform(size=(H, W)) < 0.05] = np.nan
    dc[rng.uniform(size=(H, W)) < 0.05] = -np.inf
    dr[0, 0] = -0.0
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    return a, b, dr, dc, (r + 1, r + 1), mask


def _guarded(x):
    for (H, W), r, iters in (((33, 31), 2, 3), ((9, 40), 3, 8), ((12, 35), 7, 2)):
        a, b, dr, dc, off, mask = guarded_inputs(H, W, r)
        ta, tb = x.inp(a), x.inp(b)
        assert not x.g or (ta.data_ptr() % 2 == 1 and ta.stride(0) == a.shape[1])
        tag = '%dx%d r%d' % (H, W, r)
        x.add(tag, engine.lsm_affine(ta, tb, x.inp(dr), x.inp(dc), r, iters, offset=off, max_move=2.0, max_shear=0.9,
                                     **EVERY))
        x.add(tag + ' mask', engine.lsm_affine(ta, tb, x.inp(dr), x.inp(dc), r, iters, offset=off, mask=x.inp(mask),
                                               out=(x.out(dr.shape), x.out(dr.shape)), **EVERY))
        tr, tc = x.inout(dr), x.inout(dc)      # the outputs are the inputs
        x.add(tag + ' aliased', engine.lsm_affine(ta, tb, tr, tc, r, iters, offset=off, mask=x.inp(mask), out=(tr, tc),
                                                  **EVERY))
        x.add(tag + ' no outputs', engine.lsm_affine(ta, tb, x.inp(dr), x.inp(dc), r, iters, offset=off))


GUARDED_CASE = G.Case('lsm_affine', ('dm_lsm_affine',), _guarded, None)


def test_guarded_lsm_affine(monkeypatch):
    """Guarded buffers, exact workspace, two poisons: nothing outside the buffers is written, no input is written,
    and the results equal the ordinary run's byte for byte."""
    G.run_case(GUARDED_CASE, monkeypatch)


# ---------------------------------------------------------------------------------------------
# 4. ImageCutSolver(lsm_model=) and shard.solve_image_sharded(lsm_model=)
# ---------------------------------------------------------------------------------------------
MODES = ['elevation', 'elevation2']
KW = dict(image_size=[32, 32], stride=[32, 32], window_size=5, degree_map_mode=list(MODES))
E = 2
LSM = (5, 6)


@pytest.fixture(scope='module')
def ramp():
    a, b, _ = ramp_pair(100, 100, 7, 0.03, d0=1.0)
    return a, b


def test_image_cut_solver_affine(ramp):
    """lsm_model='affine' end to end: the solver's result is the chain run stage by stage, lsm_affine_map is
    returned; 'shift' is a call that omits the keyword, bit for bit."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = ramp
    plain = ImageCutSolver(a, b, **KW)
    d0, o0 = plain()
    assert plain.lsm_model == ('shift', None) and plain.lsm_affine_map is None
    solver = ImageCutSolver(a, b, lsm=LSM, lsm_model='affine', **KW)
    d1, o1 = solver()
    row, col, score, status, aff = engine.lsm_affine(a, b, dev(d0[1]), dev(d0[0]), LSM[0], LSM[1], offset=E, **EVERY)
    assert raw_bits(d1, np.stack([host(col), host(row)])) and same_bits(o1, o0)
    assert solver.lsm_score_map.dtype == np.float64 and raw_bits(solver.lsm_score_map, host(score))
    assert solver.lsm_status_map.dtype == np.int8 and np.array_equal(solver.lsm_status_map, host(status))
    assert solver.lsm_affine_map.dtype == np.float64 and solver.lsm_affine_map.shape == (4, 64, 64)
    assert raw_bits(solver.lsm_affine_map, host(aff)) and (solver.lsm_status_map == LSM[1]).mean() > 0.5
    full = solver._execute_matching_device()      # d_map, out_map, lsm score, lsm status, lsm affine
    assert len(full) == 5 and [t.dtype for t in full[2:]] == [torch.float64, torch.int8, torch.float64]
    # with a shear bound, after the fill, before the photo score
    chain = dict(photo=(2, 0.75), fill=16)
    before = ImageCutSolver(a, b, **chain, **KW)
    d2, _ = before()
    solver = ImageCutSolver(a, b, lsm=(3, 4, 0.75), lsm_model=('affine', 0.02), **chain, **KW)
    d3, _ = solver()
    row, col, score, status, aff = engine.lsm_affine(a, b, dev(d2[1]), dev(d2[0]), 3, 4, offset=E, max_move=0.75,
                                                     max_shear=0.02, **EVERY)
    assert raw_bits(d3, np.stack([host(col), host(row)])) and raw_bits(solver.lsm_affine_map, host(aff))
    assert raw_bits(solver.photo_map, host(engine.photo_score(a, b, row, col, 2, offset=E)))
    # 'shift': today's call
    ref = ImageCutSolver(a, b, lsm=(3, 2), **chain, **KW)._execute_matching_device()
    got = ImageCutSolver(a, b, lsm=(3, 2), lsm_model='shift', **chain, **KW)._execute_matching_device()
    assert len(ref) == len(got) and all(same_bits(host(p).astype(np.float64), host(q).astype(np.float64))
                                        for p, q in zip(got, ref))
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm=(1, 2), lsm_model='affine', **KW)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm_model=('affine', 1.5), **KW)


def test_solve_image_sharded_affine_on_device(ramp):
    from deepmatching_stereo_matching_amd import shard
    a, b = ramp
    args = (a, b, [32, 32], [32, 32], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args)
    got = shard.solve_image_sharded(*args, lsm=LSM, lsm_model=('affine', 0.4))
    assert len(got) == 5
    row, col, score, status, aff = engine.lsm_affine(a, b, ref[0][1], ref[0][0], LSM[0], LSM[1], offset=E, max_shear=0.4,
                                                     **EVERY)
    assert raw_bits(host(got[0]), np.stack([host(col), host(row)])) and same_bits(host(got[1]), host(ref[1]))
    assert raw_bits(host(got[2]), host(score)) and torch.equal(got[3], status) and raw_bits(host(got[4]), host(aff))
    shift, same = shard.solve_image_sharded(*args, lsm=(3, 2)), shard.solve_image_sharded(*args, lsm=(3, 2), lsm_model='shift')
    assert len(shift) == len(same) == 4 and all(same_bits(host(s).astype(np.float64), host(r).astype(np.float64))
                                                for s, r in zip(same, shift))
    with pytest.raises(ValueError):
        shard.solve_image_sharded(*args, lsm=(1, 2), lsm_model='affine')
