"""Least-squares sub-pixel matching on the GPU: dm_lsm_refine (engine.lsm_refine) against the
restatement of the definition (tests/test_lsm_host.py: lsm_fast, pinned there to the plain-loop
lsm_restate) bit for bit -- both planes, the score and the status -- over shapes below, on and
across the workgroup tile, every row-width path of the kernel (radius 1 .. 7) with 1, 2 and 4
steps, images just large enough and with a wide margin, disparities near the truth (so that steps
are accepted), integers, fractions of both signs, -0.0, positions exactly on each image border and
one pixel past it, starts from which a step leaves the image, NaN, +-inf and +-1e300; with and
without mask, max_move 0.25 and 2.0; the content classes that hold the largest sums at radius 7;
the accuracy case; row-strided images, in place and out of place, every optional pointer omitted
in turn, a side stream, run-to-run equality, the argument errors, and the ImageCutSolver /
solve_image_sharded keyword end to end."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair

from test_fill_host import raw_bits, same_bits
from test_photo_host import INF, NAN
from test_lsm_host import PHASES, accuracy_case, all_bits, lsm_fast, lsm_restate, rms

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (65, 130)]
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def border_planes(H, W, Hi, Wi, r, oy, ox, seed=0):
    """Disparity planes around the truth of stereo_pair(dx=1), (0, 1), that mix cell by cell: the truth plus a
    fraction of either sign, the truth itself (an integer), -0.0, a far start, the values that put the img2 patch
    exactly on each image border, one pixel and a fraction past it, and NaN, +-inf, +-1e300."""
    rng = np.random.default_rng(7 * H + 13 * W + 31 * r + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for c, n, truth in ((yy + oy, Hi, 0.0), (xx + ox, Wi, 1.0)):
        c = c.astype(np.float64)
        d = truth + rng.uniform(-0.7, 0.7, (H, W))
        kind = rng.integers(0, 32, (H, W))
        d = np.where(kind == 0, truth, d)
        d = np.where(kind == 1, -0.0, d)
        d = np.where(kind == 2, c - r, d)                      # the position r: the patch starts at pixel 0
        d = np.where(kind == 3, c - (r - 1), d)                # one pixel past it
        d = np.where(kind == 4, c - (r - 0.25), d)             # a fraction past it
        d = np.where(kind == 5, c - (n - r - 2), d)            # the patch ends at the last pixel
        d = np.where(kind == 6, c - (n - r - 1), d)            # one pixel past it, though the fraction is 0
        d = np.where(kind == 7, c - (n - r - 1.5), d)          # a half before that: the last position that scores
        d = np.where(kind == 8, rng.uniform(-3.0, 3.0, (H, W)), d)
        d = np.where(kind == 9, c - (r + 0.125), d)            # just inside: a step may leave the image
        d = np.where(kind == 10, c - (n - r - 1.125), d)
        special = np.array([NAN, -NAN, INF, -INF, 1e300, -1e300])[rng.integers(0, 6, (H, W))]
        d = np.where(kind == 14, special, d)
        out.append(np.ascontiguousarray(d))
    return out


VARIANTS = [dict(), dict(max_move=0.25, mask=True), dict(max_move=2.0), dict(mask=True)]
_REF = {}


def case(shape, r, margin):
    """(img1, img2, d_row, d_col, offset, mask), made once per case.  The largest shape has a flat block in img1
    (cells whose normal equations are singular) and one in img2 (cells whose patch has no variance)."""
    key = (shape, r, margin)
    if key not in _REF:
        H, W = shape
        m = r + 1 if margin == 'tight' else r + 9
        oy, ox = m, m + 1
        a, b = stereo_pair(H + 2 * m, W + 2 * m + 2, seed=H + W + r, dx=1)
        if shape == (65, 130):
            a, b = a.copy(), b.copy()
            a[m + 8:m + 8 + 2 * r + 6, m + 20:m + 20 + 2 * r + 6] = 9
            b[m + 40:m + 40 + 2 * r + 6, m + 70:m + 70 + 2 * r + 6] = 200
        dr, dc = border_planes(H, W, a.shape[0], a.shape[1], r, oy, ox)
        mask = (np.random.default_rng(H * W + r).uniform(size=(H, W)) < 0.6).astype(np.uint8)
        _REF[key] = (a, b, dr, dc, (oy, ox), mask)
    return _REF[key]


def want(c, r, iters, max_move=1.0, mask=False):
    a, b, dr, dc, off, m = c
    key = ('want', id(c), r, iters, max_move, mask)
    if key not in _REF:
        _REF[key] = lsm_fast(a, b, dr, dc, r, iters, off, max_move, m if mask else None)
    return _REF[key]


def run(a, b, dr, dc, r, iters, off, max_move=1.0, mask=None, **kw):
    got = engine.lsm_refine(a if torch.is_tensor(a) else dev(a), b if torch.is_tensor(b) else dev(b), dev(dr), dev(dc),
                            r, iters, offset=off, max_move=max_move, mask=dev(mask), return_score=True,
                            return_status=True, **kw)
    assert [g.dtype for g in got] == [torch.float64, torch.float64, torch.float64, torch.int8]
    return [host(g) for g in got]


def check(shape, r, iters, margin):
    c = case(shape, r, margin)
    a, b, dr, dc, off, mask = c
    for v in (VARIANTS[:2] if shape == (65, 130) else VARIANTS):
        w = want(c, r, iters, **v)
        got = run(a, b, dr, dc, r, iters, off, v.get('max_move', 1.0), mask if v.get('mask') else None)
        assert all_bits(got, w), (shape, r, iters, margin, v)
        kept = w[3] != iters
        assert raw_bits(got[0][kept], dr[kept]) and raw_bits(got[1][kept], dc[kept])      # NaN payloads, -0.0: copied
    return c


# ---------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('margin', ['tight', 'wide'])
@pytest.mark.parametrize('iters', [1, 2, 4])
@pytest.mark.parametrize('r', [1, 2, 3, 7])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda v: '%dx%d' % v)
def test_against_restatement(shape, r, iters, margin):
    c = check(shape, r, iters, margin)
    if shape == (65, 130):
        w = want(c, r, iters)
        seen = set(np.unique(w[3]).tolist())
        assert seen == {-3, -2, -1, 0, iters}, seen      # a path that is never taken must not pass silently
        assert (w[3] == iters).mean() > 0.2
        by_vb = (w[3] == -1) & (w[2] == 0.0)                # -1 from a flat img2 patch (the score 0.0) and from D
        assert by_vb.any() and ((w[3] == -1) & np.isnan(w[2])).any()


@pytest.mark.parametrize('r', [4, 5, 6])
def test_other_radii(r):
    """Radius 4 and 5 take the three-dword window rows, 6 the four-dword rows with a one-byte tail."""
    for margin in ('tight', 'wide'):
        for iters in (1, 3):
            check((33, 31), r, iters, margin)


def test_fast_restatement_is_the_literal_one_here():
    c = case((5, 7), 2, 'tight')
    a, b, dr, dc, off, mask = c
    for v in VARIANTS:
        lit = lsm_restate(a, b, dr, dc, 2, 2, off, v.get('max_move', 1.0), mask if v.get('mask') else None)
        assert all_bits(lit, want(c, 2, 2, **v))


@pytest.mark.parametrize('kind', ['bright', 'high4', 'dark_bright', 'checker', 'binary', 'const', 'identical'])
def test_content_classes(kind):
    """The largest sums, at radius 7 (a 32-bit product or an int64 determinant fails here and nowhere else), and
    the classes where nothing may move."""
    H, W, r = 20, 37, 7
    m = r + 4
    a, b = content_pair(kind, H + 2 * m, W + 2 * m, 3)
    rng = np.random.default_rng(1)
    shift = 1.0 if kind == 'checker' else (0.0 if kind in ('identical', 'const') else 3.0)
    for dr, dc in ((np.zeros((H, W)), np.full((H, W), shift)),
                   (rng.uniform(-0.7, 0.7, (H, W)), shift + rng.uniform(-0.7, 0.7, (H, W)))):
        for iters in (1, 4):
            w = lsm_fast(a, b, dr, dc, r, iters, m)
            assert all_bits(run(a, b, dr, dc, r, iters, m), w)
            if kind == 'const':
                assert (w[3] == -1).all() and np.isnan(w[2]).all()
    if kind in ('const', 'identical'):
        z = np.zeros((H, W))
        w = lsm_fast(a, b, z, z, r, 2, m)
        assert not (w[3] == 2).any() and raw_bits(w[0], z) and raw_bits(w[1], z)
    r = 1                                                                     # 3 x 3 windows: many singular systems
    a, b = content_pair(kind, H + 12, W + 12, 4)
    z = np.zeros((H, W))
    assert all_bits(run(a, b, z, z + shift, r, 2, 6), lsm_fast(a, b, z, z + shift, r, 2, 6))


@pytest.mark.parametrize('ky,kx', PHASES)
def test_accuracy(ky, kx):
    """The accuracy case of tests/test_lsm_host.py on the device: the restatement's bits, hence its figures."""
    a, b, sr, sc, tr, tc, m = accuracy_case(ky, kx)
    got = run(a, b, sr, sc, 3, 4, m, 1.0)
    assert all_bits(got, lsm_fast(a, b, sr, sc, 3, 4, m, 1.0))
    after, share = rms(got[0], got[1], tr, tc), float((got[3] == 4).mean())
    print('phase (%d, %d) / 4: rms before %.3f, after %.3f, accepted %.2f %%' % (ky, kx, rms(sr, sc, tr, tc), after,
                                                                                100 * share))
    assert after <= 0.1 and share >= 0.99
    ps = host(engine.photo_score(a, b, dev(sr), dev(sc), 3, offset=m))
    acc = got[3] == 4
    assert (got[2][acc] > ps[acc]).all() and raw_bits(got[2][~acc], ps[~acc])


@pytest.mark.parametrize('r', [1, 3, 7])
def test_consequences_against_photo_score(r):
    """An accepted cell scores strictly above engine.photo_score of the input, an unaccepted scored cell reports
    its bits; identical windows at an integer disparity never move."""
    c = case((33, 31), r, 'wide')
    a, b, dr, dc, off, mask = c
    ps = host(engine.photo_score(a, b, dev(dr), dev(dc), r, offset=off))
    got = run(a, b, dr, dc, r, 3, off)
    acc = got[3] == 3
    rest = ~acc & ~np.isnan(got[2])
    assert acc.mean() > 0.2 and rest.mean() > 0.05
    assert (got[2][acc] > ps[acc]).all() and raw_bits(got[2][rest], ps[rest])
    z, one = np.zeros((33, 31)), np.ones((33, 31))
    z[4, 5] = -0.0
    got = run(a, b, z, one, r, 4, off)
    assert (got[3] == -3).all() and (got[2] == 1.0).all() and raw_bits(got[0], z) and raw_bits(got[1], one)


# ---------------------------------------------------------------------------------------------
# 2. the calling forms
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def strided():
    """img1 and img2 as views, with different row strides, into wider device tensors."""
    a, b = case((33, 31), 2, 'wide')[:2]
    Hi, Wi = a.shape
    wa = torch.full((Hi + 2, Wi + 13), 77, dtype=torch.uint8, device='cuda')
    wb = torch.full((Hi + 3, Wi + 30), 99, dtype=torch.uint8, device='cuda')
    wa[1:1 + Hi, 5:5 + Wi] = dev(a)
    wb[2:2 + Hi, 3:3 + Wi] = dev(b)
    va, vb = wa[1:1 + Hi, 5:5 + Wi], wb[2:2 + Hi, 3:3 + Wi]
    assert va.stride(0) != vb.stride(0) and not va.is_contiguous() and not vb.is_contiguous()
    return va, vb


def test_strided_images_and_host_images(strided):
    c = case((33, 31), 2, 'wide')
    a, b, dr, dc, off, mask = c
    assert off[0] != off[1]
    va, vb = strided
    w = want(c, 2, 3)
    assert all_bits(run(va, vb, dr, dc, 2, 3, off), w)
    assert all_bits(run(va, b, dr, dc, 2, 3, off), w)
    # host images and a column-strided view are copied; a bool mask is taken
    assert all_bits(run(torch.from_numpy(a), dev(np.ascontiguousarray(b.T)).T, dr, dc, 2, 3, off), w)
    got = engine.lsm_refine(a, b, dev(dr), dev(dc), 2, 3, offset=off, mask=dev(mask.astype(bool)))
    wm = want(c, 2, 3, mask=True)
    assert len(got) == 2 and raw_bits(host(got[0]), wm[0]) and raw_bits(host(got[1]), wm[1])


def test_in_place_and_out_of_place(strided):
    """out=(d_row, d_col) works in place, and the planes may be planes of one d_map: the solver's call."""
    c = case((33, 31), 2, 'wide')
    a, b, dr, dc, off, mask = c
    va, vb = strided
    w = want(c, 2, 3)
    m = dev(np.stack([dc, dr]))
    res = engine.lsm_refine(va, vb, m[1], m[0], 2, 3, offset=off, out=(m[1], m[0]), return_status=True)
    assert res[0].data_ptr() == m[1].data_ptr() and res[1].data_ptr() == m[0].data_ptr()
    assert raw_bits(host(m[1]), w[0]) and raw_bits(host(m[0]), w[1]) and np.array_equal(host(res[2]), w[3])
    tr, tc = dev(dr), dev(dc)
    o = (torch.zeros((33, 31), dtype=torch.float64, device='cuda'), torch.zeros((33, 31), dtype=torch.float64, device='cuda'))
    res = engine.lsm_refine(va, vb, tr, tc, 2, 3, offset=off, out=o, return_score=True)
    assert res[0] is o[0] and res[1] is o[1] and raw_bits(host(o[0]), w[0]) and raw_bits(host(o[1]), w[1])
    assert raw_bits(host(res[2]), w[2]) and raw_bits(host(tr), dr) and raw_bits(host(tc), dc)      # the inputs are left alone
    d, score, status = engine.lsm_stage(a, b, dev(np.stack([dc, dr])), ['elevation', 'elevation2'], (2, 3, 1.0), off)
    assert raw_bits(host(d), np.stack([w[1], w[0]])) and raw_bits(host(score), w[2]) and np.array_equal(host(status), w[3])


def test_side_stream_and_run_to_run():
    c = case((65, 130), 3, 'wide')
    a, b, dr, dc, off, mask = c
    w = want(c, 3, 4)
    first = run(a, b, dr, dc, 3, 4, off)
    assert all_bits(first, w)
    for _ in range(3):
        assert all_bits(run(a, b, dr, dc, 3, 4, off), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ta, tb, tr, tc = dev(a), dev(b), dev(dr), dev(dc)
    torch.cuda.synchronize()
    got = engine.lsm_refine(ta, tb, tr, tc, 3, 4, offset=off, return_score=True, return_status=True, stream=side)
    side.synchronize()
    assert all_bits([host(g) for g in got], w)


def test_every_optional_pointer_omitted_in_turn():
    """The C entry with each NULL-able pointer NULL in turn: the others are what they were."""
    c = case((33, 31), 3, 'tight')
    a, b, dr, dc, off, mask = c
    lib = L.load()
    ta, tb, tr, tc, tm = dev(a), dev(b), dev(dr), dev(dc), dev(mask)
    work = torch.empty(lib.dm_lsm_refine_bytes(a.shape[0], a.shape[1], 33, 31, 3, 2), dtype=torch.uint8, device='cuda')
    for give in (('mask', 'score', 'status'), ('score', 'status'), ('mask', 'status'), ('mask', 'score'), ('mask',), ()):
        o_row = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        o_col = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        score = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        status = torch.full((33, 31), 5, dtype=torch.int8, device='cuda')
        L.check(lib.dm_lsm_refine(L.ptr(ta), ta.stride(0), L.ptr(tb), tb.stride(0), a.shape[0], a.shape[1], L.ptr(tr),
                                  L.ptr(tc), 33, 31, off[0], off[1], 3, 2, 1.0, 0,
                                  L.ptr(tm if 'mask' in give else None), L.ptr(o_row), L.ptr(o_col),
                                  L.ptr(score if 'score' in give else None), L.ptr(status if 'status' in give else None),
                                  L.ptr(work), L.stream_handle()), 'dm_lsm_refine')
        torch.cuda.synchronize()
        w = want(c, 3, 2, mask='mask' in give)
        assert raw_bits(host(o_row), w[0]) and raw_bits(host(o_col), w[1]), give
        assert raw_bits(host(score), w[2]) if 'score' in give else bool((score == 5).all()), give
        assert np.array_equal(host(status), w[3]) if 'status' in give else bool((status == 5).all()), give


def test_argument_errors():
    a, b = stereo_pair(20, 24, seed=1, dx=1)
    d = torch.zeros((5, 7), dtype=torch.float64, device='cuda')
    for bad in (dict(radius=0), dict(radius=8), dict(radius=2.0), dict(iters=0), dict(iters=9), dict(iters=1.0),
                dict(offset=(1, 2, 3)), dict(offset=1.5), dict(offset=2 ** 31), dict(max_move=0.0), dict(max_move=-0.1),
                dict(max_move=2.5), dict(max_move=NAN), dict(mask=d), dict(mask=torch.ones((5, 7), dtype=torch.uint8)),
                dict(mask=torch.ones((7, 5), dtype=torch.uint8, device='cuda')), dict(out=d), dict(out=(d,)),
                dict(out=(d, d.float())), dict(out=(d, d.cpu())), dict(out=(d, d[:4])),
                dict(out=(d, torch.zeros((7, 5), dtype=torch.float64, device='cuda').T))):
        kw = dict(radius=2, iters=1, offset=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.lsm_refine(a, b, d, d, kw.pop('radius'), kw.pop('iters'), **kw)
    for args in ((a, b, d.cpu(), d), (a, b, d, d.float()), (a, b, d, d[:4]), (a, b, d[None], d[None]),
                 (a.astype(np.float64), b, d, d), (a, b[:, :20], d, d), (a[None], b[None], d, d)):
        with pytest.raises(ValueError):
            engine.lsm_refine(*args, 2, 1)
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    got = engine.lsm_refine(a, b, e, e, 2, 1, return_score=True, return_status=True)
    assert [tuple(g.shape) for g in got] == [(0, 7), (0, 7), (0, 7), (0, 7)] and got[3].dtype == torch.int8


# ---------------------------------------------------------------------------------------------
# 3. ImageCutSolver(lsm=) and shard.solve_image_sharded(lsm=)
# ---------------------------------------------------------------------------------------------
MODES = ['elevation', 'elevation2']
KW = dict(image_size=[32, 32], stride=[32, 32], window_size=5, degree_map_mode=list(MODES))
E = 2
LSM = (2, 3, 1.0)


@pytest.fixture(scope='module')
def corrupted():
    """dx = 2, a 2 x 2 grid of 32 x 32 tiles, a block of img2 overwritten: wrong cells to reject, fill and measure."""
    a, b = stereo_pair(100, 100, seed=7, dx=2)
    b = b.copy()
    b[20:36, 24:44] = np.random.default_rng(5).integers(0, 256, (16, 20)).astype(np.uint8)
    return a, b


def test_image_cut_solver_lsm(corrupted):
    """stitch -> photo reject -> fill -> refine -> lsm -> smooth -> photo score, against the stages by hand."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = corrupted
    chain = dict(photo=(2, 0.75), fill=16, refine=(2, 2, 0.05))
    before = ImageCutSolver(a, b, **chain, **KW)
    d0, o0 = before()
    assert before.lsm is None and before.lsm_score_map is None and before.lsm_status_map is None
    p0 = before._execute_matching_device()
    p1 = ImageCutSolver(a, b, lsm=None, **chain, **KW)._execute_matching_device()
    assert len(p0) == len(p1) == 7 and all(same_bits(host(p).astype(np.float64), host(q).astype(np.float64))
                                           for p, q in zip(p0, p1))
    holes = before.hole_map
    assert holes.any() and not holes.all()
    # 'filled': only the cells the fill produced are matched, after the refine stage; every other cell keeps its bits
    solver = ImageCutSolver(a, b, lsm=LSM[:2], lsm_where='filled', **chain, **KW)
    d1, o1 = solver()
    mask = holes[1] | holes[0]
    row, col, score, status = engine.lsm_refine(a, b, dev(d0[1]), dev(d0[0]), LSM[0], LSM[1], offset=E, max_move=LSM[2],
                                                mask=dev(mask), return_score=True, return_status=True)
    assert raw_bits(d1, np.stack([host(col), host(row)])) and same_bits(o1, o0)
    assert raw_bits(d1[:, ~mask], d0[:, ~mask]) and np.array_equal(solver.hole_map, holes)
    assert solver.lsm_score_map.dtype == np.float64 and raw_bits(solver.lsm_score_map, host(score))
    assert solver.lsm_status_map.dtype == np.int8 and np.array_equal(solver.lsm_status_map, host(status))
    assert solver.lsm_status_map.shape == (64, 64) and solver.lsm_status_map.any()
    assert not solver.lsm_status_map[~mask].any() and np.isnan(solver.lsm_score_map[~mask]).all()
    assert raw_bits(solver.photo_map, host(engine.photo_score(a, b, row, col, 2, offset=E)))
    assert np.array_equal(solver.refine_shift_map, before.refine_shift_map)
    full = solver._execute_matching_device()      # ..., holes, refine score, refine shift, lsm score, lsm status, rejected, score
    assert len(full) == 9 and [t.dtype for t in full[2:]] == [torch.uint8, torch.float64, torch.int8, torch.float64,
                                                              torch.int8, torch.uint8, torch.float64]
    assert tuple(full[6].shape) == (64, 64)
    # 'all' (the default), before the smoothing
    smooth = (2, 10.0, 2.0)
    plain = ImageCutSolver(a, b, **KW)
    d2, _ = plain()
    solver = ImageCutSolver(a, b, lsm=(3, 2), smooth=smooth, **KW)
    d3, _ = solver()
    row, col, score, status = engine.lsm_refine(a, b, dev(d2[1]), dev(d2[0]), 3, 2, offset=E, return_score=True,
                                                return_status=True)
    d = engine.bilateral_filter(torch.stack([col, row]), *smooth, guide=dev(np.ascontiguousarray(a[E:E + 64, E:E + 64])))
    assert same_bits(d3, host(d)) and raw_bits(solver.lsm_score_map, host(score))
    assert np.array_equal(solver.lsm_status_map, host(status)) and (solver.lsm_status_map == 2).any()
    assert solver.hole_map is None and solver.photo_map is None
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm=(2, 1), **dict(KW, degree_map_mode=MODES + ['distance']))
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm=(2, 1), lsm_where='filled', **KW)          # 'filled' needs fill=
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm=(2, 9), **KW)


def test_solve_image_sharded_lsm_on_device(corrupted):
    """shard.solve_image_sharded's own lsm stage (engine.lsm_refine on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = corrupted
    args = (a, b, [32, 32], [32, 32], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=1.0, fill=16)
    same = shard.solve_image_sharded(*args, consistency=1.0, fill=16, lsm=None)
    assert len(same) == len(ref) == 4 and all(same_bits(host(s).astype(np.float64), host(r).astype(np.float64))
                                              for s, r in zip(same, ref))
    got = shard.solve_image_sharded(*args, consistency=1.0, fill=16, lsm=LSM, lsm_where='filled', photo=2)
    assert len(got) == 7 and all(same_bits(host(s).astype(np.float64), host(r).astype(np.float64))
                                 for s, r in zip(got[1:4], ref[1:4]))
    mask = ref[3][1] | ref[3][0]
    assert bool(mask.any())
    row, col, score, status = engine.lsm_refine(a, b, ref[0][1], ref[0][0], LSM[0], LSM[1], offset=E, max_move=LSM[2],
                                                mask=mask, return_score=True, return_status=True)
    assert raw_bits(host(got[0]), np.stack([host(col), host(row)]))
    assert raw_bits(host(got[4]), host(score)) and got[5].dtype == torch.int8 and torch.equal(got[5], status)
    assert raw_bits(host(got[6]), host(engine.photo_score(a, b, row, col, 2, offset=E)))
    keep = ~host(mask).astype(bool)
    assert raw_bits(host(got[0])[:, keep], host(ref[0])[:, keep])
    every = shard.solve_image_sharded(*args, lsm=LSM)
    assert len(every) == 4 and bool((every[3] == LSM[1]).any())
    with pytest.raises(ValueError):
        shard.solve_image_sharded(a, b, [32, 32], [32, 32], 5, NCC, MODES + ['distance'], lsm=(2, 1))
    with pytest.raises(ValueError):
        shard.solve_image_sharded(*args, lsm=(2, 1), lsm_where='filled')
