"""Local re-matching on the GPU: dm_photo_refine (engine.photo_refine) against the restatement of
the definition (tests/test_refine_host.py: refine_fast, pinned there to the plain-loop
refine_restate) bit for bit -- both planes, the score and the shift -- over shapes below, on and
across the workgroup tile, every row-width path of the kernel (radius 1 .. 7) with every search
radius, images just large enough (most candidates unscored, some cells with none) and with a wide
margin, disparities that are integers, fractions of both signs, -0.0, that put the patch exactly
on each image border and one pixel past it for the centre and for the outermost candidate, NaN,
+-inf and +-1e300; with and without mask, sub-pixel step and min_gain; the content classes that
hold the largest sums at radius 7 and the ones where every candidate ties; row-strided images,
unequal offsets, in place and out of place, every optional output omitted in turn, a side stream,
run-to-run equality, the centre score against engine.photo_score, the argument errors, and the
ImageCutSolver / solve_image_sharded keyword end to end."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair

from test_fill_host import raw_bits, same_bits
from test_photo_host import INF, NAN
from test_refine_host import all_bits, candidates_fast, choose_fast, refine_restate

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (65, 130)]
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def border_planes(H, W, Hi, Wi, r, s, oy, ox, seed=0):
    """Disparity planes that mix, cell by cell: integers, fractions of both signs, -0.0, the values that put the
    img2 patch of the centre, and of the outermost candidate, exactly on each image border and one pixel past it
    (by a whole pixel and by a fraction), and NaN, +-inf, +-1e300."""
    rng = np.random.default_rng(7 * H + 13 * W + 31 * r + 3 * s + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for c, n in ((yy + oy, Hi), (xx + ox, Wi)):
        c = c.astype(np.float64)
        d = rng.uniform(-3.0, 3.0, (H, W))
        kind = rng.integers(0, 32, (H, W))
        d = np.where(kind == 0, np.round(d), d)
        d = np.where(kind == 1, -0.0, d)
        d = np.where(kind == 2, c - r, d)                      # the centre at position r: its patch starts at pixel 0
        d = np.where(kind == 3, c - (r - 1), d)                # one pixel past it: only candidates > 0 score
        d = np.where(kind == 4, c - (r - 0.25), d)             # a fraction past it
        d = np.where(kind == 5, c - (n - r - 2), d)            # the centre's patch ends at the last pixel
        d = np.where(kind == 6, c - (n - r - 1), d)            # one pixel past it, though the fraction is 0
        d = np.where(kind == 7, c - (n - r - 1.5), d)          # a half past the last position that scores
        d = np.where(kind == 8, c - (r - s), d)                # only the outermost candidate +s scores
        d = np.where(kind == 9, c - (r - s - 1), d)            # one pixel past it: no candidate scores
        d = np.where(kind == 10, c - (r - s - 0.5), d)         # (floor: the same)
        d = np.where(kind == 11, c - (n - r - 2 + s), d)       # only the outermost candidate -s scores
        d = np.where(kind == 12, c - (n - r - 1 + s), d)       # one pixel past it: none
        d = np.where(kind == 13, c - (n - r - 2 + s + 0.75), d)
        special = np.array([NAN, -NAN, INF, -INF, 1e300, -1e300])[rng.integers(0, 6, (H, W))]
        d = np.where(kind == 14, special, d)
        out.append(np.ascontiguousarray(d))
    return out


VARIANTS = [dict(), dict(subpix=True, min_gain=0.05, mask=True), dict(subpix=True), dict(min_gain=0.05, mask=True)]
_REF = {}


def case(shape, r, s, margin):
    """(img1, img2, d_row, d_col, offset, mask, the restatement's candidate scores), computed once per case."""
    key = (shape, r, s, margin)
    if key not in _REF:
        H, W = shape
        m = r + 1 if margin == 'tight' else r + s + 9
        oy, ox = m, m + 1
        a, b = stereo_pair(H + 2 * m, W + 2 * m + 2, seed=H + W + r, dx=1)
        dr, dc = border_planes(H, W, a.shape[0], a.shape[1], r, s, oy, ox)
        mask = (np.random.default_rng(H * W + r).uniform(size=(H, W)) < 0.6).astype(np.uint8)
        _REF[key] = (a, b, dr, dc, (oy, ox), mask, candidates_fast(a, b, dr, dc, r, s, (oy, ox)))
    return _REF[key]


def want(c, s, subpix=False, min_gain=0.0, mask=False):
    a, b, dr, dc, off, m, cand = c
    return choose_fast(cand, dr, dc, s, min_gain, subpix, m if mask else None)


def run(a, b, dr, dc, r, s, off, subpix=False, min_gain=0.0, mask=None, **kw):
    got = engine.photo_refine(a if torch.is_tensor(a) else dev(a), b if torch.is_tensor(b) else dev(b), dev(dr), dev(dc),
                              r, s, offset=off, min_gain=min_gain, subpix=subpix, mask=dev(mask), return_score=True,
                              return_shift=True, **kw)
    assert [g.dtype for g in got] == [torch.float64, torch.float64, torch.float64, torch.int8]
    return [host(g) for g in got]


def check(shape, r, s, margin):
    c = case(shape, r, s, margin)
    a, b, dr, dc, off, mask, cand = c
    for v in VARIANTS:
        w = want(c, s, **v)
        got = run(a, b, dr, dc, r, s, off, v.get('subpix', False), v.get('min_gain', 0.0), mask if v.get('mask') else None)
        assert all_bits(got, w), (shape, r, s, margin, v)
        kept = ~w[3].any(axis=0)
        assert raw_bits(got[0][kept], dr[kept]) and raw_bits(got[1][kept], dc[kept])      # NaN payloads, -0.0: copied
    return c


# ---------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('margin', ['tight', 'wide'])
@pytest.mark.parametrize('s', [1, 2, 3])
@pytest.mark.parametrize('r', [1, 2, 3, 7])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda v: '%dx%d' % v)
def test_against_restatement(shape, r, s, margin):
    c = check(shape, r, s, margin)
    if shape == (65, 130):
        live, sc = c[6]
        scored = ~np.isnan(sc)
        some, every = scored.any(axis=(0, 1)), scored.all(axis=(0, 1))
        w = want(c, s)
        assert (w[3] != 0).any(axis=0).mean() > 0.2 and np.isnan(w[2]).mean() > 0.05
        assert (some & ~every).mean() > 0.03 and (live & ~some).any()      # partly scored cells, live cells with none
        if margin == 'wide':
            assert every.mean() > 0.3


@pytest.mark.parametrize('r', [4, 5, 6])
def test_other_radii(r):
    """Radius 4 and 5 take the three-dword window rows, 6 the four-dword rows with a one-byte tail."""
    for margin in ('tight', 'wide'):
        for s in (1, 2, 3):
            check((33, 31), r, s, margin)


def test_fast_restatement_is_the_literal_one_here():
    c = case((5, 7), 2, 2, 'tight')
    a, b, dr, dc, off, mask, cand = c
    for v in VARIANTS:
        lit = refine_restate(a, b, dr, dc, 2, 2, off, v.get('min_gain', 0.0), v.get('subpix', False),
                             mask if v.get('mask') else None)
        assert all_bits(lit, want(c, 2, **v))


@pytest.mark.parametrize('r,s', [(1, 2), (2, 2), (3, 2), (3, 3)])
def test_planted_impulses(r, s):
    from test_refine_host import planted
    a, b, dr, dc, hit, vec, m = planted(r, s)
    out_row, out_col, score, shift = run(a, b, dr, dc, r, s, m)
    assert (out_row == 0.0).all() and (out_col == 2.0).all() and (score == 1.0).all()
    assert np.array_equal(shift, np.where(hit, vec, 0))


@pytest.mark.parametrize('kind', ['bright', 'high4', 'dark_bright', 'binary', 'const', 'identical', 'dark', 'checker'])
def test_content_classes(kind):
    """The largest sums, at radius 7 (a 32-bit S_k S_l or n sum(P_k P_l) fails here and nowhere else), and the
    classes where many or all candidates tie at 1.0 or 0.0."""
    H, W, r, s = 20, 37, 7, 3
    m = r + s + 2
    a, b = content_pair(kind, H + 2 * m, W + 2 * m, 3)
    rng = np.random.default_rng(1)
    for dr, dc in ((np.zeros((H, W)), np.full((H, W), 2.0)), (rng.uniform(-2, 2, (H, W)), rng.uniform(-2, 2, (H, W)))):
        cand = candidates_fast(a, b, dr, dc, r, s, m)
        assert not np.isnan(cand[1]).any()
        for sub in (False, True):
            assert all_bits(run(a, b, dr, dc, r, s, m, sub), choose_fast(cand, dr, dc, s, 0.0, sub))
    if kind == 'const':
        w = choose_fast(cand, dr, dc, s)
        assert raw_bits(w[2], np.zeros((H, W))) and not w[3].any()          # every candidate 0.0: nothing moves
    r = 1                                                                     # 3 x 3 windows: the ties of test_refine_host
    a, b = content_pair(kind, H + 12, W + 12, 4)
    z = np.zeros((H, W))
    assert all_bits(run(a, b, z, z, r, 2, 6), choose_fast(candidates_fast(a, b, z, z, r, 2, 6), z, z, 2))


# ---------------------------------------------------------------------------------------------
# 2. the calling forms
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def strided():
    """img1 and img2 as views, with different row strides, into wider device tensors."""
    a, b = case((33, 31), 2, 2, 'wide')[:2]
    Hi, Wi = a.shape
    wa = torch.full((Hi + 2, Wi + 13), 77, dtype=torch.uint8, device='cuda')
    wb = torch.full((Hi + 3, Wi + 30), 99, dtype=torch.uint8, device='cuda')
    wa[1:1 + Hi, 5:5 + Wi] = dev(a)
    wb[2:2 + Hi, 3:3 + Wi] = dev(b)
    va, vb = wa[1:1 + Hi, 5:5 + Wi], wb[2:2 + Hi, 3:3 + Wi]
    assert va.stride(0) != vb.stride(0) and not va.is_contiguous() and not vb.is_contiguous()
    return va, vb


def test_strided_images_and_host_images(strided):
    c = case((33, 31), 2, 2, 'wide')
    a, b, dr, dc, off, mask, cand = c
    assert off[0] != off[1]
    va, vb = strided
    w = want(c, 2, subpix=True)
    assert all_bits(run(va, vb, dr, dc, 2, 2, off, True), w)
    assert all_bits(run(va, b, dr, dc, 2, 2, off, True), w)
    # host images and a column-strided view are copied; a bool mask is taken
    assert all_bits(run(torch.from_numpy(a), dev(np.ascontiguousarray(b.T)).T, dr, dc, 2, 2, off, True), w)
    got = engine.photo_refine(a, b, dev(dr), dev(dc), 2, 2, offset=off, mask=dev(mask.astype(bool)))
    wm = want(c, 2, subpix=True, mask=True)
    assert len(got) == 2 and raw_bits(host(got[0]), wm[0]) and raw_bits(host(got[1]), wm[1])


def test_in_place_and_out_of_place(strided):
    """out=(d_row, d_col) works in place, and the planes may be planes of one d_map: the solver's call."""
    c = case((33, 31), 2, 2, 'wide')
    a, b, dr, dc, off, mask, cand = c
    va, vb = strided
    w = want(c, 2, subpix=True, min_gain=0.05)
    m = dev(np.stack([dc, dr]))
    res = engine.photo_refine(va, vb, m[1], m[0], 2, 2, offset=off, min_gain=0.05, out=(m[1], m[0]), return_shift=True)
    assert res[0].data_ptr() == m[1].data_ptr() and res[1].data_ptr() == m[0].data_ptr()
    assert raw_bits(host(m[1]), w[0]) and raw_bits(host(m[0]), w[1]) and np.array_equal(host(res[2]), w[3])
    tr, tc = dev(dr), dev(dc)
    o = (torch.zeros((33, 31), dtype=torch.float64, device='cuda'), torch.zeros((33, 31), dtype=torch.float64, device='cuda'))
    res = engine.photo_refine(va, vb, tr, tc, 2, 2, offset=off, min_gain=0.05, out=o, return_score=True)
    assert res[0] is o[0] and res[1] is o[1] and raw_bits(host(o[0]), w[0]) and raw_bits(host(o[1]), w[1])
    assert raw_bits(host(res[2]), w[2]) and raw_bits(host(tr), dr) and raw_bits(host(tc), dc)      # the inputs are left alone
    d, score, shift = engine.refine_stage(a, b, dev(np.stack([dc, dr])), ['elevation', 'elevation2'], (2, 2, 0.05), off)
    assert raw_bits(host(d), np.stack([w[1], w[0]])) and raw_bits(host(score), w[2]) and np.array_equal(host(shift), w[3])


def test_side_stream_and_run_to_run():
    c = case((65, 130), 3, 3, 'wide')
    a, b, dr, dc, off, mask, cand = c
    w = want(c, 3, subpix=True)
    first = run(a, b, dr, dc, 3, 3, off, True)
    assert all_bits(first, w)
    for _ in range(3):
        assert all_bits(run(a, b, dr, dc, 3, 3, off, True), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ta, tb, tr, tc = dev(a), dev(b), dev(dr), dev(dc)
    torch.cuda.synchronize()
    got = engine.photo_refine(ta, tb, tr, tc, 3, 3, offset=off, return_score=True, return_shift=True, stream=side)
    side.synchronize()
    assert all_bits([host(g) for g in got], w)


def test_every_optional_pointer_omitted_in_turn():
    """The C entry with each NULL-able pointer NULL in turn: the others are what they were."""
    c = case((33, 31), 3, 2, 'tight')
    a, b, dr, dc, off, mask, cand = c
    lib = L.load()
    ta, tb, tr, tc, tm = dev(a), dev(b), dev(dr), dev(dc), dev(mask)
    work = torch.empty(lib.dm_photo_refine_bytes(a.shape[0], a.shape[1], 33, 31, 3, 2), dtype=torch.uint8, device='cuda')
    for give in (('mask', 'score', 'shift'), ('score', 'shift'), ('mask', 'shift'), ('mask', 'score'), ('mask',), ()):
        o_row = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        o_col = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        score = torch.full((33, 31), 5.0, dtype=torch.float64, device='cuda')
        shift = torch.full((2, 33, 31), 5, dtype=torch.int8, device='cuda')
        L.check(lib.dm_photo_refine(L.ptr(ta), ta.stride(0), L.ptr(tb), tb.stride(0), a.shape[0], a.shape[1], L.ptr(tr),
                                    L.ptr(tc), 33, 31, off[0], off[1], 3, 2, 0.0, L.DM_REFINE_SUBPIX,
                                    L.ptr(tm if 'mask' in give else None), L.ptr(o_row), L.ptr(o_col),
                                    L.ptr(score if 'score' in give else None), L.ptr(shift if 'shift' in give else None),
                                    L.ptr(work), L.stream_handle()), 'dm_photo_refine')
        torch.cuda.synchronize()
        w = want(c, 2, subpix=True, mask='mask' in give)
        assert raw_bits(host(o_row), w[0]) and raw_bits(host(o_col), w[1]), give
        assert raw_bits(host(score), w[2]) if 'score' in give else bool((score == 5).all()), give
        assert np.array_equal(host(shift), w[3]) if 'shift' in give else bool((shift == 5).all()), give


@pytest.mark.parametrize('r', [1, 3, 7])
def test_centre_score_is_photo_score(r):
    """With a min_gain that nothing reaches the centre wins wherever it is scored: the score is engine.photo_score's."""
    c = case((33, 31), r, 2, 'wide')
    a, b, dr, dc, off, mask, cand = c
    ps = host(engine.photo_score(a, b, dev(dr), dev(dc), r, offset=off))
    got = run(a, b, dr, dc, r, 2, off, True, 2.0)
    on = ~np.isnan(ps)
    assert on.mean() > 0.3 and raw_bits(got[2][on], ps[on]) and not got[3][:, on].any()
    assert raw_bits(got[0][on], dr[on]) and raw_bits(got[1][on], dc[on])


def test_argument_errors():
    a, b = stereo_pair(20, 24, seed=1, dx=1)
    d = torch.zeros((5, 7), dtype=torch.float64, device='cuda')
    for bad in (dict(radius=0), dict(radius=8), dict(radius=2.0), dict(search=0), dict(search=4), dict(search=1.0),
                dict(offset=(1, 2, 3)), dict(offset=1.5), dict(offset=2 ** 31), dict(min_gain=-0.1), dict(min_gain=2.5),
                dict(min_gain=NAN), dict(mask=d), dict(mask=torch.ones((5, 7), dtype=torch.uint8)),
                dict(mask=torch.ones((7, 5), dtype=torch.uint8, device='cuda')), dict(out=d), dict(out=(d,)),
                dict(out=(d, d.float())), dict(out=(d, d.cpu())), dict(out=(d, d[:4])),
                dict(out=(d, torch.zeros((7, 5), dtype=torch.float64, device='cuda').T))):
        kw = dict(radius=2, search=1, offset=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.photo_refine(a, b, d, d, kw.pop('radius'), kw.pop('search'), **kw)
    for args in ((a, b, d.cpu(), d), (a, b, d, d.float()), (a, b, d, d[:4]), (a, b, d[None], d[None]),
                 (a.astype(np.float64), b, d, d), (a, b[:, :20], d, d), (a[None], b[None], d, d)):
        with pytest.raises(ValueError):
            engine.photo_refine(*args, 2, 1)
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    got = engine.photo_refine(a, b, e, e, 2, 1, return_score=True, return_shift=True)
    assert [tuple(g.shape) for g in got] == [(0, 7), (0, 7), (0, 7), (2, 0, 7)] and got[3].dtype == torch.int8


# ---------------------------------------------------------------------------------------------
# 3. ImageCutSolver(refine=) and shard.solve_image_sharded(refine=)
# ---------------------------------------------------------------------------------------------
MODES = ['elevation', 'elevation2']
KW = dict(image_size=[32, 32], stride=[32, 32], window_size=5, degree_map_mode=list(MODES))
E = 2
REFINE = (2, 2, 0.05)


@pytest.fixture(scope='module')
def corrupted():
    """dx = 2, a 2 x 2 grid of 32 x 32 tiles, a block of img2 overwritten: wrong cells to reject, fill and measure."""
    a, b = stereo_pair(100, 100, seed=7, dx=2)
    b = b.copy()
    b[20:36, 24:44] = np.random.default_rng(5).integers(0, 256, (16, 20)).astype(np.uint8)
    return a, b


def test_image_cut_solver_refine(corrupted):
    """stitch -> photo reject -> fill -> refine -> smooth -> photo score, against the stages by hand."""
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = corrupted
    chain = dict(photo=(2, 0.75), fill=16)
    before = ImageCutSolver(a, b, **chain, **KW)
    d0, o0 = before()
    assert before.refine is None and before.refine_score_map is None and before.refine_shift_map is None
    p0 = before._execute_matching_device()
    p1 = ImageCutSolver(a, b, refine=None, **chain, **KW)._execute_matching_device()
    assert len(p0) == len(p1) == 5 and all(same_bits(host(p).astype(np.float64), host(q).astype(np.float64))
                                           for p, q in zip(p0, p1))
    holes = before.hole_map
    assert holes.any() and not holes.all()
    # 'filled': only the cells the fill produced are measured again, every other cell keeps its bits
    solver = ImageCutSolver(a, b, refine=REFINE, **chain, **KW)
    d1, o1 = solver()
    mask = holes[1] | holes[0]
    row, col, score, shift = engine.photo_refine(a, b, dev(d0[1]), dev(d0[0]), REFINE[0], REFINE[1], offset=E,
                                                 min_gain=REFINE[2], mask=dev(mask), return_score=True, return_shift=True)
    assert raw_bits(d1, np.stack([host(col), host(row)])) and same_bits(o1, o0)
    assert raw_bits(d1[:, ~mask], d0[:, ~mask]) and np.array_equal(solver.hole_map, holes)
    assert solver.refine_score_map.dtype == np.float64 and raw_bits(solver.refine_score_map, host(score))
    assert solver.refine_shift_map.dtype == np.int8 and np.array_equal(solver.refine_shift_map, host(shift))
    assert solver.refine_shift_map.shape == (2, 64, 64) and solver.refine_shift_map.any()
    assert not solver.refine_shift_map[:, ~mask].any() and np.isnan(solver.refine_score_map[~mask]).all()
    assert raw_bits(solver.photo_map, host(engine.photo_score(a, b, row, col, 2, offset=E)))
    assert np.array_equal(solver.photo_reject_map, before.photo_reject_map)
    full = solver._execute_matching_device()      # ..., holes, refine score, refine shift, rejected, score
    assert len(full) == 7 and [t.dtype for t in full[2:]] == [torch.uint8, torch.float64, torch.int8, torch.uint8,
                                                              torch.float64]
    assert tuple(full[4].shape) == (2, 64, 64)
    # 'all', before the smoothing
    smooth = (2, 10.0, 2.0)
    plain = ImageCutSolver(a, b, **KW)
    d2, _ = plain()
    solver = ImageCutSolver(a, b, refine=(3, 1), refine_where='all', smooth=smooth, **KW)
    d3, _ = solver()
    row, col, score, shift = engine.photo_refine(a, b, dev(d2[1]), dev(d2[0]), 3, 1, offset=E, return_score=True,
                                                 return_shift=True)
    d = engine.bilateral_filter(torch.stack([col, row]), *smooth, guide=dev(np.ascontiguousarray(a[E:E + 64, E:E + 64])))
    assert same_bits(d3, host(d)) and raw_bits(solver.refine_score_map, host(score))
    assert np.array_equal(solver.refine_shift_map, host(shift)) and solver.hole_map is None and solver.photo_map is None
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, refine=(2, 1), refine_where='all', **dict(KW, degree_map_mode=MODES + ['distance']))
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, refine=(2, 1), **KW)                           # 'filled' needs fill=


def test_solve_image_sharded_refine_on_device(corrupted):
    """shard.solve_image_sharded's own refine stage (engine.photo_refine on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = corrupted
    args = (a, b, [32, 32], [32, 32], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=1.0, fill=16)
    same = shard.solve_image_sharded(*args, consistency=1.0, fill=16, refine=None)
    assert len(same) == len(ref) == 4 and all(same_bits(host(s).astype(np.float64), host(r).astype(np.float64))
                                              for s, r in zip(same, ref))
    got = shard.solve_image_sharded(*args, consistency=1.0, fill=16, refine=REFINE, photo=2)
    assert len(got) == 7 and all(same_bits(host(s).astype(np.float64), host(r).astype(np.float64))
                                 for s, r in zip(got[1:4], ref[1:4]))
    mask = ref[3][1] | ref[3][0]
    assert bool(mask.any())
    row, col, score, shift = engine.photo_refine(a, b, ref[0][1], ref[0][0], REFINE[0], REFINE[1], offset=E,
                                                 min_gain=REFINE[2], mask=mask, return_score=True, return_shift=True)
    assert raw_bits(host(got[0]), np.stack([host(col), host(row)]))
    assert raw_bits(host(got[4]), host(score)) and got[5].dtype == torch.int8 and torch.equal(got[5], shift)
    assert raw_bits(host(got[6]), host(engine.photo_score(a, b, row, col, 2, offset=E)))
    keep = ~host(mask).astype(bool)
    assert raw_bits(host(got[0])[:, keep], host(ref[0])[:, keep])
    with pytest.raises(ValueError):
        shard.solve_image_sharded(a, b, [32, 32], [32, 32], 5, NCC, MODES + ['distance'], refine=(2, 1), refine_where='all')
    with pytest.raises(ValueError):
        shard.solve_image_sharded(*args, refine=(2, 1))
