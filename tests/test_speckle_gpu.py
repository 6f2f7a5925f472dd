"""Speckle filter on the GPU: dm_filter_speckles (engine.filter_speckles) against the plain-loop
restatement of the definition (tests/test_speckle_host.py: speckle_restate) bit for bit -- the
filtered map, the mask, the sizes and the labels -- over shapes that reach the one-launch path,
the exact tile and one-cell-wide last tiles, over maps that stress the union-find across tiles
(one segment over the whole map, long rows and columns, a spiral, a serpentine, checkerboards,
combs, a corner contact), the threshold at a tile seam, the planted-blob case, then batches,
in place, a side stream, run-to-run and tile-side independence, and the ImageCutSolver /
solve_image_sharded keyword."""
import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import raw_bits, same_bits
from test_speckle_host import planted, speckle_restate

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31), (64, 64), (65, 130), (129, 67), (150, 150)]
PARAMS = [(0, 1.0), (4, 2.0), (16, 5.0), (3, float('inf'))]
NCC = L.METHODS['cv2.TM_CCOEFF_NORMED']
INF = float('inf')


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def noise(H, W, seed=0, share=0.1):
    rng = np.random.default_rng(1000 * H + W + seed)
    x = rng.normal(0, 5, (H, W))
    x[rng.uniform(size=x.shape) < share] = np.nan
    return x


def run(x, max_size, max_diff, **kw):
    got = engine.filter_speckles(x if torch.is_tensor(x) else dev(x), max_size, max_diff, return_removed=True,
                                 return_sizes=True, return_labels=True, **kw)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.uint8
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32
    return tuple(host(g) for g in got)


def equal(got, want):
    """All four outputs: the map bit for bit (NaN positions equal), the integers exactly."""
    return (same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(got[2].astype(np.uint32), want[2]) and np.array_equal(got[3], want[3]))


def check(x, max_size, max_diff):
    want = speckle_restate(x, max_size, max_diff)
    got = run(x, max_size, max_diff)
    assert equal(got, want)
    keep = ~want[1].astype(bool)
    assert raw_bits(got[0][keep], np.asarray(x)[keep])      # kept cells and holes: the input's own bits
    return want


# ---------------------------------------------------------------------------------------------
# 1. random maps against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('params', PARAMS, ids=lambda p: '%d-%g' % p)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_maps(shape, params):
    x = noise(*shape)
    if shape == (1, 1):
        x[0, 0] = 2.5
    want = check(x, *params)
    if shape == (65, 130) and params in ((4, 2.0), (16, 5.0)):
        fin = np.isfinite(x)
        print('%d segments, largest %d cells, %.0f %% of the finite cells removed'
              % (len(np.unique(want[3][fin])), want[2].max(), 100.0 * want[1].sum() / fin.sum()))
        assert len(np.unique(want[3][fin])) > 1000 and want[1].any() and not want[1][fin].all()


# ---------------------------------------------------------------------------------------------
# 2. maps that stress the union-find across tiles
# ---------------------------------------------------------------------------------------------
def test_one_segment_over_the_map():
    x = np.random.default_rng(1).normal(0, 5, (150, 150))
    want = check(x, 16, INF)
    assert (want[2] == 150 * 150).all() and (want[3] == 0).all() and not want[1].any()
    want = check(x, 150 * 150, INF)
    assert want[1].all()


@pytest.mark.parametrize('shape', [(1, 20000), (20000, 1)], ids=lambda s: '%dx%d' % s)
def test_long_row_and_column(shape):
    n = max(shape)
    ramp = 0.5 * np.arange(n, dtype=np.float64)
    want = check(ramp.reshape(shape), 50, 1.0)
    assert (want[2] == n).all() and (want[3] == 0).all()
    broken = (ramp + 10.0 * (np.arange(n) // 97)).reshape(shape)      # a break every 97 cells
    want = check(broken, 50, 1.0)
    assert want[2].max() == 97 and want[1].sum() == n % 97 == 18
    assert np.array_equal(np.unique(want[3]), np.arange(0, n, 97))


def spiral(n):
    """A one-cell-wide corridor winding inwards from (0, 0) between NaN walls."""
    x = np.full((n, n), np.nan)
    i, j, di, dj, k = 0, 0, 0, 1, 1
    x[0, 0] = 0.0
    while True:
        for _ in range(2):      # straight on, else one turn to the right
            ni, nj, ai, aj = i + di, j + dj, i + 2 * di, j + 2 * dj
            ahead = 0 <= ai < n and 0 <= aj < n and np.isfinite(x[ai, aj])
            if 0 <= ni < n and 0 <= nj < n and np.isnan(x[ni, nj]) and not ahead:
                break
            di, dj = dj, -di
        else:
            return x
        i, j = ni, nj
        x[i, j] = 1e-3 * k
        k += 1


def serpentine(H, W):
    x = np.full((H, W), np.nan)
    x[::2] = 1.0
    x[1::4, -1] = 1.0
    x[3::4, 0] = 1.0
    return x


def test_spiral_and_serpentine():
    x = spiral(129)
    cells = int(np.isfinite(x).sum())
    assert cells > 129 * 129 // 2 - 200
    want = check(x, 16, 0.0015)
    fin = np.isfinite(x)
    assert (want[2][fin] == cells).all() and (want[3][fin] == 0).all()
    want = check(x[::-1, ::-1], 16, 0.0015)      # the root is the corridor's far end
    assert (want[2][fin[::-1, ::-1]] == cells).all()
    x = serpentine(129, 129)
    want = check(x, 16, 0.0)
    fin = np.isfinite(x)
    assert (want[2][fin] == fin.sum()).all() and fin.sum() == 65 * 129 + 64
    want = check(serpentine(130, 67).T, 16, 0.0)
    assert len(np.unique(want[3])) == 2


def test_checkerboards():
    i, j = np.mgrid[0:129, 0:67]
    odd = (i + j) % 2 == 1
    x = noise(129, 67, share=0.0)
    x[odd] = np.nan
    want = check(x, 1, INF)
    assert (want[2][~odd] == 1).all() and np.array_equal(want[1].astype(bool), ~odd)
    assert np.array_equal(want[3][~odd], (i * 67 + j)[~odd])
    check(x, 0, INF)
    x = np.where(odd, 10.0, 0.0)
    want = check(x, 0, 1.0)
    assert (want[2] == 1).all() and np.array_equal(want[3], i * 67 + j)
    assert check(x, 1, 1.0)[1].all()
    assert (check(x, 1, 10.0)[2] == 129 * 67).all()


def test_combs_across_a_tile_edge():
    x = np.full((100, 130), np.nan)
    x[:, ::2] = 1.0                       # teeth only: 65 segments of 100 cells, each across row 64
    want = check(x, 99, 0.0)
    assert not want[1].any() and (want[2][:, ::2] == 100).all() and len(np.unique(want[3])) == 66
    assert check(x, 100, 0.0)[1][:, ::2].all()
    x[99, :] = 1.0                        # a spine at the far end: one segment, its root at (0, 0)
    want = check(x, 99, 0.0)
    fin = np.isfinite(x)
    assert (want[2][fin] == fin.sum()).all() and (want[3][fin] == 0).all()
    check(x.T, 99, 0.0)


def test_corner_contact_stays_separate():
    x = np.full((130, 130), np.nan)
    x[60:64, 60:64] = 1.0
    x[64:68, 64:68] = 1.0                 # touches the first block only across the tile corner
    x[30:32, 32] = 1.0
    x[32, 30:32] = 1.0                    # (and across the corner of a tile of 32)
    want = check(x, 15, INF)
    assert want[2].max() == 16 and len(np.unique(want[3])) == 5 and want[1].sum() == 4
    want = check(x, 16, INF)
    assert want[1].sum() == 36


# ---------------------------------------------------------------------------------------------
# 3. the threshold at a tile seam, the planted case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transpose', [False, True])
def test_threshold_at_the_seam(transpose):
    x = np.zeros((70, 130))
    x[10, 62:67] = 5.0                    # 5 cells over the edge between columns 63 and 64
    x[62:66, 100] = 5.0                   # 4 cells over the edge between rows 63 and 64
    x[63:65, 127:129] = 5.0               # 4 cells around a tile corner
    if transpose:
        x = np.ascontiguousarray(x.T)
    blob = x == 5.0
    want = check(x, 5, 1.0)
    assert np.array_equal(want[1].astype(bool), blob)
    want = check(x, 4, 1.0)               # max_size + 1 cells: kept
    assert want[1].sum() == 8 and not want[1][(10, 64) if not transpose else (64, 10)]
    assert not check(x, 3, 1.0)[1].any()


def test_planted_case():
    p, x, mark = planted()
    want = check(x, 16, 1.0)
    assert np.array_equal(want[1].astype(bool), mark) and mark.sum() == 254
    out, holes = engine.fill_holes(engine.filter_speckles(dev(x), 16, 1.0), 16, return_holes=True)
    assert np.array_equal(host(holes).astype(bool), mark)
    assert np.abs(host(out) - p).max() <= 1e-3


# ---------------------------------------------------------------------------------------------
# 4. mechanics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(33, 31), (65, 130)], ids=lambda s: '%dx%d' % s)
def test_batch_equals_single_calls(shape):
    x = np.stack([noise(*shape, seed=1), np.full(shape, np.nan), noise(*shape, seed=2, share=0.5)])
    x[1].flat[::3] = np.inf
    got = run(x, 4, 2.0)
    assert got[0].shape == x.shape
    for m in range(3):
        one = run(x[m], 4, 2.0)
        assert one[0].shape == shape
        assert raw_bits(got[0][m], one[0]) and all(np.array_equal(g[m], o) for g, o in zip(got[1:], one[1:]))
    assert equal(got, speckle_restate(x, 4, 2.0))
    assert raw_bits(got[0][1], x[1]) and not got[1][1].any() and not got[2][1].any() and (got[3][1] == -1).all()


@pytest.mark.parametrize('shape', [(33, 31), (65, 130), (150, 150)], ids=lambda s: '%dx%d' % s)
def test_in_place(shape):
    x = noise(*shape, seed=5)
    want = run(x, 4, 2.0)
    t = dev(x)
    got = engine.filter_speckles(t, 4, 2.0, out=t, return_removed=True)
    assert got[0] is t and raw_bits(host(t), want[0]) and np.array_equal(host(got[1]), want[1])
    src, o = dev(x), torch.empty(shape, dtype=torch.float64, device='cuda')
    assert engine.filter_speckles(src, 4, 2.0, out=o) is o
    assert raw_bits(host(o), want[0]) and raw_bits(host(src), x)      # the input is untouched
    only = engine.filter_speckles(dev(x), 4, 2.0, return_labels=True)
    assert len(only) == 2 and np.array_equal(host(only[1]), want[3])


def test_side_stream():
    x = noise(65, 130, seed=7)
    want = speckle_restate(x, 4, 2.0)
    s = torch.cuda.Stream()
    t = dev(x)
    torch.cuda.synchronize()
    got = engine.filter_speckles(t, 4, 2.0, return_removed=True, stream=s)
    with torch.cuda.stream(s):
        h = [g.cpu() for g in got]          # a read on that stream
    assert same_bits(h[0].numpy(), want[0]) and np.array_equal(h[1].numpy(), want[1])


def test_consecutive_calls_are_bit_identical():
    for x, params in [(noise(150, 150, seed=8), (16, 5.0)), (planted()[1], (16, 1.0))]:
        t = dev(x)
        a, b = run(t, *params), run(t, *params)
        assert raw_bits(a[0], b[0]) and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))


@pytest.mark.parametrize('tile', ['16', '32', '64', '48'])
def test_tile_side_is_invisible(tile, monkeypatch):
    """DM_SPECKLE_TILE (16, 32 or 64; anything else is 64) moves the seams only."""
    cases = [(noise(150, 150, seed=9), (16, 5.0)), (noise(33, 31, seed=9), (4, 2.0)), (planted()[1], (16, 1.0)),
             (spiral(67), (16, 0.0015))]
    ref = [run(x, *p) for x, p in cases]
    monkeypatch.setenv('DM_SPECKLE_TILE', tile)
    for (x, p), r in zip(cases, ref):
        got = run(x, *p)
        assert raw_bits(got[0], r[0]) and all(np.array_equal(g, q) for g, q in zip(got[1:], r[1:]))
    assert equal(run(*cases[0][:1], *cases[0][1]), speckle_restate(cases[0][0], *cases[0][1]))


def test_arguments():
    t = dev(noise(5, 7))
    with pytest.raises(ValueError):
        engine.filter_speckles(t.float(), 4, 1.0)
    with pytest.raises(ValueError):
        engine.filter_speckles(t.cpu(), 4, 1.0)
    with pytest.raises(ValueError):
        engine.filter_speckles(t[None, None], 4, 1.0)
    for bad in [(-1, 1.0), (1.5, 1.0), (True, 1.0), (4, -1.0), (4, float('nan')), (4, None)]:
        with pytest.raises(ValueError):
            engine.filter_speckles(t, *bad)
    with pytest.raises(ValueError):
        engine.filter_speckles(t, 4, 1.0, out=torch.empty((7, 5), dtype=torch.float64, device='cuda'))
    e = torch.empty((0, 7), dtype=torch.float64, device='cuda')
    assert tuple(engine.filter_speckles(e, 4, 1.0).shape) == (0, 7)


# ---------------------------------------------------------------------------------------------
# 5. ImageCutSolver(speckle=) and shard.solve_image_sharded(speckle=)
# ---------------------------------------------------------------------------------------------
PAIR = dict(shape=(52, 100), seed=7, dx=2, h0=16, w0=32, ws=5)
MODES = ['elevation', 'elevation2', 'distance']
SPECKLE = (3, 0.25)


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(*PAIR['shape'], seed=PAIR['seed'], dx=PAIR['dx'])


@pytest.mark.parametrize('fill', [None, 16])
@pytest.mark.parametrize('consistency', [None, 1.0])
@pytest.mark.parametrize('stride', [(16, 32), (12, 24)])
def test_image_cut_solver_speckle(pair, stride, consistency, fill):
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = pair
    kw = dict(image_size=[16, 32], stride=list(stride), window_size=5, degree_map_mode=list(MODES),
              consistency=consistency)
    plain = ImageCutSolver(a, b, **kw)
    d0, o0 = plain()
    assert plain.speckle is None and plain.speckle_map is None
    none = ImageCutSolver(a, b, speckle=None, fill=fill, **kw)
    solver = ImageCutSolver(a, b, speckle=SPECKLE, fill=fill, **kw)
    d1, o1 = solver()
    assert solver.speckle == SPECKLE and d1 is solver.d_map
    want, removed = engine.filter_speckles(dev(d0), *SPECKLE, return_removed=True)
    filtered = host(want)
    assert equal(run(d0, *SPECKLE), speckle_restate(d0, *SPECKLE))
    if fill is not None:
        want = engine.fill_holes(want, fill)
    assert same_bits(d1, host(want))
    assert solver.speckle_map.dtype == bool and solver.speckle_map.shape == d0.shape
    assert np.array_equal(solver.speckle_map, host(removed).astype(bool))
    assert not (solver.speckle_map & ~np.isfinite(d0)).any()
    print('%d of %d finite cells removed' % (solver.speckle_map.sum(), np.isfinite(d0).sum()))
    assert 0 < solver.speckle_map.sum() < np.isfinite(d0).sum() / 2
    if fill is None:
        assert solver.hole_map is None
        assert np.array_equal(np.isnan(d1), np.isnan(d0) | solver.speckle_map)
    else:
        assert np.array_equal(solver.hole_map, np.isnan(filtered))
        assert np.isfinite(d1).all()
    assert same_bits(o1, o0)
    if consistency is None:
        assert solver.consistency_map is None
    else:
        assert same_bits(solver.consistency_map, plain.consistency_map)
    # speckle=None: the bits of the solver as it was
    dn, on = none()
    assert none.speckle_map is None and same_bits(on, o0)
    assert same_bits(dn, d0 if fill is None else host(engine.fill_holes(dev(d0), fill)))


@pytest.mark.parametrize('fill', [None, 16])
@pytest.mark.parametrize('consistency', [None, 1.0])
def test_solve_image_sharded_speckle_on_device(pair, consistency, fill):
    """shard.solve_image_sharded's own speckler (engine.filter_speckles on the stitched device map)."""
    from deepmatching_stereo_matching_amd import shard
    a, b = pair
    args = (a, b, [16, 32], [12, 24], 5, NCC, MODES)
    ref = shard.solve_image_sharded(*args, consistency=consistency)
    got = shard.solve_image_sharded(*args, consistency=consistency, speckle=SPECKLE, fill=fill)
    extra = 1 if fill is None else 2
    assert len(got) == len(ref) + extra and got[len(ref)].dtype == torch.uint8
    want, removed = engine.filter_speckles(ref[0], *SPECKLE, return_removed=True)
    assert torch.equal(got[len(ref)], removed)
    if fill is not None:
        holes = torch.isnan(want)
        want = engine.fill_holes(want, fill)
        assert got[-1].dtype == torch.uint8 and torch.equal(got[-1].bool(), holes)
    assert same_bits(host(got[0]), host(want))
    for g, r in zip(got[1:len(ref)], ref[1:]):
        assert same_bits(host(g), host(r))
    same = shard.solve_image_sharded(*args, consistency=consistency, speckle=None, fill=fill)
    assert len(same) == len(ref) + extra - 1 and same_bits(host(same[1]), host(ref[1]))
    assert same_bits(host(same[0]), host(ref[0] if fill is None else engine.fill_holes(ref[0], fill)))
