"""Speckle filter, host side (no GPU): the plain-loop restatement of the definition
(speckle_restate: what dm_filter_speckles must equal bit for bit) against scipy's labelling,
the planted-blob case the filter exists for (remove the blobs first and the fill recovers the
plane), thresholds and special values, argument validation of the two C entries (it returns
before any HIP call) and of the keyword, and the sharded path with the oracle as tile solver,
a host stitcher and the restatement injected as the speckler -- single process and gloo world
size 2.

Comparisons are bitwise (int64 views, NaN positions equal)."""
import ctypes
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard

from test_fill_host import (GEOM, MODES, _case, _free_port, _host_fill, _host_stitch, _host_stitch_fb,
                            _oracle_tiles, fill_restate, plane, raw_bits, same_bits)


@pytest.fixture(scope='module', autouse=True)
def entries():
    """What this file restates and checks is the pair of C entries: without them nothing here holds."""
    lib = L.load()
    assert hasattr(lib, 'dm_filter_speckles') and hasattr(lib, 'dm_speckle_bytes')
    assert callable(getattr(engine, 'filter_speckles', None)) and callable(getattr(engine, 'speckle_params', None))


# ---------------------------------------------------------------------------------------------
# the definition: sequential union-find in plain loops, the parent always the smaller index
# ---------------------------------------------------------------------------------------------
def _speckle_one(x, max_size, max_diff):
    H, W = x.shape
    fin = np.isfinite(x)
    parent = list(range(H * W))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:      # (sequential, so compressing the path is safe)
            parent[a], a = r, parent[a]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    v = x.tolist()
    ok = fin.tolist()
    for i in range(H):
        for j in range(W):
            if not ok[i][j]:
                continue
            a = v[i][j]
            with np.errstate(all='ignore'):
                if j > 0 and ok[i][j - 1] and abs(np.float64(a) - np.float64(v[i][j - 1])) <= max_diff:
                    union(i * W + j, i * W + j - 1)
                if i > 0 and ok[i - 1][j] and abs(np.float64(a) - np.float64(v[i - 1][j])) <= max_diff:
                    union(i * W + j, (i - 1) * W + j)
    label = np.full(H * W, -1, dtype=np.int32)
    size = np.zeros(H * W, dtype=np.uint32)
    count = {}
    for c in range(H * W):
        if ok[c // W][c % W]:
            r = find(c)
            parent[c] = r
            label[c] = r
            count[r] = count.get(r, 0) + 1
    for c in range(H * W):
        if label[c] >= 0:
            size[c] = count[label[c]]
    label, size = label.reshape(H, W), size.reshape(H, W)
    removed = fin & (size <= max_size)
    out = x.copy()
    out[removed] = np.nan
    return out, removed.astype(np.uint8), size, label


def speckle_restate(maps, max_size, max_diff):
    """The definition on [H][W] or [M][H][W] float64 maps -> (out, uint8 removed, uint32 size,
    int32 label)."""
    x = np.ascontiguousarray(maps, dtype=np.float64)
    if x.ndim == 2:
        return _speckle_one(x, max_size, max_diff)
    parts = [_speckle_one(m, max_size, max_diff) for m in x]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))


def planted(H=150, W=150, seed=150, blobs=60, offset=8.0):
    """The plane of test_fill_host with `blobs` blocks of 1..3 x 1..3 cells raised by `offset`
    -> (plane, planted map, mask of the raised cells)."""
    p = plane(H, W)
    rng = np.random.default_rng(seed)
    mark = np.zeros((H, W), dtype=bool)
    for _ in range(blobs):
        h, w = rng.integers(1, 4, 2)
        i = rng.integers(0, H - h + 1)
        j = rng.integers(0, W - w + 1)
        mark[i:i + h, j:j + w] = True
    x = p.copy()
    x[mark] += offset
    return p, x, mark


# ---------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------
def test_against_scipy_label():
    from scipy import ndimage
    rng = np.random.default_rng(65130)
    x = rng.normal(size=(65, 130))
    x[rng.uniform(size=x.shape) < 0.45] = np.nan
    fin = np.isfinite(x)
    lab, n = ndimage.label(fin)      # 4-connectivity is scipy's default structure
    assert 100 < n < 1000
    sizes = np.bincount(lab.ravel())
    want = np.where(fin, sizes[lab], 0)
    out, removed, size, label = speckle_restate(x, 3, np.inf)
    assert size.dtype == np.uint32 and label.dtype == np.int32 and removed.dtype == np.uint8
    assert np.array_equal(size, want)
    first = ndimage.minimum(np.arange(x.size).reshape(x.shape), lab, np.arange(1, n + 1))
    assert np.array_equal(label[fin], first[lab[fin] - 1])
    assert (label[~fin] == -1).all() and len(np.unique(label[fin])) == n
    assert np.array_equal(removed.astype(bool), fin & (want <= 3))
    share = removed.sum() / fin.sum()
    print('%d segments, %.1f %% of the finite cells removed' % (n, 100 * share))
    assert 0.01 < share < 0.5
    assert raw_bits(out[~removed.astype(bool)], x[~removed.astype(bool)]) and np.isnan(out[removed.astype(bool)]).all()


def test_planted_blobs_are_removed_and_the_fill_recovers_the_plane():
    p, x, mark = planted()
    out, removed, size, label = speckle_restate(x, 16, 1.0)
    assert np.array_equal(removed.astype(bool), mark)
    assert mark.sum() == 254 and len(np.unique(label[mark])) == 58 and size[mark].max() == 11
    assert (size[~mark] == 22246).all() and (label[~mark] == label[~mark].min()).all()
    with_filter = np.abs(fill_restate(out, 16)[0] - p).max()
    without = np.abs(fill_restate(x, 16)[0] - p).max()
    print('max error after the fill: %.3g with the filter, %.3g without' % (with_filter, without))
    assert with_filter <= 1e-3
    assert without == 8.0


def test_threshold():
    x = np.zeros((9, 9))
    x[3:6, 3:6] = 5.0
    out, removed, size, _ = speckle_restate(x, 9, 1.0)
    assert removed.sum() == 9 and np.isnan(out[3:6, 3:6]).all() and (size[3:6, 3:6] == 9).all()
    out, removed, size, _ = speckle_restate(x, 8, 1.0)
    assert removed.sum() == 0 and raw_bits(out, x) and (size[3:6, 3:6] == 9).all() and size[0, 0] == 72


def test_joining_is_per_pair():
    out, removed, size, label = speckle_restate(np.array([[0.0, 1.0, 2.0, 3.0]]), 3, 1.0)
    assert (size == 4).all() and (label == 0).all() and removed.sum() == 0
    out, removed, size, label = speckle_restate(np.array([[0.0, 1.0, 2.0, 3.0]]), 4, 1.0)
    assert removed.all() and np.isnan(out).all()


def test_special_values():
    # a difference exactly max_diff joins; just above it does not
    _, _, size, _ = speckle_restate(np.array([[0.0, 0.5, 1.0 + 2.0 ** -52 + 0.5]]), 0, 0.5)
    assert size.tolist() == [[2, 2, 1]]
    # -0.0 and 0.0 join at max_diff 0
    x = np.array([[-0.0, 0.0], [0.0, -0.0]])
    out, _, size, label = speckle_restate(x, 0, 0.0)
    assert (size == 4).all() and (label == 0).all() and raw_bits(out, x)
    # +-inf are holes; a difference that overflows joins only at max_diff = inf
    x = np.array([[1.0, np.inf, 1.0, -np.inf, 1.0], [1.7e308, -1.7e308, np.nan, 2.0, 2.0]])
    out, removed, size, label = speckle_restate(x, 1, 1e308)
    assert size.tolist() == [[1, 0, 1, 0, 3], [1, 1, 0, 3, 3]]
    assert label.tolist() == [[0, -1, 2, -1, 4], [5, 6, -1, 4, 4]]
    assert removed.tolist() == [[1, 0, 1, 0, 0], [1, 1, 0, 0, 0]]
    assert raw_bits(out[0, [1, 3]], x[0, [1, 3]]) and np.isnan(out[1, 2])
    _, _, size, _ = speckle_restate(x, 0, np.inf)
    assert size.tolist() == [[3, 0, 1, 0, 3], [3, 3, 0, 3, 3]]
    # an all-hole map comes back bit for bit
    allh = np.full((7, 5), np.nan)
    allh[1, 1], allh[2, 3], allh[6, 4] = np.inf, -np.inf, -np.nan
    out, removed, size, label = speckle_restate(allh, 100, np.inf)
    assert raw_bits(out, allh) and not removed.any() and not size.any() and (label == -1).all()
    # max_size = 0 is a copy that still reports
    rng = np.random.default_rng(5)
    x = rng.normal(0, 5, (11, 6))
    x[4, 3] = np.nan
    out, removed, size, label = speckle_restate(x, 0, 2.0)
    assert raw_bits(out, x) and not removed.any() and size[4, 3] == 0 and (size[np.isfinite(x)] > 0).all()
    # a batch is its maps one by one
    both = speckle_restate(np.stack([x, np.full(x.shape, np.nan)]), 2, 2.0)
    one = speckle_restate(x, 2, 2.0)
    assert all(b.shape == (2, 11, 6) and np.array_equal(b[0], o, equal_nan=True) for b, o in zip(both, one))
    assert not both[1][1].any() and not both[2][1].any() and (both[3][1] == -1).all()


# ---------------------------------------------------------------------------------------------
# 2. validation of the C entries and of the keyword
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_header_declares_speckle(lib):
    syms = L.header_symbols()
    assert 'dm_filter_speckles' in syms and 'dm_speckle_bytes' in syms
    assert 'dm_filter_speckles' in L.SIGNATURES and 'dm_speckle_bytes' in L.SIGNATURES
    assert lib.dm_abi_version() == 110


@pytest.mark.parametrize('args,code,needle', [
    ((None, 1, 4, 4, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'null'),
    ((P8, 1, 4, 4, 16, 1.0, None, None, None, None, P8), L.DM_ERR_ARG, 'null'),
    ((P8, 1, 4, 4, 16, 1.0, P8, None, None, None, None), L.DM_ERR_ARG, 'null'),
    ((P8, 0, 4, 4, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 0, 4, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 4, -1, 16, 1.0, P8, P8, P8, P8, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, -2, 4, 4, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 4, 4, -1, 1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'max_size'),
    ((P8, 1, 4, 4, 16, -1.0, P8, None, None, None, P8), L.DM_ERR_ARG, 'max_diff'),
    ((P8, 1, 4, 4, 16, -0.5e-300, P8, None, None, None, P8), L.DM_ERR_ARG, 'max_diff'),
    ((P8, 1, 4, 4, 16, float('nan'), P8, None, None, None, P8), L.DM_ERR_ARG, 'max_diff'),
    ((P8, 1, 4, 4, 16, float('-inf'), P8, None, None, None, P8), L.DM_ERR_ARG, 'max_diff'),
    ((P8, 1, 65536, 32768, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_UNSUPPORTED, 'cells'),   # H W = 2^31
    ((P8, 65536, 4, 4, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_UNSUPPORTED, 'cells'),       # grid z
    ((P8, 1, 64 * 65535 + 1, 1, 16, 1.0, P8, None, None, None, P8), L.DM_ERR_UNSUPPORTED, 'cells'),   # grid y
])
def test_filter_speckles_validation(lib, args, code, needle):
    assert lib.dm_filter_speckles(*args, None) == code
    assert needle in L.last_error()


def test_speckle_bytes(lib):
    refused = [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 65536, 32768), (65536, 4, 4),
               (1, 64 * 65535 + 1, 1), (1, 1, 64 * 65535 + 1)]
    for bad in refused:
        assert lib.dm_speckle_bytes(*bad) == 0, bad
    for H, W in [(1, 1), (1, 9), (5, 7), (64, 64), (65, 130), (150, 150), (1024, 1024), (46341, 46340),
                 (64 * 65535, 1), (1, 64 * 65535)]:
        prev = 0
        for M in (1, 2, 3, 7, 65535):
            b = lib.dm_speckle_bytes(M, H, W)
            assert b >= 8 * M * H * W and b % 16 == 0 and b >= prev, (M, H, W)      # int32 labels + uint32 sizes
            prev = b
    # inf is a valid max_diff and 0 a valid max_size: the refusal then is the shape's, not the arguments'
    assert lib.dm_filter_speckles(P8, 1, 65536, 32768, 0, float('inf'), P8, None, None, None, P8, None) == \
        L.DM_ERR_UNSUPPORTED


def test_speckle_params():
    assert engine.speckle_params((16, 1.0)) == (16, 1.0)
    assert engine.speckle_params([0, 0]) == (0, 0.0)
    assert engine.speckle_params((np.int64(3), np.float32(0.5))) == (3, 0.5)
    assert engine.speckle_params((3, float('inf'))) == (3, float('inf'))
    got = engine.speckle_params((7, 2))
    assert type(got[0]) is int and type(got[1]) is float
    for bad in [None, 16, (16,), (16, 1.0, 2), (-1, 1.0), (1.5, 1.0), (True, 1.0), ('3', 1.0), (3, -1.0),
                (3, float('nan')), (3, '1'), (3, None), (3, True), (3, float('-inf')), '31', (2 ** 31, 1.0)]:
        with pytest.raises(ValueError):
            engine.speckle_params(bad)


# ---------------------------------------------------------------------------------------------
# 3. the sharded path: oracle tile solver, host stitcher, the restatement as the speckler
# ---------------------------------------------------------------------------------------------
SPECKLE = (3, 0.25)


def _host_speckle(maps, max_size, max_diff):
    """speckler hook of solve_image_sharded: (filtered maps, uint8 mask)."""
    return speckle_restate(np.asarray(maps), max_size, max_diff)[:2]


def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map, err) of the consistency-checked solve: today's call."""
    a, b = _case()
    return [np.asarray(x) for x in _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)]


@pytest.fixture(scope='module')
def filtered(plain):
    return speckle_restate(plain[0], *SPECKLE)[:2]


def _check(got, plain, filtered, fill):
    assert len(got) == (5 if fill else 4)
    want = fill_restate(filtered[0], 16) if fill else (filtered[0], None)
    assert same_bits(got[0], want[0])
    assert same_bits(got[1], plain[1]) and same_bits(got[2], plain[2])      # never touched
    m = np.asarray(got[3])
    assert m.dtype == np.uint8 and np.array_equal(m, filtered[1])           # immediately before the hole mask
    if fill:
        h = np.asarray(got[4])
        assert h.dtype == np.uint8 and np.array_equal(h, want[1])
        assert np.array_equal(h.astype(bool), np.isnan(filtered[0]))


def test_sharded_speckle_single_process(plain, filtered):
    a, b = _case()
    kw = dict(stitcher=_host_stitch_fb, consistency=1.0, speckle=SPECKLE, speckler=_host_speckle)
    _check(_sharded(a, b, **kw), plain, filtered, False)
    _check(_sharded(a, b, fill=16, filler=_host_fill, **kw), plain, filtered, True)
    finite = np.isfinite(plain[0])
    removed = int(filtered[1].sum())
    print('%d of %d finite cells removed' % (removed, finite.sum()))
    assert 1 <= removed < finite.sum() / 2
    assert not (filtered[1].astype(bool) & ~finite).any()


def test_sharded_speckle_without_consistency():
    a, b = _case()
    ref = _sharded(a, b, stitcher=_host_stitch)
    got = _sharded(a, b, stitcher=_host_stitch, speckle=SPECKLE, speckler=_host_speckle)
    assert len(ref) == 2 and len(got) == 3
    want = speckle_restate(np.asarray(ref[0]), *SPECKLE)
    assert same_bits(got[0], want[0]) and same_bits(got[1], ref[1]) and np.array_equal(np.asarray(got[2]), want[1])


def test_sharded_speckle_none_is_unchanged(plain):
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, speckle=None, speckler=_host_speckle)
    assert len(got) == 3
    for g, r in zip(got, plain):
        assert same_bits(g, r)


def test_sharded_speckle_bad_keyword():
    a, b = _case()
    for bad in ((-1, 1.0), (3, -1.0), 16, (True, 1.0), (3, float('nan'))):
        with pytest.raises(ValueError):
            _sharded(a, b, stitcher=_host_stitch, speckle=bad, speckler=_host_speckle)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        kw = dict(stitcher=_host_stitch_fb, consistency=1.0, speckler=_host_speckle, filler=_host_fill)
        all_ = _sharded(a, b, speckle=SPECKLE, fill=16, **kw)
        nofill = _sharded(a, b, speckle=SPECKLE, **kw)
        root = _sharded(a, b, speckle=SPECKLE, fill=16, result='root', **kw)
        none = _sharded(a, b, speckle=None, **kw)
        q.put((rank, [np.asarray(x) for x in all_], [np.asarray(x) for x in nofill],
               [None if x is None else np.asarray(x) for x in root], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_speckle_gloo_world_2(plain, filtered):
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
    for rank, all_, nofill, root, none in res:
        _check(all_, plain, filtered, True)
        _check(nofill, plain, filtered, False)
        if rank == 0:
            _check(root, plain, filtered, True)
        else:
            assert root == [None, None, None, None, None]
        assert len(none) == 3
        for g, r in zip(none, plain):
            assert same_bits(g, r), rank
