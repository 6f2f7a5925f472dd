"""Hole fill, host side (no GPU): the numpy restatement of the definition (fill_restate: what
dm_fill_holes must equal bit for bit), its corner cases and its quality condition, argument
validation of the two C entries (it returns before any HIP call), the sharded path with the
oracle as tile solver, a host stitcher and the restatement injected as the filler -- single
process and gloo world size 2 -- and the claim the fill exists for: the reference's
Gauss-Seidel sweep survives a filled map and not an unfilled one.

Comparisons are bitwise (int64 views, NaN positions equal)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard


# ---------------------------------------------------------------------------------------------
# the definition: cascadic push-pull with masked Jacobi relaxation, float64, no contraction
# ---------------------------------------------------------------------------------------------
def pull(v, n):                     # -> level k+1 from level k; sides ceil(H/2), ceil(W/2)
    H, W = v.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    vp = np.zeros((2 * h, 2 * w))
    nq = np.zeros((2 * h, 2 * w))
    vp[:H, :W] = v
    nq[:H, :W] = n
    c = lambda a, i, j: a[i::2, j::2]                      # out-of-range children: v = 0, n = 0
    s = ((c(nq, 0, 0) * c(vp, 0, 0) + c(nq, 0, 1) * c(vp, 0, 1)) + c(nq, 1, 0) * c(vp, 1, 0)) + c(nq, 1, 1) * c(vp, 1, 1)
    m = ((c(nq, 0, 0) + c(nq, 0, 1)) + c(nq, 1, 0)) + c(nq, 1, 1)  # exact count of finite level-0 cells below
    with np.errstate(all='ignore'):
        return np.where(m > 0, s / m, 0.0), m


def push(v, n, p):                  # cells with n == 0 take the 9/3/3/1 interpolation of level k+1
    H, W = v.shape
    h, w = p.shape
    i, j = np.arange(H), np.arange(W)
    I, J = i >> 1, j >> 1
    I2 = np.clip(I + np.where(i & 1, 1, -1), 0, h - 1)
    J2 = np.clip(J + np.where(j & 1, 1, -1), 0, w - 1)
    a, b, c_, d = p[I][:, J], p[I2][:, J], p[I][:, J2], p[I2][:, J2]
    return np.where(n > 0, v, (((9.0 * a + 3.0 * b) + 3.0 * c_) + d) * 0.0625)


def relax(v, hole, iters):          # Jacobi: all reads from the previous iterate; index-clamped neighbours
    H, W = v.shape
    r, q = np.arange(H), np.arange(W)
    for _ in range(iters):
        U, D = v[np.clip(r - 1, 0, H - 1)], v[np.clip(r + 1, 0, H - 1)]
        Lf, R = v[:, np.clip(q - 1, 0, W - 1)], v[:, np.clip(q + 1, 0, W - 1)]
        v = np.where(hole, (((U + D) + Lf) + R) * 0.25, v)
    return v


def fill(x, iters):
    hole = ~np.isfinite(x)
    if hole.all():
        return x.copy()                                    # nothing to fill from: output = input, bit for bit
    vs, ns = [np.where(hole, 0.0, x)], [(~hole).astype(np.float64)]
    while vs[-1].shape != (1, 1):
        v, n = pull(vs[-1], ns[-1])
        vs.append(v)
        ns.append(n)
    p = vs[-1]
    for k in range(len(vs) - 2, -1, -1):                   # top down; `iters` Jacobi steps at EVERY level,
        p = relax(push(vs[k], ns[k], p), ns[k] == 0, iters)  # on that level's empty cells only
    return p


def fill_restate(maps, iters=16):
    """The definition on [H][W] or [M][H][W] float64 maps -> (filled, uint8 hole mask)."""
    x = np.asarray(maps, dtype=np.float64)
    holes = (~np.isfinite(x)).astype(np.uint8)
    if x.ndim == 2:
        return fill(x, iters), holes
    return np.stack([fill(m, iters) for m in x]), holes


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def raw_bits(a, b):
    """Equality of the 64-bit patterns themselves (NaN payloads and signs included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def plane(H, W):
    i, j = np.mgrid[0:H, 0:W]
    return 0.03125 * i - 0.0625 * j + 3


def holed_plane(H, W, seed=7, share=0.3, big=40):
    """The issue's quality case: the plane with `share` random holes plus one big x big hole."""
    rng = np.random.default_rng(seed)
    x = plane(H, W)
    x[rng.uniform(size=x.shape) < share] = np.nan
    if big:
        r, c = (H - big) // 2, (W - big) // 2
        x[r:r + big, c:c + big] = np.nan
    return x


# ---------------------------------------------------------------------------------------------
# 1. validation of the C entries
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_abi_version_unchanged(lib):
    assert lib.dm_abi_version() == 110


def test_header_declares_fill():
    syms = L.header_symbols()
    assert 'dm_fill_holes' in syms and 'dm_fill_bytes' in syms
    assert 'dm_fill_holes' in L.SIGNATURES and 'dm_fill_bytes' in L.SIGNATURES


@pytest.mark.parametrize('args,code,needle', [
    ((None, 1, 4, 4, 16, P8, None, P8), L.DM_ERR_ARG, 'null'),
    ((P8, 1, 4, 4, 16, None, None, P8), L.DM_ERR_ARG, 'null'),
    ((P8, 1, 4, 4, 16, P8, None, None), L.DM_ERR_ARG, 'null'),
    ((P8, 0, 4, 4, 16, P8, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 0, 4, 16, P8, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 4, -1, 16, P8, None, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, -2, 4, 4, 16, P8, P8, P8), L.DM_ERR_ARG, 'shape'),
    ((P8, 1, 4, 4, -1, P8, None, P8), L.DM_ERR_ARG, 'iterations'),
    ((P8, 1, 4, 4, 4097, P8, None, P8), L.DM_ERR_ARG, 'iterations'),
    ((P8, 1, 65536, 32768, 16, P8, None, P8), L.DM_ERR_UNSUPPORTED, 'cells'),      # H W = 2^31
])
def test_fill_holes_validation(lib, args, code, needle):
    assert lib.dm_fill_holes(*args, None) == code
    assert needle in L.last_error()


def test_fill_bytes(lib):
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 65536, 32768)]:
        assert lib.dm_fill_bytes(*bad) == 0, bad
    for H, W in [(1, 1), (1, 9), (5, 7), (65, 130), (150, 150), (1024, 1024), (46341, 46340)]:
        prev = 0
        for M in (1, 2, 3, 7):
            b = lib.dm_fill_bytes(M, H, W)
            assert b > 0 and b >= prev, (M, H, W)
            prev = b


# ---------------------------------------------------------------------------------------------
# 2. the restatement on the definition's corner cases
# ---------------------------------------------------------------------------------------------
def test_restatement_on_specials():
    one = np.array([[np.nan]])
    assert raw_bits(fill(one, 16), one)                                 # 1 x 1 NaN stays NaN
    x = np.full((9, 13), np.nan)
    x[6, 2] = -7.25
    for iters in (0, 3, 16):
        assert raw_bits(fill(x, iters), np.full((9, 13), -7.25))        # one finite cell: a constant map
    row = np.array([[np.inf, 1.0, -np.inf, 3.0, np.nan]])
    assert raw_bits(fill(row, 0), np.array([[1.0, 1.0, 2.5, 3.0, 2.25]]))
    rng = np.random.default_rng(3)
    full = rng.normal(size=(11, 6))
    full[4, 3] = -0.0
    assert np.signbit(full[4, 3])
    for iters in (0, 16):
        assert raw_bits(fill(full, iters), full)                        # no holes: a bit-exact copy, -0.0 too
    allh = np.full((7, 5), np.nan)
    allh[1, 1], allh[2, 3], allh[6, 4] = np.inf, -np.inf, -np.nan
    assert raw_bits(fill(allh, 16), allh)                               # all holes: output = input
    filled, holes = fill_restate(np.stack([x, np.where(np.isnan(x), 1.0, np.nan)]), 2)
    assert holes.dtype == np.uint8 and holes.sum() == 9 * 13 and np.isfinite(filled).all()
    assert raw_bits(filled[1], np.ones((9, 13)))


# ---------------------------------------------------------------------------------------------
# 3. the quality condition
# ---------------------------------------------------------------------------------------------
def test_quality_on_plane():
    """150 x 150 plane, 30 % random holes + a 40 x 40 hole.  Bound 0.125 = two pixels of the
    steeper slope (0.0625 per column); the prototype measured 0.061 - 0.065."""
    truth = plane(150, 150)
    x = holed_plane(150, 150)
    hole = np.isnan(x)
    assert 0.3 < hole.mean() < 0.4
    f16, f0 = fill(x, 16), fill(x, 0)
    e16, e0 = np.abs(f16 - truth)[hole].max(), np.abs(f0 - truth)[hole].max()
    print('max hole error: iters=16 %.4f, iters=0 %.4f' % (e16, e0))
    assert e16 <= 0.125
    assert e16 < e0
    fin = x[~hole]
    A = np.abs(fin).max()
    for f in (f16, f0):
        assert raw_bits(f[~hole], fin)
        assert np.isfinite(f).all()
        assert f[hole].min() >= fin.min() - 1e-9 * A and f[hole].max() <= fin.max() + 1e-9 * A


# ---------------------------------------------------------------------------------------------
# 4. the sharded path: oracle tile solver, host stitcher, the restatement as the filler
#    (helpers as in tests/test_fb_host.py)
# ---------------------------------------------------------------------------------------------
def fb_restate(F, B, tol):
    """(err [T][h][w], masked [T][3][h][w]) of float64 maps F, B [T][3][h][w]."""
    F, B = np.asarray(F, dtype=np.float64), np.asarray(B, dtype=np.float64)
    T, _, h, w = F.shape
    ii, jj = (x.astype(np.float64) for x in np.mgrid[0:h, 0:w])
    with np.errstate(all='ignore'):
        qi, qj = np.floor(F[:, 0] + 0.5), np.floor(F[:, 1] + 0.5)
        ok = (qi >= 0) & (qi < h) & (qj >= 0) & (qj < w)
        ki, kj = np.where(ok, qi, 0.0).astype(np.int64), np.where(ok, qj, 0.0).astype(np.int64)
        tt = np.arange(T)[:, None, None]
        dr, dc = B[tt, 0, ki, kj] - ii, B[tt, 1, ki, kj] - jj
        err = np.where(ok, np.sqrt(dr * dr + dc * dc), np.nan)
        valid = err <= tol
    masked = F.copy()
    masked[:, 0][~valid] = np.nan
    masked[:, 1][~valid] = np.nan
    return err, masked


def place(tiles, n, stride, fill=np.nan):
    T, h0, w0 = tiles.shape
    out = np.full((stride[0] * (n[0] - 1) + h0, stride[1] * (n[1] - 1) + w0), fill)
    for t in range(T):
        i, j = t % n[0], t // n[0]
        out[stride[0] * i:stride[0] * i + h0, stride[1] * j:stride[1] * j + w0] = tiles[t]
    return out


def _oracle_tiles(img1, img2, origins, h0, w0, ws, method, sub_pix, filtering, fws, fnum, fmode,
                  device=None):
    from oracle import oracle as O
    feat = 'cv2.TM_CCOEFF_NORMED' if method == 5 else 'cv2.TM_CCOEFF'
    out = []
    for r, c in np.asarray(origins).reshape(-1, 2):
        a = img1[r:r + h0 + ws - 1, c:c + w0 + ws - 1]
        b = img2[r:r + h0 + ws - 1, c:c + w0 + ws - 1]
        out.append(O.solve_pair(a, b, ws, feat, sub_pix)[0])
    return torch.from_numpy(np.stack(out))


def _host_stitch(match, n, h0, w0, stride, modes):
    from oracle import oracle as O
    m = np.asarray(match)
    d = np.stack([place(np.stack([O.cal_map(x, mode) for x in m]), n, stride) for mode in modes])
    return d, place(m[:, 2], n, stride)


def _host_stitch_fb(fwd, bwd, n, h0, w0, stride, modes, tol):
    err, masked = fb_restate(np.asarray(fwd), np.asarray(bwd), tol)
    d, s = _host_stitch(masked, n, h0, w0, stride, modes)
    return d, s, place(err, n, stride)


def _host_fill(maps, iters):
    """filler hook of solve_image_sharded: (filled maps, uint8 hole mask)."""
    return fill_restate(np.asarray(maps), iters)


MODES = ('elevation', 'distance')
GEOM = dict(image_size=[16, 16], stride=[12, 16], ws=5)


def _case():
    from deepmatching_stereo_matching_amd.synthetic import stereo_pair
    return stereo_pair(16 * 2 + 4 + 8, 16 * 3 + 4 + 8, seed=11, dx=2)


def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


@pytest.fixture(scope='module')
def unfilled():
    """(d_map, out_map, err) of the consistency-checked solve, no fill: today's call."""
    a, b = _case()
    return [np.asarray(x) for x in _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)]


@pytest.fixture(scope='module')
def filled(unfilled):
    return fill_restate(unfilled[0], 16)


def _check_filled(got, unfilled, filled):
    assert len(got) == 4
    assert same_bits(got[0], filled[0])
    assert same_bits(got[1], unfilled[1]) and same_bits(got[2], unfilled[2])     # never filled
    h = np.asarray(got[3])
    assert h.dtype == np.uint8 and np.array_equal(h, filled[1])


def test_sharded_fill_single_process(unfilled, filled):
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, fill=16, filler=_host_fill)
    _check_filled(got, unfilled, filled)
    assert unfilled[0].shape == (2, 28, 32)
    share = float(filled[1].mean())
    print('hole share %.3f' % share)
    assert 0.0 < share < 0.5
    assert np.isfinite(np.asarray(got[0])).all()
    assert np.array_equal(filled[1].astype(bool), np.isnan(unfilled[0]))


def test_sharded_fill_without_consistency():
    a, b = _case()
    ref = _sharded(a, b, stitcher=_host_stitch)
    got = _sharded(a, b, stitcher=_host_stitch, fill=3, filler=_host_fill)
    assert len(ref) == 2 and len(got) == 3
    want = fill_restate(np.asarray(ref[0]), 3)
    assert same_bits(got[0], want[0]) and same_bits(got[1], ref[1]) and np.array_equal(np.asarray(got[2]), want[1])


def test_sharded_fill_none_is_unchanged(unfilled):
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, fill=None, filler=_host_fill)
    assert len(got) == 3
    for g, r in zip(got, unfilled):
        assert same_bits(g, r)
    plain = _sharded(a, b, stitcher=_host_stitch, fill=None)
    ref = _sharded(a, b, stitcher=_host_stitch)
    assert len(plain) == 2 and len(ref) == 2
    for g, r in zip(plain, ref):
        assert same_bits(g, r)


def test_sharded_fill_bad_iterations():
    a, b = _case()
    for bad in (-1, 4097, 2.5, True):
        with pytest.raises(ValueError):
            _sharded(a, b, stitcher=_host_stitch, fill=bad, filler=_host_fill)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        kw = dict(stitcher=_host_stitch_fb, consistency=1.0, filler=_host_fill)
        all_ = _sharded(a, b, fill=16, **kw)
        root = _sharded(a, b, fill=16, result='root', **kw)
        none = _sharded(a, b, fill=None, **kw)
        q.put((rank, [np.asarray(x) for x in all_], [None if x is None else np.asarray(x) for x in root],
               [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_sharded_fill_gloo_world_2(unfilled, filled):
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
    for rank, all_, root, none in res:
        _check_filled(all_, unfilled, filled)
        if rank == 0:
            _check_filled(root, unfilled, filled)
        else:
            assert root == [None, None, None, None]
        assert len(none) == 3
        for g, r in zip(none, unfilled):
            assert same_bits(g, r), rank


# ---------------------------------------------------------------------------------------------
# 5. the pipeline claim: the reference's Gauss-Seidel sweep on the elevation map
# ---------------------------------------------------------------------------------------------
def test_optimize_loop_needs_the_fill(unfilled, filled):
    from oracle import oracle as O
    raw, dense = unfilled[0][0], filled[0][0]
    H, W = raw.shape
    ones = np.ones((H, W))
    out, err = O.optimize_loop(raw, ones, 0.5, 1, [H - 1, W - 1])
    nan_share = float(np.isnan(out).mean())
    print('unfilled: %.0f %% NaN after the sweep, error %r' % (100 * nan_share, err))
    assert nan_share > 0.5 and not np.isfinite(err)
    out, err = O.optimize_loop(dense, ones, 0.5, 1, [H - 1, W - 1])
    assert not np.isnan(out).any() and np.isfinite(err)
