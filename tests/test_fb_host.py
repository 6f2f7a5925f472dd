"""Forward-backward consistency check, host side (no GPU): argument validation of the two C
entries (it returns before any HIP call), engine.bidir_origins, and the sharded path with the
oracle as the per-rank tile solver and a numpy restatement of the check as the stitcher --
single process and gloo world size 2 -- against a direct oracle computation of the same maps.

The restatement (fb_restate) is the definition the kernels implement, float64 throughout:
  qi = floor(F[0] + 0.5), qj = floor(F[1] + 0.5); err = NaN unless 0 <= qi < h, 0 <= qj < w,
  else || B[0:2, qi, qj] - (i, j) ||; valid = err <= tol.
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


def fb_restate(F, B, tol):
    """(err [T][h][w], masked [T][3][h][w]) of float64 maps F, B [T][3][h][w]."""
    F, B = np.asarray(F, dtype=np.float64), np.asarray(B, dtype=np.float64)
    T, _, h, w = F.shape
    ii, jj = (x.astype(np.float64) for x in np.mgrid[0:h, 0:w])
    with np.errstate(all='ignore'):
        qi, qj = np.floor(F[:, 0] + 0.5), np.floor(F[:, 1] + 0.5)
        ok = (qi >= 0) & (qi < h) & (qj >= 0) & (qj < w)     # on the doubles, before any cast
        ki, kj = np.where(ok, qi, 0.0).astype(np.int64), np.where(ok, qj, 0.0).astype(np.int64)
        tt = np.arange(T)[:, None, None]
        dr, dc = B[tt, 0, ki, kj] - ii, B[tt, 1, ki, kj] - jj
        err = np.where(ok, np.sqrt(dr * dr + dc * dc), np.nan)
        valid = err <= tol
    masked = F.copy()
    masked[:, 0][~valid] = np.nan
    masked[:, 1][~valid] = np.nan
    return err, masked


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def place(tiles, n, stride, fill=np.nan):
    """Per-tile [T][h0][w0] maps placed as the stitch places them (tile t = j * n0 + i at
    (stride0 i, stride1 j), later tiles overwriting earlier ones, uncovered cells NaN)."""
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


MODES = ('elevation', 'distance')
GEOM = dict(image_size=[16, 16], stride=[12, 16], ws=5)


def _case():
    from deepmatching_stereo_matching_amd.synthetic import stereo_pair
    return stereo_pair(16 * 2 + 4 + 8, 16 * 3 + 4 + 8, seed=11, dx=2)


def _sharded(a, b, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, MODES,
                                     solver=_oracle_tiles, **kw)


@pytest.fixture(scope='module')
def direct():
    """The three maps computed straight from the oracle, one crop at a time."""
    from oracle import oracle as O
    a, b = _case()
    n, org = engine.cut_grid(a.shape, GEOM['image_size'], GEOM['stride'], GEOM['ws'])
    s = 16 + 4
    fwd = np.stack([O.solve_pair(a[r:r + s, c:c + s], b[r:r + s, c:c + s], 5)[0] for r, c in org])
    bwd = np.stack([O.solve_pair(b[r:r + s, c:c + s], a[r:r + s, c:c + s], 5)[0] for r, c in org])
    err, masked = fb_restate(fwd, bwd, 1.0)
    d = np.stack([place(np.stack([O.cal_map(m, mode) for m in masked]), n, GEOM['stride']) for mode in MODES])
    return d, place(fwd[:, 2], n, GEOM['stride']), place(err, n, GEOM['stride'])


@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_abi_version_unchanged(lib):
    assert lib.dm_abi_version() == 110


@pytest.mark.parametrize('args,needle', [
    ((None, P8, 1, 4, 4, 1.0, P8, None), 'null'),
    ((P8, None, 1, 4, 4, 1.0, P8, None), 'null'),
    ((P8, P8, 1, 4, 4, 1.0, None, None), 'null'),
    ((P8, P8, 0, 4, 4, 1.0, P8, None), 'shape'),
    ((P8, P8, 1, 0, 4, 1.0, P8, None), 'shape'),
    ((P8, P8, 1, 4, -1, 1.0, P8, None), 'shape'),
    ((P8, P8, 1, 4, 4, -0.5, P8, None), 'tolerance'),
    ((P8, P8, 1, 4, 4, float('nan'), P8, None), 'tolerance'),
    ((P8, P8, 1, 4, 4, float('-inf'), P8, None), 'tolerance'),
])
def test_fb_check_validation(lib, args, needle):
    assert lib.dm_fb_check(*args, None) == L.DM_ERR_ARG
    assert needle in L.last_error()


def _stitch_args(**kw):
    a = dict(f=P8, b=P8, n0=2, n1=2, h0=4, w0=4, s0=4, s1=4, modes=(ctypes.c_int32 * 1)(0), nm=1, tol=1.0,
             d=P8, s=P8, e=P8)
    a.update(kw)
    return (a['f'], a['b'], a['n0'], a['n1'], a['h0'], a['w0'], a['s0'], a['s1'], a['modes'], a['nm'], a['tol'],
            a['d'], a['s'], a['e'], None)


@pytest.mark.parametrize('kw,needle', [
    (dict(f=None), 'stitch'), (dict(b=None), 'stitch'), (dict(d=None), 'stitch'), (dict(s=None), 'stitch'),
    (dict(e=None), 'stitch'), (dict(n0=0), 'stitch'), (dict(n1=0), 'stitch'), (dict(s0=0), 'stitch'),
    (dict(s1=-3), 'stitch'), (dict(h0=0), 'stitch'), (dict(w0=0), 'stitch'),
    (dict(modes=None), 'stitch'), (dict(nm=9), 'stitch'),
    (dict(modes=(ctypes.c_int32 * 1)(9)), 'please input valid mode! (9)'),
    (dict(tol=-1.0), 'tolerance'), (dict(tol=float('nan')), 'tolerance'),
])
def test_stitch_fb_validation(lib, kw, needle):
    assert lib.dm_stitch_fb(*_stitch_args(**kw)) == L.DM_ERR_ARG
    assert needle in L.last_error()


def test_bidir_origins():
    org = [[0, 0], [12, 0], [0, 16]]
    got = engine.bidir_origins(org, 44)
    assert got.dtype == np.int64 and got.shape == (6, 2)
    assert got.tolist() == [[0, 0], [12, 0], [0, 16], [44, 0], [56, 0], [44, 16]]
    assert engine.bidir_origins(np.zeros((0, 2)), 7).shape == (0, 2)


def test_stack_pair_host():
    a, b = _case()
    A, Bk = engine.stack_pair(a, b)
    H = a.shape[0]
    assert np.array_equal(A[:H], a) and np.array_equal(A[H:], b)
    assert np.array_equal(Bk[:H], b) and np.array_equal(Bk[H:], a)
    with pytest.raises(ValueError):
        engine.stack_pair(a, b[:-1])


def test_restatement_on_specials():
    """The numpy restatement itself on the definition's corner cases (h = 5, w = 7)."""
    h, w = 5, 7
    F = np.zeros((1, 3, h, w))
    B = np.zeros((1, 3, h, w))
    ii, jj = np.mgrid[0:h, 0:w]
    B[0, 0], B[0, 1] = ii, jj                       # identity: every in-range walk returns to (qi, qj)
    F[0, 0], F[0, 1] = ii, jj
    F[0, 0, 0, 0] = 2.5                             # tie rounds up: qi = 3 -> err 3 from (0, 0)
    F[0, 0, 0, 1] = -0.5                            # qi = 0
    F[0, 0, 0, 2] = -0.51                           # out
    F[0, 0, 0, 3] = h - 0.5                         # out
    F[0, 0, 0, 4] = np.nextafter(h - 0.5, 0)        # in: qi = h - 1
    F[0, 1, 1, 0] = np.nan
    F[0, 1, 1, 1] = np.inf
    F[0, 1, 1, 2] = -1e300
    err, masked = fb_restate(F, B, 1.0)
    assert err[0, 0, 0] == 3.0 and err[0, 0, 1] == 0.0 and err[0, 0, 4] == h - 1
    assert np.isnan(err[0, 0, [2, 3]]).all() and np.isnan(err[0, 1, :3]).all()
    assert np.isnan(masked[0, :2, 0, 0]).all() and masked[0, 0, 0, 1] == -0.5
    assert np.array_equal(masked[0, 2], F[0, 2])
    assert (err[0, 2:] == 0).all()


def test_sharded_consistency_single_process(direct):
    a, b = _case()
    d, s, e = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)
    assert same_bits(d, direct[0]) and same_bits(s, direct[1]) and same_bits(e, direct[2])
    share = float(np.mean(e <= 1.0))
    assert 0.0 < share < 1.0, share       # the mask rejects some cells and keeps some


def test_sharded_consistency_none_is_unchanged():
    a, b = _case()
    got = _sharded(a, b, stitcher=_host_stitch, consistency=None)
    ref = _sharded(a, b, stitcher=_host_stitch)
    assert len(got) == 2 and len(ref) == 2
    n, org = engine.cut_grid(a.shape, GEOM['image_size'], GEOM['stride'], GEOM['ws'])
    want = _host_stitch(_oracle_tiles(a, b, org, 16, 16, 5, 5, True, False, 3, 3, 'average'), n, 16, 16,
                        GEOM['stride'], MODES)
    for g, r, w in zip(got, ref, want):
        assert same_bits(g, r) and same_bits(g, w)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _case()
        all_ = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0)
        root = _sharded(a, b, stitcher=_host_stitch_fb, consistency=1.0, result='root')
        plain = _sharded(a, b, stitcher=_host_stitch)
        q.put((rank, [np.asarray(x) for x in all_], [None if x is None else np.asarray(x) for x in root],
               [np.asarray(x) for x in plain]))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_sharded_consistency_gloo_world_2(direct):
    a, b = _case()
    plain_ref = _sharded(a, b, stitcher=_host_stitch)
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
    for rank, all_, root, plain in res:
        assert len(all_) == 3 and len(plain) == 2
        for got, want in zip(all_, direct):
            assert same_bits(got, want), rank
        if rank == 0:
            for got, want in zip(root, direct):
                assert same_bits(got, want)
        else:
            assert root == [None, None, None]
        for got, want in zip(plain, plain_ref):
            assert same_bits(got, want), rank
