"""Photo-consistency score, host side (no GPU): the plain-loop restatement of the definition
(photo_restate: what dm_photo_score must equal bit for bit), a vectorised restatement pinned to it
(photo_fast: the one the GPU tests use), the properties the header derives, the direct
resample-then-correlate form, the planted impulses the rejection exists for, argument validation
of the two C entries (it returns before any HIP call) and of the keywords, and the sharded chain
with the oracle as tile solver, a host stitcher and the restatement injected as the photoer --
single process and gloo world size 2.

Comparisons with the restatement are bitwise (int64 views)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair

from test_fill_host import (GEOM, _free_port, _host_fill, _host_stitch, _oracle_tiles, fill_restate, raw_bits,
                            same_bits)
from test_median_host import _host_median, median_restate
from test_speckle_host import _host_speckle, speckle_restate


@pytest.fixture(scope='module', autouse=True)
def entries():
    """What this file restates and checks is the pair of C entries: without them nothing here holds."""
    lib = L.load()
    assert hasattr(lib, 'dm_photo_score') and hasattr(lib, 'dm_photo_bytes')
    assert callable(getattr(engine, 'photo_score', None)) and callable(getattr(engine, 'photo_params', None))


# ---------------------------------------------------------------------------------------------
# the definition in plain loops: Python ints are exact, Python floats are IEEE doubles with one
# rounding per operation
# ---------------------------------------------------------------------------------------------
INF, NAN = float('inf'), float('nan')
DMAX = 1.7976931348623157e308
PAIRS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]      # k outer, l inner
SHIFT = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _finite(v):
    return -DMAX <= v <= DMAX      # (NaN fails both)


def _offsets(offset):
    return tuple(offset) if isinstance(offset, (tuple, list)) else (offset, offset)


def photo_restate(img1, img2, d_row, d_col, r, offset=0, min_score=None, maps=None):
    """The definition -> (score, warped) or, with min_score, (score, warped, rejected maps, uint8 mask)."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    H, W = d_row.shape
    A_, B_ = img1.tolist(), img2.tolist()
    R_, C_ = np.asarray(d_row, dtype=np.float64).tolist(), np.asarray(d_col, dtype=np.float64).tolist()
    D = 2 * r + 1
    n = D * D
    score = np.full((H, W), NAN)
    warped = np.full((H, W), NAN)
    for y in range(H):
        for x in range(W):
            dr, dc = R_[y][x], C_[y][x]
            if not (_finite(dr) and _finite(dc)):
                continue
            cy, cx = y + oy, x + ox
            py, px = float(cy) - dr, float(cx) - dc
            if not (0.0 <= py < float(Hi - 1) and 0.0 <= px < float(Wi - 1)):
                continue
            iy, ix = math.floor(py), math.floor(px)
            fy, fx = py - float(iy), px - float(ix)
            gy, gx = 1.0 - fy, 1.0 - fx
            w = [gy * gx, gy * fx, fy * gx, fy * fx]
            warped[y, x] = ((w[0] * float(B_[iy][ix]) + w[1] * float(B_[iy][ix + 1])) +
                            w[2] * float(B_[iy + 1][ix])) + w[3] * float(B_[iy + 1][ix + 1])
            if not (r <= cy <= Hi - 1 - r and r <= cx <= Wi - 1 - r):
                continue
            if not (float(r) <= py < float(Hi - r - 1) and float(r) <= px < float(Wi - r - 1)):
                continue
            sa = saa = 0
            S = [0, 0, 0, 0]
            AP = [0, 0, 0, 0]
            PP = {kl: 0 for kl in PAIRS}
            for u in range(D):
                for v in range(D):
                    a = A_[cy - r + u][cx - r + v]
                    p = [B_[iy - r + u + sy][ix - r + v + sx] for sy, sx in SHIFT]
                    sa += a
                    saa += a * a
                    for k in range(4):
                        S[k] += p[k]
                        AP[k] += a * p[k]
                    for k, l in PAIRS:
                        PP[k, l] += p[k] * p[l]
            VA = float(n * saa - sa * sa)
            CA = [float(n * AP[k] - sa * S[k]) for k in range(4)]
            num = ((w[0] * CA[0] + w[1] * CA[1]) + w[2] * CA[2]) + w[3] * CA[3]
            vb = None
            for k, l in PAIRS:
                t = ((1.0 if k == l else 2.0) * (w[k] * w[l])) * float(n * PP[k, l] - S[k] * S[l])
                vb = t if vb is None else vb + t
            if VA > 0.0 and vb > 0.0:
                t = num / math.sqrt(VA * vb)
                score[y, x] = 1.0 if t > 1.0 else (-1.0 if t < -1.0 else t)
            else:
                score[y, x] = 0.0
    if min_score is None:
        return score, warped
    return (score, warped) + _reject(score, min_score, maps)


def _reject(score, min_score, maps):
    rej = score < min_score      # (False where the score is NaN)
    out = np.array(maps, dtype=np.float64, copy=True)
    out[..., rej] = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
    return np.ascontiguousarray(out), rej.astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# the fast restatement: the windows as gathered stacks of planes, the integer sums in int64
# ---------------------------------------------------------------------------------------------
def photo_fast(img1, img2, d_row, d_col, r, offset=0, min_score=None, maps=None):
    """photo_restate, vectorised."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    D = 2 * r + 1
    n = D * D
    A64, B64 = img1.astype(np.int64), img2.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy + oy, xx + ox
    with np.errstate(invalid='ignore', over='ignore'):
        fin = (np.abs(d_row) <= DMAX) & (np.abs(d_col) <= DMAX)
        py = np.where(fin, cy.astype(np.float64) - np.where(fin, d_row, 0.0), -1.0)
        px = np.where(fin, cx.astype(np.float64) - np.where(fin, d_col, 0.0), -1.0)
    in4 = fin & (py >= 0.0) & (py < float(Hi - 1)) & (px >= 0.0) & (px < float(Wi - 1))
    iy = np.where(in4, np.floor(np.where(in4, py, 0.0)), 0.0).astype(np.int64)
    ix = np.where(in4, np.floor(np.where(in4, px, 0.0)), 0.0).astype(np.int64)
    fy, fx = py - iy.astype(np.float64), px - ix.astype(np.float64)
    gy, gx = 1.0 - fy, 1.0 - fx
    w = [gy * gx, gy * fx, fy * gx, fy * fx]
    ok = in4 & (cy >= r) & (cy <= Hi - 1 - r) & (cx >= r) & (cx <= Wi - 1 - r) & \
        (iy >= r) & (iy <= Hi - 2 - r) & (ix >= r) & (ix <= Wi - 2 - r)

    def at(img, rows, cols, good):
        return img[np.where(good, rows, 0), np.where(good, cols, 0)]

    q = [at(B64, iy + sy, ix + sx, in4).astype(np.float64) for sy, sx in SHIFT] if Hi > 1 and Wi > 1 else [0.0] * 4
    warped = np.where(in4, ((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2]) + w[3] * q[3], NAN)
    z = np.zeros((H, W), dtype=np.int64)
    sa, saa = z.copy(), z.copy()
    S = [z.copy() for _ in range(4)]
    AP = [z.copy() for _ in range(4)]
    PP = {kl: z.copy() for kl in PAIRS}
    for u in range(D):
        for v in range(D):
            a = at(A64, cy - r + u, cx - r + v, ok)
            p = [at(B64, iy - r + u + sy, ix - r + v + sx, ok) for sy, sx in SHIFT]
            sa += a
            saa += a * a
            for k in range(4):
                S[k] += p[k]
                AP[k] += a * p[k]
            for k, l in PAIRS:
                PP[k, l] += p[k] * p[l]
    VA = (n * saa - sa * sa).astype(np.float64)
    CA = [(n * AP[k] - sa * S[k]).astype(np.float64) for k in range(4)]
    num = ((w[0] * CA[0] + w[1] * CA[1]) + w[2] * CA[2]) + w[3] * CA[3]
    vb = None
    for k, l in PAIRS:
        t = ((1.0 if k == l else 2.0) * (w[k] * w[l])) * (n * PP[k, l] - S[k] * S[l]).astype(np.float64)
        vb = t if vb is None else vb + t
    pos = ok & (VA > 0.0) & (vb > 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        t = num / np.sqrt(np.where(pos, VA * vb, 1.0))
    t = np.where(t > 1.0, 1.0, np.where(t < -1.0, -1.0, t))
    score = np.where(ok, np.where(pos, t, 0.0), NAN)
    if min_score is None:
        return score, warped
    return (score, warped) + _reject(score, min_score, maps)


def photo_direct(img1, img2, d_row, d_col, r, offset=0):
    """The direct form: the bilinearly resampled patch, then the mean-removed correlation, in floating point."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    H, W = d_row.shape
    A, B = img1.astype(np.float64), img2.astype(np.float64)
    out = np.full((H, W), NAN)
    for y in range(H):
        for x in range(W):
            cy, cx = y + oy, x + ox
            py, px = cy - d_row[y, x], cx - d_col[y, x]
            if not (np.isfinite(py) and np.isfinite(px)):
                continue
            iy, ix = int(np.floor(py)), int(np.floor(px))
            if not (r <= cy <= Hi - 1 - r and r <= cx <= Wi - 1 - r and r <= iy <= Hi - 2 - r and r <= ix <= Wi - 2 - r):
                continue
            fy, fx = py - iy, px - ix
            a = A[cy - r:cy + r + 1, cx - r:cx + r + 1]
            p = [B[iy - r + sy:iy + r + 1 + sy, ix - r + sx:ix + r + 1 + sx] for sy, sx in SHIFT]
            b = (1 - fy) * (1 - fx) * p[0] + (1 - fy) * fx * p[1] + fy * (1 - fx) * p[2] + fy * fx * p[3]
            a0, b0 = a - a.mean(), b - b.mean()
            va, vb = (a0 * a0).sum(), (b0 * b0).sum()
            out[y, x] = (a0 * b0).sum() / np.sqrt(va * vb) if va > 0 and vb > 0 else 0.0
    return out


def planes(H, W, seed, kind='frac', amp=3.0):
    """Disparity planes: 'int' integers, 'frac' fractions of both signs, 'mixed' both plus -0.0 and specials."""
    rng = np.random.default_rng(100 * H + W + seed)
    dr, dc = rng.uniform(-amp, amp, (H, W)), rng.uniform(-amp, amp, (H, W))
    if kind == 'int':
        return np.round(dr), np.round(dc)
    if kind == 'mixed':
        u = rng.uniform(size=(H, W))
        dr, dc = np.where(u < 0.3, np.round(dr), dr), np.where((u > 0.2) & (u < 0.5), np.round(dc), dc)
        pool = np.array([-0.0, 0.0, NAN, -NAN, INF, -INF, 1e300, -1e300, 0.5, -0.25])
        for d in (dr, dc):
            m = rng.uniform(size=(H, W)) < 0.15
            d[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return np.ascontiguousarray(dr), np.ascontiguousarray(dc)


# ---------------------------------------------------------------------------------------------
# 1. the restatements and the properties of the definition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (5, 7), (12, 11)])
@pytest.mark.parametrize('r', [1, 2, 3])
def test_fast_equals_literal(shape, r):
    H, W = shape
    for seed, kind in enumerate(['int', 'frac', 'mixed']):
        for margin, off in [(r + 4, (r + 4, r + 4)), (r + 1, (r + 1, r + 2)), (2, (0, 1))]:
            a, b = stereo_pair(H + 2 * margin, W + 2 * margin + 1, seed=seed, dx=2)
            dr, dc = planes(H, W, seed, kind)
            maps = np.stack([dr, dc, dr + dc])
            lit = photo_restate(a, b, dr, dc, r, off, 0.5, maps)
            fast = photo_fast(a, b, dr, dc, r, off, 0.5, maps)
            for p, q in zip(lit, fast):
                assert raw_bits(p.astype(np.float64), q.astype(np.float64)), (shape, r, kind, margin)
                if margin == r + 4 and kind != 'mixed':      # this margin covers every disparity of `planes`
                    assert np.isfinite(lit[0]).all()


def test_borders_and_specials():
    """The patch exactly on each image border scores; one pixel past it, or a non-finite or huge disparity, does
    not; the extra row and column are required even at an integer position; warped follows its own rule."""
    r = 2
    a, b = stereo_pair(12, 14, seed=1, dx=0)
    one = lambda v: np.full((1, 1), float(v))
    sc = lambda dr, dc, off: photo_restate(a, b, one(dr), one(dc), r, off)
    # cell at pixel (5, 6): rows 3..7 of 12, patch rows iy-2..iy+3
    assert np.isfinite(sc(3, 0, (5, 6))[0][0, 0])              # iy = 2: patch rows 0..5
    assert np.isnan(sc(3.5, 0, (5, 6))[0][0, 0])               # iy = 1
    assert np.isfinite(sc(-3, 0, (5, 6))[0][0, 0])             # iy = 8: patch rows 6..11
    assert np.isnan(sc(-4, 0, (5, 6))[0][0, 0])                # iy = 9: row 12 is outside, though fy = 0
    assert np.isfinite(sc(0, 4, (5, 6))[0][0, 0]) and np.isnan(sc(0, 4.25, (5, 6))[0][0, 0])
    assert np.isfinite(sc(0, -4, (5, 6))[0][0, 0]) and np.isnan(sc(0, -5, (5, 6))[0][0, 0])
    # the img1 window: pixel (1, 6) has no window of radius 2, but a warped value
    s, w = sc(0, 0, (1, 6))
    assert np.isnan(s[0, 0]) and w[0, 0] == float(b[1, 6])
    s, w = sc(0, 0, (11, 6))                                   # the last row has no pixel below it
    assert np.isnan(s[0, 0]) and np.isnan(w[0, 0])
    for bad in (NAN, INF, -INF, 1e300, -1e300):
        for args in ((bad, 0), (0, bad)):
            s, w = sc(*args, (5, 6))
            assert np.isnan(s[0, 0]) and np.isnan(w[0, 0])
    s, w = sc(-0.0, -0.0, (5, 6))
    assert s[0, 0] == 1.0 and w[0, 0] == float(b[5, 6])
    s, w = sc(0.5, 0.25, (5, 6))
    want = 0.5 * (0.25 * float(b[4, 5]) + 0.75 * float(b[4, 6])) + 0.5 * (0.25 * float(b[5, 5]) + 0.75 * float(b[5, 6]))
    assert abs(w[0, 0] - want) < 1e-12 and -1.0 <= s[0, 0] <= 1.0


@pytest.mark.parametrize('r', [1, 2, 3])
def test_exact_one_on_true_shift(r):
    a, b = stereo_pair(52, 52, seed=3, dx=2)
    H = W = 48
    for fn in (photo_restate, photo_fast):
        s, w = fn(a, b, np.zeros((H, W)), np.full((H, W), 2.0), r, 2)
        scored = ~np.isnan(s)
        assert scored.sum() > 0.5 * H * W and (s[scored] == 1.0).all()
        assert np.array_equal(w[scored], a[2:2 + H, 2:2 + W][scored].astype(np.float64))


def test_content_classes():
    H = W = 24
    z = np.zeros((H, W))
    for r in (1, 2, 7):
        a, b = content_pair('const', H + 2 * r + 8, W + 2 * r + 8, 5)
        s = photo_fast(a, b, z, z, r, r + 2)[0]
        assert not np.isnan(s).any() and raw_bits(s, z)                    # exactly +0.0 everywhere
        for kind, shift in (('binary', 3.0), ('checker', 1.0)):
            a, b = content_pair(kind, H + 2 * r + 8, W + 2 * r + 8, 5)
            s = photo_fast(a, b, z, z + shift, r, r + 4)[0]
            win = np.lib.stride_tricks.sliding_window_view(a, (2 * r + 1, 2 * r + 1))[4:4 + H, 4:4 + W]
            flat = win.min(axis=(2, 3)) == win.max(axis=(2, 3))      # (i.i.d. binary 3 x 3 windows can be flat)
            assert flat.mean() < 0.02 and (kind == 'binary' and r == 1 or not flat.any())
            assert not np.isnan(s).any() and raw_bits(s, np.where(flat, 0.0, 1.0)), (kind, r)
    a, b = content_pair('checker', 12, 12, 5)
    assert (photo_restate(a, b, np.zeros((3, 3)), np.full((3, 3), 1.0), 1, 5)[0] == 1.0).all()


@pytest.mark.parametrize('r', [1, 2, 3, 7])
def test_direct_form(r):
    """The integer-moment form against resample-then-correlate on random fractional disparities: 1e-12."""
    H, W = 14, 15
    a, b = stereo_pair(H + 2 * r + 10, W + 2 * r + 10, seed=r, dx=1)
    dr, dc = planes(H, W, r, 'frac')
    got = photo_fast(a, b, dr, dc, r, r + 5)[0]
    want = photo_direct(a, b, dr, dc, r, r + 5)
    assert not np.isnan(want).any() and np.abs(got - want).max() <= 1e-12
    assert np.abs(want).max() > 0.1


def planted(seed=0):
    """The pair of test_exact_one_on_true_shift with 5 % of the cells moved by +-3 .. 6 columns."""
    a, b = stereo_pair(52, 52, seed=3, dx=2)
    H = W = 48
    rng = np.random.default_rng(seed)
    hit = rng.uniform(size=(H, W)) < 0.05
    move = rng.integers(3, 7, (H, W)) * rng.choice([-1, 1], (H, W))
    dc = np.where(hit, 2.0 + move, 2.0)
    return a, b, np.zeros((H, W)), dc, hit


def test_planted_impulses():
    """At r = 3 and min_score = 0.75 every scored impulse is rejected and no clean cell is.  With this file's
    draw the restatement's highest impulse score is 0.545 at r = 3; r = 2 (0.871) and r = 1 (0.940) do not
    separate the two at 0.75 on this draw and are not asserted."""
    r = 3
    a, b, dr, dc, hit = planted()
    maps = np.stack([dc, dr])
    s, _, out, rej = photo_fast(a, b, dr, dc, r, 2, 0.75, maps)
    scored = ~np.isnan(s)
    assert (hit & scored).sum() > 50
    print('highest impulse score at r = %d: %.3f' % (r, s[hit & scored].max()))
    assert rej[hit & scored].all() and not rej[~hit].any()                  # every scored impulse, no clean cell
    assert (s[~hit & scored] == 1.0).all()
    assert np.isnan(out[:, rej.astype(bool)]).all() and raw_bits(out[:, ~rej.astype(bool)], maps[:, ~rej.astype(bool)])


# ---------------------------------------------------------------------------------------------
# 2. validation of the C entries and of the keywords
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_header_declares_photo(lib):
    syms = L.header_symbols()
    assert 'dm_photo_score' in syms and 'dm_photo_bytes' in syms
    assert 'dm_photo_score' in L.SIGNATURES and 'dm_photo_bytes' in L.SIGNATURES
    assert lib.dm_abi_version() == 110
    assert L.DM_PHOTO_REJECT == 1


def _args(img1=P8, s1=16, img2=P8, s2=16, Hi=16, Wi=16, d_row=P8, d_col=P8, H=4, W=4, oy=2, ox=2, r=2, flags=0,
          min_score=0.0, maps=None, M=1, score=P8, warped=None, rejected=None, work=P8):
    return (img1, s1, img2, s2, Hi, Wi, d_row, d_col, H, W, oy, ox, r, flags, min_score, maps, M, score, warped,
            rejected, work, None)


@pytest.mark.parametrize('kw,code,needle', [
    (dict(img1=None), L.DM_ERR_ARG, 'null'),
    (dict(img2=None), L.DM_ERR_ARG, 'null'),
    (dict(d_row=None), L.DM_ERR_ARG, 'null'),
    (dict(d_col=None), L.DM_ERR_ARG, 'null'),
    (dict(work=None), L.DM_ERR_ARG, 'null'),
    (dict(Hi=0), L.DM_ERR_ARG, 'image shape'),
    (dict(Wi=-1), L.DM_ERR_ARG, 'image shape'),
    (dict(s1=15), L.DM_ERR_ARG, 'stride'),
    (dict(s2=-16), L.DM_ERR_ARG, 'stride'),
    (dict(H=0), L.DM_ERR_ARG, 'map shape'),
    (dict(W=-4), L.DM_ERR_ARG, 'map shape'),
    (dict(oy=2 ** 30 + 1), L.DM_ERR_ARG, 'offset'),
    (dict(ox=-2 ** 30 - 1), L.DM_ERR_ARG, 'offset'),
    (dict(r=0), L.DM_ERR_ARG, 'radius'),
    (dict(r=8), L.DM_ERR_ARG, 'radius'),
    (dict(r=-1), L.DM_ERR_ARG, 'radius'),
    (dict(flags=2), L.DM_ERR_ARG, 'flags'),
    (dict(flags=-1), L.DM_ERR_ARG, 'flags'),
    (dict(flags=1), L.DM_ERR_ARG, 'd_maps'),
    (dict(flags=1, maps=P8, M=0), L.DM_ERR_ARG, 'map count'),
    (dict(flags=1, maps=P8, min_score=1.5), L.DM_ERR_ARG, 'min_score'),
    (dict(flags=1, maps=P8, min_score=-1.0000001), L.DM_ERR_ARG, 'min_score'),
    (dict(flags=1, maps=P8, min_score=NAN), L.DM_ERR_ARG, 'min_score'),
    (dict(rejected=P8), L.DM_ERR_ARG, 'd_rejected'),
    (dict(score=None), L.DM_ERR_ARG, 'no output'),
    (dict(H=65536, W=32768), L.DM_ERR_UNSUPPORTED, 'cells'),                       # H W = 2^31
    (dict(flags=1, maps=P8, M=65536), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=64 * 65535 + 1, W=1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(H=1, W=64 * 65535 + 1, flags=1, maps=P8, M=3, min_score=-1.0, r=7, warped=P8, rejected=P8),
     L.DM_ERR_UNSUPPORTED, 'cells'),                                             # every argument valid but the shape
])
def test_photo_score_validation(lib, kw, code, needle):
    assert lib.dm_photo_score(*_args(**kw)) == code
    assert needle in L.last_error()


def test_photo_bytes(lib):
    refused = [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 65536, 32768), (65536, 4, 4),
               (1, 64 * 65535 + 1, 1), (1, 1, 64 * 65535 + 1)]
    for bad in refused:
        assert lib.dm_photo_bytes(*bad) == 0, bad
        assert lib.dm_median_bytes(*bad) == 0, bad                                 # the same limits
    for H, W in [(1, 1), (5, 7), (65, 130), (1024, 1024), (46341, 46340), (64 * 65535, 1), (1, 64 * 65535)]:
        for M in (1, 3, 65535):
            assert lib.dm_photo_bytes(M, H, W) > 0 and lib.dm_median_bytes(M, H, W) > 0, (M, H, W)


def test_photo_params():
    assert engine.photo_params(1) == (1, None)
    assert engine.photo_params((2, 0.75)) == (2, 0.75)
    assert engine.photo_params([np.int64(7), np.float32(-1)]) == (7, -1.0)
    assert engine.photo_params((3, 1)) == (3, 1.0)
    got = engine.photo_params((np.int32(2), np.float64(0.5)))
    assert type(got[0]) is int and type(got[1]) is float
    for bad in [None, 0, 8, -1, 1.0, True, '3', (), (1,), (1, 2, 3), (0, 0.5), (8, 0.5), (1, 1.5), (1, -1.01),
                (1, NAN), (1, None), (1, True), (1, '0.5'), (1.5, 0.5), (True, 0.5), ((1,), 0.5)]:
        with pytest.raises(ValueError):
            engine.photo_params(bad)
    assert engine.photo_planes(['elevation', 'elevation2']) == (1, 0)
    assert engine.photo_planes(('elevation2', 'distance', 'elevation')) == (0, 2)
    for bad in (['elevation'], ['elevation2', 'distance'], []):
        with pytest.raises(ValueError):
            engine.photo_planes(bad)


# ---------------------------------------------------------------------------------------------
# 3. the keyword and the sharded path: oracle tile solver, host stitcher, the restatement as photoer
# ---------------------------------------------------------------------------------------------
PMODES = ('elevation', 'elevation2')
PHOTO = (2, 0.75)
SPECKLE = (3, 0.25)
MEDIAN = (1, 1)


def _pcase():
    """The pair of test_fill_host._case with a corrupted block in img2: wrong cells to reject."""
    a, b = stereo_pair(16 * 2 + 4 + 8, 16 * 3 + 4 + 8, seed=11, dx=2)
    b = b.copy()
    b[14:24, 20:32] = np.random.default_rng(2).integers(0, 256, (10, 12)).astype(np.uint8)
    return a, b


def _host_photo(img1, img2, d_row, d_col, radius, offset, min_score, maps):
    """photoer hook of solve_image_sharded."""
    res = photo_fast(np.asarray(img1), np.asarray(img2), np.asarray(d_row), np.asarray(d_col), radius, offset,
                     min_score, None if maps is None else np.asarray(maps))
    return res[0] if min_score is None else (res[0], res[2], res[3])


def _sharded(a, b, modes=PMODES, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, modes,
                                     solver=_oracle_tiles, stitcher=_host_stitch, **kw)


def test_photo_keyword():
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = _pcase()
    s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 16], degree_map_mode=list(PMODES), photo=PHOTO)
    assert s.photo == PHOTO and s.photo_map is None and s.photo_reject_map is None
    s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 16])
    assert s.photo is None and s.photo_map is None and s.photo_reject_map is None
    assert ImageCutSolver(a, b, degree_map_mode=['elevation2', 'elevation'], photo=3).photo == (3, None)
    for modes in (['elevation'], ['elevation2'], ['elevation', 'distance']):      # a plane is missing
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, degree_map_mode=modes, photo=2)
        with pytest.raises(ValueError):
            _sharded(a, b, modes=modes, photo=2, photoer=_host_photo)
        assert ImageCutSolver(a, b, degree_map_mode=modes).photo is None
    for bad in (0, 8, 1.0, True, (1,), (1, 2.0), (1, 0.5, 1)):
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, degree_map_mode=list(PMODES), photo=bad)
        with pytest.raises(ValueError):
            _sharded(a, b, photo=bad, photoer=_host_photo)


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map): today's call."""
    a, b = _pcase()
    return [np.asarray(x) for x in _sharded(a, b)]


@pytest.fixture(scope='module')
def chain(plain):
    """The chain in the restatements: median -> photo reject -> speckle -> fill -> photo score."""
    a, b = _pcase()
    med = median_restate(plain[0], None, *MEDIAN)[0]
    _, _, rejd, rej = photo_restate(a, b, med[1], med[0], PHOTO[0], 2, PHOTO[1], med)
    spk = speckle_restate(rejd, *SPECKLE)
    fil = fill_restate(spk[0], 16)
    score = photo_restate(a, b, fil[0][1], fil[0][0], PHOTO[0], 2)[0]
    return med, rejd, rej, spk, fil, score


def _check_chain(got, plain, chain):
    med, rejd, rej, spk, fil, score = chain
    assert len(got) == 6
    assert same_bits(got[0], fil[0]) and same_bits(got[1], plain[1])
    assert np.array_equal(np.asarray(got[2]), spk[1]) and np.array_equal(np.asarray(got[3]), fil[1])
    assert np.array_equal(np.asarray(got[4]), rej) and raw_bits(np.asarray(got[5]), score)


def _check_score_only(got, plain):
    a, b = _pcase()
    assert len(got) == 3
    assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1])
    assert raw_bits(np.asarray(got[2]), photo_restate(a, b, plain[0][1], plain[0][0], PHOTO[0], 2)[0])


def test_sharded_photo_single_process(plain, chain):
    a, b = _pcase()
    _check_score_only(_sharded(a, b, photo=PHOTO[0], photoer=_host_photo), plain)
    got = _sharded(a, b, photo=PHOTO, photoer=_host_photo, median=MEDIAN, medianer=_host_median, speckle=SPECKLE,
                   speckler=_host_speckle, fill=16, filler=_host_fill)
    _check_chain(got, plain, chain)
    med, rejd, rej, spk, fil, score = chain
    # the planted block is found: cells are rejected, they are NaN in both planes before the fill, finite after it
    assert rej.any() and np.isnan(rejd[:, rej.astype(bool)]).all() and np.isfinite(fil[0]).all()
    assert fil[1][:, rej.astype(bool)].all()
    # with a min_score alone: (d_map, out_map, rejected, score), the rejected cells are holes of d_map
    got = _sharded(a, b, photo=PHOTO, photoer=_host_photo)
    assert len(got) == 4 and np.asarray(got[2]).any()
    assert np.array_equal(np.isnan(np.asarray(got[0])[0]), np.isnan(plain[0][0]) | np.asarray(got[2]).astype(bool))
    assert np.isnan(np.asarray(got[3])[np.asarray(got[2]).astype(bool)]).all()


def test_sharded_photo_none_is_unchanged(plain):
    a, b = _pcase()
    got = _sharded(a, b, photo=None, photoer=_host_photo)
    assert len(got) == 2
    for g, r in zip(got, plain):
        assert same_bits(g, r)


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _pcase()
        only = _sharded(a, b, photo=PHOTO[0], photoer=_host_photo)
        all_ = _sharded(a, b, photo=PHOTO, photoer=_host_photo, median=MEDIAN, medianer=_host_median, speckle=SPECKLE,
                        speckler=_host_speckle, fill=16, filler=_host_fill)
        root = _sharded(a, b, photo=PHOTO, photoer=_host_photo, result='root')
        none = _sharded(a, b, photo=None, photoer=_host_photo)
        q.put((rank, [np.asarray(x) for x in only], [np.asarray(x) for x in all_],
               [None if x is None else np.asarray(x) for x in root], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_photo_gloo_world_2(plain, chain):
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
    for rank, only, all_, root, none in res:
        _check_score_only(only, plain)
        _check_chain(all_, plain, chain)
        if rank == 0:
            assert len(root) == 4 and root[2].any()
        else:
            assert root == [None, None, None, None]
        assert len(none) == 2
        for g, r in zip(none, plain):
            assert same_bits(g, r), rank
