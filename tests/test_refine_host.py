"""Local re-matching of a disparity map, host side (no GPU): the plain-loop restatement of the
definition (refine_restate: what dm_photo_refine must equal bit for bit; a candidate's score is
photo_restate's per-cell code), a vectorised restatement pinned to it (refine_fast: the one the GPU
tests use; its candidate scores are computed once per case and shared by the variants), the
properties of the definition, the planted impulses the search exists for, the sub-pixel step on a
smoothly varying shift, argument validation of the two C entries (it returns before any HIP call)
and of the keywords, and the sharded chain with the oracle as tile solver, a host stitcher and the
restatement injected as the refiner -- single process and gloo world size 2.

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
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair, texture

from test_fill_host import GEOM, _free_port, _host_fill, _host_stitch, _oracle_tiles, fill_restate, raw_bits, same_bits
from test_photo_host import (DMAX, INF, NAN, PAIRS, SHIFT, _finite, _host_photo, _offsets, _pcase, photo_fast,
                             photo_restate, planes)


@pytest.fixture(scope='module', autouse=True)
def entries():
    """What this file restates and checks is the pair of C entries: without them nothing here holds."""
    lib = L.load()
    assert hasattr(lib, 'dm_photo_refine') and hasattr(lib, 'dm_photo_refine_bytes')
    assert callable(getattr(engine, 'photo_refine', None)) and callable(getattr(engine, 'refine_params', None))


POSMAX = float(2 ** 30)
QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------
# the definition in plain loops
# ---------------------------------------------------------------------------------------------
def cand_score(A_, B_, cy, cx, ty, tx, w, r):
    """photo_restate's per-cell code (rules 4 and 5 of dm_photo_score) with the four img2 windows at
    (ty - r, tx - r) + SHIFT: ty = iy + dy, tx = ix + dx."""
    D = 2 * r + 1
    n = D * D
    sa = saa = 0
    S = [0, 0, 0, 0]
    AP = [0, 0, 0, 0]
    PP = {kl: 0 for kl in PAIRS}
    for u in range(D):
        for v in range(D):
            a = A_[cy - r + u][cx - r + v]
            p = [B_[ty - r + u + sy][tx - r + v + sx] for sy, sx in SHIFT]
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
        return 1.0 if t > 1.0 else (-1.0 if t < -1.0 else t)
    return 0.0


def peak(sm, s0, sp):
    den = (sm + sp) - 2.0 * s0
    if not den < 0.0:
        return 0.0
    t = (0.5 * (sm - sp)) / den
    return 0.5 if t > 0.5 else (-0.5 if t < -0.5 else t)


def refine_restate(img1, img2, d_row, d_col, r, s, offset=0, min_gain=0.0, subpix=False, mask=None):
    """The definition -> (out_row, out_col, score, int8 shift [2][H][W])."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    A_, B_ = img1.tolist(), img2.tolist()
    R_, C_ = d_row.tolist(), d_col.tolist()
    out_row, out_col = d_row.copy(), d_col.copy()      # a cell that is not moved keeps its bits
    score = np.full((H, W), QNAN)
    shift = np.zeros((2, H, W), dtype=np.int8)
    for y in range(H):
        for x in range(W):
            if mask is not None and not mask[y][x]:
                continue
            dr, dc = R_[y][x], C_[y][x]
            if not (_finite(dr) and _finite(dc)):
                continue
            cy, cx = y + oy, x + ox
            if not (r <= cy <= Hi - 1 - r and r <= cx <= Wi - 1 - r):
                continue
            py, px = float(cy) - dr, float(cx) - dc
            if not (-POSMAX <= py <= POSMAX and -POSMAX <= px <= POSMAX):
                continue
            iy, ix = math.floor(py), math.floor(px)
            fy, fx = py - float(iy), px - float(ix)
            gy, gx = 1.0 - fy, 1.0 - fx
            w = [gy * gx, gy * fx, fy * gx, fy * fx]
            sc = {}
            for dy in range(-s, s + 1):
                for dx in range(-s, s + 1):
                    if r <= iy + dy <= Hi - r - 2 and r <= ix + dx <= Wi - r - 2:
                        sc[dy, dx] = cand_score(A_, B_, cy, cx, iy + dy, ix + dx, w, r)
            if not sc:
                continue
            best = None
            for (dy, dx), v in sc.items():
                if best is None or v > sc[best] or \
                        (v == sc[best] and (dy * dy + dx * dx, dy, dx) < (best[0] ** 2 + best[1] ** 2, best[0], best[1])):
                    best = (dy, dx)
            if (0, 0) in sc and not sc[best] > sc[0, 0] + min_gain:
                best = (0, 0)
            score[y, x] = sc[best]
            if best == (0, 0):
                continue
            dy, dx = best
            ty = tx = 0.0
            if subpix:
                if (dy - 1, dx) in sc and (dy + 1, dx) in sc:
                    ty = peak(sc[dy - 1, dx], sc[best], sc[dy + 1, dx])
                if (dy, dx - 1) in sc and (dy, dx + 1) in sc:
                    tx = peak(sc[dy, dx - 1], sc[best], sc[dy, dx + 1])
            out_row[y, x] = dr - (float(dy) + ty)
            out_col[y, x] = dc - (float(dx) + tx)
            shift[0, y, x], shift[1, y, x] = dy, dx
    return out_row, out_col, score, shift


# ---------------------------------------------------------------------------------------------
# the fast restatement: the candidates' scores [2s+1][2s+1][H][W] once per case (NaN: not scored),
# then the choice among them, which is cheap and is what mask, min_gain and subpix change
# ---------------------------------------------------------------------------------------------
def candidates_fast(img1, img2, d_row, d_col, r, s, offset=0):
    """-> (live [H][W]: not skipped by rule 1 apart from the mask, sc [2s+1][2s+1][H][W])."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    D = 2 * r + 1
    n = D * D
    K = 2 * s + 2
    A64, B64 = img1.astype(np.int64), img2.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy + oy, xx + ox
    with np.errstate(invalid='ignore', over='ignore'):
        fin = (np.abs(d_row) <= DMAX) & (np.abs(d_col) <= DMAX)
        py = np.where(fin, cy.astype(np.float64) - np.where(fin, d_row, 0.0), NAN)
        px = np.where(fin, cx.astype(np.float64) - np.where(fin, d_col, 0.0), NAN)
        live = fin & (cy >= r) & (cy <= Hi - 1 - r) & (cx >= r) & (cx <= Wi - 1 - r) & \
            (py >= -POSMAX) & (py <= POSMAX) & (px >= -POSMAX) & (px <= POSMAX)
    py, px = np.where(live, py, 0.0), np.where(live, px, 0.0)
    iy, ix = np.floor(py).astype(np.int64), np.floor(px).astype(np.int64)
    fy, fx = py - iy.astype(np.float64), px - ix.astype(np.float64)
    gy, gx = 1.0 - fy, 1.0 - fx
    w = [gy * gx, gy * fx, fy * gx, fy * fx]
    # the img1 window and the img2 patch of every cell, indices clipped (a clipped tap belongs to no scored candidate)
    t = np.arange(D)
    Aw = A64[np.clip(cy[:, :, None, None] - r + t[None, None, :, None], 0, Hi - 1),
             np.clip(cx[:, :, None, None] - r + t[None, None, None, :], 0, Wi - 1)]
    t = np.arange(D + K - 1)
    Bp = B64[np.clip(iy[:, :, None, None] - s - r + t[None, None, :, None], 0, Hi - 1),
             np.clip(ix[:, :, None, None] - s - r + t[None, None, None, :], 0, Wi - 1)]
    sa, saa = Aw.sum((2, 3)), (Aw * Aw).sum((2, 3))
    Q = [[Bp[:, :, u:u + D, v:v + D] for v in range(K)] for u in range(K)]      # window (u - s, v - s)
    Sq = [[Q[u][v].sum((2, 3)) for v in range(K)] for u in range(K)]
    AQ = [[(Aw * Q[u][v]).sum((2, 3)) for v in range(K)] for u in range(K)]
    VA = (n * saa - sa * sa).astype(np.float64)
    sc = np.full((2 * s + 1, 2 * s + 1, H, W), NAN)
    prod = {}

    def qq(a, b):      # sum of the products of two windows, each pair once
        key = (a, b) if a <= b else (b, a)
        if key not in prod:
            prod[key] = (Q[a[0]][a[1]] * Q[b[0]][b[1]]).sum((2, 3))
        return prod[key]

    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            ok = live & (iy + dy >= r) & (iy + dy <= Hi - r - 2) & (ix + dx >= r) & (ix + dx <= Wi - r - 2)
            if not ok.any():
                continue
            win = [(dy + s + sy, dx + s + sx) for sy, sx in SHIFT]
            S = [Sq[u][v] for u, v in win]
            CA = [(n * AQ[u][v] - sa * S[k]).astype(np.float64) for k, (u, v) in enumerate(win)]
            num = ((w[0] * CA[0] + w[1] * CA[1]) + w[2] * CA[2]) + w[3] * CA[3]
            vb = None
            for k, l in PAIRS:
                term = ((1.0 if k == l else 2.0) * (w[k] * w[l])) * (n * qq(win[k], win[l]) - S[k] * S[l]).astype(np.float64)
                vb = term if vb is None else vb + term
            pos = ok & (VA > 0.0) & (vb > 0.0)
            with np.errstate(invalid='ignore', divide='ignore'):
                q = num / np.sqrt(np.where(pos, VA * vb, 1.0))
            q = np.where(q > 1.0, 1.0, np.where(q < -1.0, -1.0, q))
            sc[dy + s, dx + s] = np.where(ok, np.where(pos, q, 0.0), NAN)
    return live, sc


def choose_fast(cand, d_row, d_col, s, min_gain=0.0, subpix=False, mask=None):
    """Rules 3 to 5 on candidates_fast's result -> (out_row, out_col, score, int8 shift)."""
    live, sc = cand
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    NC = 2 * s + 1
    if mask is not None:
        live = live & (np.asarray(mask) != 0)
    best = np.full((H, W), NAN)
    bdy, bdx = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    bd2 = np.zeros((H, W), dtype=np.int64)
    found = np.zeros((H, W), dtype=bool)
    with np.errstate(invalid='ignore'):
        for dy in range(-s, s + 1):      # dy, then dx upwards: among equal scores and distances the first one stays
            for dx in range(-s, s + 1):
                v = sc[dy + s, dx + s]
                d2 = dy * dy + dx * dx
                take = live & ~np.isnan(v) & (~found | (v > best) | ((v == best) & (d2 < bd2)))
                best, bdy, bdx, bd2 = np.where(take, v, best), np.where(take, dy, bdy), np.where(take, dx, bdx), \
                    np.where(take, d2, bd2)
                found |= take
        centre = sc[s, s]
        stay = found & ~np.isnan(centre) & ~(best > centre + min_gain)
    best, bdy, bdx = np.where(stay, centre, best), np.where(stay, 0, bdy), np.where(stay, 0, bdx)
    moved = found & ((bdy != 0) | (bdx != 0))
    ty, tx = np.zeros((H, W)), np.zeros((H, W))
    if subpix:
        yy, xx = np.mgrid[0:H, 0:W]

        def at(dy, dx):      # the score of candidate (dy, dx) per cell; NaN outside [-s, s]^2
            inside = (np.abs(dy) <= s) & (np.abs(dx) <= s)
            return np.where(inside, sc[np.clip(dy + s, 0, NC - 1), np.clip(dx + s, 0, NC - 1), yy, xx], NAN)

        def peaks(sm, sp):
            with np.errstate(invalid='ignore', divide='ignore'):
                den = (sm + sp) - 2.0 * best
                t = (0.5 * (sm - sp)) / np.where(den < 0.0, den, 1.0)
                t = np.where(t > 0.5, 0.5, np.where(t < -0.5, -0.5, t))
                return np.where(moved & ~np.isnan(sm) & ~np.isnan(sp) & (den < 0.0), t, 0.0)

        ty = peaks(at(bdy - 1, bdx), at(bdy + 1, bdx))
        tx = peaks(at(bdy, bdx - 1), at(bdy, bdx + 1))
    out_row, out_col = d_row.copy(), d_col.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        out_row[moved] = (d_row - (bdy.astype(np.float64) + ty))[moved]
        out_col[moved] = (d_col - (bdx.astype(np.float64) + tx))[moved]
    score = np.where(found, best, QNAN)
    shift = np.stack([np.where(moved, bdy, 0), np.where(moved, bdx, 0)]).astype(np.int8)
    return out_row, out_col, score, shift


def refine_fast(img1, img2, d_row, d_col, r, s, offset=0, min_gain=0.0, subpix=False, mask=None):
    """refine_restate, vectorised."""
    return choose_fast(candidates_fast(img1, img2, d_row, d_col, r, s, offset), d_row, d_col, s, min_gain, subpix, mask)


def all_bits(p, q):
    """Four outputs against four outputs: the planes and the score as 64-bit patterns, the shift as int8."""
    return raw_bits(p[0], q[0]) and raw_bits(p[1], q[1]) and raw_bits(p[2], q[2]) and \
        np.asarray(p[3]).dtype == np.int8 and np.array_equal(np.asarray(p[3]), np.asarray(q[3]))


# ---------------------------------------------------------------------------------------------
# 1. the restatements and the properties of the definition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (5, 7), (9, 8)])
@pytest.mark.parametrize('r,s', [(1, 1), (2, 2), (3, 1), (1, 3)])
def test_fast_equals_literal(shape, r, s):
    H, W = shape
    rng = np.random.default_rng(H + W)
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    for seed, kind in enumerate(['int', 'frac', 'mixed']):
        for margin, off in [(r + s + 4, (r + s + 4, r + s + 4)), (r + 1, (r + 1, r + 2)), (2, (0, 1))]:
            a, b = stereo_pair(H + 2 * margin, W + 2 * margin + 1, seed=seed, dx=2)
            dr, dc = planes(H, W, seed, kind)
            cand = candidates_fast(a, b, dr, dc, r, s, off)
            for kw in (dict(), dict(subpix=True), dict(min_gain=0.05, subpix=True, mask=mask)):
                lit = refine_restate(a, b, dr, dc, r, s, off, **kw)
                assert all_bits(lit, choose_fast(cand, dr, dc, s, **kw)), (shape, r, s, kind, margin, kw)
                kept = ~lit[3].any(axis=0)
                assert raw_bits(lit[0][kept], dr[kept]) and raw_bits(lit[1][kept], dc[kept])      # NaN payloads, -0.0
            if margin == r + s + 4 and kind != 'mixed':      # this margin covers every candidate of `planes`
                assert not np.isnan(cand[1]).any()


@pytest.mark.parametrize('r', [1, 2, 3])
def test_centre_score_is_photo_score(r):
    """Candidate (0, 0) is scored exactly where dm_photo_score scores, with its bits."""
    H, W = 9, 11
    for seed, kind in enumerate(['int', 'frac', 'mixed']):
        for margin in (r + 4, r + 1):
            a, b = stereo_pair(H + 2 * margin, W + 2 * margin, seed=seed + 3, dx=1)
            dr, dc = planes(H, W, seed, kind)
            want = photo_restate(a, b, dr, dc, r, margin)[0]
            _, sc = candidates_fast(a, b, dr, dc, r, 2, margin)
            assert raw_bits(sc[2, 2], want), (r, kind, margin)
            assert raw_bits(sc[2, 2], photo_fast(a, b, dr, dc, r, margin)[0])
            # through the literal restatement: with a min_gain nothing can reach, the centre wins wherever it is scored
            lit = refine_restate(a, b, dr, dc, r, 1, margin, min_gain=2.0)
            assert raw_bits(lit[2][~np.isnan(want)], want[~np.isnan(want)]) and not lit[3][:, ~np.isnan(want)].any()


def test_second_pass_is_identity():
    """min_gain = 0, no subpix, integer planes within s of the truth: the first pass ends on a position that is the
    best of its own neighbourhood (score 1.0), so a second pass changes nothing, to the bit."""
    for r, s in [(1, 1), (2, 2), (3, 3)]:
        a, b, dr, dc, hit, vec, m = planted(r, s, 20, 20, share=0.5)
        one = refine_fast(a, b, dr, dc, r, s, m)
        assert one[3].any() and (one[2] == 1.0).all()
        two = refine_fast(a, b, one[0], one[1], r, s, m)
        assert raw_bits(two[0], one[0]) and raw_bits(two[1], one[1]) and not two[3].any()
        assert raw_bits(two[2], one[2])


def test_skipped_cells_keep_their_bits():
    r, s = 2, 1
    a, b = stereo_pair(20, 22, seed=1, dx=0)
    payload = np.array([0x7ff8000000001234, 0xfff8000000000001, 0x7ff0000000000000, 0xfff0000000000000,
                        0x8000000000000000], dtype=np.uint64).view(np.float64)
    for v in payload[:4]:
        for dr, dc in ((v, 0.0), (0.0, v), (v, -0.0)):
            res = refine_restate(a, b, np.full((1, 1), dr), np.full((1, 1), dc), r, s, (8, 9))
            assert raw_bits(res[0], np.full((1, 1), dr)) and raw_bits(res[1], np.full((1, 1), dc))
            assert raw_bits(res[2], np.full((1, 1), QNAN)) and not res[3].any()
    # -0.0 on a cell whose own position wins (identical images at the centre) and on a masked cell
    z = np.full((1, 1), payload[4])
    res = refine_restate(a, a, z, z, r, s, (8, 9))
    assert raw_bits(res[0], z) and raw_bits(res[1], z) and res[2][0, 0] == 1.0
    res = refine_restate(a, b, z, z, r, s, (8, 9), mask=np.zeros((1, 1), dtype=np.uint8))
    assert raw_bits(res[0], z) and raw_bits(res[2], np.full((1, 1), QNAN))
    # the img1 window leaves the image; a position past 2^30; no scored candidate
    for off, dr in (((1, 9), 0.0), ((8, 9), 1e300), ((8, 9), 2.0 ** 30 + 9), ((8, 9), 12.0)):
        res = refine_restate(a, b, np.full((1, 1), dr), np.full((1, 1), 0.5), r, s, off)
        assert raw_bits(res[0], np.full((1, 1), dr)) and raw_bits(res[2], np.full((1, 1), QNAN)) and not res[3].any()
    # the centre is not scored but a neighbour is: the cell moves there
    res = refine_restate(a, b, np.full((1, 1), 7.0), np.zeros((1, 1)), r, s, (8, 9))      # iy = 1 < r; dy = 1 scores
    assert res[3][0, 0, 0] == 1 and res[0][0, 0] == 6.0 and np.isfinite(res[2][0, 0])


@pytest.mark.parametrize('kind', ['identical', 'binary', 'dark'])
def test_ties(kind):
    """Many candidates tie at 1.0 or 0.0: the centre stays when it is among the best; else the nearest wins, then
    the smaller dy, then the smaller dx."""
    H, W, r, s = 12, 13, 1, 2
    m = r + s + 3
    a, b = content_pair(kind, H + 2 * m, W + 2 * m, 4)
    z = np.zeros((H, W))
    lit = refine_restate(a, b, z, z, r, s, m)
    assert all_bits(lit, refine_fast(a, b, z, z, r, s, m))
    _, sc = candidates_fast(a, b, z, z, r, s, m)
    top = sc.max(axis=(0, 1))
    ties = ((sc == top).sum(axis=(0, 1)) > 1)
    assert ties.mean() > {'dark': 0.5, 'binary': 0.02, 'identical': 0.0}[kind]
    centre_best = sc[s, s] == top
    assert not lit[3][:, centre_best].any() and raw_bits(lit[2][centre_best], sc[s, s][centre_best])
    for y, x in zip(*np.nonzero(ties & ~centre_best)):
        cands = sorted((dy * dy + dx * dx, dy, dx) for dy in range(-s, s + 1) for dx in range(-s, s + 1)
                       if sc[dy + s, dx + s, y, x] == top[y, x])
        assert (lit[3][0, y, x], lit[3][1, y, x]) == cands[0][1:]
    if kind == 'identical':
        assert not lit[3].any() and raw_bits(lit[2], sc[s, s])
        assert np.isin(lit[2], (0.0, 1.0)).all() and (lit[2] == 1.0).mean() > 0.9      # (0.0: a flat 3 x 3 window)
    if kind == 'dark':      # flat windows: every candidate scores exactly 0.0 and nothing moves
        flat = (sc == 0.0).all(axis=(0, 1))
        assert flat.mean() > 0.3 and not lit[3][:, flat].any()


def planted(r, s, H=48, W=48, share=0.05):
    """stereo_pair(dx=2) with 5 % of the cells moved by a non-zero integer vector with components in -s .. s."""
    m = r + s + 2
    a, b = stereo_pair(H + 2 * m, W + 2 * m, seed=5, dx=2)
    rng = np.random.default_rng(1)
    hit = rng.uniform(size=(H, W)) < share
    vec = rng.integers(-s, s + 1, (2, H, W))
    hit &= (vec != 0).any(axis=0)
    dr, dc = np.where(hit, 0.0 + vec[0], 0.0), np.where(hit, 2.0 + vec[1], 2.0)
    return a, b, dr, dc, hit, vec, m


@pytest.mark.parametrize('r,s', [(1, 2), (2, 2), (3, 2), (3, 3)])
def test_planted_impulses(r, s):
    """Every moved cell returns to the truth exactly, no clean cell changes, every score is exactly 1.0: no
    threshold is involved, and radius 1 works."""
    a, b, dr, dc, hit, vec, m = planted(r, s)
    out_row, out_col, score, shift = refine_fast(a, b, dr, dc, r, s, m)
    centre = photo_fast(a, b, dr, dc, r, m)[0]
    print('(r, s) = (%d, %d): %d moved cells, highest centre score of one %.3f' % (r, s, hit.sum(), centre[hit].max()))
    assert hit.sum() > 80
    assert (out_row == 0.0).all() and (out_col == 2.0).all()
    assert np.array_equal(shift[0], np.where(hit, vec[0], 0)) and np.array_equal(shift[1], np.where(hit, vec[1], 0))
    assert raw_bits(out_row[~hit], dr[~hit]) and raw_bits(out_col[~hit], dc[~hit])
    assert (score == 1.0).all()


def sinus_case(H=40, W=56, m=8, max_disp=6):
    """A pair whose shift varies smoothly, img1(y, x) = T(y, x), img2(y, x) = T(y, x + d(y, x)) with T bilinear in a
    texture and d real: the truth 'elevation' of img1's pixel x is x - x', x' + d(y, x') = x (a fixed point)."""
    Hi, Wi = H + 2 * m, W + 2 * m
    tex = texture(Hi + 8, Wi + 8 + max_disp + 2, 21).astype(np.float64)
    yy, xx = np.mgrid[0:Hi, 0:Wi]

    def disp(x):
        return 0.5 * max_disp * (1.0 + np.sin(2 * np.pi * x / Wi) * np.cos(2 * np.pi * yy[:, :1] / Hi))

    pos = xx + disp(xx)
    i = np.floor(pos).astype(np.int64)
    f = pos - i
    b = np.rint((1 - f) * tex[4 + yy, 4 + i] + f * tex[4 + yy, 5 + i]).astype(np.uint8)
    a = tex[4:4 + Hi, 4:4 + Wi].astype(np.uint8)
    xp = xx.astype(np.float64)
    for _ in range(60):
        xp = xx - disp(xp)
    truth = (xx - xp)[m:m + H, m:m + W]
    return a, b, truth, m


def test_subpix_on_a_smooth_shift():
    """Mean |error| of the column disparity against the truth, r = 3, s = 2, from a prior that is the rounded truth
    with a third of the cells off by one or two pixels: 0.586 before, 0.272 after the integer step, 0.221 with the
    parabola (printed below).  The condition is only that the sub-pixel step does not make it grow."""
    a, b, truth, m = sinus_case()
    H, W = truth.shape
    rng = np.random.default_rng(3)
    off = np.where(rng.uniform(size=(H, W)) < 0.33, rng.integers(-2, 3, (H, W)), 0)
    dc = np.rint(truth) + off
    dr = np.zeros((H, W))
    cand = candidates_fast(a, b, dr, dc, 3, 2, m)
    whole = choose_fast(cand, dr, dc, 2)
    sub = choose_fast(cand, dr, dc, 2, subpix=True)
    before, mid, after = np.abs(dc - truth).mean(), np.abs(whole[1] - truth).mean(), np.abs(sub[1] - truth).mean()
    print('mean |error|: prior %.3f, integer step %.3f, with the parabola %.3f' % (before, mid, after))
    assert np.array_equal(whole[3], sub[3]) and whole[3].any()
    assert after <= before and after <= mid


# ---------------------------------------------------------------------------------------------
# 2. validation of the C entries and of the keywords
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_header_declares_refine(lib):
    syms = L.header_symbols()
    assert 'dm_photo_refine' in syms and 'dm_photo_refine_bytes' in syms
    assert 'dm_photo_refine' in L.SIGNATURES and 'dm_photo_refine_bytes' in L.SIGNATURES
    assert lib.dm_abi_version() == 110
    assert L.DM_REFINE_SUBPIX == 1


def _args(img1=P8, s1=16, img2=P8, s2=16, Hi=16, Wi=16, d_row=P8, d_col=P8, H=4, W=4, oy=2, ox=2, r=2, s=1, min_gain=0.0,
          flags=0, mask=None, out_row=P8, out_col=P8, score=None, shift=None, work=P8):
    return (img1, s1, img2, s2, Hi, Wi, d_row, d_col, H, W, oy, ox, r, s, min_gain, flags, mask, out_row, out_col,
            score, shift, work, None)


@pytest.mark.parametrize('kw,code,needle', [
    (dict(img1=None), L.DM_ERR_ARG, 'null'),
    (dict(img2=None), L.DM_ERR_ARG, 'null'),
    (dict(d_row=None), L.DM_ERR_ARG, 'null'),
    (dict(d_col=None), L.DM_ERR_ARG, 'null'),
    (dict(out_row=None), L.DM_ERR_ARG, 'null'),
    (dict(out_col=None), L.DM_ERR_ARG, 'null'),
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
    (dict(s=0), L.DM_ERR_ARG, 'search'),
    (dict(s=4), L.DM_ERR_ARG, 'search'),
    (dict(s=-1), L.DM_ERR_ARG, 'search'),
    (dict(min_gain=-1e-9), L.DM_ERR_ARG, 'min_gain'),
    (dict(min_gain=2.0000001), L.DM_ERR_ARG, 'min_gain'),
    (dict(min_gain=NAN), L.DM_ERR_ARG, 'min_gain'),
    (dict(flags=2), L.DM_ERR_ARG, 'flags'),
    (dict(flags=-1), L.DM_ERR_ARG, 'flags'),
    (dict(H=65536, W=32768), L.DM_ERR_UNSUPPORTED, 'cells'),                       # H W = 2^31
    (dict(H=64 * 65535 + 1, W=1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(Hi=2 ** 30 + 1, s1=16), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(Wi=2 ** 30 + 1, s1=2 ** 31, s2=2 ** 31, r=7, s=3, min_gain=2.0, flags=1, mask=P8, score=P8, shift=P8),
     L.DM_ERR_UNSUPPORTED, 'cells'),                                             # every argument valid but the shape
])
def test_photo_refine_validation(lib, kw, code, needle):
    assert lib.dm_photo_refine(*_args(**kw)) == code
    assert needle in L.last_error()


def test_photo_refine_bytes(lib):
    ok = (16, 16, 4, 4, 2, 1)
    assert lib.dm_photo_refine_bytes(*ok) > 0
    for i, bad in [(0, 0), (0, 2 ** 30 + 1), (1, -1), (1, 2 ** 30 + 1), (2, 0), (3, 0), (2, 64 * 65535 + 1), (4, 0), (4, 8),
                   (5, 0), (5, 4)]:
        args = list(ok)
        args[i] = bad
        assert lib.dm_photo_refine_bytes(*args) == 0, args
    assert lib.dm_photo_refine_bytes(16, 16, 65536, 32768, 2, 1) == 0
    for Hi, Wi, H, W in [(1, 1, 1, 1), (2 ** 30, 2 ** 30, 46341, 46340), (100, 100, 64 * 65535, 1)]:
        for r, s in [(1, 1), (7, 3)]:
            assert lib.dm_photo_refine_bytes(Hi, Wi, H, W, r, s) > 0


def test_refine_params():
    assert engine.refine_params((1, 2)) == (1, 2, 0.0)
    assert engine.refine_params([np.int64(7), np.int32(3), np.float32(0.5)]) == (7, 3, 0.5)
    got = engine.refine_params((np.int32(2), np.int64(1), 1))
    assert got == (2, 1, 1.0) and type(got[0]) is int and type(got[1]) is int and type(got[2]) is float
    for bad in [None, 2, 1.0, True, '3', (), (1,), (1, 2, 0.1, 3), (0, 1), (8, 1), (1, 0), (1, 4), (1.0, 1), (1, 1.0),
                (True, 1), (1, True), (1, 1, -0.1), (1, 1, 2.5), (1, 1, NAN), (1, 1, None), (1, 1, True), (1, 1, '0')]:
        with pytest.raises(ValueError):
            engine.refine_params(bad)
    assert engine.refine_planes(['elevation', 'elevation2']) == (1, 0)
    for bad in (['elevation'], ['elevation2'], ['elevation', 'elevation2', 'distance'], []):
        with pytest.raises(ValueError):
            engine.refine_planes(bad)


# ---------------------------------------------------------------------------------------------
# 3. the keywords and the sharded path: oracle tile solver, host stitcher, the restatement as refiner
# ---------------------------------------------------------------------------------------------
PMODES = ('elevation', 'elevation2')
REFINE = (2, 2, 0.05)
PHOTO = (2, 0.75)


def _host_refine(img1, img2, d_row, d_col, radius, search, offset, min_gain, mask):
    """refiner hook of solve_image_sharded (the stage runs with the sub-pixel step)."""
    return refine_fast(np.asarray(img1), np.asarray(img2), np.asarray(d_row), np.asarray(d_col), radius, search, offset,
                       min_gain, True, None if mask is None else np.asarray(mask))


def _sharded(a, b, modes=PMODES, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, modes,
                                     solver=_oracle_tiles, stitcher=_host_stitch, **kw)


def test_refine_keyword():
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = _pcase()
    kw = dict(image_size=[16, 16], stride=[12, 16], degree_map_mode=list(PMODES))
    s = ImageCutSolver(a, b, refine=REFINE, fill=16, **kw)
    assert s.refine == REFINE and s.refine_where == 'filled' and s.refine_score_map is None and s.refine_shift_map is None
    assert ImageCutSolver(a, b, refine=(3, 1), refine_where='all', **kw).refine == (3, 1, 0.0)
    s = ImageCutSolver(a, b, **kw)
    assert s.refine is None and s.refine_score_map is None and s.refine_shift_map is None
    for modes in (['elevation'], ['elevation2'], ['elevation', 'distance'], ['elevation', 'elevation2', 'distance']):
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, **dict(kw, degree_map_mode=modes), refine=(2, 1), refine_where='all')
        with pytest.raises(ValueError):
            _sharded(a, b, modes=modes, refine=(2, 1), refine_where='all', refiner=_host_refine)
        assert ImageCutSolver(a, b, **dict(kw, degree_map_mode=modes)).refine is None
    for bad in (2, (2,), (0, 1), (2, 4), (2, 1, 3.0), (2.0, 1), (2, 1, 0.0, 0)):
        with pytest.raises(ValueError):
            ImageCutSolver(a, b, refine=bad, refine_where='all', **kw)
        with pytest.raises(ValueError):
            _sharded(a, b, refine=bad, refine_where='all', refiner=_host_refine)
    with pytest.raises(ValueError):      # 'filled' needs fill=
        ImageCutSolver(a, b, refine=(2, 1), **kw)
    with pytest.raises(ValueError):
        _sharded(a, b, refine=(2, 1), refiner=_host_refine)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, refine=(2, 1), refine_where='holes', fill=16, **kw)
    with pytest.raises(ValueError):
        _sharded(a, b, refine=(2, 1), refine_where='holes', fill=16, filler=_host_fill, refiner=_host_refine)


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map): today's call."""
    a, b = _pcase()
    return [np.asarray(x) for x in _sharded(a, b)]


@pytest.fixture(scope='module')
def chain(plain):
    """photo reject -> fill -> refine (the filled cells) -> photo score, in the restatements."""
    a, b = _pcase()
    _, _, rejd, rej = photo_restate(a, b, plain[0][1], plain[0][0], PHOTO[0], 2, PHOTO[1], plain[0])
    fil = fill_restate(rejd, 16)
    mask = fil[1][1] | fil[1][0]
    row, col, rscore, rshift = refine_restate(a, b, fil[0][1], fil[0][0], REFINE[0], REFINE[1], 2, REFINE[2], True, mask)
    d = np.stack([col, row])
    score = photo_restate(a, b, row, col, PHOTO[0], 2)[0]
    return rej, fil, d, rscore, rshift, score


def _check_chain(got, plain, chain):
    rej, fil, d, rscore, rshift, score = chain
    # (d_map, out_map, holes, refine score, refine shift, rejected, score): the refine pair comes before the photo pair
    assert len(got) == 7
    assert same_bits(got[0], d) and same_bits(got[1], plain[1])
    assert np.array_equal(np.asarray(got[2]), fil[1])
    assert raw_bits(np.asarray(got[3]), rscore)
    assert np.asarray(got[4]).dtype == np.int8 and np.array_equal(np.asarray(got[4]), rshift)
    assert np.array_equal(np.asarray(got[5]), rej) and raw_bits(np.asarray(got[6]), score)


def _check_all(got, plain):
    a, b = _pcase()
    assert len(got) == 4
    want = refine_restate(a, b, plain[0][1], plain[0][0], 2, 1, 2, 0.0, True)
    assert same_bits(got[0], np.stack([want[1], want[0]])) and same_bits(got[1], plain[1])
    assert raw_bits(np.asarray(got[2]), want[2]) and np.array_equal(np.asarray(got[3]), want[3])


CHAIN_KW = dict(photo=PHOTO, photoer=_host_photo, fill=16, filler=_host_fill, refine=REFINE, refiner=_host_refine)


def test_sharded_refine_single_process(plain, chain):
    a, b = _pcase()
    _check_all(_sharded(a, b, refine=(2, 1), refine_where='all', refiner=_host_refine), plain)
    _check_chain(_sharded(a, b, **CHAIN_KW), plain, chain)
    rej, fil, d, rscore, rshift, score = chain
    hole = (fil[1][0] | fil[1][1]).astype(bool)
    # the position in the chain: after the fill (only filled cells are touched, and they were measured: a score that
    # is not NaN), before the final score (which is the score of the refined planes)
    assert rej.any() and hole[rej.astype(bool)].all()
    assert same_bits(d[:, ~hole], fil[0][:, ~hole]) and np.isnan(rscore[~hole]).all() and not rshift[:, ~hole].any()
    assert np.isfinite(rscore[hole]).any() and rshift[:, hole].any()
    moved = rshift.any(axis=0)
    assert (score[moved] >= photo_restate(a, b, fil[0][1], fil[0][0], PHOTO[0], 2)[0][moved]).mean() > 0.5


def test_sharded_refine_none_is_unchanged(plain):
    a, b = _pcase()
    got = _sharded(a, b, refine=None, refiner=_host_refine)
    assert len(got) == 2
    for g, r in zip(got, plain):
        assert same_bits(g, r)


def _layout_cases():
    """Keyword sets of solve_image_sharded, every stage as its host hook."""
    from test_bilateral_host import _host_smooth
    from test_fill_host import _host_stitch_fb
    from test_median_host import _host_median
    from test_merge_host import _host_merge
    from test_speckle_host import _host_speckle
    fill = dict(fill=16, filler=_host_fill)
    speckle = dict(speckle=(3, 0.5), speckler=_host_speckle)
    return {
        'none': {},
        'fill': fill,
        'speckle+fill': dict(fill, **speckle),
        'refine+fill+photo': dict(CHAIN_KW),
        'fb+fill': dict(fill, consistency=1.0, stitcher=_host_stitch_fb),
        'everything': dict(CHAIN_KW, consistency=1.0, merge='feather', merger=_host_merge, median=(1, 2),
                           median_weight='correlation', medianer=_host_median, smooth=(2, 0.5, 1.5),
                           smoother=_host_smooth, **speckle),
    }


@pytest.mark.parametrize('case', ['none', 'fill', 'speckle+fill', 'refine+fill+photo', 'fb+fill', 'everything'])
def test_sharded_tuple_is_the_layout(case):
    """The tuple solve_image_sharded returns is chain.Chain.layout entry for entry: as many tensors, each
    of the entry's shape and dtype (the receive tensors of the broadcast and the attributes of
    ImageCutSolver are made from the same list)."""
    import torch
    from deepmatching_stereo_matching_amd import chain
    kw = _layout_cases()[case]
    a, b = _pcase()
    n, _ = engine.cut_grid(a.shape, GEOM['image_size'], GEOM['stride'], GEOM['ws'])
    H, W = (GEOM['stride'][i] * (n[i] - 1) + GEOM['image_size'][i] for i in range(2))
    stages = {k: v for k, v in kw.items() if k in ('fill', 'speckle', 'smooth', 'median', 'median_weight', 'photo',
                                                   'refine')}
    layout = chain.Chain(PMODES, **stages).layout(H, W, kw.get('consistency'), kw.get('merge'))
    want = {'none': ['d_map', 'out_map'], 'fill': ['d_map', 'out_map', 'holes'],
            'speckle+fill': ['d_map', 'out_map', 'speckles', 'holes'],
            'refine+fill+photo': ['d_map', 'out_map', 'holes', 'refine_score', 'refine_shift', 'rejected', 'score'],
            'fb+fill': ['d_map', 'out_map', 'err', 'holes'],
            'everything': ['d_map', 'out_map', 'err', 'spread', 'count', 'speckles', 'holes', 'refine_score',
                           'refine_shift', 'rejected', 'score']}[case]
    assert [name for name, _, _ in layout] == want
    got = shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, PMODES,
                                    solver=_oracle_tiles, **dict({'stitcher': _host_stitch}, **kw))
    assert len(got) == len(layout)
    for t, (name, shape, dtype) in zip(got, layout):
        t = np.asarray(t)
        assert t.shape == shape and t.dtype == torch.empty(0, dtype=dtype).numpy().dtype, name


def _worker(rank, size, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        a, b = _pcase()
        every = _sharded(a, b, refine=(2, 1), refine_where='all', refiner=_host_refine)
        all_ = _sharded(a, b, **CHAIN_KW)
        root = _sharded(a, b, result='root', **CHAIN_KW)
        none = _sharded(a, b, refine=None, refiner=_host_refine)
        q.put((rank, [np.asarray(x) for x in every], [np.asarray(x) for x in all_],
               [None if x is None else np.asarray(x) for x in root], [np.asarray(x) for x in none]))
    finally:
        dist.destroy_process_group()


def test_sharded_refine_gloo_world_2(plain, chain):
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
    for rank, every, all_, root, none in res:
        _check_all(every, plain)
        _check_chain(all_, plain, chain)
        if rank == 0:
            _check_chain(root, plain, chain)
        else:
            assert root == [None] * 7
        assert len(none) == 2
        for g, r in zip(none, plain):
            assert same_bits(g, r), rank
