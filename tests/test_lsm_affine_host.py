"""Affine least-squares matching of a disparity map, host side (no GPU): the plain-loop restatement of
the definition in include/dmstereo_lsm.h (lsm_affine_restate: what dm_lsm_affine must equal bit for
bit; Python ints for the moments, numpy float64 scalars for the rest), a vectorised restatement pinned
to it (lsm_affine_fast: the one the GPU tests use), the consequences the header derives, the content
classes that hold the largest moments, the accuracy on pairs whose disparity is a ramp, argument
validation of the two C entries (it returns before any HIP call) and of the keywords, and the sharded
chain with the oracle as tile solver, a host stitcher and the restatement injected as the lsmer.

Comparisons with the restatement are bitwise (int64 views)."""
import ctypes
import math

import numpy as np
import pytest

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import chain as chain_mod
from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd import synthetic
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair

from test_fill_host import GEOM, _host_stitch, _oracle_tiles, raw_bits, same_bits
from test_lsm_host import _inside, _moments, _position, _zncc, _zncc_fast, lsm_fast
from test_photo_host import DMAX, NAN, _finite, _offsets, _pcase, photo_fast, planes
from test_refine_host import QNAN


@pytest.fixture(scope='module', autouse=True)
def entries():
    """What this file restates and checks is the pair of C entries: without them nothing here holds."""
    lib = L.load()
    assert hasattr(lib, 'dm_lsm_affine') and hasattr(lib, 'dm_lsm_affine_bytes')
    assert callable(getattr(engine, 'lsm_affine', None)) and callable(getattr(engine, 'lsm_model_params', None))


F = np.float64
PIVOT = F(2.0 ** -20)
CORNERS = ((-1, -1), (1, -1), (-1, 1), (1, 1))      # (u, v) / r of the four corner taps


# ---------------------------------------------------------------------------------------------
# the definition in plain loops
# ---------------------------------------------------------------------------------------------
def _moments6(A_, cy, cx, r):
    """Rule 2 on one cell, Python ints -> (sa, saa, f[6], N[k][l] for k >= l, RA[6]) and, in raster order, the taps'
    A and phi."""
    D = 2 * r + 1
    n = D * D
    sa = saa = 0
    f, ra = [0] * 6, [0] * 6
    M = [[0] * 6 for _ in range(6)]
    taps = []
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            a = A_[cy + v][cx + u]
            gx, gy = A_[cy + v][cx + u + 1] - A_[cy + v][cx + u - 1], A_[cy + v + 1][cx + u] - A_[cy + v - 1][cx + u]
            phi = (gx, gx * u, gx * v, gy, gy * u, gy * v)
            taps.append((u, v, a, phi))
            sa += a
            saa += a * a
            for k in range(6):
                f[k] += phi[k]
                ra[k] += phi[k] * a
                for l in range(k + 1):
                    M[k][l] += phi[k] * phi[l]
    N = [[n * M[k][l] - f[k] * f[l] for l in range(k + 1)] for k in range(6)]
    RA = [n * ra[k] - f[k] * sa for k in range(6)]
    assert all(abs(t) < 2 ** 53 for row in N for t in row) and all(abs(t) < 2 ** 53 for t in RA)
    return sa, saa, f, N, RA, taps


def _factor(N):
    """Rule 3 -> (L, d), or None when a pivot fails."""
    Lf = [[None] * 6 for _ in range(6)]
    c = [[None] * 6 for _ in range(6)]
    d = [None] * 6
    for j in range(6):
        for i in range(j, 6):
            t = F(N[i][j])
            for k in range(j):
                t = t - Lf[i][k] * c[j][k]
            c[i][j] = t
        d[j] = c[j][j]
        if not d[j] > F(N[j][j]) * PIVOT:
            return None
        for i in range(j + 1, 6):
            Lf[i][j] = c[i][j] / d[j]
    return Lf, d


def _solve(Lf, d, rhs):
    z = [None] * 6
    for i in range(6):
        t = rhs[i]
        for k in range(i):
            t = t - Lf[i][k] * z[k]
        z[i] = t
    for i in range(5, -1, -1):
        t = z[i] / d[i]
        for k in range(i + 1, 6):
            t = t - Lf[k][i] * z[k]
        z[i] = t
    return z


def _warp_ok(p, r, Hi, Wi):
    a1, d1 = F(1.0) + p[1], F(1.0) + p[5]
    for su, sv in CORNERS:
        u, v = F(su * r), F(sv * r)
        X, Y = p[0] + (a1 * u + p[2] * v), p[3] + (p[4] * u + d1 * v)
        if not (F(0.0) <= Y < F(Hi - 1) and F(0.0) <= X < F(Wi - 1)):      # (NaN fails)
            return False
    return True


def _warp_sums(B_, taps, p, grad):
    """The sums of rule 5 under the warp p -> (Sp, Spp, Sap, T[6])."""
    a1, d1 = F(1.0) + p[1], F(1.0) + p[5]
    Sp = Spp = Sap = F(0.0)
    T = [F(0.0)] * 6
    for u, v, a, phi in taps:
        X, Y = p[0] + (a1 * F(u) + p[2] * F(v)), p[3] + (p[4] * F(u) + d1 * F(v))
        iy, ix = math.floor(Y), math.floor(X)
        fy, fx = Y - F(iy), X - F(ix)
        g_y, g_x = F(1.0) - fy, F(1.0) - fx
        P = ((g_y * g_x * F(B_[iy][ix]) + g_y * fx * F(B_[iy][ix + 1])) + fy * g_x * F(B_[iy + 1][ix])) + \
            fy * fx * F(B_[iy + 1][ix + 1])
        Sp = Sp + P
        Spp = Spp + P * P
        Sap = Sap + F(a) * P
        if grad:
            T = [T[k] + F(phi[k]) * P for k in range(6)]
    return Sp, Spp, Sap, T


def lsm_affine_restate(img1, img2, d_row, d_col, r, iters, offset=0, max_move=1.0, max_shear=0.5, mask=None,
                       trace=None):
    """The definition -> (out_row, out_col, score, int8 status [H][W], affine [4][H][W]).  ``trace``: a list that
    receives (y, x, t, alpha, rhs) of every step that was solved."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    A_, B_ = img1.tolist(), img2.tolist()
    out_row, out_col = d_row.copy(), d_col.copy()      # a cell that is not accepted keeps its bits
    score = np.full((H, W), QNAN)
    affine = np.full((4, H, W), QNAN)
    status = np.zeros((H, W), dtype=np.int8)
    max_move, max_shear = F(max_move), F(max_shear)
    n = (2 * r + 1) ** 2
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                if mask is not None and not mask[y][x]:
                    continue
                dr, dc = d_row[y, x], d_col[y, x]
                if not (_finite(dr) and _finite(dc)):
                    continue
                cy, cx = y + oy, x + ox
                if not (r + 1 <= cy <= Hi - r - 2 and r + 1 <= cx <= Wi - r - 2):
                    continue
                sa, saa, f, N, RA, taps = _moments6(A_, cy, cx, r)
                fac = _factor(N)
                if fac is None:
                    status[y, x] = -1
                    continue
                Lf, d = fac
                py0, px0 = F(cy) - dr, F(cx) - dc
                if not _inside(py0, px0, Hi, Wi, r):
                    status[y, x] = -2
                    continue
                VA = F(n * saa - sa * sa)
                (_, _, gx, gy, *_), Gx, Gy = _moments(A_, cy, cx, r)
                num, vb, _, _ = _position(A_, B_, Gx, Gy, sa, gx, gy, cy, cx, py0, px0, r)
                s0 = _zncc(VA, num, vb)
                score[y, x] = s0
                p = [px0, F(0.0), F(0.0), py0, F(0.0), F(0.0)]
                st = iters if _warp_ok(p, r, Hi, Wi) else -2
                nn, fsa = F(n), F(sa)
                for t in range(1, iters + 1):
                    if st != iters:
                        break
                    Sp, Spp, Sap, T = _warp_sums(B_, taps, p, True)
                    num, vb = nn * Sap - fsa * Sp, nn * Spp - Sp * Sp
                    if not vb > 0.0:
                        st = -1
                        break
                    alpha = num / vb
                    rhs = [F(RA[k]) - alpha * (nn * T[k] - F(f[k]) * Sp) for k in range(6)]
                    if trace is not None:
                        trace.append((y, x, t, alpha, rhs))
                    delta = _solve(Lf, d, rhs)
                    p = [p[k] + F(2.0) * delta[k] for k in range(6)]
                    if not (abs(p[0] - px0) <= max_move and abs(p[3] - py0) <= max_move and
                            all(abs(p[k]) <= max_shear for k in (1, 2, 4, 5)) and _warp_ok(p, r, Hi, Wi)):
                        st = -2
                if st == iters:
                    Sp, Spp, Sap, _ = _warp_sums(B_, taps, p, False)
                    s1 = _zncc(VA, nn * Sap - fsa * Sp, nn * Spp - Sp * Sp)
                    if s1 > s0:
                        out_row[y, x], out_col[y, x], score[y, x] = F(cy) - p[3], F(cx) - p[0], s1
                        affine[:, y, x] = (p[1], p[2], p[4], p[5])
                    else:
                        st = -3
                status[y, x] = st
    return out_row, out_col, score, status, affine


# ---------------------------------------------------------------------------------------------
# the fast restatement: the live cells as one axis, the taps in a loop, the moments in int64
# ---------------------------------------------------------------------------------------------
def _warp_ok_fast(p, r, Hi, Wi):
    a1, d1 = 1.0 + p[1], 1.0 + p[5]
    ok = np.ones(p[0].shape, dtype=bool)
    for su, sv in CORNERS:
        u, v = float(su * r), float(sv * r)
        X, Y = p[0] + (a1 * u + p[2] * v), p[3] + (p[4] * u + d1 * v)
        ok &= (Y >= 0.0) & (Y < float(Hi - 1)) & (X >= 0.0) & (X < float(Wi - 1))
    return ok


def _warp_sums_fast(B64, Aw, phi, p, r, grad):
    a1, d1 = 1.0 + p[1], 1.0 + p[5]
    z = np.zeros(p[0].shape)
    Sp, Spp, Sap, T = z.copy(), z.copy(), z.copy(), [z.copy() for _ in range(6)]
    f = lambda t: t.astype(np.float64)
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            X, Y = p[0] + (a1 * float(u) + p[2] * float(v)), p[3] + (p[4] * float(u) + d1 * float(v))
            fly, flx = np.floor(Y), np.floor(X)
            iy, ix = fly.astype(np.int64), flx.astype(np.int64)
            fy, fx = Y - fly, X - flx
            g_y, g_x = 1.0 - fy, 1.0 - fx
            P = ((g_y * g_x * f(B64[iy, ix]) + g_y * fx * f(B64[iy, ix + 1])) + fy * g_x * f(B64[iy + 1, ix])) + \
                fy * fx * f(B64[iy + 1, ix + 1])
            Sp = Sp + P
            Spp = Spp + P * P
            Sap = Sap + f(Aw[:, v + r, u + r]) * P
            if grad:
                T = [T[k] + f(phi[k][:, v + r, u + r]) * P for k in range(6)]
    return Sp, Spp, Sap, T


def lsm_affine_fast(img1, img2, d_row, d_col, r, iters, offset=0, max_move=1.0, max_shear=0.5, mask=None):
    """lsm_affine_restate, vectorised."""
    oy, ox = _offsets(offset)
    Hi, Wi = img1.shape
    d_row, d_col = np.asarray(d_row, dtype=np.float64), np.asarray(d_col, dtype=np.float64)
    H, W = d_row.shape
    D = 2 * r + 1
    n = D * D
    A64, B64 = img1.astype(np.int64), img2.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy + oy, xx + ox
    with np.errstate(invalid='ignore'):
        live = (np.abs(d_row) <= DMAX) & (np.abs(d_col) <= DMAX)
    live = live & (cy >= r + 1) & (cy <= Hi - r - 2) & (cx >= r + 1) & (cx <= Wi - r - 2)
    if mask is not None:
        live = live & (np.asarray(mask) != 0)
    out_row, out_col = d_row.copy(), d_col.copy()
    score = np.full(H * W, QNAN)
    affine = np.full((4, H * W), QNAN)
    status = np.zeros(H * W, dtype=np.int8)
    idx = np.nonzero(live.ravel())[0]
    if idx.size:
        f = lambda t: t.astype(np.float64)
        cyl, cxl = cy.ravel()[idx], cx.ravel()[idx]
        t = np.arange(D + 2)
        Ah = A64[cyl[:, None, None] - r - 1 + t[None, :, None], cxl[:, None, None] - r - 1 + t[None, None, :]]
        Aw = Ah[:, 1:-1, 1:-1]
        Gx, Gy = Ah[:, 1:-1, 2:] - Ah[:, 1:-1, :-2], Ah[:, 2:, 1:-1] - Ah[:, :-2, 1:-1]
        V, U = np.mgrid[-r:r + 1, -r:r + 1]
        phi = [Gx, Gx * U, Gx * V, Gy, Gy * U, Gy * V]
        sa = Aw.sum((1, 2))
        VA = f(n * (Aw * Aw).sum((1, 2)) - sa * sa)
        fk = [q.sum((1, 2)) for q in phi]
        N = [[f(n * (phi[k] * phi[l]).sum((1, 2)) - fk[k] * fk[l]) for l in range(k + 1)] for k in range(6)]
        RA = [f(n * (phi[k] * Aw).sum((1, 2)) - fk[k] * sa) for k in range(6)]
        with np.errstate(all='ignore'):
            Lf = [[None] * 6 for _ in range(6)]
            c = [[None] * 6 for _ in range(6)]
            d = [None] * 6
            ok = np.ones(idx.size, dtype=bool)
            for j in range(6):
                for i in range(j, 6):
                    q = N[i][j]
                    for k in range(j):
                        q = q - Lf[i][k] * c[j][k]
                    c[i][j] = q
                d[j] = c[j][j]
                ok &= d[j] > N[j][j] * PIVOT
                for i in range(j + 1, 6):
                    Lf[i][j] = c[i][j] / d[j]
            py0, px0 = f(cyl) - d_row.ravel()[idx], f(cxl) - d_col.ravel()[idx]
            inside = (py0 >= float(r)) & (py0 < float(Hi - r - 1)) & (px0 >= float(r)) & (px0 < float(Wi - r - 1))
            st = np.where(ok, np.where(inside, iters, -2), -1)
            s0 = np.full(idx.size, QNAN)
            scored = st == iters
            ps = photo_fast(img1, img2, d_row, d_col, r, offset)[0].ravel()[idx]
            s0[scored] = ps[scored]
            zero = np.zeros(idx.size)
            p = [px0.copy(), zero.copy(), zero.copy(), py0.copy(), zero.copy(), zero.copy()]
            st[scored & ~_warp_ok_fast(p, r, Hi, Wi)] = -2
            nn, fsa = float(n), f(sa)
            for step in range(1, iters + 1):
                g = np.nonzero(st == iters)[0]
                if not g.size:
                    break
                pg = [q[g] for q in p]
                Sp, Spp, Sap, T = _warp_sums_fast(B64, Aw[g], [q[g] for q in phi], pg, r, True)
                num, vb = nn * Sap - fsa[g] * Sp, nn * Spp - Sp * Sp
                pos = vb > 0.0
                alpha = num / np.where(pos, vb, 1.0)
                z = [None] * 6
                for i in range(6):
                    q = RA[i][g] - alpha * (nn * T[i] - f(fk[i][g]) * Sp)
                    for k in range(i):
                        q = q - Lf[i][k][g] * z[k]
                    z[i] = q
                for i in range(5, -1, -1):
                    q = z[i] / d[i][g]
                    for k in range(i + 1, 6):
                        q = q - Lf[k][i][g] * z[k]
                    z[i] = q
                new = [pg[k] + 2.0 * z[k] for k in range(6)]
                good = pos & (np.abs(new[0] - px0[g]) <= max_move) & (np.abs(new[3] - py0[g]) <= max_move)
                for k in (1, 2, 4, 5):
                    good &= np.abs(new[k]) <= max_shear
                good &= _warp_ok_fast(new, r, Hi, Wi)
                st[g[~pos]] = -1
                st[g[pos & ~good]] = -2
                for k in range(6):
                    p[k][g[good]] = new[k][good]
            g = np.nonzero(st == iters)[0]
            sc = s0.copy()
            if g.size:
                pg = [q[g] for q in p]
                Sp, Spp, Sap, _ = _warp_sums_fast(B64, Aw[g], None, pg, r, False)
                s1 = _zncc_fast(VA[g], nn * Sap - fsa[g] * Sp, nn * Spp - Sp * Sp)
                acc = s1 > s0[g]
                st[g[~acc]] = -3
                a = g[acc]
                sc[a] = s1[acc]
                out_row.ravel()[idx[a]] = f(cyl[a]) - p[3][a]
                out_col.ravel()[idx[a]] = f(cxl[a]) - p[0][a]
                for j, k in enumerate((1, 2, 4, 5)):
                    affine[j, idx[a]] = p[k][a]
        score[idx] = sc
        status[idx] = st.astype(np.int8)
    return out_row, out_col, score.reshape(H, W), status.reshape(H, W), affine.reshape(4, H, W)


def all_bits5(p, q):
    """Five outputs against five outputs: the planes, the score and the affine values as 64-bit patterns, the status
    as int8."""
    return raw_bits(p[0], q[0]) and raw_bits(p[1], q[1]) and raw_bits(p[2], q[2]) and \
        np.asarray(p[3]).dtype == np.int8 and np.array_equal(np.asarray(p[3]), np.asarray(q[3])) and \
        raw_bits(np.asarray(p[4]), np.asarray(q[4]))


def ramp_case(seed, g, axis=1, r=5, noise=0.0, d0=2.0, size=56):
    """ramp_pair(size, size, seed, g) as a whole-image map: the truth and a start that is the truth plus uniform
    +-0.6 px per axis from default_rng([seed, 11]) -> (img1, img2, start row, start col, true row, true col)."""
    a, b, d = synthetic.ramp_pair(size, size, seed, g, axis=axis, d0=d0, noise=noise)
    z = np.zeros_like(d)
    tr, tc = (z, d) if axis == 1 else (d, z)
    rng = np.random.default_rng([seed, 11])
    return a, b, tr + rng.uniform(-0.6, 0.6, d.shape), tc + rng.uniform(-0.6, 0.6, d.shape), tr, tc


def central(status, axis):
    """The cells the accuracy is measured on: status not 0 or -2, in the central half along the ramp."""
    H, W = status.shape
    yy, xx = np.mgrid[0:H, 0:W]
    t, side = (xx, W) if axis == 1 else (yy, H)
    return (status != 0) & (status != -2) & (t >= side // 4) & (t < side - side // 4)


def rms_at(row, col, tr, tc, sel):
    return float(np.sqrt(np.mean((row[sel] - tr[sel]) ** 2 + (col[sel] - tc[sel]) ** 2)))


# ---------------------------------------------------------------------------------------------
# 1. the restatements and the consequences of the definition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (6, 4)])
@pytest.mark.parametrize('r,iters', [(2, 1), (2, 3), (3, 2)])
def test_fast_equals_literal(shape, r, iters):
    H, W = shape
    rng = np.random.default_rng(H + W)
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    seen = set()
    for seed, kind in enumerate(['int', 'frac', 'mixed']):
        for margin, off in [(r + 5, (r + 5, r + 5)), (r + 2, (r + 2, r + 3)), (2, (0, 1))]:
            a, b = stereo_pair(H + 2 * margin, W + 2 * margin + 1, seed=seed, dx=2)
            dr, dc = planes(H, W, seed, kind, amp=1.0)
            dc = dc + 2.0 if kind != 'mixed' else dc      # near the truth, so that warps are accepted too
            for kw in (dict(), dict(max_move=0.25, mask=mask), dict(max_move=2.0, max_shear=0.05)):
                lit = lsm_affine_restate(a, b, dr, dc, r, iters, off, **kw)
                assert all_bits5(lit, lsm_affine_fast(a, b, dr, dc, r, iters, off, **kw)), (shape, r, iters, kind, kw)
                kept = lit[3] != iters
                assert raw_bits(lit[0][kept], dr[kept]) and raw_bits(lit[1][kept], dc[kept])      # NaN payloads, -0.0
                assert np.isnan(lit[4][:, kept]).all() and not np.isnan(lit[4][:, ~kept]).any()
                seen |= set(np.unique(lit[3]).tolist())
    if shape == (6, 4):
        assert {0, -2, -3, iters} <= seen


def test_fast_equals_literal_on_a_ramp():
    """The same pin where the affine parameters are not small, on both axes."""
    for axis, g in ((1, 0.2), (0, -0.15)):
        a, b, sr, sc, tr, tc = ramp_case(1, g, axis, size=24)
        sl = (slice(9, 13), slice(8, 14))
        lit = lsm_affine_restate(a, b, sr[sl], sc[sl], 3, 4, (9, 8))
        assert all_bits5(lit, lsm_affine_fast(a, b, sr[sl], sc[sl], 3, 4, (9, 8)))
        assert (lit[3] == 4).any()


def test_identical_windows_at_an_integer_disparity_never_move():
    """P = A exactly, alpha = 1.0 and rhs = 0.0, status -3, the score 1.0: the map comes out unchanged to the bit."""
    for r, iters in [(2, 3), (3, 2)]:
        m = r + 4
        a, b = stereo_pair(6 + 2 * m, 7 + 2 * m, seed=3, dx=2)
        dr, dc = np.zeros((6, 7)), np.full((6, 7), 2.0)
        dr[3, 4] = -0.0
        trace = []
        res = lsm_affine_restate(a, b, dr, dc, r, iters, m, trace=trace)
        assert len(trace) == 6 * 7 * iters
        assert all(alpha == 1.0 and all(q == 0.0 for q in rhs) for _, _, _, alpha, rhs in trace)
        assert (res[3] == -3).all() and (res[2] == 1.0).all() and np.isnan(res[4]).all()
        assert raw_bits(res[0], dr) and raw_bits(res[1], dc)
        assert all_bits5(res, lsm_affine_fast(a, b, dr, dc, r, iters, m))
        z = np.zeros((6, 7))
        res = lsm_affine_fast(a, a, z, z, r, iters, m)      # img2 == img1 at disparity 0 likewise
        assert (res[3] == -3).all() and raw_bits(res[0], z) and raw_bits(res[1], z)


@pytest.mark.parametrize('r', [2, 3, 5])
def test_accepted_is_strictly_better_and_the_rest_is_photo_score(r):
    """An accepted cell scores strictly above dm_photo_score of the input; an unaccepted scored cell reports its
    bits; a cell that was not scored is NaN."""
    H, W = 20, 23
    for seed, kind in enumerate(['int', 'frac', 'mixed']):
        for margin in (r + 5, r + 2):
            a, b = stereo_pair(H + 2 * margin, W + 2 * margin, seed=seed + 3, dx=1)
            dr, dc = planes(H, W, seed, kind, amp=1.5)
            dc = dc + 1.0
            ps = photo_fast(a, b, dr, dc, r, margin)[0]
            row, col, score, status, aff = lsm_affine_fast(a, b, dr, dc, r, 3, margin)
            acc = status == 3
            assert acc.any() and (~acc).any()
            assert (score[acc] > ps[acc]).all()
            rest = ~acc & ~np.isnan(score)
            assert rest.any() and raw_bits(score[rest], ps[rest])
            assert np.isin(status[np.isnan(score)], (0, -1, -2)).all() and np.isin(status[rest], (-1, -2, -3)).all()
            assert raw_bits(row[~acc], dr[~acc]) and raw_bits(col[~acc], dc[~acc])
            assert np.isnan(aff[:, ~acc]).all() and (np.abs(aff[:, acc]) <= 0.5).all()


def test_skipped_and_failed_cells():
    r = 2
    a, b = stereo_pair(24, 26, seed=1, dx=0)
    one = lambda v: np.full((1, 1), v)
    run = lambda dr, dc, off, **kw: lsm_affine_restate(a, b, one(dr), one(dc), r, 2, off, **kw)
    payload = np.array([0x7ff8000000001234, 0xfff8000000000001, 0x7ff0000000000000, 0xfff0000000000000],
                       dtype=np.uint64).view(np.float64)
    for v in payload:
        for dr, dc in ((v, 0.0), (0.0, v), (v, -0.0)):
            res = run(dr, dc, (8, 9))
            assert raw_bits(res[0], one(dr)) and raw_bits(res[1], one(dc)) and raw_bits(res[2], one(QNAN))
            assert res[3][0, 0] == 0 and raw_bits(res[4], np.full((4, 1, 1), QNAN))
    assert run(0.3, 0.3, (8, 9), mask=np.zeros((1, 1), dtype=np.uint8))[3][0, 0] == 0
    # the halo: cy = r + 1 is the first row that is matched
    assert run(0.3, 0.3, (r, 9))[3][0, 0] == 0 and run(0.3, 0.3, (r + 1, 9))[3][0, 0] != 0
    assert run(0.3, 0.3, (24 - r - 1, 9))[3][0, 0] == 0 and run(0.3, 0.3, (24 - r - 2, 9))[3][0, 0] != 0
    assert run(0.3, 0.3, (8, 26 - r - 1))[3][0, 0] == 0 and run(0.3, 0.3, (8, r))[3][0, 0] == 0
    # the start leaves the image: -2 and NaN; 1e300 likewise
    for dr in (8.0 - r + 0.5, 8.0 - (24 - r - 1), 1e300, -1e300):
        res = run(dr, 0.0, (8, 9))
        assert res[3][0, 0] == -2 and raw_bits(res[2], one(QNAN)) and raw_bits(res[0], one(dr))
    # a flat img1 window: no pivot, status -1, NaN; a flat img2 patch under a textured window: -1 and the score 0.0
    flat = np.full_like(a, 7)
    res = lsm_affine_restate(flat, b, one(0.25), one(0.25), r, 2, (8, 9))
    assert res[3][0, 0] == -1 and raw_bits(res[2], one(QNAN))
    res = lsm_affine_restate(a, flat, one(0.25), one(0.25), r, 2, (8, 9))
    assert res[3][0, 0] == -1 and raw_bits(res[2], one(0.0)) and raw_bits(res[0], one(0.25))
    # max_shear: on a ramp of slope 0.2 the stretch is -1/6; a bound of 0.05 ends the cells at -2 with photo_score's bits
    a2, b2, sr, sc, tr, tc = ramp_case(2, 0.2, size=40)
    wide, tight = lsm_affine_fast(a2, b2, sr, sc, 5, 4), lsm_affine_fast(a2, b2, sr, sc, 5, 4, max_shear=0.05)
    far = (wide[3] == 4) & (np.abs(wide[4][0]) > 0.1)
    assert far.any() and (tight[3][far] == -2).all()
    assert raw_bits(tight[0][far], sr[far]) and raw_bits(tight[2][far], photo_fast(a2, b2, sr, sc, 5)[0][far])


@pytest.mark.parametrize('kind', ['const', 'identical'])
def test_no_cell_is_accepted(kind):
    H, W = 5, 6
    for r, iters in [(2, 2), (3, 3)]:
        m = r + 3
        a, b = content_pair(kind, H + 2 * m, W + 2 * m, 4)
        z = np.zeros((H, W))
        res = lsm_affine_restate(a, b, z, z, r, iters, m)
        assert all_bits5(res, lsm_affine_fast(a, b, z, z, r, iters, m))
        assert not (res[3] == iters).any() and raw_bits(res[0], z) and raw_bits(res[1], z)
        if kind == 'const':
            assert (res[3] == -1).all() and np.isnan(res[2]).all()      # no gradient: the first pivot is 0
        else:
            assert np.isin(res[3], (-1, -3)).all() and (res[3] == -3).mean() > 0.9


@pytest.mark.parametrize('kind', ['binary', 'dark_bright'])
def test_largest_moments_at_radius_7(kind):
    """The classes that hold the largest moments: every difference is 0 or +-255, so n sum(phi_k^2) passes 2^32 and
    the products of the factorisation pass 2^63; a 32-bit moment or an integer factorisation fails here."""
    H, W, r = 2, 3, 7
    m = r + 3
    a, b = content_pair(kind, H + 2 * m, W + 2 * m, 3)
    rng = np.random.default_rng(2)
    dr, dc = rng.uniform(-1, 1, (H, W)), rng.uniform(-1, 1, (H, W)) + (0.0 if kind == 'dark_bright' else 3.0)
    lit = lsm_affine_restate(a, b, dr, dc, r, 2, m)
    assert all_bits5(lit, lsm_affine_fast(a, b, dr, dc, r, 2, m))
    assert (lit[3] != 0).all()
    if kind == 'binary':
        N = _moments6(a.tolist(), m, m, r)[3]
        assert max(N[k][k] for k in range(6)) >= 2 ** 32 and N[1][1] * N[2][2] >= 2 ** 63


def test_pivot_bound_keeps_textured_cells():
    """2^-20 rejects no cell of the textured pairs: the smallest pivot ratio d_k / N_kk met on ramp_pair and
    stereo_pair at radius 2 .. 7 is printed; it stays four orders of magnitude above the bound."""
    worst = 1.0
    for r in (2, 3, 5, 7):
        for img in (synthetic.ramp_pair(40, 40, 1, 0.2)[0], stereo_pair(40, 40, seed=2, dx=1)[0]):
            A_ = img.tolist()
            for cy in range(r + 1, 40 - r - 1, 3):
                for cx in range(r + 1, 40 - r - 1, 3):
                    N = _moments6(A_, cy, cx, r)[3]
                    fac = _factor(N)
                    assert fac is not None
                    worst = min(worst, min(float(fac[1][k]) / N[k][k] for k in range(6)))
    print('smallest pivot ratio %.3g (bound %.3g)' % (worst, float(PIVOT)))
    assert worst > 100 * float(PIVOT)


# ---------------------------------------------------------------------------------------------
# 2. ramp_pair and the accuracy on it
# ---------------------------------------------------------------------------------------------
def test_ramp_pair():
    a, b, d = synthetic.ramp_pair(20, 30, 3, 0.2)
    assert a.shape == b.shape == d.shape == (20, 30) and a.dtype == b.dtype == np.uint8 and d.dtype == np.float64
    xx = np.arange(30.0)
    assert np.array_equal(d, np.tile(xx - (xx - 2.0 + 0.2 * 15) / 1.2, (20, 1)))
    a0, b0, d0 = synthetic.ramp_pair(30, 20, 3, 0.2, axis=0)
    assert np.array_equal(a0, a.T) and np.array_equal(b0, b.T) and np.array_equal(d0, d.T)
    # g = 0 with an integer d0 is a plain shift: img2 is img1 moved by d0 columns, exactly
    a, b, d = synthetic.ramp_pair(12, 16, 1, 0.0, d0=3.0)
    assert np.array_equal(a[:, 3:], b[:, :-3]) and (d == 3.0).all()
    # the draws: the same seed gives the same pair, the noise is added to both images
    assert all(np.array_equal(p, q) for p, q in zip(synthetic.ramp_pair(12, 16, 1, 0.1, noise=2.0),
                                                    synthetic.ramp_pair(12, 16, 1, 0.1, noise=2.0)))
    n1, n2, _ = synthetic.ramp_pair(12, 16, 1, 0.1, noise=2.0)
    c1, c2, _ = synthetic.ramp_pair(12, 16, 1, 0.1)
    assert not np.array_equal(n1, c1) and not np.array_equal(n2, c2)
    # the sign of the truth: photo_score is highest at +d, for both signs of the slope
    for g in (0.2, -0.15):
        a, b, d = synthetic.ramp_pair(40, 40, 2, g)
        z = np.zeros_like(d)
        at = lambda s: np.nanmean(photo_fast(a, b, z, s * d, 2)[0][:, 10:30])
        assert at(1.0) > 0.95 and at(1.0) > at(-1.0) and at(1.0) > at(0.0)
    for bad in (dict(axis=2), dict(g=-1.0)):
        with pytest.raises(ValueError):
            synthetic.ramp_pair(8, 8, 0, **dict(dict(g=0.1), **bad))


SEEDS = (1, 2, 4, 5)


@pytest.mark.parametrize('noise', [0.0, 2.0])
@pytest.mark.parametrize('axis,g', [(1, 0.2), (0, 0.2), (1, -0.15), (0, -0.15)])
def test_accuracy_on_a_ramp(axis, g, noise):
    """ramp_pair(56, 56, seed, g), radius 5: 6 affine steps against 4 shift steps from the same start (the truth plus
    uniform +-0.6 px per axis), on the cells in the central half along the ramp whose affine status is not 0 or -2.
    The bounds are the issue's: the affine rms error below a quarter of the shift solve's, and the median recovered
    stretch within 0.01 of -g / (1 + g).  (The figures are printed; DESIGN.md 4p quotes them.)"""
    for seed in SEEDS:
        a, b, sr, sc, tr, tc = ramp_case(seed, g, axis, noise=noise)
        row, col, score, status, aff = lsm_affine_fast(a, b, sr, sc, 5, 6)
        sel = central(status, axis)
        srow, scol, _, sstatus = lsm_fast(a, b, sr, sc, 5, 4)
        e_aff, e_shift = rms_at(row, col, tr, tc, sel), rms_at(srow, scol, tr, tc, sel)
        acc = sel & (status == 6)
        stretch = float(np.median(aff[0 if axis == 1 else 3][acc]))
        print('axis %d g %+.2f noise %.0f seed %d: affine %.4f px, shift %.4f px, accepted %.3f, stretch %+.4f (truth %+.4f)'
              % (axis, g, noise, seed, e_aff, e_shift, acc.sum() / sel.sum(), stretch, -g / (1 + g)))
        assert sel.sum() > 500
        assert e_aff < 0.25 * e_shift
        assert abs(stretch - (-g / (1 + g))) < 0.01


def test_accuracy_on_flat_terrain():
    """At g = 0 the four extra parameters cost nothing that matters: within 0.02 px rms of the truth."""
    for seed in SEEDS:
        a, b, sr, sc, tr, tc = ramp_case(seed, 0.0)
        row, col, score, status, aff = lsm_affine_fast(a, b, sr, sc, 5, 6)
        sel = central(status, 1)
        e = rms_at(row, col, tr, tc, sel)
        print('g 0 seed %d: affine %.4f px, accepted %.3f' % (seed, e, (status[sel] == 6).mean()))
        assert sel.sum() > 500 and e < 0.02


# ---------------------------------------------------------------------------------------------
# 3. validation of the C entries and of the keywords
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return L.load()


P8 = ctypes.c_void_p(8)   # a non-null pointer that validation never dereferences


def test_header_declares_lsm_affine(lib):
    assert L.header_symbols(L.HEADER_LSM) == ['dm_lsm_affine', 'dm_lsm_affine_bytes']
    assert all(s in L.SIGNATURES and hasattr(lib, s) for s in L.header_symbols(L.HEADER_LSM))
    assert not set(L.header_symbols(L.HEADER_LSM)) & set(L.header_symbols())
    assert '#include "dmstereo.h"' in open(L.HEADER_LSM).read()
    assert lib.dm_abi_version() == 110


def _args(img1=P8, s1=24, img2=P8, s2=24, Hi=24, Wi=24, d_row=P8, d_col=P8, H=4, W=4, oy=4, ox=4, r=2, iters=2,
          max_move=1.0, max_shear=0.5, flags=0, mask=None, out_row=P8, out_col=P8, score=None, status=None,
          affine=None, work=P8):
    return (img1, s1, img2, s2, Hi, Wi, d_row, d_col, H, W, oy, ox, r, iters, max_move, max_shear, flags, mask,
            out_row, out_col, score, status, affine, work, None)


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
    (dict(s1=23), L.DM_ERR_ARG, 'stride'),
    (dict(s2=-24), L.DM_ERR_ARG, 'stride'),
    (dict(H=0), L.DM_ERR_ARG, 'map shape'),
    (dict(W=-4), L.DM_ERR_ARG, 'map shape'),
    (dict(oy=2 ** 30 + 1), L.DM_ERR_ARG, 'offset'),
    (dict(ox=-2 ** 30 - 1), L.DM_ERR_ARG, 'offset'),
    (dict(r=0), L.DM_ERR_ARG, 'radius'),
    (dict(r=1), L.DM_ERR_ARG, 'radius'),
    (dict(r=8), L.DM_ERR_ARG, 'radius'),
    (dict(iters=0), L.DM_ERR_ARG, 'iters'),
    (dict(iters=9), L.DM_ERR_ARG, 'iters'),
    (dict(max_move=0.0), L.DM_ERR_ARG, 'max_move'),
    (dict(max_move=2.0000001), L.DM_ERR_ARG, 'max_move'),
    (dict(max_move=NAN), L.DM_ERR_ARG, 'max_move'),
    (dict(max_shear=0.0), L.DM_ERR_ARG, 'max_shear'),
    (dict(max_shear=1.0), L.DM_ERR_ARG, 'max_shear'),
    (dict(max_shear=-0.5), L.DM_ERR_ARG, 'max_shear'),
    (dict(max_shear=NAN), L.DM_ERR_ARG, 'max_shear'),
    (dict(flags=1), L.DM_ERR_ARG, 'flags'),
    (dict(flags=-1), L.DM_ERR_ARG, 'flags'),
    (dict(H=65536, W=32768), L.DM_ERR_UNSUPPORTED, 'cells'),                       # H W = 2^31
    (dict(H=64 * 65535 + 1, W=1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(Hi=2 ** 30 + 1), L.DM_ERR_UNSUPPORTED, 'cells'),
    (dict(Wi=2 ** 30 + 1, s1=2 ** 31, s2=2 ** 31, r=7, iters=8, max_move=2.0, max_shear=0.999, mask=P8, score=P8,
          status=P8, affine=P8), L.DM_ERR_UNSUPPORTED, 'cells'),                   # every argument valid but the shape
])
def test_lsm_affine_validation(lib, kw, code, needle):
    assert lib.dm_lsm_affine(*_args(**kw)) == code
    assert needle in L.last_error()


def test_lsm_affine_bytes(lib):
    ok = (24, 24, 4, 4, 2, 2)
    assert lib.dm_lsm_affine_bytes(*ok) > 0
    for i, bad in [(0, 0), (0, 2 ** 30 + 1), (1, -1), (1, 2 ** 30 + 1), (2, 0), (3, 0), (2, 64 * 65535 + 1), (4, 0), (4, 1),
                   (4, 8), (5, 0), (5, 9)]:
        args = list(ok)
        args[i] = bad
        assert lib.dm_lsm_affine_bytes(*args) == 0, args
    assert lib.dm_lsm_affine_bytes(24, 24, 65536, 32768, 2, 1) == 0
    for Hi, Wi, H, W in [(1, 1, 1, 1), (2 ** 30, 2 ** 30, 46341, 46340), (100, 100, 64 * 65535, 1)]:
        for r, iters in [(2, 1), (7, 8)]:
            assert lib.dm_lsm_affine_bytes(Hi, Wi, H, W, r, iters) > 0


def test_lsm_model_params():
    assert engine.lsm_model_params('shift') == ('shift', None)
    assert engine.lsm_model_params('affine') == ('affine', 0.5)
    got = engine.lsm_model_params(['affine', np.float32(0.25)])
    assert got == ('affine', 0.25) and type(got[1]) is float
    for bad in [None, 'Affine', 'projective', 1, ('affine',), ('shift', 0.5), ('affine', 0.0), ('affine', 1.0),
                ('affine', -0.1), ('affine', NAN), ('affine', None), ('affine', True), ('affine', '0.5'),
                ('affine', 0.5, 1)]:
        with pytest.raises(ValueError):
            engine.lsm_model_params(bad)


PMODES = ('elevation', 'elevation2')
LSM = (2, 3, 1.0)


def test_chain_layout_and_names():
    import torch
    c = chain_mod.Chain(PMODES, lsm=(3, 2), lsm_model='affine')
    assert c.lsm == (3, 2, 1.0) and c.lsm_model == ('affine', 0.5)
    assert c.names(None, None) == ['d_map', 'out_map', 'lsm_score', 'lsm_status', 'lsm_affine']
    assert c.layout(5, 7, None, None)[2:] == [('lsm_score', (5, 7), torch.float64), ('lsm_status', (5, 7), torch.int8),
                                              ('lsm_affine', (4, 5, 7), torch.float64)]
    c = chain_mod.Chain(PMODES, fill=4, refine=(2, 1), lsm=LSM, lsm_where='filled', lsm_model=('affine', 0.25),
                        photo=(2, 0.75))
    assert c.lsm_model == ('affine', 0.25)
    assert c.names(1.0, 'feather') == ['d_map', 'out_map', 'err', 'spread', 'count', 'holes', 'refine_score',
                                       'refine_shift', 'lsm_score', 'lsm_status', 'lsm_affine', 'rejected', 'score']
    # 'shift', the default: the layouts of a call without the keyword, entry for entry
    for kw in (dict(), dict(lsm=(3, 2)), dict(fill=4, lsm=LSM, lsm_where='filled', photo=(2, 0.75))):
        c = chain_mod.Chain(PMODES, lsm_model='shift', **kw)
        assert c.lsm_model == ('shift', None)
        assert c.layout(3, 4, 1.0, None) == chain_mod.Chain(PMODES, **kw).layout(3, 4, 1.0, None)
        assert 'lsm_affine' not in c.names(None, None)
    # without lsm= the affine model adds nothing, but the keyword is validated all the same
    assert 'lsm_affine' not in chain_mod.Chain(PMODES, lsm_model='affine').names(None, None)
    for bad in ('projective', ('affine', 1.0), ('affine', 0.0), 3, None):
        with pytest.raises(ValueError):
            chain_mod.Chain(PMODES, lsm_model=bad)
        with pytest.raises(ValueError):
            chain_mod.Chain(PMODES, lsm=(3, 2), lsm_model=bad)
    with pytest.raises(ValueError):      # nine taps cannot carry eight unknowns
        chain_mod.Chain(PMODES, lsm=(1, 2), lsm_model='affine')
    assert chain_mod.Chain(PMODES, lsm=(1, 2), lsm_model='shift').lsm == (1, 2, 1.0)


def test_lsm_model_keyword():
    from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
    a, b = _pcase()
    kw = dict(image_size=[16, 16], stride=[12, 16], degree_map_mode=list(PMODES))
    s = ImageCutSolver(a, b, lsm=(2, 3), lsm_model='affine', **kw)
    assert s.lsm == LSM and s.lsm_model == ('affine', 0.5) and s.lsm_affine_map is None
    assert ImageCutSolver(a, b, lsm=(2, 3), lsm_model=('affine', 0.3), **kw).lsm_model == ('affine', 0.3)
    s = ImageCutSolver(a, b, lsm=(2, 3), **kw)
    assert s.lsm_model == ('shift', None) and s.lsm_affine_map is None
    assert ImageCutSolver(a, b, **kw).lsm_model == ('shift', None)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm_model='projective', **kw)
    with pytest.raises(ValueError):
        ImageCutSolver(a, b, lsm=(1, 3), lsm_model='affine', **kw)
    with pytest.raises(ValueError):
        _sharded(a, b, lsm_model=('affine', 2.0))
    with pytest.raises(ValueError):
        _sharded(a, b, lsm=(1, 3), lsm_model='affine', lsmer=_host_lsm_affine)


# ---------------------------------------------------------------------------------------------
# 4. the sharded path: oracle tile solver, host stitcher, the restatement as lsmer
# ---------------------------------------------------------------------------------------------
def _host_lsm_affine(img1, img2, d_row, d_col, radius, iters, offset, max_move, max_shear, mask):
    """lsmer hook of solve_image_sharded under the affine model: the affine planes are the fifth value."""
    return lsm_affine_fast(np.asarray(img1), np.asarray(img2), np.asarray(d_row), np.asarray(d_col), radius, iters,
                           offset, max_move, max_shear, None if mask is None else np.asarray(mask))


def _host_lsm(img1, img2, d_row, d_col, radius, iters, offset, max_move, mask):
    """lsmer hook under the shift model: today's contract."""
    return lsm_fast(np.asarray(img1), np.asarray(img2), np.asarray(d_row), np.asarray(d_col), radius, iters, offset,
                    max_move, None if mask is None else np.asarray(mask))


def _sharded(a, b, modes=PMODES, **kw):
    return shard.solve_image_sharded(a, b, GEOM['image_size'], GEOM['stride'], GEOM['ws'], 5, modes,
                                     solver=_oracle_tiles, stitcher=_host_stitch, **kw)


@pytest.fixture(scope='module')
def plain():
    """(d_map, out_map): today's call."""
    a, b = _pcase()
    return [np.asarray(x) for x in _sharded(a, b)]


def test_sharded_lsm_affine(plain):
    a, b = _pcase()
    got = _sharded(a, b, lsm=LSM, lsm_model=('affine', 0.4), lsmer=_host_lsm_affine)
    assert len(got) == 5
    want = lsm_affine_restate(a, b, plain[0][1], plain[0][0], LSM[0], LSM[1], 2, LSM[2], 0.4)
    assert same_bits(got[0], np.stack([want[1], want[0]])) and same_bits(got[1], plain[1])
    assert raw_bits(np.asarray(got[2]), want[2])
    assert np.asarray(got[3]).dtype == np.int8 and np.array_equal(np.asarray(got[3]), want[3])
    assert np.asarray(got[4]).shape == (4,) + want[2].shape and raw_bits(np.asarray(got[4]), want[4])
    assert (want[3] == LSM[1]).any()


def test_sharded_shift_model_is_todays_call(plain):
    """lsm_model='shift' against a call that omits the keyword, bit for bit; and without lsm= nothing changes."""
    a, b = _pcase()
    ref = _sharded(a, b, lsm=LSM, lsmer=_host_lsm)
    got = _sharded(a, b, lsm=LSM, lsm_model='shift', lsmer=_host_lsm)
    assert len(got) == len(ref) == 4
    assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]) and raw_bits(np.asarray(got[2]), np.asarray(ref[2]))
    assert np.array_equal(np.asarray(got[3]), np.asarray(ref[3]))
    got = _sharded(a, b, lsm=None, lsm_model='affine', lsmer=_host_lsm_affine)
    assert len(got) == 2 and all(same_bits(g, r) for g, r in zip(got, plain))
