"""A/B of engine.lsm_affine (dm_lsm_affine.hip) against the shift-only engine.lsm_refine at the same
(radius, iters), and against the same definition built from PyTorch tensor ops on the same device.

The PyTorch chain follows include/dmstereo_lsm.h rule by rule: the img1 window and its halo as
shifted slices, the six regressors per tap, the moments in int64, the L D L^T factorisation and the
solve unrolled over tensors, the four img2 pixels of every tap gathered by integer index under the
current warp of every cell, the float64 sums tap by tap in raster order, one tensor op per
operation; in bands of rows.  The start score s0 is engine.photo_score (dm_photo_score's bits by
definition).  Maps of 1024^2 and 4096^2 cells (`--sides`), (radius, iters) in (3,4), (5,4), (5,6),
(7,6) (`--cases`).  The pair is synthetic.ramp_pair of slope `--slope` (0.1) at up = 4, 1024 + 2 * 16
pixels a side, tiled for the larger map (the seams and the two ends of the ramp, where the match
leaves the image, cost some cells their acceptance, nothing else); the start is the truth plus
uniform noise of +-0.6 px per axis.

The chain's output must first agree with the kernel's: equal status planes, the same NaN positions,
planes, score and affine values within 1e-9 (`agrees`; the run stops otherwise); `bit_identical`
says whether the 64-bit patterns are equal too.  That the kernel equals the definition bit for bit
is what tests/test_lsm_affine_gpu.py shows, not this tool.

The three are alternated (`reps` windows of about 0.15 s each, at least one call, device events
around every window) after a warm-up.  Prints one JSON line per case; `--out FILE` writes the list.

    python tools/lsm_affine_bench.py [--sides 1024,4096] [--cases 3:4,5:4,5:6,7:6] [--reps 5] [--out FILE]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import ramp_pair

BAND_CELLS = 1 << 22      # cells of one band of the chain
MARGIN = 16               # radius 7 + halo 1 + noise 0.6 + max_move 1 + the shear of the corner taps, rounded up
BASE = 1024               # cells a side of the generated pair; larger maps tile it


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_zncc(VA, num, vb):
    pos = (VA > 0) & (vb > 0)
    t = (num / torch.sqrt(torch.where(pos, VA * vb, torch.ones_like(vb)))).clamp_(-1.0, 1.0)
    return torch.where(pos, t, torch.zeros_like(t))


def t_warp_ok(p, r, Hi, Wi):
    a1, d1 = 1.0 + p[1], 1.0 + p[5]
    ok = torch.ones_like(p[0], dtype=torch.bool)
    for u, v in ((-r, -r), (r, -r), (-r, r), (r, r)):
        X, Y = p[0] + (a1 * float(u) + p[2] * float(v)), p[3] + (p[4] * float(u) + d1 * float(v))
        ok &= (Y >= 0.0) & (Y < float(Hi - 1)) & (X >= 0.0) & (X < float(Wi - 1))
    return ok


def t_sums(A, bflat, Wi, p, go, r, grad):
    """Rule 5's sums under the warps p of the cells `go` (the others sample pixel (0, 0): never used)."""
    a1, d1 = 1.0 + p[1], 1.0 + p[5]
    z = torch.zeros_like(p[0])
    Sp, Spp, Sap, T = z.clone(), z.clone(), z.clone(), [z.clone() for _ in range(6)]
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            X, Y = p[0] + (a1 * float(u) + p[2] * float(v)), p[3] + (p[4] * float(u) + d1 * float(v))
            X, Y = torch.where(go, X, z), torch.where(go, Y, z)
            flx, fly = torch.floor(X), torch.floor(Y)
            fx, fy = X - flx, Y - fly
            g_x, g_y = 1.0 - fx, 1.0 - fy
            base = fly.long() * Wi + flx.long()
            P = ((g_y * g_x * bflat[base] + g_y * fx * bflat[base + 1]) + fy * g_x * bflat[base + Wi]) + \
                fy * fx * bflat[base + Wi + 1]
            a = A(v, u)
            Sp = Sp + P
            Spp = Spp + P * P
            Sap = Sap + a * P
            if grad:
                gx, gy = A(v, u + 1) - A(v, u - 1), A(v + 1, u) - A(v - 1, u)
                for k, phi in enumerate((gx, gx * u, gx * v, gy, gy * u, gy * v)):
                    T[k] = T[k] + phi * P
    return Sp, Spp, Sap, T


def t_affine(a64, b64, ta, tb, dr, dc, r, iters, off, max_move=1.0, max_shear=0.5):
    """The definition for a finite map whose every img1 halo window lies inside the image (the margin sees to it)
    -> (out_row, out_col, score, int8 status, affine [4][H][W])."""
    Hi, Wi = a64.shape
    H, W = dr.shape
    n = (2 * r + 1) ** 2
    nn = float(n)
    bflat = b64.reshape(-1)
    nan = float('nan')
    out_row, out_col, score = dr.clone(), dc.clone(), torch.full_like(dr, nan)
    affine = torch.full((4, H, W), nan, dtype=torch.float64, device=dr.device)
    status = torch.zeros((H, W), dtype=torch.int8, device=dr.device)
    photo = engine.photo_score(ta, tb, dr, dc, r, offset=off)
    rows = max(1, BAND_CELLS // W)
    xs = torch.arange(W, device=dr.device)
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)

        def A(v, u):      # tap (u, v) of the img1 window of every cell of the band, as float64 (exact)
            return a64[y0 + off + v:y1 + off + v, off + u:off + u + W]

        zi = torch.zeros((y1 - y0, W), dtype=torch.int64, device=dr.device)
        sa, saa = zi.clone(), zi.clone()
        f, ra = [zi.clone() for _ in range(6)], [zi.clone() for _ in range(6)]
        M = [[zi.clone() for _ in range(k + 1)] for k in range(6)]
        for v in range(-r, r + 1):
            for u in range(-r, r + 1):
                a = A(v, u).long()
                gx, gy = (A(v, u + 1) - A(v, u - 1)).long(), (A(v + 1, u) - A(v - 1, u)).long()
                phi = (gx, gx * u, gx * v, gy, gy * u, gy * v)
                sa += a
                saa += a * a
                for k in range(6):
                    f[k] += phi[k]
                    ra[k] += phi[k] * a
                    for l in range(k + 1):
                        M[k][l] += phi[k] * phi[l]
        VA = (n * saa - sa * sa).double()
        N = [[(n * M[k][l] - f[k] * f[l]).double() for l in range(k + 1)] for k in range(6)]
        RA = [(n * ra[k] - f[k] * sa).double() for k in range(6)]
        fd, fsa = [q.double() for q in f], sa.double()
        del M, ra, f
        Lf = [[None] * 6 for _ in range(6)]
        c = [[None] * 6 for _ in range(6)]
        d = [None] * 6
        ok = torch.ones_like(VA, dtype=torch.bool)
        for j in range(6):
            for i in range(j, 6):
                q = N[i][j]
                for k in range(j):
                    q = q - Lf[i][k] * c[j][k]
                c[i][j] = q
            d[j] = c[j][j]
            ok &= d[j] > N[j][j] * 2.0 ** -20
            for i in range(j + 1, 6):
                Lf[i][j] = c[i][j] / d[j]
        del c, N
        cy = (torch.arange(y0, y1, device=dr.device) + off)[:, None].double()
        cx = (xs + off)[None, :].double()
        py0, px0 = cy - dr[y0:y1], cx - dc[y0:y1]
        inside = (py0 >= float(r)) & (py0 < float(Hi - r - 1)) & (px0 >= float(r)) & (px0 < float(Wi - r - 1))
        st = torch.where(ok, torch.where(inside, iters, -2), -1)
        scored = st == iters
        s0 = torch.where(scored, photo[y0:y1], torch.full_like(py0, nan))
        z = torch.zeros_like(py0)
        p = [px0.clone(), z.clone(), z.clone(), py0.clone(), z.clone(), z.clone()]
        st = torch.where(scored & ~t_warp_ok(p, r, Hi, Wi), torch.full_like(st, -2), st)
        go = st == iters
        for step in range(1, iters + 1):
            Sp, Spp, Sap, T = t_sums(A, bflat, Wi, p, go, r, True)
            num, vb = nn * Sap - fsa * Sp, nn * Spp - Sp * Sp
            pos = go & (vb > 0)
            alpha = num / torch.where(pos, vb, torch.ones_like(vb))
            zz = [None] * 6
            for i in range(6):
                q = RA[i] - alpha * (nn * T[i] - fd[i] * Sp)
                for k in range(i):
                    q = q - Lf[i][k] * zz[k]
                zz[i] = q
            for i in range(5, -1, -1):
                q = zz[i] / d[i]
                for k in range(i + 1, 6):
                    q = q - Lf[k][i] * zz[k]
                zz[i] = q
            new = [p[k] + 2.0 * zz[k] for k in range(6)]
            good = pos & ((new[0] - px0).abs() <= max_move) & ((new[3] - py0).abs() <= max_move)
            for k in (1, 2, 4, 5):
                good &= new[k].abs() <= max_shear
            good &= t_warp_ok(new, r, Hi, Wi)
            st = torch.where(go & ~pos, torch.full_like(st, -1), st)
            st = torch.where(pos & ~good, torch.full_like(st, -2), st)
            p = [torch.where(good, new[k], p[k]) for k in range(6)]
            go = good
        Sp, Spp, Sap, _ = t_sums(A, bflat, Wi, p, go, r, False)
        s1 = t_zncc(VA, nn * Sap - fsa * Sp, nn * Spp - Sp * Sp)
        acc = go & (s1 > s0)
        st = torch.where(go & ~acc, torch.full_like(st, -3), st)
        out_row[y0:y1] = torch.where(acc, cy - p[3], dr[y0:y1])
        out_col[y0:y1] = torch.where(acc, cx - p[0], dc[y0:y1])
        score[y0:y1] = torch.where(acc, s1, s0)
        for j, k in enumerate((1, 2, 4, 5)):
            affine[j, y0:y1] = torch.where(acc, p[k], torch.full_like(z, nan))
        status[y0:y1] = st.to(torch.int8)
    return out_row, out_col, score, status, affine


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


_BASE = {}


def make(side, slope):
    """(img1, img2, d_row, d_col, true row, true col): the tiled ramp pair, its truth plus uniform +-0.6 px."""
    if 'pair' not in _BASE:
        _BASE['pair'] = ramp_pair(BASE + 2 * MARGIN, BASE + 2 * MARGIN, 11, slope, up=4)
    h = side + 2 * MARGIN
    reps = -(-h // (BASE + 2 * MARGIN))
    a, b, d = (np.ascontiguousarray(np.tile(t, (reps, reps))[:h, :h]) for t in _BASE['pair'])
    tc = np.ascontiguousarray(d[MARGIN:MARGIN + side, MARGIN:MARGIN + side])
    tr = np.zeros_like(tc)
    rng = np.random.default_rng(side + 1)
    return a, b, tr + rng.uniform(-0.6, 0.6, tr.shape), tc + rng.uniform(-0.6, 0.6, tc.shape), tr, tc


def rms(row, col, tr, tc, sel):
    return float(torch.sqrt((((row - tr) ** 2 + (col - tc) ** 2)[sel]).mean()))


if __name__ == '__main__':
    sides = [int(v) for v in arg('--sides', '1024,4096').split(',')]
    cases = [tuple(int(v) for v in c.split(':')) for c in arg('--cases', '3:4,5:4,5:6,7:6').split(',')]
    reps = int(arg('--reps', '5'))
    slope = float(arg('--slope', '0.1'))
    out = []
    for side in sides:
        a, b, dr_, dc_, tr_, tc_ = make(side, slope)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        a64, b64 = ta.double(), tb.double()
        dr, dc, tr, tc = (torch.from_numpy(t).cuda() for t in (dr_, dc_, tr_, tc_))
        for r, iters in cases:
            every = dict(offset=MARGIN, return_score=True, return_status=True)
            variants = dict(torch_chain=lambda: t_affine(a64, b64, ta, tb, dr, dc, r, iters, MARGIN),
                            hip_shift=lambda: engine.lsm_refine(ta, tb, dr, dc, r, iters, **every),
                            hip=lambda: engine.lsm_affine(ta, tb, dr, dc, r, iters, return_affine=True, **every))
            ref = variants['hip']()
            chain = variants['torch_chain']()
            status_equal = bool(torch.equal(ref[3], chain[3]))
            nan_equal = all(bool(torch.equal(torch.isnan(ref[k]), torch.isnan(chain[k]))) for k in (2, 4))
            diff = max(float(torch.nan_to_num(ref[k] - chain[k]).abs().max()) for k in (0, 1, 2, 4))
            agrees = bool(status_equal and nan_equal and diff <= 1e-9)
            bit_equal = all(bool(torch.equal(ref[k].view(torch.int64), chain[k].view(torch.int64))) for k in (0, 1, 2, 4))
            again = variants['hip']()
            run_to_run = all(bool(torch.equal(p.view(torch.int8), q.view(torch.int8))) for p, q in zip(ref, again))
            shift = variants['hip_shift']()
            sel = (ref[3] != 0) & (ref[3] != -2)
            acc = ref[3] == iters
            res = dict(side=side, radius=r, iters=iters, slope=slope,
                       accepted_share=float(acc.double().mean()), shift_accepted_share=float((shift[3] == iters).double().mean()),
                       status_counts={str(k): int((ref[3] == k).sum()) for k in (-3, -2, -1, 0, iters)},
                       rms_before_px=rms(dr, dc, tr, tc, sel), rms_affine_px=rms(ref[0], ref[1], tr, tc, sel),
                       rms_shift_px=rms(shift[0], shift[1], tr, tc, sel),
                       median_a=float(ref[4][0][acc].median()), true_a=-slope / (1.0 + slope),
                       check=dict(status_equal=status_equal, nan_positions_equal=nan_equal, max_abs_diff=diff,
                                  bit_identical=bit_equal, agrees=agrees), hip_run_to_run_identical=run_to_run)
            del ref, chain, again, shift, sel, acc
            if not agrees:
                raise SystemExit('side %d radius %d iters %d: the chain and the kernel disagree (status_equal %s, nan_equal '
                                 '%s, max diff %g)' % (side, r, iters, status_equal, nan_equal, diff))
            # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            ms = {k: stat(t) for k, t in times.items()}
            samples = (iters + 1) * (2 * r + 1) ** 2
            res.update(shape='%d^2 cells, uint8 pair of %d^2 (ramp_pair slope %g, up 4, of %d^2, tiled), truth + U(-0.6, 0.6) '
                             'per axis; radius %d, %d steps, max_move 1.0, max_shear 0.5, score, status and affine'
                             % (side, side + 2 * MARGIN, slope, BASE + 2 * MARGIN, r, iters),
                       inner=inner, reps=reps, ms=ms, samples_per_cell=samples,
                       ratio_to_shift_kernel=ms['hip']['median'] / ms['hip_shift']['median'],
                       speedup_over_torch_chain=ms['torch_chain']['median'] / ms['hip']['median'],
                       hip_beats_torch_chain=bool(ms['torch_chain']['median'] > ms['hip']['median']),
                       samples_per_s=side * side * samples / (ms['hip']['median'] * 1e-3),
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            if '--out' in sys.argv:
                with open(arg('--out', None), 'w') as fh:
                    json.dump(out, fh, indent=1)
            del variants
        del ta, tb, a64, b64, dr, dc, tr, tc
        torch.cuda.empty_cache()
