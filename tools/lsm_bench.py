"""A/B of engine.lsm_refine (dm_lsm.hip) against the same definition built from PyTorch tensor ops on
the same device, and against the floor its walk count predicts: iters + 1 engine.photo_score calls
at the same radius (a cell makes one walk over its img2 patch per step and one for the final score).

The PyTorch chain follows include/dmstereo.h rule by rule: the img1 window and its halo as shifted
slices, the (2 r + 2)^2 pixels of the img2 patch gathered by integer index at the current position
of every cell, the integer sums tap by tap in int32 (the four windows P0..P3 of a tap as one stacked
tensor), the products with n in int64, the float64 tail in the header's order, one tensor op per
operation; in bands of rows, so that a band's gathered patch stays near 1 GiB.  Maps of 1024^2 and
4096^2 cells (`--sides`), (radius, iters) in (2,2), (3,2), (3,4), (5,4) (`--cases`).  The pair is
synthetic.subpixel_pair at the phase (1, 2) / 4 -- a true disparity of (0.25, 0.5) px -- of
1024 + 2 * 12 pixels a side, tiled for the larger map (the seams cost a few cells their acceptance,
nothing else); the start is the truth plus uniform noise of +-0.6 px per axis.  The margin of 12
pixels keeps every window, halo and step inside the image.

The chain's output must first agree with the kernel's: equal status planes, the same NaN positions
of the score, both planes and the score within 1e-12 (`agrees`; the run stops otherwise);
`bit_identical` says whether the 64-bit patterns of the planes and the score are equal too.  That
the kernel equals the definition bit for bit is what tests/test_lsm_gpu.py shows, not this tool.

The three are alternated (`reps` windows of about 0.15 s each, at least one call, device events
around every window) after a warm-up.  Prints one JSON line per case; `--out FILE` writes the list.

    python tools/lsm_bench.py [--sides 1024,4096] [--cases 2:2,3:2,3:4,5:4] [--out profiles/lsm_bench.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import subpixel_pair

BAND_BYTES = 1 << 30      # int32 pixels of one band's gathered patch
MARGIN = 12               # radius 5 + halo 1 + truth 0.5 + noise 0.6 + max_move 1 + the bilinear neighbour, rounded up
BASE = 1024               # cells a side of the generated pair; larger maps tile it
KI = [0, 0, 0, 0, 1, 1, 1, 2, 2, 3]      # the pairs k <= l, k outer
LI = [0, 1, 2, 3, 1, 2, 3, 2, 3, 3]
SHIFT = [(0, 0), (0, 1), (1, 0), (1, 1)]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_sums(A, bflat, Wi, base, w, sa, gx, gy, r, grad):
    """Rules 4 and 5 of dm_photo_score for the img2 windows at `base` (flat index of the patch's top-left pixel),
    and GX_k, GY_k with `grad` -> (num, vb, gbx, gby)."""
    D = 2 * r + 1
    n = D * D
    patch = [[bflat[base + (u * Wi + v)] for v in range(D + 1)] for u in range(D + 1)]
    z4 = torch.zeros((4,) + tuple(base.shape), dtype=torch.int32, device=base.device)
    S, AP, XP, YP = z4.clone(), z4.clone(), z4.clone(), z4.clone()
    PP = torch.zeros((10,) + tuple(base.shape), dtype=torch.int32, device=base.device)
    for u in range(D):
        for v in range(D):
            P4 = torch.stack([patch[u + sy][v + sx] for sy, sx in SHIFT])
            S += P4
            AP += A(u, v) * P4
            if grad:
                XP += (A(u, v + 1) - A(u, v - 1)) * P4
                YP += (A(u + 1, v) - A(u - 1, v)) * P4
            PP += P4[KI] * P4[LI]
    del patch
    S = S.long()
    CA = (n * AP.long() - sa * S).double()
    CB = (n * PP.long() - S[KI] * S[LI]).double()
    num = ((w[0] * CA[0] + w[1] * CA[1]) + w[2] * CA[2]) + w[3] * CA[3]
    vb = None
    for i, (k, l) in enumerate(zip(KI, LI)):
        t = ((1.0 if k == l else 2.0) * (w[k] * w[l])) * CB[i]
        vb = t if vb is None else vb + t
    if not grad:
        return num, vb, None, None
    GX, GY = (n * XP.long() - gx * S).double(), (n * YP.long() - gy * S).double()
    gbx = ((w[0] * GX[0] + w[1] * GX[1]) + w[2] * GX[2]) + w[3] * GX[3]
    gby = ((w[0] * GY[0] + w[1] * GY[1]) + w[2] * GY[2]) + w[3] * GY[3]
    return num, vb, gbx, gby


def t_zncc(VA, num, vb):
    pos = (VA > 0) & (vb > 0)
    t = (num / torch.sqrt(torch.where(pos, VA * vb, torch.ones_like(vb)))).clamp_(-1.0, 1.0)
    return torch.where(pos, t, torch.zeros_like(t))


def t_lsm(a32, b32, dr, dc, r, iters, off, max_move=1.0):
    """The definition for a finite map whose every img1 halo window lies inside the image (the margin sees to it)
    -> (out_row, out_col, score, int8 status)."""
    Hi, Wi = a32.shape
    H, W = dr.shape
    D = 2 * r + 1
    n = D * D
    bflat = b32.reshape(-1)
    out_row, out_col, score = dr.clone(), dc.clone(), torch.full_like(dr, float('nan'))
    status = torch.zeros((H, W), dtype=torch.int8, device=dr.device)
    rows = max(1, BAND_BYTES // (4 * (D + 1) * (D + 1) * W))
    xs = torch.arange(W, device=dr.device)
    safe = float(r)      # a position that passes rule 3, for the cells that have stopped

    def inside(py, px):
        return (py >= float(r)) & (py < float(Hi - r - 1)) & (px >= float(r)) & (px < float(Wi - r - 1))

    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)

        def A(u, v):      # tap (u, v) of the img1 window of every cell of the band; -1 and D are the halo
            return a32[y0 + off - r + u:y1 + off - r + u, off - r + v:off - r + v + W]

        z = torch.zeros((y1 - y0, W), dtype=torch.int32, device=dr.device)
        sa, saa, gx, gy, gxx, gyy, gxy, gxa, gya = (z.clone() for _ in range(9))
        for u in range(D):
            for v in range(D):
                a, p, q = A(u, v), A(u, v + 1) - A(u, v - 1), A(u + 1, v) - A(u - 1, v)
                sa += a
                saa += a * a
                gx += p
                gy += q
                gxx += p * p
                gyy += q * q
                gxy += p * q
                gxa += p * a
                gya += q * a
        sa, gx, gy = sa.long(), gx.long(), gy.long()
        VA = (n * saa.long() - sa * sa).double()
        Hxx, Hyy, Hxy = (n * gxx.long() - gx * gx).double(), (n * gyy.long() - gy * gy).double(), \
            (n * gxy.long() - gx * gy).double()
        RAx, RAy = (n * gxa.long() - gx * sa).double(), (n * gya.long() - gy * sa).double()
        Dd = Hxx * Hyy - Hxy * Hxy
        cy = (torch.arange(y0, y1, device=dr.device) + off)[:, None].double()
        cx = (xs + off)[None, :].double()
        py0, px0 = cy - dr[y0:y1], cx - dc[y0:y1]
        st = torch.where(Dd > 0, torch.where(inside(py0, px0), iters, -2), -1)
        go = st == iters
        py, px = py0.clone(), px0.clone()
        s0 = torch.full_like(py, float('nan'))

        def sums(grad):
            qy, qx = torch.where(go, py, torch.full_like(py, safe)), torch.where(go, px, torch.full_like(px, safe))
            fly, flx = torch.floor(qy), torch.floor(qx)
            fy, fx = qy - fly, qx - flx
            g_y, g_x = 1.0 - fy, 1.0 - fx
            w = [g_y * g_x, g_y * fx, fy * g_x, fy * fx]
            base = (fly.long() - r) * Wi + (flx.long() - r)
            return t_sums(A, bflat, Wi, base, w, sa, gx, gy, r, grad)

        for step in range(1, iters + 1):
            num, vb, gbx, gby = sums(True)
            if step == 1:
                s0 = torch.where(go, t_zncc(VA, num, vb), s0)
            ok = go & (vb > 0)
            alpha = num / torch.where(ok, vb, torch.ones_like(vb))
            bx, by = RAx - alpha * gbx, RAy - alpha * gby
            one = torch.ones_like(Dd)
            ux = ((Hyy * bx) - (Hxy * by)) / torch.where(go, Dd, one)
            uy = ((Hxx * by) - (Hxy * bx)) / torch.where(go, Dd, one)
            qx, qy = px + 2.0 * ux, py + 2.0 * uy
            good = ok & ((qy - py0).abs() <= max_move) & ((qx - px0).abs() <= max_move) & inside(qy, qx)
            st = torch.where(go & ~ok, torch.full_like(st, -1), st)
            st = torch.where(ok & ~good, torch.full_like(st, -2), st)
            py, px = torch.where(good, qy, py), torch.where(good, qx, px)
            go = good
        num, vb, _, _ = sums(False)
        s1 = t_zncc(VA, num, vb)
        acc = go & (s1 > s0)
        st = torch.where(go & ~acc, torch.full_like(st, -3), st)
        out_row[y0:y1] = torch.where(acc, cy - py, dr[y0:y1])
        out_col[y0:y1] = torch.where(acc, cx - px, dc[y0:y1])
        score[y0:y1] = torch.where(acc, s1, s0)
        status[y0:y1] = st.to(torch.int8)
    return out_row, out_col, score, status


def score_floor(ta, tb, dr, dc, r, iters, off):
    """iters + 1 engine.photo_score calls: the walks of a cell, without the gradient sums."""
    for _ in range(iters + 1):
        v = engine.photo_score(ta, tb, dr, dc, r, offset=off)
    return v


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


def make(side):
    """(img1, img2, d_row, d_col, true row, true col): the tiled sub-pixel pair, its truth plus uniform +-0.6 px."""
    if 'pair' not in _BASE:
        _BASE['pair'] = subpixel_pair(BASE + 2 * MARGIN, BASE + 2 * MARGIN, 11, 1, 2)
    h = side + 2 * MARGIN
    reps = -(-h // (BASE + 2 * MARGIN))
    a, b = (np.ascontiguousarray(np.tile(t, (reps, reps))[:h, :h]) for t in _BASE['pair'])
    rng = np.random.default_rng(side + 1)
    return a, b, 0.25 + rng.uniform(-0.6, 0.6, (side, side)), 0.5 + rng.uniform(-0.6, 0.6, (side, side)), 0.25, 0.5


if __name__ == '__main__':
    sides = [int(v) for v in arg('--sides', '1024,4096').split(',')]
    cases = [tuple(int(v) for v in c.split(':')) for c in arg('--cases', '2:2,3:2,3:4,5:4').split(',')]
    reps = int(arg('--reps', '7'))
    out = []
    for side in sides:
        a, b, dr_, dc_, tr, tc = make(side)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        a32, b32 = ta.int(), tb.int()
        dr, dc = torch.from_numpy(dr_).cuda(), torch.from_numpy(dc_).cuda()
        for r, iters in cases:
            variants = dict(torch_chain=lambda: t_lsm(a32, b32, dr, dc, r, iters, MARGIN),
                            photo_score_floor=lambda: score_floor(ta, tb, dr, dc, r, iters, MARGIN),
                            hip=lambda: engine.lsm_refine(ta, tb, dr, dc, r, iters, offset=MARGIN, return_score=True,
                                                          return_status=True))
            ref = variants['hip']()
            chain = variants['torch_chain']()
            status_equal = bool(torch.equal(ref[3], chain[3]))
            nan_equal = bool(torch.equal(torch.isnan(ref[2]), torch.isnan(chain[2])))
            diff = max(float(torch.nan_to_num(ref[k] - chain[k]).abs().max()) for k in (0, 1, 2))
            agrees = bool(status_equal and nan_equal and diff <= 1e-12)
            bit_equal = all(bool(torch.equal(ref[k].view(torch.int64), chain[k].view(torch.int64))) for k in (0, 1, 2))
            again = variants['hip']()
            run_to_run = all(bool(torch.equal(p.view(torch.int8), q.view(torch.int8))) for p, q in zip(ref, again))
            accepted = float((ref[3] == iters).double().mean())
            rms_before = float(torch.sqrt(((dr - tr) ** 2 + (dc - tc) ** 2).mean()))
            rms_after = float(torch.sqrt(((ref[0] - tr) ** 2 + (ref[1] - tc) ** 2).mean()))
            counts = {str(k): int((ref[3] == k).sum()) for k in (-3, -2, -1, 0, iters)}
            del ref, chain, again
            if not agrees:
                raise SystemExit('side %d radius %d iters %d: the chain and the kernel disagree (status_equal %s, nan_equal '
                                 '%s, max diff %g)' % (side, r, iters, status_equal, nan_equal, diff))
            variants['photo_score_floor']()
            # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            ms = {k: stat(t) for k, t in times.items()}
            res = dict(side=side, radius=r, iters=iters,
                       shape='%d^2 cells, uint8 pair of %d^2 (subpixel_pair phase (1, 2) / 4 of %d^2, tiled), truth '
                             '(0.25, 0.5) + U(-0.6, 0.6) per axis; radius %d, %d steps, max_move 1.0, score and status'
                             % (side, side + 2 * MARGIN, BASE + 2 * MARGIN, r, iters),
                       accepted_share=accepted, status_counts=counts, rms_before_px=rms_before, rms_after_px=rms_after,
                       check=dict(status_equal=status_equal, nan_positions_equal=nan_equal, max_abs_diff=diff,
                                  bit_identical=bit_equal, agrees=agrees),
                       hip_run_to_run_identical=run_to_run, inner=inner, reps=reps, ms=ms,
                       speedup_over_torch_chain=ms['torch_chain']['median'] / ms['hip']['median'],
                       ratio_to_photo_score_floor=ms['hip']['median'] / ms['photo_score_floor']['median'],
                       hip_beats_torch_chain=bool(ms['torch_chain']['median'] > ms['hip']['median']),
                       walk_taps_per_s=side * side * (iters + 1) * (2 * r + 1) ** 2 / (ms['hip']['median'] * 1e-3),
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            if '--out' in sys.argv:
                with open(arg('--out', None), 'w') as fh:
                    json.dump(out, fh, indent=1)
            del variants
        del ta, tb, a32, b32, dr, dc
        torch.cuda.empty_cache()
