"""A/B of engine.photo_refine (dm_photo_refine.hip) against the same definition built from PyTorch
tensor ops on the same device, and against the only way the library had before to get the
candidates: (2 s + 1)^2 engine.photo_score calls on shifted planes with a running maximum.

The PyTorch chain scores every candidate as tools/photo_ab.py scores the centre -- the (2 r + 2)^2
pixels of the candidate's img2 patch gathered by integer index, the img1 window as shifted slices,
the twenty integer sums tap by tap in int32, the products with n in int64, the float64 tail in the
header's order -- then takes the winner in the header's order of preference, the min_gain rule and
the parabola per axis; in bands of rows, so that a band's gathered patch stays near 1 GiB.  Maps of
1024^2 and 4096^2 cells (`--sides`), (radius, search) in (1,1), (2,2), (3,2), (3,3) (`--cases`).
The pair is synthetic.stereo_pair(sinusoidal=True, max_disp=8); d_col is its integer truth plus
uniform sub-pixel noise in (-0.25, 0.25), with 30 % of the cells moved by an integer in [-s, s] in
each plane; d_row that noise and those moves alone; the image has a margin of 21 pixels round the
map, so every candidate of every cell is scored (checked).

The chain's output must first agree with the kernel's: the same NaN positions of the score, equal
shifts, both planes within 1e-12 (`agrees`; the run stops otherwise).  That the kernel equals the
definition bit for bit is what tests/test_refine_gpu.py shows, not this tool.  The photo_score loop
is timed only: a shifted plane rounds differently from the shifted window, so it is not the same
definition, and it gives no sub-pixel step.

The three are alternated (`reps` windows of about 0.15 s each, at least one call, device events
around every window) after a warm-up.  Prints one JSON line per case; `--out FILE` writes the list.

    python tools/refine_ab.py [--sides 1024,4096] [--cases 1:1,2:2,3:2,3:3] [--out profiles/refine_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

BAND_BYTES = 1 << 30      # int32 pixels of one band's gathered patch
MARGIN = 21               # radius 7 + search 3 + the largest disparity 8 + 3.25 + the bilinear neighbour, rounded up
PAIRS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
SHIFT = [(0, 0), (0, 1), (1, 0), (1, 1)]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_candidate(a32, bflat, Wi, base, w, y0, y1, W, r, off):
    """dm_photo_score's rules 4 and 5 for the img2 windows at `base` (flat index of the top-left pixel)."""
    D = 2 * r + 1
    n = D * D
    patch = [[bflat[base + (u * Wi + v)] for v in range(D + 1)] for u in range(D + 1)]
    z = torch.zeros_like(patch[0][0])
    sa, saa = z.clone(), z.clone()
    S = [z.clone() for _ in range(4)]
    AP = [z.clone() for _ in range(4)]
    PP = {kl: z.clone() for kl in PAIRS}
    for u in range(D):
        for v in range(D):
            a = a32[y0 + off - r + u:y1 + off - r + u, off - r + v:off - r + v + W]
            p = [patch[u + sy][v + sx] for sy, sx in SHIFT]
            sa += a
            saa += a * a
            for k in range(4):
                S[k] += p[k]
                AP[k] += a * p[k]
            for k, l in PAIRS:
                PP[k, l] += p[k] * p[l]
    del patch
    sa, saa = sa.long(), saa.long()
    S = [s.long() for s in S]
    VA = (n * saa - sa * sa).double()
    CA = [(n * AP[k].long() - sa * S[k]).double() for k in range(4)]
    num = ((w[0] * CA[0] + w[1] * CA[1]) + w[2] * CA[2]) + w[3] * CA[3]
    vb = None
    for k, l in PAIRS:
        t = ((1.0 if k == l else 2.0) * (w[k] * w[l])) * (n * PP[k, l].long() - S[k] * S[l]).double()
        vb = t if vb is None else vb + t
    pos = (VA > 0) & (vb > 0)
    t = (num / torch.sqrt(torch.where(pos, VA * vb, torch.ones_like(vb)))).clamp_(-1.0, 1.0)
    return torch.where(pos, t, torch.zeros_like(t))


def t_peak(sm, s0, sp, on):
    den = (sm + sp) - 2.0 * s0
    t = ((0.5 * (sm - sp)) / torch.where(den < 0, den, torch.ones_like(den))).clamp_(-0.5, 0.5)
    return torch.where(on & (den < 0), t, torch.zeros_like(t))


def t_refine(a32, b32, dr, dc, r, s, off, min_gain=0.0):
    """The definition, sub-pixel step included, for a map whose every img1 window lies inside the image (the margin
    sees to it) -> (out_row, out_col, score, int8 shift)."""
    Hi, Wi = a32.shape
    H, W = dr.shape
    D = 2 * r + 1
    NC = 2 * s + 1
    bflat = b32.reshape(-1)
    out_row, out_col, score = dr.clone(), dc.clone(), torch.full_like(dr, float('nan'))
    shift = torch.zeros((2, H, W), dtype=torch.int8, device=dr.device)
    rows = max(1, BAND_BYTES // (4 * (D + 1) * (D + 1) * W))
    xs = torch.arange(W, device=dr.device)
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        cy = (torch.arange(y0, y1, device=dr.device) + off)[:, None]
        cx = (xs + off)[None, :]
        py, px = cy.double() - dr[y0:y1], cx.double() - dc[y0:y1]
        live = (py >= -2.0 ** 30) & (py <= 2.0 ** 30) & (px >= -2.0 ** 30) & (px <= 2.0 ** 30)      # (false for NaN, +-inf)
        py, px = torch.where(live, py, torch.full_like(py, r)), torch.where(live, px, torch.full_like(px, r))
        fly, flx = torch.floor(py), torch.floor(px)
        fy, fx = py - fly, px - flx
        gy, gx = 1.0 - fy, 1.0 - fx
        w = [gy * gx, gy * fx, fy * gx, fy * fx]
        iy, ix = fly.long(), flx.long()
        sc = torch.full((NC, NC) + tuple(py.shape), float('nan'), dtype=torch.float64, device=dr.device)
        best = torch.full_like(py, float('nan'))
        bdy, bdx, bd2 = torch.zeros_like(iy), torch.zeros_like(iy), torch.zeros_like(iy)
        found = torch.zeros_like(live)
        for dy in range(-s, s + 1):
            for dx in range(-s, s + 1):
                ok = live & (iy + dy >= r) & (iy + dy <= Hi - r - 2) & (ix + dx >= r) & (ix + dx <= Wi - r - 2)
                base = torch.where(ok, (iy + dy - r) * Wi + (ix + dx - r), torch.zeros_like(iy))
                v = torch.where(ok, t_candidate(a32, bflat, Wi, base, w, y0, y1, W, r, off), torch.full_like(py, float('nan')))
                sc[dy + s, dx + s] = v
                d2 = dy * dy + dx * dx
                take = ok & (~found | (v > best) | ((v == best) & (d2 < bd2)))
                best = torch.where(take, v, best)
                bdy, bdx = torch.where(take, torch.full_like(bdy, dy), bdy), torch.where(take, torch.full_like(bdx, dx), bdx)
                bd2 = torch.where(take, torch.full_like(bd2, d2), bd2)
                found |= take
        centre = sc[s, s]
        stay = found & ~torch.isnan(centre) & ~(best > centre + min_gain)
        best = torch.where(stay, centre, best)
        bdy, bdx = torch.where(stay, torch.zeros_like(bdy), bdy), torch.where(stay, torch.zeros_like(bdx), bdx)
        moved = found & ((bdy != 0) | (bdx != 0))
        flat = sc.reshape(NC * NC, -1)
        nan = torch.full_like(py, float('nan'))

        def at(ddy, ddx):
            inside = (ddy.abs() <= s) & (ddx.abs() <= s)
            k = (ddy.clamp(-s, s) + s) * NC + (ddx.clamp(-s, s) + s)
            return torch.where(inside, flat.gather(0, k.reshape(1, -1)).reshape(py.shape), nan)

        sm, sp = at(bdy - 1, bdx), at(bdy + 1, bdx)
        ty = t_peak(sm, best, sp, moved & ~torch.isnan(sm) & ~torch.isnan(sp))
        sm, sp = at(bdy, bdx - 1), at(bdy, bdx + 1)
        tx = t_peak(sm, best, sp, moved & ~torch.isnan(sm) & ~torch.isnan(sp))
        out_row[y0:y1] = torch.where(moved, dr[y0:y1] - (bdy.double() + ty), dr[y0:y1])
        out_col[y0:y1] = torch.where(moved, dc[y0:y1] - (bdx.double() + tx), dc[y0:y1])
        score[y0:y1] = torch.where(found, best, nan)
        shift[0, y0:y1] = torch.where(moved, bdy, torch.zeros_like(bdy)).to(torch.int8)
        shift[1, y0:y1] = torch.where(moved, bdx, torch.zeros_like(bdx)).to(torch.int8)
        del sc, flat
    return out_row, out_col, score, shift


def score_loop(ta, tb, dr, dc, r, s, off):
    """(2 s + 1)^2 engine.photo_score calls on shifted planes, the best score and its index kept."""
    best = idx = None
    k = 0
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            v = engine.photo_score(ta, tb, dr - float(dy), dc - float(dx), r, offset=off)
            if best is None:
                best, idx = v, torch.zeros(v.shape, dtype=torch.int8, device=v.device)
            else:
                take = v > best
                best, idx = torch.where(take, v, best), torch.where(take, torch.full_like(idx, k), idx)
            k += 1
    return best, idx


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


def make(side, s):
    """(img1, img2, d_row, d_col): the sinusoidal pair, its integer truth plus sub-pixel noise and integer moves."""
    h = w = side + 2 * MARGIN
    a, b = stereo_pair(h, w, seed=side, max_disp=8, sinusoidal=True)
    yy, xx = np.mgrid[MARGIN:MARGIN + side, MARGIN:MARGIN + side]
    truth = np.rint(0.5 * 8 * (1.0 + np.sin(2 * np.pi * xx / w) * np.cos(2 * np.pi * yy / h)))
    rng = np.random.default_rng(side + 1)
    hit = rng.uniform(size=(2, side, side)) < 0.3
    move = np.where(hit, rng.integers(-s, s + 1, (2, side, side)), 0)
    return a, b, rng.uniform(-0.25, 0.25, (side, side)) + move[0], truth + rng.uniform(-0.25, 0.25, (side, side)) + move[1]


if __name__ == '__main__':
    sides = [int(v) for v in arg('--sides', '1024,4096').split(',')]
    cases = [tuple(int(v) for v in c.split(':')) for c in arg('--cases', '1:1,2:2,3:2,3:3').split(',')]
    reps = int(arg('--reps', '7'))
    out = []
    for side in sides:
        for r, s in cases:
            a, b, dr_, dc_ = make(side, s)
            ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            a32, b32 = ta.int(), tb.int()
            dr, dc = torch.from_numpy(dr_).cuda(), torch.from_numpy(dc_).cuda()
            variants = dict(torch_chain=lambda: t_refine(a32, b32, dr, dc, r, s, MARGIN),
                            photo_score_loop=lambda: score_loop(ta, tb, dr, dc, r, s, MARGIN),
                            hip=lambda: engine.photo_refine(ta, tb, dr, dc, r, s, offset=MARGIN, return_score=True,
                                                            return_shift=True))
            ref = variants['hip']()
            chain = variants['torch_chain']()
            scored = int((~torch.isnan(ref[2])).sum())
            nan_equal = bool(torch.equal(torch.isnan(ref[2]), torch.isnan(chain[2])))
            shifts_equal = bool(torch.equal(ref[3], chain[3]))
            diff = max(float((ref[k] - chain[k]).abs().max()) for k in (0, 1))
            agrees = bool(nan_equal and shifts_equal and diff <= 1e-12 and scored == side * side)
            bit_equal = all(bool(torch.equal(ref[k].view(torch.int64), chain[k].view(torch.int64))) for k in (0, 1, 2))
            again = variants['hip']()
            run_to_run = all(bool(torch.equal(p.view(torch.int8), q.view(torch.int8))) for p, q in zip(ref, again))
            moved = float((ref[3] != 0).any(dim=0).double().mean())
            mean_score = float(ref[2].mean())
            del ref, chain, again
            if not agrees:
                raise SystemExit('side %d radius %d search %d: the chain and the kernel disagree (nan_equal %s, shifts_equal '
                                 '%s, max diff %g, %d scored)' % (side, r, s, nan_equal, shifts_equal, diff, scored))
            variants['photo_score_loop']()
            # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            ms = {k: stat(t) for k, t in times.items()}
            res = dict(side=side, radius=r, search=s,
                       shape='%d^2 cells, uint8 pair of %d^2, sinusoidal truth in [0, 8] + U(-0.25, 0.25), 30 %% of the cells '
                             'moved by an integer in [-%d, %d] per plane; radius %d, search %d, sub-pixel step, score and '
                             'shift' % (side, side + 2 * MARGIN, s, s, r, s),
                       scored_cells=scored, moved_share=moved, mean_score=mean_score,
                       check=dict(nan_positions_equal=nan_equal, shifts_equal=shifts_equal, max_abs_diff=diff,
                                  bit_identical=bit_equal, agrees=agrees),
                       hip_run_to_run_identical=run_to_run, inner=inner, reps=reps, ms=ms,
                       speedup_over_torch_chain=ms['torch_chain']['median'] / ms['hip']['median'],
                       speedup_over_photo_score_loop=ms['photo_score_loop']['median'] / ms['hip']['median'],
                       hip_beats_torch_chain=bool(ms['torch_chain']['median'] > ms['hip']['median']),
                       candidate_taps_per_s=side * side * (2 * s + 1) ** 2 * (2 * r + 1) ** 2 / (ms['hip']['median'] * 1e-3),
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            del variants, ta, tb, a32, b32, dr, dc
            torch.cuda.empty_cache()
    if '--out' in sys.argv:
        with open(arg('--out', None), 'w') as fh:
            json.dump(out, fh, indent=1)
