"""A/B of engine.photo_score (dm_photo.hip) against the same definition built from PyTorch tensor
ops on the same device: the (2 r + 2)^2 pixels of a cell's img2 patch gathered by integer index
(no grid_sample), the img1 window as shifted slices, the twenty integer sums accumulated tap by
tap in int32, the products with n in int64 and the float64 tail in the header's order -- in bands
of rows, so that a band's gathered patch stays near 1 GiB.  Maps of 1024^2 and 4096^2 cells
(`--sides`), radius 1, 2, 3 and 7 (`--radii`).  The pair is synthetic.stereo_pair(sinusoidal=True,
max_disp=8); d_col is its integer truth plus uniform sub-pixel noise in (-0.5, 0.5), d_row that
noise alone; the image has a margin of 17 pixels round the map, so every cell is scored (checked).

The chain's output must first agree with the kernel's: the same NaN positions and a largest
difference of at most 1e-12 (`agrees`; the run stops otherwise).  That the kernel equals the
definition bit for bit is what tests/test_photo_gpu.py shows, not this tool.

The two are alternated (`reps` windows of about 0.15 s each, at least one call, device events
around every window) after a warm-up.  The kernel's own time comes from one torch.profiler run of
5 calls (null where the profiler gives no device times); taps_per_s is cells * (2 r + 1)^2 over
that time, or over the call's median where there is none.  Prints one JSON line per case; `--out
FILE` writes the list.

    python tools/photo_ab.py [--sides 1024,4096] [--radii 1,2,3,7] [--out profiles/photo_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

BAND_BYTES = 1 << 30      # int32 pixels of one band's gathered patch
MARGIN = 17               # radius 7 + the largest disparity 8.5 + the bilinear neighbour, rounded up
PAIRS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
SHIFT = [(0, 0), (0, 1), (1, 0), (1, 1)]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_photo(a32, b32, dr, dc, r, off):
    """The definition for a map whose every img1 window lies inside the image (the margin sees to it)."""
    Hi, Wi = a32.shape
    H, W = dr.shape
    D = 2 * r + 1
    n = D * D
    bflat = b32.reshape(-1)
    out = torch.empty_like(dr)
    rows = max(1, BAND_BYTES // (4 * (D + 1) * (D + 1) * W))
    xs = torch.arange(W, device=dr.device)
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        cy = (torch.arange(y0, y1, device=dr.device) + off)[:, None]
        cx = (xs + off)[None, :]
        py, px = cy.double() - dr[y0:y1], cx.double() - dc[y0:y1]
        ok = (py >= r) & (py < Hi - r - 1) & (px >= r) & (px < Wi - r - 1)      # (false for NaN and +-inf)
        py, px = torch.where(ok, py, torch.full_like(py, r)), torch.where(ok, px, torch.full_like(px, r))
        fly, flx = torch.floor(py), torch.floor(px)
        fy, fx = py - fly, px - flx
        gy, gx = 1.0 - fy, 1.0 - fx
        w = [gy * gx, gy * fx, fy * gx, fy * fx]
        base = (fly.long() - r) * Wi + (flx.long() - r)
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
        s = torch.where(pos, t, torch.zeros_like(t))
        out[y0:y1] = torch.where(ok, s, torch.full_like(s, float('nan')))
    return out


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def kernel_time(fn, calls=5):
    """Mean device time in ms of k_photo over `calls` calls, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if 'k_photo' in ev.key:
                total = getattr(ev, 'device_time_total', None)
                if total is None:
                    total = ev.cuda_time_total
                return dict(ms=total / 1e3 / ev.count, launches_per_call=ev.count / calls)
        return None
    except Exception as e:      # no device tracing on this build: say so, the A/B itself stands
        return dict(error=repr(e))


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def make(side):
    """(img1, img2, d_row, d_col): the sinusoidal pair, its integer truth plus sub-pixel noise."""
    h = w = side + 2 * MARGIN
    a, b = stereo_pair(h, w, seed=side, max_disp=8, sinusoidal=True)
    yy, xx = np.mgrid[MARGIN:MARGIN + side, MARGIN:MARGIN + side]
    truth = np.rint(0.5 * 8 * (1.0 + np.sin(2 * np.pi * xx / w) * np.cos(2 * np.pi * yy / h)))
    rng = np.random.default_rng(side + 1)
    return a, b, rng.uniform(-0.5, 0.5, (side, side)), truth + rng.uniform(-0.5, 0.5, (side, side))


sides = [int(s) for s in arg('--sides', '1024,4096').split(',')]
radii = [int(s) for s in arg('--radii', '1,2,3,7').split(',')]
reps = int(arg('--reps', '9'))
out = []
for side in sides:
    a, b, dr_, dc_ = make(side)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    a32, b32 = ta.int(), tb.int()
    dr, dc = torch.from_numpy(dr_).cuda(), torch.from_numpy(dc_).cuda()
    for r in radii:
        variants = dict(torch_chain=lambda: t_photo(a32, b32, dr, dc, r, MARGIN),
                        hip=lambda: engine.photo_score(ta, tb, dr, dc, r, offset=MARGIN))
        ref = variants['hip']()
        chain = variants['torch_chain']()
        scored = int((~torch.isnan(ref)).sum())
        nan_equal = bool(torch.equal(torch.isnan(ref), torch.isnan(chain)))
        fin = ~torch.isnan(ref) & ~torch.isnan(chain)
        diff = float((ref[fin] - chain[fin]).abs().max())
        agrees = bool(nan_equal and diff <= 1e-12 and scored == side * side)
        bit_equal = bool(torch.equal(ref.view(torch.int64), chain.view(torch.int64)))
        run_to_run = bool(torch.equal(variants['hip']().view(torch.int64), ref.view(torch.int64)))
        mean_score = float(ref[fin].mean())
        del ref, chain, fin
        if not agrees:
            raise SystemExit('side %d radius %d: the chain and the kernel disagree (nan_equal %s, max diff %g, %d scored)'
                             % (side, r, nan_equal, diff, scored))
        for fn in variants.values():
            fn()
        # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
        inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, inner[k]))
        kern = kernel_time(variants['hip'])
        ms = {k: stat(t) for k, t in times.items()}
        kms = kern['ms'] if kern and 'ms' in kern else ms['hip']['median']
        speedup = ms['torch_chain']['median'] / ms['hip']['median']
        res = dict(side=side, radius=r,
                   shape='%d^2 cells, uint8 pair of %d^2, sinusoidal truth in [0, 8] + U(-0.5, 0.5) in both planes; '
                         'radius %d, score only' % (side, side + 2 * MARGIN, r),
                   scored_cells=scored, mean_score=mean_score,
                   check=dict(nan_positions_equal=nan_equal, max_abs_diff=diff, bit_identical=bit_equal, agrees=agrees),
                   hip_run_to_run_identical=run_to_run, inner=inner, reps=reps, ms=ms, speedup_median=speedup,
                   hip_beats_torch_chain=bool(speedup > 1.0), hip_kernel=kern,
                   taps_per_s=side * side * (2 * r + 1) ** 2 / (kms * 1e-3), device=torch.cuda.get_device_name(0))
        out.append(res)
        print(json.dumps(res), flush=True)
        del variants
        torch.cuda.empty_cache()
    del ta, tb, a32, b32, dr, dc
    torch.cuda.empty_cache()
if '--out' in sys.argv:
    with open(arg('--out', None), 'w') as fh:
        json.dump(out, fh, indent=1)
