"""A/B of engine.bilateral_filter (dm_bilateral.hip) against what a user could write without it:
the same definition (include/dmstereo.h, tests/test_bilateral_host.py) in PyTorch tensor ops on
the same device -- one shifted slice of the zero-padded planes per tap, torch.exp, masked sums.
Maps of 1024^2 and 4096^2 cells (`--sides`), radius 3 and 7 (`--radii`), three guides
(`--guides`): a uint8 image, the same image as float64 with noise, and the map itself.  The map
is two planes 4 px apart with N(0, 0.3) noise and 8 % NaN, the image 60 / 180 either side of the
step; sigma_color 10, sigma_space = the radius; one pass.

The torch chain uses another exp and another summation order than the kernel, so the two are
compared within an absolute 1e-9 on the finite cells, with the NaN positions equal (`close`);
that the kernel equals the definition bit for bit is what tests/test_bilateral_gpu.py shows,
not this tool.  The HIP path with DM_BILATERAL_TILE = 16 and 32 is compared with the path as
built (which picks the side itself) bit for bit.

The variants are alternated (`reps` windows of about 0.15 s each, at least one call, device
events around every window) after a warm-up.  The kernel's own time comes from one
torch.profiler run of 5 calls (null where the profiler gives no device times); taps_per_s is
cells * (2 r + 1)^2 over that time, or over the call's median where there is none.  Prints one
JSON line per case; `--out FILE` writes the list.

    python tools/bilateral_ab.py [--sides 1024,4096] [--radii 3,7] [--guides u8,f64,self] [--out profiles/bilateral_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F
from deepmatching_stereo_matching_amd import engine


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_bilateral(x, guide, r, sigma_color, sigma_space):
    """One pass of the definition without the fill flag."""
    H, W = x.shape
    dc, ds = engine.bilateral_den(sigma_color), engine.bilateral_den(sigma_space)
    g = x if guide is None else guide.double()
    ok = torch.isfinite(x) & torch.isfinite(g)
    zero = torch.zeros_like(x)
    g0 = torch.where(ok, g, zero)
    xp = F.pad(torch.where(ok, x, zero), (r, r, r, r))
    gp = F.pad(g0, (r, r, r, r))
    mp = F.pad(ok.double(), (r, r, r, r))
    num, den = torch.zeros_like(x), torch.zeros_like(x)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sl = (slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
            w = torch.exp(-(g0 - gp[sl]) ** 2 / dc) * (mp[sl] * float(np.exp(-(dy * dy + dx * dx) / ds)))
            num += w * xp[sl]
            den += w
    take = ok & (den > 0)
    return torch.where(take, num / torch.where(take, den, torch.ones_like(den)), x)


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def hip(x, g, p, tile):
    def run():
        if tile is None:
            os.environ.pop('DM_BILATERAL_TILE', None)
        else:
            os.environ['DM_BILATERAL_TILE'] = str(tile)
        return engine.bilateral_filter(x, p[0], p[1], p[2], guide=g)
    return run


def kernel_time(fn, calls=5):
    """Mean device time in ms of k_bilat over `calls` calls, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if 'k_bilat' in ev.key:
                total = getattr(ev, 'device_time_total', None)
                if total is None:
                    total = ev.cuda_time_total
                return dict(ms=total / 1e3 / ev.count, launches_per_call=ev.count / calls)
        return None
    except Exception as e:      # no device tracing on this build: say so, the A/B itself stands
        return dict(error=repr(e))


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def make(side, kind):
    rng = np.random.default_rng(side)
    j = np.arange(side)[None, :]
    i = np.arange(side)[:, None]
    step = j >= (29 * side) // 64
    x = 0.02 * i + 0.01 * j + np.where(step, 4.0, 0.0) + rng.normal(0, 0.3, (side, side))
    x[rng.uniform(size=x.shape) < 0.08] = np.nan
    img = np.clip(np.rint(np.where(step, 180.0, 60.0) + rng.normal(0, 2, (side, side))), 0, 255).astype(np.uint8)
    if kind == 'u8':
        return x, img
    if kind == 'f64':
        return x, img + rng.normal(0, 0.25, (side, side))
    return x, None


sides = [int(s) for s in arg('--sides', '1024,4096').split(',')]
radii = [int(s) for s in arg('--radii', '3,7').split(',')]
kinds = arg('--guides', 'u8,f64,self').split(',')
out = []
for side in sides:
    for kind in kinds:
        a, ga = make(side, kind)
        x = torch.from_numpy(a).cuda()
        g = torch.from_numpy(ga).cuda() if ga is not None else None
        for r in radii:
            p = (r, 10.0, float(r))
            variants = dict(torch_chain=lambda: t_bilateral(x, g, *p), hip=hip(x, g, p, None),
                            hip_tile_16=hip(x, g, p, 16), hip_tile_32=hip(x, g, p, 32))
            ref = variants['hip']()
            chain = variants['torch_chain']()
            fin = torch.isfinite(ref)
            nan_equal = bool(torch.equal(torch.isnan(ref), torch.isnan(chain)) and
                             torch.equal(torch.isnan(ref), torch.isnan(x)))
            max_abs = float((ref[fin] - chain[fin]).abs().max())
            tile_same = {k: bool(torch.equal(variants[k]().view(torch.int64), ref.view(torch.int64)))
                         for k in ('hip_tile_16', 'hip_tile_32')}
            run_to_run = bool(torch.equal(variants['hip']().view(torch.int64), ref.view(torch.int64)))
            cells = int(fin.sum())
            del ref, chain, fin
            reps = 9
            for fn in variants.values():
                fn()
            # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            os.environ.pop('DM_BILATERAL_TILE', None)
            kern = kernel_time(variants['hip'])
            ms = {k: stat(t) for k, t in times.items()}
            kms = kern['ms'] if kern and 'ms' in kern else ms['hip']['median']
            res = dict(guide=kind, side=side, radius=r,
                       shape='%d^2 float64, two planes + N(0, 0.3), 8 %% NaN; (radius, sigma_color, sigma_space) = '
                             '(%d, %g, %g), 1 pass' % (side, p[0], p[1], p[2]),
                       smoothed_cells=cells, close=dict(tolerance=1e-9, max_abs_diff=max_abs, nan_positions_equal=nan_equal,
                                                        within=bool(nan_equal and max_abs <= 1e-9)),
                       hip_tiles_bit_identical=tile_same, hip_run_to_run_identical=run_to_run, inner=inner, reps=reps,
                       ms=ms, speedup_median=ms['torch_chain']['median'] / ms['hip']['median'], hip_kernel=kern,
                       taps_per_s=side * side * (2 * r + 1) ** 2 / (kms * 1e-3),
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            del variants
        del x, g
        torch.cuda.empty_cache()
if '--out' in sys.argv:
    with open(arg('--out', None), 'w') as fh:
        json.dump(out, fh, indent=1)
