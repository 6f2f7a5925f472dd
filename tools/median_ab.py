"""A/B of engine.median_filter (dm_median.hip) against what a user could write without it, in
PyTorch tensor ops on the same device:
  unweighted  the NaN-padded map unfolded into its (2 r + 1)^2 taps, then torch.nanmedian over the
              taps (it returns the lower median too)
  weighted    the taps sorted, the weights gathered into that order, torch.cumsum, the first
              value at which the cumulated weight reaches half the total
both in bands of rows, so that the unfolded taps of a band stay near 1 GiB.  Maps of 1024^2 and
4096^2 cells (`--sides`), radius 1, 3 and 7 (`--radii`), unweighted and weighted (`--forms`).
The map is two planes 4 px apart with N(0, 0.3) noise and 8 % NaN; the weights are uniform in
[0.05, 1), as a correlation score is; one pass, min_count 1, no fill.

The torch chain orders +-0 as equal and sums the weights in sorted order, not in window order,
so the two are compared only loosely: the NaN positions must be equal, and the values equal on
this map, which has no ties and no signed zeros (`loose`: the count of differing cells is
reported; a weighted cell whose half-total falls within a rounding of a partial sum may differ).
That the kernel equals the definition bit for bit is what tests/test_median_gpu.py shows, not
this tool.  The HIP path with DM_MEDIAN_TILE = 16 and 32 is compared with the path as built
(which picks the side itself) bit for bit.  As context, dm_bilateral_filter (self-guided,
sigma_color 10, sigma_space = the radius) is timed at the same radius on the same map.

The variants are alternated (`reps` windows of about 0.15 s each, at least one call, device
events around every window) after a warm-up.  The kernel's own time comes from one
torch.profiler run of 5 calls (null where the profiler gives no device times); taps_per_s is
cells * (2 r + 1)^2 over that time, or over the call's median where there is none.  Prints one
JSON line per case; `--out FILE` writes the list.

    python tools/median_ab.py [--sides 1024,4096] [--radii 1,3,7] [--forms unweighted,weighted] [--out profiles/median_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F
from deepmatching_stereo_matching_amd import engine

BAND_TAPS = 1 << 27      # float64 taps of one band: 1 GiB


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bands(xp, H, W, r):
    """(first row, the band's taps [K][rows * W]) of the padded plane xp."""
    D = 2 * r + 1
    rows = max(1, BAND_TAPS // (D * D * W))
    for a in range(0, H, rows):
        b = min(H, a + rows)
        yield a, b, F.unfold(xp[None, None, a:b + 2 * r], D)[0]


def t_median(x, w, r):
    """One pass of the definition without the fill flag (ties and +-0 aside)."""
    H, W = x.shape
    nan = float('nan')
    out = torch.empty_like(x)
    if w is None:
        xp = F.pad(torch.where(torch.isfinite(x), x, torch.full_like(x, nan)), (r, r, r, r), value=nan)
        for a, b, taps in bands(xp, H, W, r):
            out[a:b] = torch.nanmedian(taps, dim=0).values.view(b - a, W)
    else:
        ok = torch.isfinite(x) & (w > 0) & (w < float('inf'))
        inf = float('inf')
        xp = F.pad(torch.where(ok, x, torch.full_like(x, inf)), (r, r, r, r), value=inf)      # unusable taps sort last
        wp = F.pad(torch.where(ok, w, torch.zeros_like(w)), (r, r, r, r))
        for (a, b, taps), (_, _, wt) in zip(bands(xp, H, W, r), bands(wp, H, W, r)):
            v, idx = torch.sort(taps, dim=0)
            cs = torch.cumsum(torch.gather(wt, 0, idx), dim=0)
            first = (cs < 0.5 * cs[-1:]).sum(dim=0, keepdim=True).clamp_(max=taps.shape[0] - 1)
            m = torch.gather(v, 0, first)[0]
            out[a:b] = torch.where(cs[-1] > 0, m, torch.full_like(m, nan)).view(b - a, W)
    return torch.where(torch.isfinite(x) & ~torch.isnan(out), out, x)


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def hip(x, w, r, tile):
    def run():
        if tile is None:
            os.environ.pop('DM_MEDIAN_TILE', None)
        else:
            os.environ['DM_MEDIAN_TILE'] = str(tile)
        return engine.median_filter(x, r, weight=w)
    return run


def kernel_time(fn, calls=5):
    """Mean device time in ms of k_median over `calls` calls, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if 'k_median' in ev.key:
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
    rng = np.random.default_rng(side)
    j = np.arange(side)[None, :]
    i = np.arange(side)[:, None]
    x = 0.02 * i + 0.01 * j + np.where(j >= (29 * side) // 64, 4.0, 0.0) + rng.normal(0, 0.3, (side, side))
    x[rng.uniform(size=x.shape) < 0.08] = np.nan
    return x, rng.uniform(0.05, 1.0, (side, side))


sides = [int(s) for s in arg('--sides', '1024,4096').split(',')]
radii = [int(s) for s in arg('--radii', '1,3,7').split(',')]
forms = arg('--forms', 'unweighted,weighted').split(',')
reps = int(arg('--reps', '9'))
out = []
for side in sides:
    a, wa = make(side)
    x = torch.from_numpy(a).cuda()
    wt = torch.from_numpy(wa).cuda()
    for form in forms:
        w = wt if form == 'weighted' else None
        for r in radii:
            variants = dict(torch_chain=lambda: t_median(x, w, r), hip=hip(x, w, r, None),
                            hip_tile_16=hip(x, w, r, 16), hip_tile_32=hip(x, w, r, 32),
                            bilateral_self=lambda: engine.bilateral_filter(x, r, 10.0, float(r)))
            ref = variants['hip']()
            chain = variants['torch_chain']()
            fin = torch.isfinite(ref)
            nan_equal = bool(torch.equal(torch.isnan(ref), torch.isnan(chain)) and
                             torch.equal(torch.isnan(ref), torch.isnan(x)))
            differ = int((ref[fin] != chain[fin]).sum())
            changed = int((ref[fin] != x[fin]).sum())
            tile_same = {k: bool(torch.equal(variants[k]().view(torch.int64), ref.view(torch.int64)))
                         for k in ('hip_tile_16', 'hip_tile_32')}
            run_to_run = bool(torch.equal(variants['hip']().view(torch.int64), ref.view(torch.int64)))
            cells = int(fin.sum())
            del ref, chain, fin
            for fn in variants.values():
                fn()
            # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            os.environ.pop('DM_MEDIAN_TILE', None)
            kern = kernel_time(variants['hip'])
            ms = {k: stat(t) for k, t in times.items()}
            kms = kern['ms'] if kern and 'ms' in kern else ms['hip']['median']
            speedup = ms['torch_chain']['median'] / ms['hip']['median']
            res = dict(form=form, side=side, radius=r,
                       shape='%d^2 float64, two planes + N(0, 0.3), 8 %% NaN; radius %d, %s, 1 pass, min_count 1'
                             % (side, r, 'weights uniform in [0.05, 1)' if w is not None else 'no weights'),
                       filtered_cells=cells, changed_cells=changed,
                       loose=dict(nan_positions_equal=nan_equal, differing_cells=differ,
                                  agrees=bool(nan_equal and differ == 0)),
                       hip_tiles_bit_identical=tile_same, hip_run_to_run_identical=run_to_run, inner=inner, reps=reps,
                       ms=ms, speedup_median=speedup, hip_beats_torch_chain=bool(speedup > 1.0),
                       bilateral_over_median=ms['bilateral_self']['median'] / ms['hip']['median'], hip_kernel=kern,
                       taps_per_s=side * side * (2 * r + 1) ** 2 / (kms * 1e-3),
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            del variants
            torch.cuda.empty_cache()
    del x, wt
    torch.cuda.empty_cache()
if '--out' in sys.argv:
    with open(arg('--out', None), 'w') as fh:
        json.dump(out, fh, indent=1)
