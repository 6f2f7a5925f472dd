"""A/B of engine.filter_speckles (dm_speckle.hip) against what a user could write without it: the
same definition (tests/test_speckle_host.py) as min-label propagation in PyTorch tensor ops on
the same device -- every cell takes the smallest label among itself and its joined
4-neighbours, then jumps to its label's label, until nothing changes (checked every 4 rounds;
at most `--cap` rounds, reported when reached); sizes by bincount.  Maps of 1024^2 and 4096^2
cells (`--sides`), three inputs:

    a  the plane with planted blobs of 1..3 x 1..3 cells (60 per 150^2 cells), offset 8, at
       (16, 1.0): one huge segment and many small ones, the workload's own shape
    b  N(0, 5) noise with 7 % NaN at (16, 5.0): many mid-size segments
    c  N(0, 5) noise without holes at (16, inf): a single segment, the worst case for the counts

The variants (the torch chain, the HIP path as built, and with DM_SPECKLE_TILE = 32 and 16) are
alternated (`reps` windows of about 0.15 s each, at least one call, device events around every
window) after a warm-up.  Outputs are compared bit for bit.  The time of each kernel of the HIP
path comes from one torch.profiler run of 5 calls (null where the profiler gives no device
times).  Prints one JSON line per case; `--out FILE` writes the list.

    python tools/speckle_ab.py [--sides 1024,4096] [--cases a,b,c] [--cap 4096] [--out profiles/speckle_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


CAP = int(arg('--cap', '4096'))
ROUNDS = {}


def t_speckle(x, max_size, max_diff, key=None):
    H, W = x.shape
    fin = torch.isfinite(x)
    idx = torch.arange(H * W, device=x.device).view(H, W)
    lab = torch.where(fin, idx, torch.full_like(idx, H * W))
    jh = fin[:, 1:] & fin[:, :-1] & ((x[:, 1:] - x[:, :-1]).abs() <= max_diff)      # joined with the left neighbour
    jv = fin[1:] & fin[:-1] & ((x[1:] - x[:-1]).abs() <= max_diff)                  # joined with the upper one
    big = torch.full_like(idx, H * W)
    pad = torch.cat([lab.flatten(), lab.new_tensor([H * W])])      # (a hole's label points at a sentinel)
    rounds = 0
    while rounds < CAP:
        for _ in range(4):
            new = lab.clone()
            new[:, 1:] = torch.minimum(new[:, 1:], torch.where(jh, lab[:, :-1], big[:, 1:]))
            new[:, :-1] = torch.minimum(new[:, :-1], torch.where(jh, lab[:, 1:], big[:, 1:]))
            new[1:] = torch.minimum(new[1:], torch.where(jv, lab[:-1], big[1:]))
            new[:-1] = torch.minimum(new[:-1], torch.where(jv, lab[1:], big[1:]))
            pad[:-1] = new.flatten()
            prev, lab = lab, pad[new]                                # jump: the label's own label
            rounds += 1
        if torch.equal(prev, lab):
            break
    if key is not None:
        ROUNDS[key] = rounds
    counts = torch.bincount(lab[fin], minlength=H * W + 1)
    size = torch.where(fin, counts[lab], torch.zeros_like(lab))
    removed = fin & (size <= max_size)
    return torch.where(removed, torch.full_like(x, float('nan')), x), removed.to(torch.uint8), size, \
        torch.where(fin, lab, torch.full_like(lab, -1))


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def hip(x, p, tile):
    def run():
        if tile is None:
            os.environ.pop('DM_SPECKLE_TILE', None)
        else:
            os.environ['DM_SPECKLE_TILE'] = str(tile)
        return engine.filter_speckles(x, p[0], p[1], return_removed=True, return_sizes=True, return_labels=True)
    return run


def kernel_times(fn, calls=5):
    """Mean device time in ms of each k_spk_* kernel over `calls` calls, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if 'k_spk_' in ev.key:
                total = getattr(ev, 'device_time_total', None)
                if total is None:
                    total = ev.cuda_time_total
                name = ev.key[ev.key.index('k_spk_'):].split('(')[0]
                out[name] = dict(ms=total / 1e3 / ev.count, launches_per_call=ev.count / calls)
        return out or None
    except Exception as e:      # no device tracing on this build: say so, the A/B itself stands
        return dict(error=repr(e))


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def make(case, side):
    rng = np.random.default_rng(side)
    if case == 'a':
        i, j = np.mgrid[0:side, 0:side]
        a = 0.03125 * i - 0.0625 * j + 3
        n = int(round(60 * side * side / 150.0 ** 2))
        h, w = rng.integers(1, 4, n), rng.integers(1, 4, n)
        r, c = rng.integers(0, side - 3, n), rng.integers(0, side - 3, n)
        mark = np.zeros((side, side), dtype=bool)
        for dy in range(3):
            for dx in range(3):
                k = (h > dy) & (w > dx)
                mark[r[k] + dy, c[k] + dx] = True
        a[mark] += 8.0
        return a, (16, 1.0), 'plane + %d planted blobs (%d cells), offset 8' % (n, mark.sum())
    a = rng.normal(0, 5, (side, side))
    if case == 'b':
        a[rng.uniform(size=a.shape) < 0.07] = np.nan
        return a, (16, 5.0), 'N(0, 5) noise, 7 % NaN'
    return a, (16, float('inf')), 'N(0, 5) noise, no holes: one segment'


sides = [int(s) for s in arg('--sides', '1024,4096').split(',')]
cases = arg('--cases', 'a,b,c').split(',')
out = []
for side in sides:
    for case in cases:
        a, p, what = make(case, side)
        x = torch.from_numpy(a).cuda()
        key = (case, side)
        variants = dict(torch_chain=lambda: t_speckle(x, p[0], p[1], key), hip=hip(x, p, None),
                        hip_tile_32=hip(x, p, 32), hip_tile_16=hip(x, p, 16))
        ref = variants['hip']()
        same = {}
        for k, fn in variants.items():
            got = fn()
            same[k] = bool(torch.equal(got[0].view(torch.int64), ref[0].view(torch.int64)) and
                           all(torch.equal(g.to(torch.int64), r.to(torch.int64)) for g, r in zip(got[1:], ref[1:])))
        again = variants['hip']()
        run_to_run = bool(all(torch.equal(g.view(torch.uint8), r.view(torch.uint8)) for g, r in zip(again, ref)))
        fin = torch.isfinite(x)
        segments = int(torch.unique(ref[3][fin]).numel())
        removed = int(ref[1].sum())
        largest = int(ref[2].max())
        del ref, again, got
        reps = 9
        for fn in variants.values():
            fn()
        # windows of about 0.15 s each, whatever the variant's speed (a slow chain: one call per window)
        inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, inner[k]))
        os.environ.pop('DM_SPECKLE_TILE', None)
        kern = kernel_times(variants['hip'])
        res = dict(case=case, shape='%d^2 float64, %s, (max_size, max_diff) = (%d, %g)' % (side, what, p[0], p[1]),
                   segments=segments, largest=largest, removed=removed, finite=int(fin.sum()),
                   bit_identical=same, hip_run_to_run_identical=run_to_run, inner=inner, reps=reps,
                   ms={k: stat(t) for k, t in times.items()},
                   torch_chain_rounds=ROUNDS.get(key), torch_chain_capped=ROUNDS.get(key, 0) >= CAP,
                   launches=dict(hip=4, hip_tile_32=4, hip_tile_16=4), hip_kernels_ms=kern,
                   device=torch.cuda.get_device_name(0))
        out.append(res)
        print(json.dumps(res), flush=True)
        del x, variants
        torch.cuda.empty_cache()
if '--out' in sys.argv:
    with open(arg('--out', None), 'w') as fh:
        json.dump(out, fh, indent=1)
