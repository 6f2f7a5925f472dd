"""What the coarse-to-fine solve costs: engine.solve_coarse_to_fine with coarse=1 and coarse=2,
followed by the stitch, against the plain path (engine.solve_tiles and the stitch, what
ImageCutSolver runs without the keyword) on the C3 pair: 1024^2 cells, S = 128, stride 128, 64
tiles, ws 5, full pyramid, sub-pixel.  The three are alternated (`reps` windows of `inner` solves
each, device events around every window) after a warm-up; the medians are reported.  A coarse
level is solved in both directions, so the tile counts predict (T_0 + 2 sum T_j) / T_0; the
measured ratio stands beside it.  Prints one JSON line; `--out FILE` also writes it.

    python tools/prior_bench.py [--out profiles/prior_bench.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from deepmatching_stereo_matching_amd import engine, _lib as L
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

tile, grid, ws = 128, 8, 5
side = (grid + 1) * tile + ws - 1
a, b = stereo_pair(side, side, seed=1000, dx=2, max_disp=tile // 4, sinusoidal=True)
n, org = engine.cut_grid(a.shape, [tile, tile], [tile, tile], ws)
assert len(org) == 64, len(org)
dev = engine.default_device()
da, db = engine.to_device_u8(a, dev), engine.to_device_u8(b, dev)
M = L.DM_TM_CCOEFF_NORMED
MODES = ['elevation', 'elevation2']

def plain():
    return engine.stitch(engine.solve_tiles(da, db, org, tile, tile, ws, M), n, tile, tile, [tile, tile], MODES)

def coarse(k):
    def run():
        match = engine.solve_coarse_to_fine(da, db, [tile, tile], [tile, tile], ws, M, k)[0]
        return engine.stitch(match, n, tile, tile, [tile, tile], MODES)
    return run

def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner

runs = {'plain': plain, 'coarse1': coarse(1), 'coarse2': coarse(2)}
tiles = {k: [len(g[1]) for g in engine.coarse_grids(a.shape, [tile, tile], [tile, tile], ws, k)] for k in (1, 2)}
for _ in range(3):
    for fn in runs.values():
        fn()
inner, reps = 3, 9
if '--reps' in sys.argv:
    reps = int(sys.argv[sys.argv.index('--reps') + 1])
t = {name: [] for name in runs}
for _ in range(reps):
    for name, fn in runs.items():
        t[name].append(timed(fn, inner))
ms = {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in t.items()}
res = dict(shape='C3 1024^2 S=128 64 tiles ws5 full pyramid sub-pixel', inner=inner, reps=reps, ms=ms,
           device=torch.cuda.get_device_name(0))
for k in (1, 2):
    res['coarse%d' % k] = dict(tiles_per_level=tiles[k], expected_ratio=(tiles[k][0] + 2 * sum(tiles[k][1:])) / tiles[k][0],
                               measured_ratio=ms['coarse%d' % k]['median'] / ms['plain']['median'])
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res))
