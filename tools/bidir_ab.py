"""A/B of engine.solve_tiles_bidir (both directions in one stream of 2T tiles) against two
engine.solve_tiles calls (img1 -> img2, img2 -> img1) on the C2 shape: 512^2 pair, S = 64, 64
tiles, ws 5, full pyramid, sub-pixel.  The two are alternated (`reps` windows of `inner` solves
each, device events around every window) after a warm-up, and their outputs compared bit for
bit.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bidir_ab.py [--out profiles/fb_bidir_c2.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine, _lib as L
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

tile, grid, ws = 64, 8, 5
side = (grid + 1) * tile + ws - 1
a, b = stereo_pair(side, side, seed=1000, dx=2, max_disp=tile // 4, sinusoidal=True)
n, org = engine.cut_grid(a.shape, [tile, tile], [tile, tile], ws)
assert len(org) == 64, len(org)
dev = engine.default_device()
da, db = engine.to_device_u8(a, dev), engine.to_device_u8(b, dev)
M = L.DM_TM_CCOEFF_NORMED

def two():
    return engine.solve_tiles(da, db, org, tile, tile, ws, M), engine.solve_tiles(db, da, org, tile, tile, ws, M)

def one():
    return engine.solve_tiles_bidir(da, db, org, tile, tile, ws, M)

def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner

f2, b2 = two(); f1, b1 = one()
same = bool(torch.equal(f1.view(torch.int64), f2.view(torch.int64)) and torch.equal(b1.view(torch.int64), b2.view(torch.int64)))
for _ in range(10):
    two(); one()
inner, reps = 20, 15
t2, t1 = [], []
for _ in range(reps):
    t2.append(timed(two, inner)); t1.append(timed(one, inner))
res = dict(shape='C2 512^2 S=64 64 tiles ws5 full pyramid sub-pixel', bit_identical=same, inner=inner, reps=reps,
           two_calls_ms=dict(median=statistics.median(t2), min=min(t2), max=max(t2)),
           bidir_ms=dict(median=statistics.median(t1), min=min(t1), max=max(t1)),
           device=torch.cuda.get_device_name(0))
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res))
