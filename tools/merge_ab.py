"""Timing of dm_stitch_merge (dm_merge.hip) against the overwriting stitch it replaces.

Case: a 15 x 15 grid of S = 128 tiles at stride 64 (a 1024^2 map, four covering tiles at every
interior pixel), forward and backward tiles float64 [225][3][128][128] with matches near their
cells and 1 % NaN, one mode, tolerance 1.  Baseline: four back-to-back dm_stitch_fb launches on
the same tensors (the parent's kernel, reading what one candidate costs, four times).  Variants:
dm_stitch_merge under each rule with every output.  All calls go to the library with outputs
allocated once; the variants are alternated in `reps` windows of about 0.15 s each after a
warm-up, device events around every window.  Prints one JSON line; `--out FILE` writes it.

    python tools/merge_ab.py [--out profiles/merge_ab.json]
"""
import ctypes, json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine

N, S, STRIDE, TOL = (15, 15), 128, (64, 64), 1.0
T = N[0] * N[1]
H, W = STRIDE[0] * (N[0] - 1) + S, STRIDE[1] * (N[1] - 1) + S


def tiles(seed, sigma):
    g = torch.Generator(device='cuda').manual_seed(seed)
    ii = torch.arange(S, device='cuda', dtype=torch.float64)[:, None].expand(S, S)
    jj = torch.arange(S, device='cuda', dtype=torch.float64)[None, :].expand(S, S)
    m = torch.empty((T, 3, S, S), dtype=torch.float64, device='cuda')
    m[:, 0] = ii + sigma * torch.randn((T, S, S), generator=g, device='cuda', dtype=torch.float64)
    m[:, 1] = jj + sigma * torch.randn((T, S, S), generator=g, device='cuda', dtype=torch.float64)
    m[:, 2] = 5 * torch.rand((T, S, S), generator=g, device='cuda', dtype=torch.float64)
    m[torch.rand(m.shape, generator=g, device='cuda') < 0.01] = float('nan')
    return m


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


fwd, bwd = tiles(1, 0.6), tiles(2, 0.3)
lib = L.load()
modes = (ctypes.c_int32 * 1)(L.CAL_MODES['elevation'])
f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')
dmap, score, err, spread = f64(1, H, W), f64(H, W), f64(H, W), f64(1, H, W)
count = torch.empty((H, W), dtype=torch.uint8, device='cuda')


def stitch_fb_x4():
    for _ in range(4):
        L.check(lib.dm_stitch_fb(L.ptr(fwd), L.ptr(bwd), N[0], N[1], S, S, STRIDE[0], STRIDE[1], modes, 1, TOL,
                                 L.ptr(dmap), L.ptr(score), L.ptr(err), L.stream_handle()))


def merge(rule):
    def run():
        L.check(lib.dm_stitch_merge(L.ptr(fwd), L.ptr(bwd), N[0], N[1], S, S, STRIDE[0], STRIDE[1], modes, 1, TOL,
                                    L.MERGE_RULES[rule], 1, L.ptr(dmap), L.ptr(score), L.ptr(err), L.ptr(spread),
                                    L.ptr(count), L.stream_handle()))
    return run


variants = {'stitch_fb_x4': stitch_fb_x4}
variants.update({'merge_' + r: merge(r) for r in L.MERGE_RULES})
# the anchor at the timed size: rule 'last' is dm_stitch_fb bit for bit
ref = engine.stitch_fb(fwd, bwd, N, S, S, STRIDE, ['elevation'], TOL)
got = engine.stitch_merge(fwd, bwd, N, S, S, STRIDE, ['elevation'], TOL, 'last')
anchor = all(bool(torch.equal(a.view(torch.int64), b.view(torch.int64))) for a, b in zip(ref, got[:3]))
holes = {r: float(torch.isnan(engine.stitch_merge(fwd, bwd, N, S, S, STRIDE, ['elevation'], TOL, r)[0]).double().mean())
         for r in L.MERGE_RULES}
for fn in variants.values():
    for _ in range(3):
        fn()
reps = 9
inner = {k: int(min(2000, max(3, 150.0 // timed(fn, 3) + 1))) for k, fn in variants.items()}
times = {k: [] for k in variants}
for _ in range(reps):
    for k, fn in variants.items():
        times[k].append(timed(fn, inner[k]))
ms = {k: stat(t) for k, t in times.items()}
base = ms['stitch_fb_x4']['median']
res = dict(shape='%d x %d tiles of %d^2 at stride %d: map %d x %d, 1 mode, tol %g' % (N + (S, STRIDE[0], H, W, TOL)),
           last_equals_stitch_fb=anchor, hole_share=holes, inner=inner, reps=reps, ms=ms,
           ratio_to_stitch_fb_x4={k: v['median'] / base for k, v in ms.items()},
           device=torch.cuda.get_device_name(0))
print(json.dumps(res), flush=True)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as fh:
        json.dump(res, fh, indent=1)
