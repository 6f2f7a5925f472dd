"""A/B of engine.fill_holes (dm_fill.hip) against what a user could write without it: the same
definition (tests/test_fill_host.py) as a chain of PyTorch tensor ops on the same device.  Maps
of 1024^2 and 4096^2 cells (`--sides`), 7 % random holes, iters = 16.  Four variants are
alternated (`reps` windows of about 0.15 s each, device events around every window) after a
warm-up: the torch chain, the HIP path as built (16 Jacobi steps per k_fill_tile launch), the
HIP path with DM_FILL_STEPS=8 (a halo of 8 cells, two launches per level) and with
DM_FILL_STEPS=1 (the plain relaxation: one step per launch, the same kernel with a halo of one
cell).  Outputs are compared bit for bit.  Prints one JSON line per side;
`--out FILE` writes the list.

    python tools/fill_ab.py [--sides 1024,4096] [--out profiles/fill_ab.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F
from deepmatching_stereo_matching_amd import engine

ITERS = 16


def t_pull(v, n):
    H, W = v.shape
    v, n = F.pad(v, (0, W & 1, 0, H & 1)), F.pad(n, (0, W & 1, 0, H & 1))
    c = lambda a, i, j: a[i::2, j::2]
    s = ((c(n, 0, 0) * c(v, 0, 0) + c(n, 0, 1) * c(v, 0, 1)) + c(n, 1, 0) * c(v, 1, 0)) + c(n, 1, 1) * c(v, 1, 1)
    m = ((c(n, 0, 0) + c(n, 0, 1)) + c(n, 1, 0)) + c(n, 1, 1)
    return torch.where(m > 0, s / m, torch.zeros_like(s)), m


def t_push(v, n, p):
    H, W = v.shape
    h, w = p.shape
    i, j = torch.arange(H, device=v.device), torch.arange(W, device=v.device)
    I, J = i >> 1, j >> 1
    I2 = (I + torch.where((i & 1) > 0, 1, -1)).clamp(0, h - 1)
    J2 = (J + torch.where((j & 1) > 0, 1, -1)).clamp(0, w - 1)
    a, b, c, d = p[I][:, J], p[I2][:, J], p[I][:, J2], p[I2][:, J2]
    return torch.where(n > 0, v, (((9.0 * a + 3.0 * b) + 3.0 * c) + d) * 0.0625)


def t_relax(v, hole, iters):
    for _ in range(iters):
        q = F.pad(v[None, None], (1, 1, 1, 1), mode='replicate')[0, 0]
        v = torch.where(hole, (((q[:-2, 1:-1] + q[2:, 1:-1]) + q[1:-1, :-2]) + q[1:-1, 2:]) * 0.25, v)
    return v


def t_fill(x, iters):
    hole = ~torch.isfinite(x)
    vs, ns = [torch.where(hole, torch.zeros_like(x), x)], [(~hole).to(torch.float64)]
    while tuple(vs[-1].shape) != (1, 1):
        v, n = t_pull(vs[-1], ns[-1])
        vs.append(v)
        ns.append(n)
    p = vs[-1]
    for k in range(len(vs) - 2, -1, -1):
        p = t_relax(t_push(vs[k], ns[k], p), ns[k] == 0, iters)
    return p


def launches(H, W, iters, per=16, topc=4096, pull=6):
    """Kernel launches of dm_fill_holes (dm_fill.hip: FILL_TOPC, FILL_PULL, FILL_K)."""
    k = 0
    while H * W > topc:
        H, W, k = (H + 1) // 2, (W + 1) // 2, k + 1
    return -(-k // pull) + 1 + k * max(1, -(-iters // per))


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def steps(per):
    def run():
        if per is None:
            os.environ.pop('DM_FILL_STEPS', None)
        else:
            os.environ['DM_FILL_STEPS'] = str(per)
        return engine.fill_holes(x, ITERS)
    return run


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


sides = [int(s) for s in sys.argv[sys.argv.index('--sides') + 1].split(',')] if '--sides' in sys.argv else [1024, 4096]
out = []
for side in sides:
    rng = np.random.default_rng(side)
    a = rng.normal(0, 5, (side, side))
    a[rng.uniform(size=a.shape) < 0.07] = np.nan
    x = torch.from_numpy(a).cuda()
    variants = dict(torch_chain=lambda: t_fill(x, ITERS), hip=steps(None), hip_8_steps_per_launch=steps(8),
                    hip_one_step_per_launch=steps(1))
    ref = variants['hip']().view(torch.int64)
    same = {k: bool(torch.equal(fn().view(torch.int64), ref)) for k, fn in variants.items()}
    reps = 9
    for fn in variants.values():
        for _ in range(3):
            fn()
    # windows of about 0.15 s each, whatever the variant's speed
    inner = {k: int(min(500, max(3, 150.0 // timed(fn, 3) + 1))) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed(fn, inner[k]))
    os.environ.pop('DM_FILL_STEPS', None)
    res = dict(shape='%d^2 float64, 7 %% random holes, iters %d' % (side, ITERS), bit_identical=same, inner=inner,
               reps=reps, ms={k: stat(t) for k, t in times.items()},
               launches=dict(hip=launches(side, side, ITERS), hip_8_steps_per_launch=launches(side, side, ITERS, 8),
                             hip_one_step_per_launch=launches(side, side, ITERS, 1)),
               device=torch.cuda.get_device_name(0))
    out.append(res)
    print(json.dumps(res), flush=True)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as fh:
        json.dump(out, fh, indent=1)
