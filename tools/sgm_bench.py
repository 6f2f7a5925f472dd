"""A/B of engine.sgm_refine (dm_sgm.hip) against engine.photo_refine at the same (radius, search)
-- the per-cell search it replaces, whose kernel walks four windows per candidate where k_sgm_cost
walks one -- and against the same definition built from PyTorch tensor ops on the same device.

The PyTorch chain follows include/dmstereo_sgm.h rule by rule for a map whose every cell is free and
whose every candidate is scored (the margin sees to it): the costs tap by tap in int32 from gathered
img2 pixels, the float64 tail one tensor op per operation, the paths as one step per row (or column)
of the map with all lines of a direction in one tensor -- the predecessor row shifted by the
direction's column step, V from the Chebyshev distance of the displacements as a [lines][L][L]
tensor -- and the winner by one argmin over the key (S, ay^2 + ax^2, label index).  Its planes,
score and shift must equal the kernel's bit for bit (`bit_identical`; the run stops otherwise).

Maps of 1024^2 and 4096^2 cells (`--sides`), (radius, search, paths) in (2,2,4), (2,2,8), (3,2,8),
(3,3,8) (`--cases`), penalties (2.0, 8.0), sub-pixel step on.  The pair is synthetic.stereo_pair
(dx = 2) of 1024 + 2 * 12 pixels a side, tiled for the larger map; the start is the truth (0, 2)
plus integers uniform in [-1, 1] per plane.

The variants are alternated (`--reps` windows of about 0.15 s each, at least one call, device
events around every window) after a warm-up; medians are reported.  The share of each launch comes
from one profiled call (torch.profiler's device activity; `kernel_us` is null where the profiler
reports no device kernels).  `path_ns_per_cell` is the path kernel's time over the length of the
longest line, `path_rounds` the number of wavefronts it launches over the 8192 a device of 256 CUs
holds at 8 per SIMD: with more than one round the step latency is that figure over the rounds.
Prints one JSON line per case; `--out FILE` writes the list.

    python tools/sgm_bench.py [--sides 1024,4096] [--cases 2:2:4,2:2:8,3:2:8,3:3:8] [--torch-max-side 1024]
                              [--out profiles/sgm_bench.json]
"""
import json, os, sys, statistics
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

MARGIN = 12               # radius 3 + search 3 + disparity 2 + noise 1 + the extra row and column, rounded up
BASE = 1024               # cells a side of the generated pair; larger maps tile it
P1, P2 = 2.0, 8.0
DIRS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def t_costs(a32, b32, by, bx, r, s, off):
    """Rule 2 for free cells whose candidates are all scored -> (C int64 [H][W][L], score float64 [H][W][L])."""
    Hi, Wi = a32.shape
    H, W = by.shape
    D = 2 * r + 1
    n = D * D
    bflat = b32.reshape(-1)

    def A(u, v):
        return a32[off - r + u:off - r + u + H, off - r + v:off - r + v + W]

    z = torch.zeros((H, W), dtype=torch.int32, device=by.device)
    sa, saa = z.clone(), z.clone()
    for u in range(D):
        for v in range(D):
            sa += A(u, v)
            saa += A(u, v) * A(u, v)
    sa = sa.long()
    VA = (n * saa.long() - sa * sa).double()
    C, SC = [], []
    for ay in range(-s, s + 1):
        for ax in range(-s, s + 1):
            base = (by + ay - r) * Wi + (bx + ax - r)
            sp, spp, sap = z.clone(), z.clone(), z.clone()
            for u in range(D):
                for v in range(D):
                    p = bflat[base + (u * Wi + v)]
                    sp += p
                    spp += p * p
                    sap += A(u, v) * p
            sp = sp.long()
            CA, CB = (n * sap.long() - sa * sp).double(), (n * spp.long() - sp * sp).double()
            pos = (VA > 0) & (CB > 0)
            t = (CA / torch.sqrt(torch.where(pos, VA * CB, torch.ones_like(CB)))).clamp_(-1.0, 1.0)
            sc = torch.where(pos, t, torch.zeros_like(t))
            SC.append(sc)
            C.append(torch.round((1.0 - sc) * 1024.0).long())
    return torch.stack(C, dim=2), torch.stack(SC, dim=2)


def t_paths(C, dy, dx, s, p1, p2, paths):
    """Rule 3 for a map without dead cells -> S int64 [H][W][L].  dy, dx: the base displacements [H][W]."""
    H, W, nl = C.shape
    dev = C.device
    ly = torch.arange(-s, s + 1, device=dev).repeat_interleave(2 * s + 1)
    lx = torch.arange(-s, s + 1, device=dev).repeat(2 * s + 1)
    ddy, ddx = (ly[:, None] - ly[None, :])[None], (lx[:, None] - lx[None, :])[None]      # label a minus label b
    S = torch.zeros_like(C)

    def step(Cp, Lq, ey, ex):
        """L of the cells p from L of their predecessors q; ey, ex = base_p - base_q."""
        cheb = torch.maximum((ddy + ey[:, None, None]).abs(), (ddx + ex[:, None, None]).abs())
        V = torch.where(cheb == 0, 0, torch.where(cheb == 1, p1, p2))
        return Cp + (Lq[:, None, :] + V).amin(dim=2) - Lq.amin(dim=1, keepdim=True)

    for ry, rx in DIRS[:paths]:
        if ry == 0:      # the lines are the rows: one step per column
            xs = range(W) if rx > 0 else range(W - 1, -1, -1)
            Lq = None
            for x in xs:
                Lp = C[:, x] if Lq is None else step(C[:, x], Lq, dy[:, x] - dy[:, x - rx], dx[:, x] - dx[:, x - rx])
                S[:, x] += Lp
                Lq = Lp
        else:            # one step per row; the predecessor of (y, x) is (y - ry, x - rx)
            ys = range(H) if ry > 0 else range(H - 1, -1, -1)
            Lq = None
            for y in ys:
                if Lq is None:
                    Lp = C[y].clone()
                else:
                    lo, hi = max(0, rx), W + min(0, rx)      # the cells of the row that have a predecessor
                    Lp = C[y].clone()
                    Lp[lo:hi] = step(C[y, lo:hi], Lq[lo - rx:hi - rx], dy[y, lo:hi] - dy[y - ry, lo - rx:hi - rx],
                                     dx[y, lo:hi] - dx[y - ry, lo - rx:hi - rx])
                S[y] += Lp
                Lq = Lp
    return S


def t_sgm(a32, b32, dr, dc, r, s, p1, p2, paths, off):
    """The definition for a finite map of free cells whose candidates are all scored, with the sub-pixel step
    -> (out_row, out_col, score, int8 shift)."""
    H, W = dr.shape
    dev = dr.device
    nc = 2 * s + 1
    cy = (torch.arange(H, device=dev) + off)[:, None].expand(H, W)
    cx = (torch.arange(W, device=dev) + off)[None, :].expand(H, W)
    by, bx = torch.round(cy.double() - dr).long(), torch.round(cx.double() - dc).long()
    C, SC = t_costs(a32, b32, by, bx, r, s, off)
    S = t_paths(C, by - cy, bx - cx, s, p1, p2, paths)
    ly = torch.arange(-s, s + 1, device=dev).repeat_interleave(nc)
    lx = torch.arange(-s, s + 1, device=dev).repeat(nc)
    key = (S * 32 + (ly * ly + lx * lx)[None, None]) * 64 + torch.arange(nc * nc, device=dev)[None, None]
    k = key.argmin(dim=2)
    ay, ax = ly[k], lx[k]
    s0 = S.gather(2, k[..., None])[..., 0]

    def valley(okm, km, kp):
        sm = S.gather(2, km.clamp(0, nc * nc - 1)[..., None])[..., 0]
        sp = S.gather(2, kp.clamp(0, nc * nc - 1)[..., None])[..., 0]
        den = (sm + sp) - 2 * s0
        ok = okm & (den > 0)
        t = ((0.5 * (sm - sp).double()) / torch.where(ok, den, torch.ones_like(den)).double()).clamp_(-0.5, 0.5)
        return torch.where(ok, t, torch.zeros_like(t))

    ty = valley((ay > -s) & (ay < s), k - nc, k + nc)
    tx = valley((ax > -s) & (ax < s), k - 1, k + 1)
    moved = (ay != 0) | (ax != 0)
    out_row = torch.where(moved, (cy - by - ay).double() - ty, dr)
    out_col = torch.where(moved, (cx - bx - ax).double() - tx, dc)
    score = SC.gather(2, k[..., None])[..., 0]
    return out_row, out_col, score, torch.stack([ay, ax]).to(torch.int8)


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


def kernel_us(fn):
    """Device time in microseconds of the kernels of one call, by name prefix; None if the profiler sees none."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0)
        for name in ('k_sgm_cost', 'k_sgm_path', 'k_sgm_pick', 'k_refine'):
            if name in ev.key and t:
                out[name] = out.get(name, 0.0) + float(t)
    return out or None


_BASE = {}


def make(side):
    if 'pair' not in _BASE:
        _BASE['pair'] = stereo_pair(BASE + 2 * MARGIN, BASE + 2 * MARGIN, seed=11, dx=2)
    h = side + 2 * MARGIN
    reps = -(-h // (BASE + 2 * MARGIN))
    a, b = (np.ascontiguousarray(np.tile(t, (reps, reps))[:h, :h]) for t in _BASE['pair'])
    rng = np.random.default_rng(side + 1)
    return (a, b, 0.0 + rng.integers(-1, 2, (side, side)).astype(np.float64),
            2.0 + rng.integers(-1, 2, (side, side)).astype(np.float64))


if __name__ == '__main__':
    sides = [int(v) for v in arg('--sides', '1024,4096').split(',')]
    cases = [tuple(int(v) for v in c.split(':')) for c in arg('--cases', '2:2:4,2:2:8,3:2:8,3:3:8').split(',')]
    reps = int(arg('--reps', '7'))
    torch_max = int(arg('--torch-max-side', '4096'))
    q1, q2 = int(round(P1 * 1024)), int(round(P2 * 1024))
    out = []
    for side in sides:
        a, b, dr_, dc_ = make(side)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        a32, b32 = ta.int(), tb.int()
        dr, dc = torch.from_numpy(dr_).cuda(), torch.from_numpy(dc_).cuda()
        for r, s, paths in cases:
            variants = dict(hip=lambda: engine.sgm_refine(ta, tb, dr, dc, r, s, P1, P2, paths=paths, offset=MARGIN,
                                                          return_score=True, return_shift=True),
                            photo_refine=lambda: engine.photo_refine(ta, tb, dr, dc, r, s, offset=MARGIN,
                                                                     return_score=True, return_shift=True))
            with_torch = side <= torch_max
            if with_torch:
                variants['torch_chain'] = lambda: t_sgm(a32, b32, dr, dc, r, s, q1, q2, paths, MARGIN)
            ref = variants['hip']()
            again = variants['hip']()
            run_to_run = all(bool(torch.equal(p.view(torch.int8), q.view(torch.int8))) for p, q in zip(ref, again))
            bit_equal = None
            if with_torch:
                chain = variants['torch_chain']()
                bit_equal = all(bool(torch.equal(ref[k].view(torch.int64), chain[k].view(torch.int64))) for k in (0, 1, 2)) \
                    and bool(torch.equal(ref[3], chain[3]))
                del chain
                if not bit_equal:
                    raise SystemExit('side %d radius %d search %d paths %d: the chain and the kernel disagree'
                                     % (side, r, s, paths))
            moved = float(ref[3].ne(0).any(dim=0).double().mean())
            wrong = float(((ref[0].round() != 0) | (ref[1].round() != 2)).double().mean())
            del ref, again
            variants['photo_refine']()
            kus = {k: kernel_us(variants[k]) for k in ('hip', 'photo_refine')}
            inner = {k: int(min(500, max(1, 150.0 // timed(fn, 1) + 1))) for k, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, inner[k]))
            ms = {k: stat(t) for k, t in times.items()}
            waves = (2 * side + 2 * side + (4 * (2 * side - 1) if paths == 8 else 0))
            res = dict(side=side, radius=r, search=s, paths=paths, penalties=[P1, P2],
                       shape='%d^2 cells, uint8 pair of %d^2 (stereo_pair dx 2 of %d^2, tiled), truth (0, 2) + integers in '
                             '[-1, 1] per plane; sub-pixel step, score and shift' % (side, side + 2 * MARGIN, BASE + 2 * MARGIN),
                       moved_share=moved, wrong_share=wrong, check=dict(bit_identical=bit_equal),
                       hip_run_to_run_identical=run_to_run, inner=inner, reps=reps, ms=ms, kernel_us=kus,
                       ratio_to_photo_refine=ms['hip']['median'] / ms['photo_refine']['median'],
                       speedup_over_torch_chain=(ms['torch_chain']['median'] / ms['hip']['median']) if with_torch else None,
                       path_lines=waves, path_rounds=waves / 8192.0,
                       path_ns_per_cell=(kus['hip']['k_sgm_path'] * 1e3 / side) if kus['hip'] and 'k_sgm_path' in kus['hip']
                       else None,
                       device=torch.cuda.get_device_name(0))
            out.append(res)
            print(json.dumps(res), flush=True)
            if '--out' in sys.argv:
                with open(arg('--out', None), 'w') as fh:
                    json.dump(out, fh, indent=1)
            del variants
        del ta, tb, a32, b32, dr, dc
        torch.cuda.empty_cache()
