"""The w0 = 128 level kernel with num taken whole from the f16 MFMA in its second sweep
(k_level1_mfq<..., F16 = true>, csrc/dm_mfma.h) against the oracle, bit for bit, at the smallest
shapes that reach the instance: tiles of h0 in {16, 32} x 128, ws in {3, 5}, both methods, two
or three tiles per batch, level 1 stored and not stored.

Content: the smooth texture of stereo_pair plus the content classes at the ends of the value
range -- binary, checker, edge (the largest |num| and the most negative products), dark, bright,
dark_bright (the largest sums: the digit slots), const (flat patches and windows: num == 0
everywhere, NaN maps).

Compared with the oracle (pinned pow): every level >= 1, the matching indices and sub-pixel
offsets, and the per-patch rmin / rmax the kernel leaves in the stats workspace -- through the
min/max-known level-0 volume, which is (r - rmin) / (rmax - rmin) of exactly those two, and
bitwise against the rmin / rmax the standalone volume kernel finds on a fresh workspace with
the i8 row-pair strips.

Every test asserts dm_level_num_f16 (the predicate dm_corr_stats and the launcher share), so a
batch that silently took the i8 path cannot pass."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from deepmatching_stereo_matching_amd.synthetic import content_pair, stereo_pair
from test_shape_lattice import _crop, _feat, _same

W0 = 128
ORIGINS = {16: [(0, 0), (3, 7), (2, 5)], 32: [(1, 0), (2, 7)]}   # odd offsets, odd image pitch
KINDS = ['texture', 'binary', 'checker', 'edge', 'dark', 'bright', 'dark_bright', 'const']
CASES = [(h0, ws, m) for h0 in (16, 32) for ws in (3, 5) for m in (5, 4)]


@pytest.fixture(scope='module')
def pinned_pow():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    O.set_pow_mode('pinned')
    yield
    O.set_pow_mode('libm')


def images(kind, h0, ws):
    h, w = h0 + ws - 1 + 3, W0 + ws - 1 + 7
    if kind == 'texture':
        return stereo_pair(h, w, seed=7 * h0 + ws, dx=3)
    return content_pair(kind, h, w, 12)


def took_f16_path(L, batch):
    return L.load().dm_level_num_f16(batch.ref()) == 1


def stats_minmax(pyr, T, P):
    n = T * P
    raw = pyr.stats[16 * n:24 * n].cpu().numpy().view(np.uint32)
    return raw[:n].copy(), raw[n:].copy()


@pytest.mark.gpu
@pytest.mark.parametrize('h0,ws,method', CASES, ids=lambda v: str(v))
@pytest.mark.parametrize('kind', KINDS)
def test_f16_level_kernel_vs_oracle(kind, h0, ws, method, pinned_pow):
    import torch
    from deepmatching_stereo_matching_amd import _lib as L
    from deepmatching_stereo_matching_amd import engine
    a, b = images(kind, h0, ws)
    org = ORIGINS[h0]
    T, P = len(org), h0 * W0
    batch = engine.TileBatch(a, b, org, h0, W0, ws, method)
    assert took_f16_path(L, batch), 'the batch did not take the f16 path'
    ref = []
    for r, c in org:
        l0 = O.corr_l0(_crop(a, r, c, h0, W0, ws), _crop(b, r, c, h0, W0, ws), ws, _feat(method))
        lev, _, _ = O.pyramid(l0)
        ref.append((l0.reshape(P, P), lev, O.match(lev, sub_pix=True)))
    nlev = len(ref[0][1])
    want_match = np.stack([m for _, _, m in ref])
    # level 1 stored (modes 0, 1) and not stored (mode 2), then both outputs of the fused call
    for mode in (0, 1, 2):
        pyr = engine.DevicePyramid(batch, fuse_level2=mode)
        assert pyr.nlev == nlev and (pyr.levels[1] is None) == (mode == 2)
        _same(pyr.match(sub_pix=True).cpu().numpy(), want_match)
        for k in range(1, nlev):
            got = pyr.level(k).cpu().numpy()
            for t in range(T):
                _same(got[t], ref[t][1][k].reshape(got[t].shape))
        del pyr
    pyr = engine.DevicePyramid(batch, fuse_level2=2)
    l1, l2 = torch.empty_like(pyr.level(1)), torch.empty_like(pyr.levels[2])
    lib = L.load()
    L.check(lib.dm_corr_level12(batch.ref(), L.ptr(pyr.stats), L.ptr(l1), L.ptr(l2), L.stream_handle()))
    for t in range(T):
        _same(l1[t].cpu().numpy(), ref[t][1][1].reshape(l1[t].shape))
        _same(l2[t].cpu().numpy(), ref[t][1][2].reshape(l2[t].shape))
    # rmin / rmax left by the f16 kernel: the min/max-known volume is the oracle's level 0 ...
    assert pyr._have_minmax
    vol = torch.empty((T, P, P), dtype=torch.float32, device='cuda')
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN, L.ptr(vol),
                                  L.stream_handle()))
    got = vol.cpu().numpy()
    for t in range(T):
        _same(got[t], ref[t][0])
    # ... and they are, bit for bit, what the standalone volume's own i8 sweep finds
    mn, mx = stats_minmax(pyr, T, P)
    fresh = engine.DevicePyramid(batch, build=False).compute_stats()
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh.stats), 0, L.ptr(vol), L.stream_handle()))
    torch.cuda.synchronize()
    mn2, mx2 = stats_minmax(fresh, T, P)
    assert np.array_equal(mn, mn2) and np.array_equal(mx, mx2)


def test_predicate_is_the_w0_128_packed_y_shape():
    from deepmatching_stereo_matching_amd import _lib as L
    lib = L.load()

    def f16(h0, w0, ws):
        t = L.DmTiles(1, 1, w0 + ws, w0 + ws, 1, 2, h0, w0, ws, 5)
        return lib.dm_level_num_f16(ctypes.byref(t))
    for h0, w0, ws, want in [(16, 128, 5, 1), (32, 128, 3, 1), (4, 128, 1, 1), (128, 128, 5, 1),
                             (16, 128, 7, 0), (16, 64, 5, 0), (16, 256, 5, 0), (18, 128, 5, 0),
                             (16, 96, 5, 0)]:
        assert f16(h0, w0, ws) == want, (h0, w0, ws)
    assert lib.dm_level_num_f16(None) == 0
