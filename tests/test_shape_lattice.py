"""Every kernel instance the launchers can pick, on at least one small tile, against the oracle.

The library takes any tile with w0 in {32, 64, 128, 256}, h0 % 4 == 0 and ws <= 15 on its MFMA
paths (mf16_eligible, csrc/dm_mfma.h), and launch_level / launch_volume_ls / launch_volume_mfq
(csrc/dm_kernels.hip) turn the shape into one of several dozen template instances.  The cases
below are the smallest tiles that reach each instance, plus the edges the row-pair sweeps have
(h0 = 4 and 8: every row both top and bottom border), the runtime window side (ws != 5) on the
GW = 4 kernels, h0 = 3 w0 (a 3 x 1 top level), a grid that is no multiple of 8 (wg_logical's
identity branch), and an odd image pitch with odd tile origins on the dword paths.

Comparison rules are DESIGN.md section 2's: with the pinned pow every output equals the CPU
oracle bit for bit, the binary16 volume equals np.float16 of the oracle's level 0.  No tolerance.

test_ledger_covers_every_dispatch_key (CPU) restates the launch rules in dispatch_key() and
fails when the launchers' enumeration produces an instance no case here runs.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O

ORIGINS = [(0, 0), (3, 7), (2, 5)]     # T = 3, odd offsets; the image pitch w0 + ws + 6 is odd
STREAM_ABOVE_P = 8192                  # oracle level 0 not materialised above this many patches

# (h0, w0, ws): the GW = 2 instances of k_level1_mfq no other test launches (KS, NW in comments)
GW2_CASES = [(8, 64, 7),      # (1, 2)
             (8, 256, 7),     # (1, 8)
             (8, 32, 9),      # (2, 1)
             (8, 64, 11),     # (2, 2)
             (8, 256, 9),     # (2, 8)
             (8, 32, 13),     # (3, 1)
             (8, 128, 13),    # (3, 4)
             (8, 256, 13),    # (3, 8)
             (8, 32, 15),     # (4, 1)
             (8, 128, 15),    # (4, 4)
             (8, 256, 15)]    # (4, 8)
# the GW = 4 kernels (C2 / C3 / C5 instances) at small h0 and with the runtime window side;
# (4, 64, 3) with T = 3 is a grid of 12 workgroups: wg_logical's identity branch
GW4_CASES = [(4, 64, 5), (4, 64, 3), (8, 64, 1),
             (4, 128, 5), (8, 128, 3), (16, 128, 1),
             (4, 256, 5), (8, 256, 3), (16, 256, 1)]
NPOT_CASES = [(96, 32, 5), (192, 64, 3)]          # h0 = 3 w0: the top level is 3 x 1
# instances other tests reach at larger h0; run here too, so the ledger below closes on this
# file's cases alone
LEDGER_CASES = [(8, 32, 3), (8, 32, 7), (8, 128, 7), (8, 128, 9), (8, 64, 13), (8, 64, 15)]
LEVEL_CASES = GW2_CASES + GW4_CASES + NPOT_CASES + LEDGER_CASES
FLAT_CASES = [c for c in GW4_CASES if c[2] in (3, 5)]

VOLUME_CASES = [(8, 256, 7), (8, 256, 9), (8, 256, 13), (8, 256, 15), (8, 128, 13), (8, 32, 13),
                (4, 64, 5), (4, 128, 3), (4, 256, 5), (8, 32, 3),
                (8, 64, 7), (8, 64, 9), (8, 64, 15)]   # the last three: ledger (LS_ = true, KS 1 / 2 / 4)

FUSED_PREDICATE_CASES = [(16, 192, 5), (32, 96, 5), (16, 320, 3), (8, 512, 5), (16, 64, 5), (8, 128, 7),
                         (4, 256, 3)]


def dispatch_key(h0, w0, ws):
    """(level kernel key, volume kernel key) of an MFMA-eligible tile: a restatement of the
    launch rules of csrc/dm_kernels.hip.

    level:  (launcher branch, KS, GW, NW, ws == 5)
        KS, NW, GW          launch_level, mfq_nw (strip_shape)
        packed y (ws <= 5)  launch_level's DM_MQ(1, 1, true)
        'c5' / 'c2' / 'c3'  level_kernel's LK_STRIP (w0 = 256 / 64) and LK_MFQ_F16 (w0 = 128):
                            KS == 1, GW == 4, NW = 4 / 1 / 2
        'mq_y' / 'mq'       LK_MFQ, the DM_MQ table (GW = 2; KS >= 2 only without packed y)
        ws == 5             the compile-time window side of fill_ptab / k_prep_strips /
                            k_prep_windows16 (dm_mfma.h, dm_strip.h, dm_corr_stats)
    volume: ('ls', G, None) launch_volume_ls (volume_ls_shape), or
            ('mfq', KS, LS_) launch_volume_mfq (LS_ = w0 <= 128, GW == 2 only)"""
    if not (h0 % 4 == 0 and w0 in (32, 64, 128, 256) and 1 <= ws <= 15 and ws % 2 == 1):
        raise ValueError('not an MFMA shape (mf16_eligible, dm_mfma.h): %r' % ((h0, w0, ws),))
    G, KS = w0 // 16, (ws * ws + 63) // 64
    g4 = ws * ws <= 25 and G % 4 == 0 and G // 4 in (1, 2, 4)
    NW = G // 4 if g4 else min(G // 2, 8)
    GW = G // NW
    if KS == 1 and GW == 4:
        branch = {4: 'c5', 1: 'c2', 2: 'c3'}[NW]
    else:
        assert GW == 2 and NW in (1, 2, 4, 8) and (KS == 1 or ws > 5)
        branch = 'mq_y' if ws <= 5 else 'mq'
    level = (branch, KS, GW, NW, ws == 5)
    bpt = (h0 // 4) * (w0 // 4)
    if ws <= 5 and bpt % 8 == 0:
        volume = ('ls', G, None)
    else:
        assert GW == 2, 'ws <= 5 with cell blocks per tile % 8 != 0: the generic volume kernels'
        volume = ('mfq', KS, w0 <= 128)
    return level, volume


def test_ledger_covers_every_dispatch_key():
    """Every kernel instance the launchers pick over w0 in {32, 64, 128, 256} x ws in {1, 3, ..,
    15} is the instance of at least one case of this file: a launcher instance added without a
    lattice case fails here, on the CPU."""
    level_have = {dispatch_key(*c)[0] for c in LEVEL_CASES}
    volume_have = {dispatch_key(*c)[1] for c in VOLUME_CASES}
    missing = []
    for w0 in (32, 64, 128, 256):
        for ws in range(1, 16, 2):
            level, volume = dispatch_key(8, w0, ws)
            if level not in level_have:
                missing.append(('level', w0, ws, level))
            if volume not in volume_have:
                missing.append(('volume', w0, ws, volume))
    assert not missing, missing
    # the GW = 2 cases are one instance each (no case shadows another)
    assert len({dispatch_key(*c)[0] for c in GW2_CASES}) == len(GW2_CASES)
    # (4, 64, 3) at T = 3: grid = T * bpt / C2_NB = 12, not a multiple of 8 (wg_logical)
    assert (len(ORIGINS) * (4 // 4) * (64 // 4) // 4) % 8 != 0


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=True), 'max |d| = %r' % np.nanmax(np.abs(a - b))


@pytest.fixture(scope='module')
def pinned_pow():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    O.set_pow_mode('pinned')
    yield
    O.set_pow_mode('libm')


def _feat(method):
    return 'cv2.TM_CCOEFF_NORMED' if method == 5 else 'cv2.TM_CCOEFF'


def _images(h0, w0, ws):
    """One tile padded by 3 rows and 7 columns: width w0 + ws + 6 (odd), as ORIGINS needs."""
    from deepmatching_stereo_matching_amd.synthetic import stereo_pair
    return stereo_pair(h0 + ws - 1 + 3, w0 + ws - 1 + 7, seed=5 * h0 + w0 + 3 * ws, dx=3)


def flat_images(h0, w0, ws):
    """_images with a constant (ws + 3) x (ws + 5) block in image 1 (constant patches: NaN maps
    with NORMED) that every tile of ORIGINS holds at least one whole patch row of, and a flat
    window region in image 2 (dI == 0 -> 0)."""
    a, b = _images(h0, w0, ws)
    a, b = a.copy(), b.copy()
    a[3:3 + ws + 3, 20:20 + ws + 5] = 200
    b[1:1 + ws + 2, 36:36 + ws + 9] = 90
    return a, b


def _crop(img, r, c, h0, w0, ws):
    return img[r:r + h0 + ws - 1, c:c + w0 + ws - 1]


def oracle_tile(a, b, r, c, h0, w0, ws, method):
    """(levels, match with sub-pixel) of one tile; levels[0] is None where level 0 is streamed."""
    ca, cb = _crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws)
    if h0 * w0 > STREAM_ABOVE_P:
        lev, _, _ = O.pyramid_stream(ca, cb, ws, _feat(method))
        return lev, O.match_stream(ca, cb, ws, lev, sub_pix=True, feature=_feat(method))
    lev, _, _ = O.pyramid(O.corr_l0(ca, cb, ws, _feat(method)))
    return lev, O.match(lev, sub_pix=True)


def check_levels_and_match(a, b, h0, w0, ws, method, ref=None):
    """All three DevicePyramid modes and the direct two-output dm_corr_level12 call against the
    oracle: every level >= 1 of every tile, and match(sub_pix=True)."""
    from deepmatching_stereo_matching_amd import _lib as L
    from deepmatching_stereo_matching_amd import engine
    if ref is None:
        ref = [oracle_tile(a, b, r, c, h0, w0, ws, method) for r, c in ORIGINS]
    nlev = len(ref[0][0])
    want_match = np.stack([m for _, m in ref])
    assert engine.level12_fused(h0, w0, ws)
    for mode in (0, 1, 2):
        pyr = engine.DevicePyramid(engine.TileBatch(a, b, ORIGINS, h0, w0, ws, method), fuse_level2=mode)
        assert pyr.nlev == nlev
        assert (pyr.levels[1] is None) == (mode == 2)
        # (mode 2: matching evaluates level 1 on demand, before level(1) below stores it)
        _same(pyr.match(sub_pix=True).cpu().numpy(), want_match)
        for k in range(1, nlev):
            got = pyr.level(k).cpu().numpy()
            for t in range(len(ORIGINS)):
                _same(got[t], ref[t][0][k].reshape(got[t].shape))
        if mode == 2:   # both outputs at once
            l1 = torch.empty_like(pyr.levels[1])
            l2 = torch.empty_like(pyr.levels[2])
            L.check(L.load().dm_corr_level12(pyr.b.ref(), L.ptr(pyr.stats), L.ptr(l1), L.ptr(l2),
                                             L.stream_handle()))
            for t in range(len(ORIGINS)):
                _same(l1[t].cpu().numpy(), ref[t][0][1].reshape(l1[t].shape))
                _same(l2[t].cpu().numpy(), ref[t][0][2].reshape(l2[t].shape))
        del pyr


@pytest.mark.gpu
@pytest.mark.parametrize('h0,w0,ws,method', [c + (5 - i % 2,) for i, c in enumerate(LEVEL_CASES)],
                         ids=lambda v: str(v))
def test_level_lattice_vs_oracle(h0, w0, ws, method, pinned_pow):
    """Levels >= 1 and matching of every lattice case, fuse_level2 = 0 / 1 / 2, bit for bit.
    (ws = 1: every NORMED map is NaN -- the NaN writes and the argmax over NaN.)"""
    a, b = _images(h0, w0, ws)
    check_levels_and_match(a, b, h0, w0, ws, method)


@pytest.mark.gpu
@pytest.mark.parametrize('h0,w0,ws', FLAT_CASES, ids=lambda v: str(v))
def test_level_lattice_flat_patches(h0, w0, ws, pinned_pow):
    """The GW = 4 kernels with constant patches (NaN child maps, written by the fused kernel
    itself: norm_clamp in dm_mfma.h) and flat windows, NORMED.  Every tile's level 2 holds
    some NaN and is not all NaN, so the comparison is not vacuous."""
    a, b = flat_images(h0, w0, ws)
    ref = [oracle_tile(a, b, r, c, h0, w0, ws, 5) for r, c in ORIGINS]
    for lev, _ in ref:
        assert np.isnan(lev[2]).any() and not np.isnan(lev[2]).all()
    check_levels_and_match(a, b, h0, w0, ws, 5, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('method', [5, 4])
@pytest.mark.parametrize('h0,w0,ws', VOLUME_CASES, ids=lambda v: str(v))
def test_volume_lattice_vs_oracle(h0, w0, ws, method, pinned_pow):
    """The level-0 volume kernels: float32 == oracle, binary16 == np.float16(oracle), and the
    min/max-known call after the level kernel == the standalone call, on every tile; a constant
    patch (NaN row of the NORMED volume) included."""
    from deepmatching_stereo_matching_amd import _lib as L
    from deepmatching_stereo_matching_amd import engine
    a, b = _images(h0, w0, ws)
    a = a.copy()
    a[2:2 + ws, 5:5 + ws] = 77          # tile 0's patch (2, 5) is constant
    P, T = h0 * w0, len(ORIGINS)
    batch = engine.TileBatch(a, b, ORIGINS, h0, w0, ws, method)
    lib = L.load()
    fresh = engine.DevicePyramid(batch, build=False).compute_stats()
    v32 = torch.empty((T, P, P), dtype=torch.float32, device='cuda')
    v16 = torch.empty((T, P, P), dtype=torch.float16, device='cuda')
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh.stats), 0, L.ptr(v32), L.stream_handle()))
    # (binary16 standalone: on a second fresh workspace, so it sweeps for its own min / max)
    fresh16 = engine.DevicePyramid(batch, build=False).compute_stats()
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(fresh16.stats), L.DM_VOLUME_F16, L.ptr(v16),
                                  L.stream_handle()))
    r32, r16 = v32.cpu().numpy(), v16.cpu().numpy()
    assert r16.dtype == np.float16
    for t, (r, c) in enumerate(ORIGINS):
        l0 = O.corr_l0(_crop(a, r, c, h0, w0, ws), _crop(b, r, c, h0, w0, ws), ws, _feat(method)).reshape(P, P)
        _same(r32[t], l0)
        _same(r16[t], l0.astype(np.float16))
    if method == 5:
        assert np.isnan(r32[0][2 * w0 + 5]).all() and not np.isnan(r32[0]).all()
    # min / max left in the stats workspace by the level kernel
    pyr = engine.DevicePyramid(batch, fuse_level2=2)
    assert pyr._have_minmax
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN, L.ptr(v32),
                                  L.stream_handle()))
    L.check(lib.dm_corr_volume_ex(batch.ref(), L.ptr(pyr.stats), L.DM_VOLUME_MINMAX_KNOWN | L.DM_VOLUME_F16,
                                  L.ptr(v16), L.stream_handle()))
    _same(v32.cpu().numpy(), r32)
    _same(v16.cpu().numpy(), r16)


@pytest.mark.gpu
@pytest.mark.parametrize('h0,w0,ws', FUSED_PREDICATE_CASES, ids=lambda v: str(v))
def test_level12_fused_predicate(h0, w0, ws, pinned_pow):
    """engine.level12_fused == 'a mode-2 DevicePyramid does not store level 1' == 'dm_corr_level12
    takes the shape'; where it does not, the stored level 1 and level 2 still equal the oracle."""
    from deepmatching_stereo_matching_amd import _lib as L
    from deepmatching_stereo_matching_amd import engine
    from deepmatching_stereo_matching_amd.synthetic import stereo_pair
    a, b = stereo_pair(h0 + ws - 1, w0 + ws - 1, seed=h0 + w0 + ws, dx=2)
    fused = engine.level12_fused(h0, w0, ws)
    batch = engine.TileBatch(a, b, [(0, 0)], h0, w0, ws, 5)
    pyr = engine.DevicePyramid(batch, fuse_level2=2)
    assert (pyr.levels[1] is None) == fused
    l2 = torch.empty_like(pyr.levels[2])
    rc = L.load().dm_corr_level12(batch.ref(), L.ptr(pyr.stats), None, L.ptr(l2), L.stream_handle())
    assert rc in (L.DM_OK, L.DM_ERR_UNSUPPORTED), L.last_error()
    assert (rc != L.DM_ERR_UNSUPPORTED) == fused
    lev, _, _ = O.pyramid(O.corr_l0(a, b, ws))
    for k in (1, 2):
        got = pyr.level(k)[0].cpu().numpy()
        _same(got, lev[k].reshape(got.shape))
    if fused:
        _same(l2[0].cpu().numpy(), lev[2].reshape(l2[0].shape))
