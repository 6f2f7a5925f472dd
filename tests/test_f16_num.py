"""num = n * sum_k T'_k I'_k - sum(T') sum(I') as ONE v_mfma_f32_16x16x32_f16 (csrc/dm_mfma.h,
num_tile_f16; DESIGN.md section 2, 'num from the f16 MFMA').

CPU: the argument that makes the float32 result exact whatever order the matrix core adds in --
every K slot is an integer binary16 holds, the four digit products sum to -sT sI, and the mass
of the positive and of the negative terms each stay below 2^24.

GPU: dm_debug_num_tile_f16 -- the device helpers a level kernel would use (operand builders,
digit split, MFMA call) -- against int64 numpy, with exact equality: the one thing the proof
assumes about the hardware is that the f16 MFMA returns the exact sum when every partial sum
is representable.

Cases (ws 3 and 5): random taps; every tap at an extreme, in every sign pairing of patch and
window and per tap; nearly flat patches and windows with a few flipped taps; and the 16 patch /
window pairs of the largest one-signed mass a CPU search found
(tests/golden/f16_num_worst16.npz, make_golden_f16_num.py)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'f16_num_worst16.npz')
KINDS = ('random', 'extreme_pairs', 'extreme_taps', 'near_flat', 'opposed')
TILES = 6   # 16 x 16 tiles per kind on the GPU


def taps(kind, ws, tiles, rng):
    """(T, I): int64 [tiles][16][n] in [-128, 127] -- 16 patches and 16 windows per tile"""
    n, sh = ws * ws, (tiles, 16, ws * ws)
    if kind == 'random':
        return rng.integers(-128, 128, sh), rng.integers(-128, 128, sh)
    if kind == 'extreme_pairs':   # whole patches / windows at one extreme: all four pairings
        sel = np.arange(16)
        T = np.where((sel & 1)[None, :, None] != 0, 127, -128) * np.ones(sh, np.int64)
        I = np.where((sel & 2)[None, :, None] != 0, 127, -128) * np.ones(sh, np.int64)
        return T, I
    if kind == 'extreme_taps':    # every tap at an extreme of its own
        return rng.choice([-128, 127], sh), rng.choice([-128, 127], sh)
    if kind == 'near_flat':       # a constant with 0 .. 3 taps flipped to the far extreme
        def flat():
            base = rng.choice([-128, -127, -1, 0, 1, 100, 126, 127], (tiles, 16, 1))
            k = rng.integers(0, 4, (tiles, 16, 1))
            flip = np.argsort(rng.random(sh), axis=2) < k
            return np.where(flip, np.where(base >= 0, -128, 127), base * np.ones(sh, np.int64))
        return flat(), flat()
    if kind == 'opposed':         # runs of one extreme against runs of the other
        k = rng.integers(0, n + 1, (tiles, 16, 1))
        k2 = rng.integers(0, n + 1, (tiles, 16, 1))
        idx = np.arange(n)[None, None, :]
        return np.where(idx < k, 127, -128), np.where(idx < k2, -128, 127)
    raise ValueError(kind)


def digits(s):
    hi = 64 * np.floor_divide(s, 64)
    return hi, s - hi


def terms(T, I, ws):
    """the n + 4 integer products of every (patch, window) pair of every tile: [tiles][16][16][n + 4]"""
    tap = (ws * T)[:, :, None, :] * (ws * I)[:, None, :, :]
    th, tl = digits(T.sum(2))
    ih, il = digits(I.sum(2))
    a = np.stack([th, th, tl, tl], 2)[:, :, None, :]
    b = np.stack([-ih, -il, -ih, -il], 2)[:, None, :, :]
    return np.concatenate([tap, a * b], 3).astype(np.int64)


def num_ref(T, I, ws):
    n = ws * ws
    return n * np.einsum('tpk,tqk->tpq', T, I) - T.sum(2)[:, :, None] * I.sum(2)[:, None, :]


def golden():
    z = np.load(GOLD)
    return z['T'].astype(np.int64)[None], z['I'].astype(np.int64)[None]   # one tile, ws = 5


def all_cases(ws, tiles, seed):
    rng = np.random.default_rng(seed)
    out = [(k, *taps(k, ws, tiles, rng)) for k in KINDS]
    if ws == 5:
        out.append(('golden', *golden()))
    return out


@pytest.mark.parametrize('ws', [3, 5])
def test_operands_fit_binary16_and_masses_stay_below_2_24(ws):
    worst = 0
    for kind, T, I in all_cases(ws, 400, seed=ws):
        n = ws * ws
        assert np.abs(ws * T).max() <= 640 and np.abs(ws * I).max() <= 640   # integers <= 2048: exact
        for s in (T.sum(2), I.sum(2)):
            hi, lo = digits(s)
            assert np.array_equal(hi + lo, s) and lo.min() >= 0 and lo.max() <= 63
            assert np.abs(hi).max() <= 3200 and not (hi % 64).any()          # <= 50 * 64: exact
            assert np.array_equal(hi.astype(np.float16).astype(np.int64), hi)
        t = terms(T, I, ws)
        assert t.shape[-1] == n + 4 <= 32
        assert np.array_equal(t.sum(3), num_ref(T, I, ws)), kind             # the digit identity
        sp, sm = np.where(t > 0, t, 0).sum(3), -np.where(t < 0, t, 0).sum(3)
        assert np.abs(t.sum(3)).max() <= n * n * 255 * 255 // 4
        assert (sp + sm).max() <= n * n * 128 * 128 + 3263 ** 2
        worst = max(worst, int(sp.max()), int(sm.max()))
        assert worst < 2 ** 24, kind
    print('ws %d: largest one-signed mass %d = %.3f * 2^24' % (ws, worst, worst / 2.0 ** 24))


def test_golden_fixture_is_the_heavy_end_of_the_search():
    T, I = golden()
    t = terms(T, I, 5)
    d = np.arange(16)
    sp, sm = np.where(t > 0, t, 0).sum(3)[0, d, d], -np.where(t < 0, t, 0).sum(3)[0, d, d]
    assert np.maximum(sp, sm).min() > 0.55 * 2 ** 24   # pair i = (patch i, window i) of the search


@pytest.fixture(scope='module')
def lib():
    from deepmatching_stereo_matching_amd import _lib as L
    return L


def _dev(lib, T, I, ws):
    import torch
    p = torch.from_numpy(np.ascontiguousarray(T + 128, dtype=np.uint8)).cuda()
    w = torch.from_numpy(np.ascontiguousarray(I + 128, dtype=np.uint8)).cuda()
    out = torch.full((16, 16), float('nan'), dtype=torch.float32, device='cuda')
    lib.check(lib.load().dm_debug_num_tile_f16(lib.ptr(p), lib.ptr(w), ws, lib.ptr(out), lib.stream_handle()),
              'dm_debug_num_tile_f16')
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('ws', [3, 5])
def test_f16_mfma_num_is_exact(lib, ws):
    for kind, T, I in all_cases(ws, TILES, seed=100 + ws):
        ref = num_ref(T, I, ws)
        for t in range(T.shape[0]):
            got = _dev(lib, T[t], I[t], ws)
            assert got.dtype == np.float32
            # exact: the float32 IS the integer (|num| < 2^24), not close to it
            assert np.array_equal(got.astype(np.float64), ref[t].astype(np.float64)), (
                '%s ws %d tile %d: max |dev - ref| = %g' % (kind, ws, t, np.abs(got - ref[t]).max()))
            # a zero num is +0, as the i8 path's fma(sT, -sI, n * acc) gives it (y = num * b_q
            # would carry a -0 into the pooling maxima)
            assert not np.signbit(got[ref[t] == 0]).any(), '%s ws %d tile %d: -0' % (kind, ws, t)


@pytest.mark.gpu
def test_f16_num_tile_layout_is_patch_rows_by_window_columns(lib):
    # asymmetric data: a swapped row / column map or a wrong K order cannot pass
    rng = np.random.default_rng(7)
    T, I = rng.integers(-128, 128, (1, 16, 25)), rng.integers(-128, 128, (1, 16, 25))
    got, ref = _dev(lib, T[0], I[0], 5), num_ref(T, I, 5)[0]
    assert not np.array_equal(ref, ref.T)
    assert np.array_equal(got.astype(np.int64), ref)


def test_debug_entry_validates_its_arguments(lib):
    import ctypes
    h = lib.load()
    one = ctypes.c_void_p(8)
    assert h.dm_debug_num_tile_f16(None, one, 5, one, None) == lib.DM_ERR_ARG
    assert h.dm_debug_num_tile_f16(one, one, 7, one, None) == lib.DM_ERR_UNSUPPORTED   # 49 + 4 > 32 slots
    assert h.dm_debug_num_tile_f16(one, one, 4, one, None) == lib.DM_ERR_UNSUPPORTED
