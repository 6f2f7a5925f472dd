"""tests/golden/f16_num_worst16.npz: the 16 (patch, window) tap pairs, ws = 5, of the largest
one-signed mass max(S+, S-) among the n + 4 integer products that v_mfma_f32_16x16x32_f16 adds
up to num (csrc/dm_mfma.h, num_tile_f16), from a CPU search over 2.4 M random and adversarial
tap sets.  T[i], I[i] (int16 [16][25], values in [-128, 127]) are pair i; tests/test_f16_num.py
runs all 256 combinations of them on the GPU.

    python tests/golden/make_golden_f16_num.py
"""
import os

import numpy as np

WS, N = 5, 400000


def digits(s):
    hi = 64 * np.floor_divide(s, 64)
    return hi, s - hi


def masses(T, I):
    tap = (WS * T) * (WS * I)
    th, tl = digits(T.sum(1))
    ih, il = digits(I.sum(1))
    t = np.concatenate([tap, np.stack([th * -ih, th * -il, tl * -ih, tl * -il], 1)], 1)
    assert np.array_equal(t.sum(1), WS * WS * (T * I).sum(1) - T.sum(1) * I.sum(1))
    return np.maximum(np.where(t > 0, t, 0).sum(1), -np.where(t < 0, t, 0).sum(1))


def main():
    rng = np.random.default_rng(0)
    n, sh = WS * WS, (N, WS * WS)
    idx = np.arange(n)[None, :]
    best = []
    for kind in range(6):
        if kind == 0:
            T, I = rng.integers(-128, 128, sh), rng.integers(-128, 128, sh)
        elif kind == 1:
            T, I = rng.choice([-128, 127], sh), rng.choice([-128, 127], sh)
        elif kind == 2:
            T = np.where(rng.random(sh) < 0.9, 127, -128)
            I = np.where(idx < rng.integers(0, n + 1, (N, 1)), 127, -128)
        elif kind == 3:
            T = np.where(idx < rng.integers(0, n + 1, (N, 1)), 127, -128)
            I = np.where(idx < rng.integers(0, n + 1, (N, 1)), -128, 127)
        elif kind == 4:
            T, I = np.full(sh, 127), rng.choice([-128, 127], sh, p=[0.8, 0.2])
        else:
            T, I = np.full(sh, -128), rng.choice([-128, 127], sh)
        T, I = T.astype(np.int64), I.astype(np.int64)
        m = masses(T, I)
        assert m.max() < 2 ** 24
        # distinct tap sets only: the structured kinds repeat themselves
        _, first = np.unique(np.concatenate([T, I], 1), axis=0, return_index=True)
        for i in first[np.argsort(-m[first])[:16]]:
            best.append((int(m[i]), T[i], I[i]))
    best.sort(key=lambda b: -b[0])
    best = best[:16]
    print('one-signed masses:', [b[0] for b in best], 'largest = %.3f * 2^24' % (best[0][0] / 2.0 ** 24))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'f16_num_worst16.npz')
    np.savez_compressed(out, T=np.stack([b[1] for b in best]).astype(np.int16),
                        I=np.stack([b[2] for b in best]).astype(np.int16),
                        mass=np.array([b[0] for b in best], np.int64))


if __name__ == '__main__':
    main()
