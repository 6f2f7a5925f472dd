"""Generate the Matching._filter fixtures (tests/golden/filter_*.npz) by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_filter.py

Same method as make_golden.py: ``oracle/cv2_shim`` in front of ``sys.path``, the reference
modules ``misc.Correlation_map``, ``misc.Matching`` and ``misc.image_cut_solver`` imported
unchanged, joblib on the threading backend.  Only inputs and outputs are written (npz data).

The pairs are the ones on which the filter acts ("Where Matching._filter acts"):
independent uniform noise, rolled noise, the sinusoidal texture, one TM_CCOEFF pair.  Per pair
the reference's ``Matching(co, filter_window_size=w, filtering=True, filtering_num=n,
filtering_mode=m, sub_pix=s)()`` is stored for a lattice of (w, m, n) and both s.  Many
settings give the same map (a count <= 2 runs no pass on a full square pyramid, windows 1 and
2 reach no neighbour), so the file holds every distinct result once:

    keys   [N] str   'w<window>_<mode>_n<count>', and 'none' for filtering=False
    uid    [N] int   index of key k's result in nosub / sub
    nosub  [U][3][h][w]   sub_pix=False result (row, col, score)
    sub    [U][2][h][w]   row, col of the sub_pix=True result (its score plane equals nosub's)

Every pair holds the full lattice: windows 1..7 x both modes x counts {1, 2, 3, 4, nlev,
nlev + 2}, the reference driver's setting (ex_deepmatching_rawinput.py: window 3, count 4,
median) among them.

filter_edges.npz records what the reference does outside the lattice (see main()).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('DM_REFERENCE', '/root/reference')

sys.path.insert(0, os.path.join(REPO, 'oracle', 'cv2_shim'))
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
sys.dont_write_bytecode = True

from joblib import parallel_backend  # noqa: E402
from misc.Correlation_map import Correlation_map  # noqa: E402
from misc.Matching import Matching  # noqa: E402
from misc.image_cut_solver import ImageCutSolver  # noqa: E402

from deepmatching_stereo_matching_amd.synthetic import stereo_pair  # noqa: E402

FEATURES = {'normed': 'cv2.TM_CCOEFF_NORMED', 'ccoeff': 'cv2.TM_CCOEFF'}
WINDOWS = (1, 2, 3, 4, 5, 6, 7)
FMODES = ('median', 'average')


def key(w, mode, n):
    return 'w%d_%s_n%d' % (w, mode, n)


def counts(nlev):
    return tuple(dict.fromkeys((1, 2, 3, 4, nlev, nlev + 2)))


def lattice(nlev):
    return [(w, m, n) for w in WINDOWS for m in FMODES for n in counts(nlev)]


def run_pair(img1, img2, ws, feature):
    with parallel_backend('threading'):
        co = Correlation_map(img1, img2, window_size=ws, feature_name=FEATURES[feature])
        levels = co()
    nlev = len(levels)
    keys, uid, nosub, sub = [], [], [], []

    def add(k, **kw):
        a = Matching(co, sub_pix=False, **kw)()
        b = Matching(co, sub_pix=True, **kw)()
        assert np.array_equal(a[2], b[2], equal_nan=True)
        for u in range(len(nosub)):
            if np.array_equal(nosub[u], a, equal_nan=True) and np.array_equal(sub[u], b[:2], equal_nan=True):
                break
        else:
            u = len(nosub)
            nosub.append(a.copy())
            sub.append(b[:2].copy())
        keys.append(k)
        uid.append(u)

    add('none')
    for w, m, n in lattice(nlev):
        add(key(w, m, n), filter_window_size=w, filtering=True, filtering_num=n, filtering_mode=m)
    return {'img1': img1, 'img2': img2, 'ws': np.int64(ws), 'feature': np.array(FEATURES[feature]),
            'nlev': np.int64(nlev), 'keys': np.array(keys), 'uid': np.array(uid, dtype=np.int64),
            'nosub': np.array(nosub), 'sub': np.array(sub)}


def save(name, d):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **d)
    print('%-28s %8.1f KB' % (name, os.path.getsize(path) / 1024))


def raised(fn):
    """'' when fn() returns, else 'ExceptionType: message' of what it raised."""
    try:
        fn()
    except Exception as e:  # noqa: BLE001 -- the point is to record whatever the reference raises
        return '%s: %s' % (type(e).__name__, e)
    return ''


class Levels:
    """What Matching reads of a Correlation_map: co_map_list and N_map."""

    def __init__(self, levels):
        self.co_map_list = levels
        self.N_map = 2 ** (len(levels) - 1)


def steered_levels(sides=(16, 8, 4)):
    """A hand-made co_map_list that drives every position as far towards a border as Matching
    allows: map (i, j) of each level peaks at a target far outside the map -- down-right for
    the upper half of the rows, up-left for the lower half -- so every step moves by one towards
    it until the border stops it, and the two halves meet in a row of large opposite
    displacements for the filter to act on."""
    out = []
    for n in sides:
        lv = np.empty((n, n, n, n))
        for i in range(n):
            t = 4 * n if i < n // 2 else -4 * n
            for j in range(n):
                for r in range(n):
                    for c in range(n):
                        lv[i, j, r, c] = 1.0 / (1.0 + (abs(r - (i + t)) + abs(c - (j + t))) / (8.0 * n))
        out.append(lv)
    return out


def main():
    rng = np.random.default_rng(7)
    # S = 16: two independent uniform-noise images
    a = rng.integers(0, 256, (20, 20), dtype=np.uint8)
    b = rng.integers(0, 256, (20, 20), dtype=np.uint8)
    save('filter_s16_noise', run_pair(a, b, 5, 'normed'))
    # S = 8: the same, smallest tile whose full pyramid runs two passes at window 3
    a = rng.integers(0, 256, (10, 10), dtype=np.uint8)
    b = rng.integers(0, 256, (10, 10), dtype=np.uint8)
    save('filter_s8_noise', run_pair(a, b, 3, 'normed'))
    # S = 16, TM_CCOEFF, ws 3: noise against itself rolled by 3 columns and -2 rows
    a = rng.integers(0, 256, (18, 18), dtype=np.uint8)
    b = np.roll(np.roll(a, 3, axis=1), -2, axis=0)
    save('filter_s16_ccoeff', run_pair(a, b, 3, 'ccoeff'))
    # S = 32: the sinusoidal texture of pair_s32_ws5_sin
    a, b = stereo_pair(36, 36, seed=11, dx=3, max_disp=8, sinusoidal=True)
    save('filter_s32_sin', run_pair(a, b, 5, 'normed'))
    # S = 32: noise, img2 = img1 rolled by -7 columns and -5 rows
    a = rng.integers(0, 256, (36, 36), dtype=np.uint8)
    b = np.roll(np.roll(a, -7, axis=1), -5, axis=0)
    save('filter_s32_roll', run_pair(a, b, 5, 'normed'))

    # --- ImageCutSolver with the filter on: 3 x 3 overlapping S = 16 tiles of a noise image
    a = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    b = np.roll(np.roll(a, -3, axis=1), 2, axis=0)
    cut = {'img1': a, 'img2': b, 'image_size': np.array([16, 16]), 'stride': np.array([12, 12]),
           'ws': np.int64(5), 'modes': np.array(['elevation', 'elevation2', 'distance'])}
    for name, kw in (('w3_average', {}),                                   # the default mode
                     ('w3_median', {'filtering_mode': 'median'}),
                     ('w5_median', {'filtering_mode': 'median', 'filtering_window_size': 5}),
                     ('off', None)):
        with parallel_backend('threading'):
            if kw is None:
                s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 12], window_size=5,
                                   degree_map_mode=['elevation', 'elevation2', 'distance'])
            else:
                s = ImageCutSolver(a, b, image_size=[16, 16], stride=[12, 12], window_size=5,
                                   degree_map_mode=['elevation', 'elevation2', 'distance'],
                                   filtering=True, filtering_num=4, **kw)
            cut['d_map_' + name], cut['score_' + name] = s()
    save('filter_cut_64_s16_st12', cut)

    # --- outside the lattice: what the reference does, recorded as data
    edges = {}
    # a 16 x 32 map: the pyramid has 5 levels (1 x 2 ... 16 x 32); with window 3 the third pass is
    # the first on a map the size check admits (4 x 8), and _filter's square d_map meets it
    a, b = stereo_pair(20, 36, seed=3, dx=2)
    with parallel_backend('threading'):
        co = Correlation_map(a, b, window_size=5)
        co()
    edges['nonsquare_img1'], edges['nonsquare_img2'] = a, b
    edges['nonsquare_plain'] = Matching(co, sub_pix=True)()
    for n in (1, 2, 3):
        m = Matching(co, filter_window_size=3, filtering=True, filtering_num=n, sub_pix=True)
        box = {}
        edges['nonsquare_n%d_raises' % n] = np.array(raised(lambda: box.setdefault('m', m())))
        if 'm' in box:
            edges['nonsquare_n%d' % n] = box['m']
    # hand-made levels that push every position against the borders: no pass carries one out
    lv = steered_levels()
    for k, x in enumerate(lv):
        edges['steered_level%d' % k] = x
    for w, fm in ((3, 'median'), (3, 'average'), (5, 'median'), (5, 'average'), (7, 'average')):
        for s in (False, True):
            m = Matching(Levels(lv), filter_window_size=w, filtering=True, filtering_num=3,
                         filtering_mode=fm, sub_pix=s)
            box = {}
            tag = 'steered_w%d_%s_%s' % (w, fm, 'sub' if s else 'nosub')
            edges[tag + '_raises'] = np.array(raised(lambda: box.setdefault('m', m())))
            if 'm' in box:
                edges[tag] = box['m']
    edges['steered_plain'] = Matching(Levels(lv), sub_pix=False)()
    for k in sorted(edges):
        if k.endswith('_raises'):
            print('%-36s %r' % (k, str(edges[k])))
    save('filter_edges', edges)


if __name__ == '__main__':
    main()
