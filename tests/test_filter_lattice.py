"""Matching._filter where it acts: every window, pass count and mode, on the CPU.

``filter_restate`` below is a plain-loop restatement of the reference's filtered descent
(misc/Matching.py:80-149, :177-255), standalone: it shares no code with ``oracle.match``.  Both
are held to each other bit for bit and to fixtures the reference itself produced
(tests/golden/make_golden_filter.py) at the tolerances of test_oracle_golden.py: integer
correspondences exact, scores within 1e-12, sub-pixel coordinates within 1e-9.

Every lattice case asserts its premise, so none passes vacuously: a case in which a pass with
a reach >= 1 runs must differ from the unfiltered match, and each such pass, switched on
alone, must change its intermediate map; a case in which no such pass runs must equal the
unfiltered match bit for bit.  The premises are facts about the pairs, established by the
restatement and the reference fixtures alone ("Where Matching._filter acts").

What no input can reach, stated once: a window holds 1, 9, 25 or 49 integers (windows 2, 4, 6
take the reach of 1, 3, 5), an odd number.  The mean of an odd number of integers is never at
.5 and their median is an element, never fractional.  So round-half-even against half-away,
and truncation against floor in the int64 cast of a whole number, give the same value on
every input; no test here pretends to tell them apart.

A position never leaves the map either (test_no_pass_carries_a_position_out_of_the_map has the
argument), so the zero reads of the kernels outside a map and the reference's exception there
are not observable through Matching.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
TOL_F64 = 1e-12
TOL_SUBPIX = 1e-9
PAIRS = ('filter_s8_noise', 'filter_s16_noise', 'filter_s16_ccoeff', 'filter_s32_sin', 'filter_s32_roll')
WINDOWS = (1, 2, 3, 4, 5, 6, 7)
FMODES = ('median', 'average')


# ---- the restatement ---------------------------------------------------------------------------

def near(M, pd0, pd1):
    """_calc_near_match (:58-78) with total reads: a window cell or a centre outside the map
    reads 0 (what window_lvl / near_pick of csrc/dm_kernels.hip do).  -> (row, col, score)."""
    h, w = M.shape

    def rd(r, c):
        return M[r, c] if 0 <= r < h and 0 <= c < w else 0.0
    win = [rd(pd0 - 1 + a, pd1 - 1 + b) for a in range(3) for b in range(3)]
    m, best, nan = 0, win[0], win[0] != win[0]
    for k in range(1, 9):                 # np.argmax: the first maximum, or the first NaN
        if nan:
            break
        if win[k] != win[k]:
            m, nan = k, True
        elif win[k] > best:
            m, best = k, win[k]
    if not nan and best < 0.0001:
        m = 4
    return pd0 + m // 3 - 1, pd1 + m % 3 - 1, win[m] + win[4]


def reach(fw):
    return (fw - 1) // 2


def filter_pass(mp, fw, mode):
    """_filter (:224-255) on a square (3, n, n) map -> (new map, did the size check admit it)."""
    _, h, w = mp.shape
    if h < fw or w < fw:
        return mp, False
    assert h == w, 'the restatement covers square maps only'
    ex = reach(fw)
    d = [[(int(mp[0, i, j]) - i, int(mp[1, i, j]) - j) for j in range(w)] for i in range(h)]
    out = mp.copy()
    for i in range(ex, h - ex):
        for j in range(ex, w - ex):
            for plane, base in ((0, i), (1, j)):
                v = [d[a][b][plane] for a in range(i - ex, i + ex + 1) for b in range(j - ex, j + ex + 1)]
                out[plane, i, j] = (sorted(v)[len(v) // 2] if mode == 'median' else round(sum(v) / len(v))) + base
    return out, True


def pass_plan(sides, fw, fnum):
    """Per level, top first: does the _filter hook run its pass there?  A hook whose map fails
    the size check still uses up one of the ``fnum`` counts (:91-93, :136-138)."""
    plan = []
    for n in sides:
        plan.append(fnum > 0 and n >= fw)
        fnum -= fnum > 0
    return plan


def descent(levels, fw=3, fnum=0, mode='median', only=None):
    """_initial_move_map + _calc_match with the _filter hooks.  ``only``: run the pass of that
    one level (index into the descent, top = 0) and no other.  -> dict(map, before, after, left):
    the final (3, h0, w0) map, the intermediate maps around every hook, and whether any position
    (a window centre) lay outside its map."""
    left = False
    before, after = [], []

    def hook(mp, k):
        nonlocal fnum
        before.append(mp)
        if fnum > 0:
            if only is None or only == k:
                mp, _ = filter_pass(mp, fw, mode)
            fnum -= 1
        after.append(mp)
        return mp

    top = levels[-1]
    h, w = top.shape[:2]
    mp = np.zeros((3, h, w))
    for i in range(h):
        for j in range(w):
            mp[:, i, j] = near(top[i, j], i, j)
    mp = hook(mp, 0)
    for k, lv in enumerate(reversed(levels[:-1]), 1):
        h, w = mp.shape[1:]
        nx = np.empty((3, 2 * h, 2 * w))
        for i in range(2 * h):
            for j in range(2 * w):
                pd0 = int(mp[0, i // 2, j // 2] * 2) + (i & 1)
                pd1 = int(mp[1, i // 2, j // 2] * 2) + (j & 1)
                left |= not (0 <= pd0 < 2 * h and 0 <= pd1 < 2 * w)
                nx[:, i, j] = near(lv[i, j], pd0, pd1)
        mp = hook(nx, k)
    return dict(map=mp, before=before, after=after, left=left)


def sub_pix(mp, L0):
    """_sub_pix_cal (:177-209).  co_map_list[0][i, j] is indexed as numpy indexes it: an index in
    [-n, 0) wraps, one outside [-n, n) raises IndexError into the bare except."""
    h0, w0 = L0.shape[2:]
    out = mp.copy()

    def comp(r0, r1, r_):
        return -(r1 - r_) / (2 * (r1 + r_ - 2 * r0)) if (r0 > r1 and r0 > r_) else 0

    for i in range(mp.shape[1]):
        for j in range(mp.shape[2]):
            c0, c1 = int(mp[0, i, j]), int(mp[1, i, j])
            M = L0[i, j]
            d_x = i - mp[0, i, j]
            try:
                out[0, i, j] = i - d_x + comp(M[c0, c1], M[c0 + 1, c1], M[c0 - 1, c1])
            except IndexError:
                out[0, i, j] = i - d_x
            d_y = j - mp[1, i, j]
            try:
                out[1, i, j] = j - d_y + comp(M[c0, c1], M[c0, c1 + 1], M[c0, c1 - 1])
            except IndexError:
                out[1, i, j] = j - d_y
    return out


def filter_restate(levels, sub_pix_=True, filtering=False, filter_window_size=3, filtering_num=3,
                   filtering_mode='median'):
    """Matching(...)() on a level list -> (map, left)."""
    r = descent(levels, filter_window_size, filtering_num if filtering else 0, filtering_mode)
    return (sub_pix(r['map'], levels[0]) if sub_pix_ else r['map']), r['left']


# ---- fixtures ---------------------------------------------------------------------------------------

def key(w, mode, n):
    return 'w%d_%s_n%d' % (w, mode, n)


def counts(nlev):
    return tuple(dict.fromkeys((1, 2, 3, 4, nlev, nlev + 2)))


def sides(levels):
    return [lv.shape[0] for lv in reversed(levels)]


@functools.lru_cache(maxsize=None)
def load(name, pow_mode='libm'):
    """(fixture dict, oracle levels) of one pair; the levels under the given pow."""
    g = dict(np.load(os.path.join(GOLD, name + '.npz')))
    O.set_pow_mode(pow_mode)
    try:
        levels, _, _ = O.pyramid(O.corr_l0(g['img1'], g['img2'], int(g['ws']), str(g['feature'])))
    finally:
        O.set_pow_mode('libm')
    assert len(levels) == int(g['nlev'])
    g['index'] = {str(k): int(u) for k, u in zip(g['keys'], g['uid'])}
    return g, levels


def stored(g, k, sub):
    """The reference's result for key k: (3, h, w)."""
    u = g['index'][k]
    return np.concatenate([g['sub'][u], g['nosub'][u][2:]]) if sub else g['nosub'][u]


def held_to_fixture(m, ref, sub):
    assert m.shape == ref.shape
    if sub:
        assert np.max(np.abs(m[:2] - ref[:2])) <= TOL_SUBPIX
    else:
        assert np.array_equal(m[:2], ref[:2])
    assert np.max(np.abs(m[2] - ref[2])) <= TOL_F64


def lattice_counts(g, w, mode):
    return [n for n in counts(int(g['nlev'])) if key(w, mode, n) in g['index']]


@functools.lru_cache(maxsize=None)
def restated(name, w, mode, n, sub):
    g, levels = load(name)
    if n == 0:
        return filter_restate(levels, sub)
    return filter_restate(levels, sub, True, w, n, mode)


@functools.lru_cache(maxsize=None)
def pass_alone_changes(name, w, mode, k):
    """Does the pass of level k of the descent, switched on alone, change its map?"""
    g, levels = load(name)
    r = descent(levels, w, len(levels), mode, only=k)
    return not np.array_equal(r['before'][k], r['after'][k])


def acting_levels(levels, w, n):
    """The levels of the descent whose pass runs and reaches a neighbour."""
    return [k for k, runs in enumerate(pass_plan(sides(levels), w, n)) if runs and reach(w) >= 1]


def quiet_levels(name, levels, w):
    return [k for k, n in enumerate(sides(levels)) if (name, n, reach(w)) in QUIET]


# The one pass of the lattice that runs, reaches its neighbours and still changes nothing: the
# 4 x 4 map of the sinusoidal pair holds one displacement over the 3 x 3 windows of its 2 x 2
# interior, so its mean and median are what is there.  (pair, side of the map, reach); the cases
# assert that exactly -- the pass alone leaves its map unchanged -- and count it as not acting.
QUIET = frozenset([('filter_s32_sin', 4, 1)])


# ---- the lattice ------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', FMODES)
@pytest.mark.parametrize('w', WINDOWS)
@pytest.mark.parametrize('name', PAIRS)
def test_lattice(name, w, mode):
    g, levels = load(name)
    plain = restated(name, 0, 'median', 0, False)[0]
    ns = lattice_counts(g, w, mode)
    assert ns, 'the fixture holds no case of this window and mode'
    for n in ns:
        act = [k for k in acting_levels(levels, w, n) if k not in quiet_levels(name, levels, w)]
        for sub in (False, True):
            m, left = restated(name, w, mode, n, sub)
            assert not left
            o = O.match(levels, sub_pix=sub, filtering=True, filter_window_size=w, filtering_num=n,
                        filtering_mode=mode)
            assert np.array_equal(m, o), (n, sub)
            held_to_fixture(m, stored(g, key(w, mode, n), sub), sub)
            if not act:     # nothing may change: bit-equal to the unfiltered match, in all three
                assert np.array_equal(m, restated(name, 0, 'median', 0, sub)[0])
                assert np.array_equal(o, O.match(levels, sub_pix=sub))
                assert g['index'][key(w, mode, n)] == g['index']['none']
        m = restated(name, w, mode, n, False)[0]
        changed = int(np.any(m[:2] != plain[:2], axis=0).sum())
        print('%s %s: %d of %d cells differ from the unfiltered match' % (name, key(w, mode, n), changed, plain[0].size))
        if act:
            for k in act:
                assert pass_alone_changes(name, w, mode, k), 'the pass of level %d changes nothing' % k
            assert changed > 0, 'count %d: the filtered match equals the unfiltered one' % n
            assert g['index'][key(w, mode, n)] != g['index']['none']
    for k in quiet_levels(name, levels, w):
        assert sides(levels)[k] >= w and not pass_alone_changes(name, w, mode, k)


@pytest.mark.parametrize('name', PAIRS)
def test_both_planes_change(name):
    """The row plane and the column plane each change in at least one case of the pair (a
    k_filter that filters one plane and copies the other would pass a pair that moves one)."""
    g, levels = load(name)
    plain = restated(name, 0, 'median', 0, False)[0]
    rows = cols = 0
    for w in (3, 5, 7):
        for mode in FMODES:
            n = int(g['nlev'])
            m = restated(name, w, mode, n, False)[0]
            rows += int((m[0] != plain[0]).sum())
            cols += int((m[1] != plain[1]).sum())
    assert rows > 0 and cols > 0, (rows, cols)


def test_reference_driver_setting():
    """ex_deepmatching_rawinput.py runs window 3, count 4, median: on every pair it differs from
    the suite's older setting (count 3) and from the unfiltered match."""
    for name in PAIRS:
        g, _ = load(name)
        i = g['index']
        assert i[key(3, 'median', 4)] != i[key(3, 'median', 3)], name
        assert i[key(3, 'median', 4)] != i['none'], name


# ---- even windows, skipped passes ----------------------------------------------------------------------

def test_even_windows_and_skipped_passes():
    """Windows 2, 4, 6 take the reach of 1, 3, 5, but the size check compares the map's side with
    2, 4, 6: window 4 runs on a 4 x 4 map, window 5 does not; and a skipped pass uses up a count."""
    assert [reach(w) for w in WINDOWS] == [0, 0, 1, 1, 2, 2, 3]
    g, levels = load('filter_s16_noise')
    assert sides(levels) == [1, 2, 4, 8, 16]
    m4 = descent(levels, 4, 0)['before'][2]           # the unfiltered 4 x 4 map
    for mode in FMODES:
        a, ran = filter_pass(m4, 4, mode)
        b, _ = filter_pass(m4, 3, mode)
        assert ran and np.array_equal(a, b) and not np.array_equal(a, m4)
        c, ran = filter_pass(m4, 5, mode)
        assert not ran and c is m4
    assert pass_plan([1, 2, 4, 8, 16], 4, 3) == [False, False, True, False, False]
    assert pass_plan([1, 2, 4, 8, 16], 5, 3) == [False] * 5           # three counts, all skipped
    assert pass_plan([1, 2, 4, 8, 16], 5, 4) == [False, False, False, True, False]
    assert pass_plan([1, 2, 4, 8, 16], 2, 1) == [False] * 5 and pass_plan([1, 2, 4, 8, 16], 1, 1)[0]
    i = g['index']
    for mode in FMODES:
        for n in counts(5):
            assert i[key(4, mode, n)] == i[key(3, mode, n)]      # the reference agrees: same reach,
            assert i[key(6, mode, n)] == i[key(5, mode, n)]      # and no map side lies between
            assert i[key(1, mode, n)] == i[key(2, mode, n)] == i['none']
        assert i[key(5, mode, 3)] == i['none'] != i[key(4, mode, 3)]
        assert i[key(5, mode, 4)] != i['none']
    # a map whose side lies between a window and the even window above it: 3 x 3 under 3 and 4
    m3 = np.array([[[0, 1, 2], [1, 2, 0], [2, 2, 1]], [[2, 2, 2], [0, 1, 1], [0, 0, 1]], np.zeros((3, 3))], dtype=float)
    assert filter_pass(m3, 3, 'median')[1] and not filter_pass(m3, 4, 'median')[1]


def test_counter_of_one_object():
    """One reference Matching object called three times with filtering_num = nlev + 2 runs nlev
    passes, then has 2 left -- used up on the skipped 1 x 1 and 2 x 2 maps -- then 0: calls two
    and three give the unfiltered match.  The oracle's results for those counts (the mirror's
    attribute bookkeeping is held to them in test_filter_lattice_gpu.py)."""
    g, levels = load('filter_s16_noise')
    nlev = len(levels)
    left = nlev + 2
    for call in range(3):
        m = O.match(levels, sub_pix=True, filtering=True, filtering_num=left)
        want = key(3, 'median', nlev + 2) if call == 0 else 'none'
        held_to_fixture(m, stored(g, want, True), True)
        assert (call == 0) == bool(acting_levels(levels, 3, left))
        left = max(0, left - nlev)
    assert left == 0


# ---- outside the lattice ---------------------------------------------------------------------------------

def test_no_pass_carries_a_position_out_of_the_map():
    """Before a pass every position lies in the map: 0 <= j + d[i][j] <= n - 1, so d[i][b] <=
    n - 1 - b.  In the window of an interior cell (i, j) the columns b >= j are (ex + 1) of the
    2 ex + 1, more than half of the cells, and all of them hold d <= n - 1 - j: the median is one
    of them or smaller.  The mean is at most the mean of the bounds, n - 1 - j, a whole number, so
    the rounded mean is too.  The lower bound and the rows go the same way; by induction over the
    passes and the steps (a child's centre 2 p + o of an in-map p is in the child map, and
    _calc_near_match moves to a non-zero, so in-map, cell or stays) no position ever leaves.  Here
    the same on every extreme: random in-map maps, and maps with every cell on a border."""
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 7, 8, 9):
        for trial in range(12):
            mp = np.zeros((3, n, n))
            if trial < 4:     # all positions on one border / in one corner
                mp[0], mp[1] = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)][trial]
            elif trial < 8:   # each cell on a random border
                mp[:2] = rng.integers(0, 2, (2, n, n)) * (n - 1)
            else:
                mp[:2] = rng.integers(0, n, (2, n, n))
            for w in WINDOWS:
                for mode in FMODES:
                    out, _ = filter_pass(mp, w, mode)
                    assert out[:2].min() >= 0 and out[:2].max() <= n - 1


def test_steered_levels():
    """Hand-made levels that drive every position against the borders, with the filter acting on
    the seam between the two halves: the reference raises nothing, and the restatement and the
    oracle give its maps."""
    g = np.load(os.path.join(GOLD, 'filter_edges.npz'))
    levels = [g['steered_level%d' % k] for k in range(3)]
    plain = O.match(levels, sub_pix=False)
    assert np.array_equal(plain, g['steered_plain'])
    assert plain[:2].min() == 0 and plain[:2].max() == 15
    for w, mode in ((3, 'median'), (3, 'average'), (5, 'median'), (5, 'average'), (7, 'average')):
        for sub in (False, True):
            tag = 'steered_w%d_%s_%s' % (w, mode, 'sub' if sub else 'nosub')
            assert str(g[tag + '_raises']) == ''
            m, left = filter_restate(levels, sub, True, w, 3, mode)
            assert not left
            assert np.array_equal(m, O.match(levels, sub_pix=sub, filtering=True, filter_window_size=w,
                                             filtering_num=3, filtering_mode=mode))
            held_to_fixture(m, g[tag], sub)
            if not sub:
                assert not np.array_equal(m[:2], plain[:2])


def test_oracle_near_refuses_a_position_outside_the_map():
    """oracle._near used to wrap a negative centre the numpy way, which neither the reference (it
    raises in the next _B) nor the kernels (they read 0) do.  No descent reaches it; it raises."""
    M = np.arange(16.0).reshape(4, 4)
    assert O._near(M, 0, 0) == near(M, 0, 0) == (1, 1, 5.0)
    # the restatement's reads are total: a centre outside reads 0, the window what of it is in the
    # map (on a constant map its first in-map cell wins), and a window wholly outside stays put
    H = np.full((4, 4), 0.5)
    for pd, want in (((-1, 0), (0, 0, 0.5)), ((0, -1), (0, 0, 0.5)), ((4, 0), (3, 0, 0.5)), ((0, 4), (0, 3, 0.5)),
                     ((9, 9), (9, 9, 0.0)), ((-2, 1), (-2, 1, 0.0))):
        with pytest.raises(IndexError):
            O._near(H, *pd)
        assert near(H, *pd) == want


def test_non_square_maps():
    """16 x 32, window 3: counts 1 and 2 are used up on the 1 x 2 and 2 x 4 maps and the result is
    the unfiltered match; with count 3 the 4 x 8 map meets _filter's square d_map (:235-236) and
    the reference raises (recorded by the generator); the oracle raises the same type."""
    g = np.load(os.path.join(GOLD, 'filter_edges.npz'))
    levels, _, _ = O.pyramid(O.corr_l0(g['nonsquare_img1'], g['nonsquare_img2'], 5))
    assert [lv.shape[:2] for lv in levels] == [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]
    plain = O.match(levels, sub_pix=True)
    held_to_fixture(plain, g['nonsquare_plain'], True)
    for n in (1, 2):
        assert str(g['nonsquare_n%d_raises' % n]) == ''
        assert np.array_equal(g['nonsquare_n%d' % n], g['nonsquare_plain'])
        assert np.array_equal(O.match(levels, sub_pix=True, filtering=True, filtering_num=n), plain)
    exc = str(g['nonsquare_n3_raises'])
    print('the reference on a 4 x 8 map: %s' % exc)
    assert exc.startswith('ValueError')          # round() of the median of an empty slice
    with pytest.raises(ValueError):
        O.match(levels, sub_pix=True, filtering=True, filtering_num=3)
