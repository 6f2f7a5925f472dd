"""The cross-stream hand-offs of the pipelined solve on the device (DESIGN.md section 5c's ledger,
tests/test_streams_host.py's rows): every pipelined configuration gives the bytes of the plain
single-stream solve, with one stream of the hand-off held back by a busy-wait and every recycled
block holding a valid but foreign pyramid.

How a case runs
  decoy     the same configuration runs first on the decoy pair (tests/test_streams_host.py: its matches
            differ from the real pair's in most cells of every tile) and is dropped, so the blocks the
            caching allocator hands to the real pass hold the decoy's stats, levels and maps;
  stall     a bounded busy-wait (torch.cuda._sleep, or without it a fixed chain of large matrix
            products; either calibrated once with timing events; 100 ms, then 300 ms and 1 s only
            for a case whose run proved nothing) goes on
            one stream of the hand-off, a marker event right behind it; the real pass is then enqueued
            as usual: images uploaded on the pair stream, build, match, the pyramid dropped;
  refill    with the stream still held back, tensors of the freed sizes are allocated on every stream of
            the case and clones of the decoy's stats / levels / maps copied into them: a block the
            library let go too early is overwritten with the decoy's data (never with a byte pattern:
            the stats workspace holds operands and tables a kernel addresses through);
  verdict   the marker must still be pending when the host has finished enqueuing (else the case proves
            nothing and fails), the stall must be at least 5 x the host's enqueue time, the map must
            equal the plain solve's byte for byte, and every refilled tensor must still hold the
            decoy's bytes (a late kernel of the dropped pyramid writes into the next owner's block
            even where it rewrites everything it reads itself).

HIP maps streams onto a few hardware queues, and two streams on one queue run one after the other, which
would hide a missing wait.  So before a case uses two streams as producer and consumer, a race planted
with torch operations alone -- a read without a wait, and a tensor freed and overwritten while a
held-back stream still reads it, without record_stream -- must be seen on that very pair (a wrong sum);
if not, another stream is taken for one of the two, what was known of the replaced stream is forgotten,
and every pair of the case is looked at again on the streams it now has, at most 8 times: a case runs only
when the race shows on every pair of streams it uses, the default stream included where torch's current
stream is the default one.
"""
import collections
import time

import numpy as np
import pytest
import torch

import test_streams_host as H
from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard

pytestmark = pytest.mark.gpu

STALLS_MS = (100.0, 300.0, 1000.0)      # every stall starts at the first; a case whose marker was no longer
STALL_MS = STALLS_MS[0]                 # pending, or whose enqueue took over a fifth of it, runs again with the next
NCC = L.DM_TM_CCOEFF_NORMED
Case = collections.namedtuple('Case', 'row name kind shape kw stall')


def _cases():
    all3 = dict(ss=True, ls=True)
    c = []

    def add(row, name, kind, shape, kw, stalls):
        for s in stalls:
            c.append(Case(row, '%s-%s-stall_%s' % (row, name, s), kind, shape, kw, s))
    add('H1', 'stats_stream', 'pyramid', 'mfma32', dict(ss=True), ['pair', 'stats'])
    add('H1', 'own_stream', 'pyramid', 'mfma32', dict(all3, own=True), ['pair'])
    add('H2', 'stats_stream', 'pyramid', 'mfma32', dict(ss=True), ['stats', 'pair'])
    add('H2', 'fuse0', 'pyramid', 'mfma32', dict(ss=True, fuse=0), ['stats'])
    add('H3', 'three_streams', 'pyramid', 'mfma32', dict(all3), ['stats', 'level'])
    add('H4', 'level_stream', 'pyramid', 'mfma32', dict(ls=True), ['pair', 'level'])
    add('H4', 'fuse1_cut', 'pyramid', 'cut64', dict(ls=True, fuse=1, cut=True), ['pair'])
    add('H5', 'wait_level_stream', 'pyramid', 'mfma32', dict(all3, wait=True), ['ext'])
    add('H5', 'wait_pair_stream', 'pyramid', 'mfma32', dict(wait=True), ['ext'])
    add('H5', 'wait_fallback', 'pyramid', 'fallback16', dict(ls=True, wait=True), ['ext'])
    for fuse in (0, 1, 2):
        add('H6', 'fuse%d' % fuse, 'pyramid', 'mfma32', dict(all3, fuse=fuse), ['level', 'pair'])
    add('H6', 'fuse2_cut', 'pyramid', 'cut64', dict(all3, fuse=2, cut=True), ['level'])
    add('H6', 'fallback', 'pyramid', 'fallback16', dict(all3, fuse=2), ['level', 'pair'])
    add('H7', 'stats_and_levels_outlive', 'pyramid', 'mfma32', dict(all3, fuse=1), ['pair', 'level'])
    add('H7', 'constructed_under_another_stream', 'pyramid', 'mfma32', dict(all3, ctor=True), ['pair'])
    add('H7', 'late_l1_outlives', 'pyramid', 'fallback16', dict(ls=True, fuse=2), ['pair'])
    add('H8', 'stream_not_current', 'pyramid', 'mfma32', dict(own=True), ['pair'])
    add('H8', 'stream_not_current_fuse0_cut', 'pyramid', 'cut64', dict(all3, own=True, fuse=0, cut=True), ['pair'])
    add('H9', 'own_stream', 'refine', 'mfma32', dict(own=True), ['pair', 'side'])
    add('H9', 'no_stream', 'refine', 'mfma32', dict(own=False), ['pair', 'side'])
    add('H9', 'no_stream_other_current', 'refine', 'mfma32', dict(own=False, current='default'), ['pair'])
    add('H9', 'built_fuse0', 'refine', 'fallback16', dict(own=False, built=True, fuse=0), ['pair', 'side'])
    add('H10', 'band', 'band', 'band16', dict(ss=True, ls=True, wait=True), ['level', 'stats', 'pair'])
    add('H10', 'band_pair_only', 'band', 'band16', dict(ss=False, ls=False, wait=True), ['ext'])
    add('H11', 'level_and_stats_streams', 'pipeline', 'mfma32', dict(ls=True, ss=True), ['level', 'stats', 'pair'])
    add('H11', 'chained_by_wait', 'pipeline', 'mfma32', dict(ls=False, ss=False), ['pair', 'pair2'])
    return c


CASES = _cases()


# ---------------------------------------------------------------------------------------------
# the harness: stall, streams, planted race
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda', torch.cuda.current_device())


class Busy:
    """A bounded busy-wait on torch's current stream: ``busy(ms)``.  ``sleep``: torch.cuda._sleep, its
    cycles per millisecond calibrated once with timing events; else (a torch without it) a fixed chain
    of large matrix products, calibrated the same way."""

    N = 2048          # the side of the fallback's matrices

    def __init__(self, dev, sleep):
        self.sleep = sleep
        if not sleep:
            self.a = torch.full((self.N, self.N), 1.0 / self.N, dtype=torch.float32, device=dev)
            self.b = torch.empty_like(self.a)
        self.per_ms = 1.0
        unit = 20_000_000 if sleep else 64
        self._run(1000 if sleep else 4)      # (first launch: the code object)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._run(unit)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 1.0, ms
        self.per_ms = unit / ms
        print('\n[streams] %s: %d units in %.2f ms = %.0f units / ms'
              % ('_sleep' if sleep else 'chain of %d^2 products' % self.N, unit, ms, self.per_ms))

    def _run(self, units):
        if self.sleep:
            torch.cuda._sleep(int(units))
        else:
            for _ in range(max(1, int(units))):      # a (all 1 / N) times itself is itself: values stay put
                torch.mm(self.a, self.a, out=self.b)

    def __call__(self, ms):
        self._run(ms * self.per_ms)


@pytest.fixture(scope='module')
def busy(dev):
    return Busy(dev, hasattr(torch.cuda, '_sleep'))


class Stall:
    """A busy-wait of ``ms`` on ``stream`` with a marker event right behind it."""

    def __init__(self, stream, ms, busy):
        self.ms = ms
        self.marker = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            busy(ms)
            self.marker.record(stream)

    def pending(self):
        return not self.marker.query()


def planted_race_seen(a, b, busy, dev):
    """A race made of torch operations only, ``a`` held back: ``b`` reads what ``a`` has yet to write
    without waiting, and a tensor of ``b``'s pool that ``a`` has yet to read is freed without
    record_stream, allocated again and overwritten.  True when both wrong sums show, i.e. when work on
    ``b`` does overtake work on ``a``."""
    n = 1 << 18
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    with torch.cuda.stream(b):
        y = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    y_ptr = y.data_ptr()
    with torch.cuda.stream(a):
        busy(STALL_MS)
        x.fill_(1.0)                  # the producer, late
        r = y.sum()                   # a consumer, late
    del y                             # freed, not recorded on a
    with torch.cuda.stream(b):
        z = torch.empty(n, dtype=torch.float32, device=dev)
        same = z.data_ptr() == y_ptr
        s = x.sum()                   # the read without a wait
        z.fill_(9.0)                  # the block, overwritten
    torch.cuda.synchronize()
    seen = float(s) != float(n) and same and float(r) != 7.0 * n
    del x, z, r, s
    return seen


class Streams:
    """The streams of the module by role, at most 5 alive; a pair of roles qualifies once the planted
    race has been seen on its two streams."""

    ROLES = ('pair', 'level', 'stats', 'pair2', 'side')
    ALIAS = {'ext': 'pair2'}          # the stream of a ``wait`` event: the other pair's

    def __init__(self, dev, busy):
        self.dev, self.busy = dev, busy
        self.by_role, self.qualified, self.made = {}, set(), 0

    def get(self, role):
        if role == 'default':
            return torch.cuda.default_stream(self.dev)
        role = self.ALIAS.get(role, role)
        assert role in self.ROLES, role
        if role not in self.by_role:
            self.by_role[role] = torch.cuda.Stream(device=self.dev)
            self.made += 1
        return self.by_role[role]

    def replace(self, role):
        """Another stream for ``role``; what was known of the old one goes with it (a handle can come back)."""
        role = self.ALIAS.get(role, role)
        old = self.by_role.pop(role).cuda_stream          # at most 5 alive
        self.qualified = {k for k in self.qualified if old not in k}

    def qualify(self, links):
        """Every (held-back role, overtaking role) of ``links`` shows the planted race on the streams the
        roles have when this returns: after a replacement the whole pass starts again, at most 8 times."""
        for _ in range(8):
            for ra, rb in links:
                a, b = self.get(ra), self.get(rb)
                assert a != b, (ra, rb)
                key = frozenset((a.cuda_stream, b.cuda_stream))
                if key in self.qualified:
                    continue
                if planted_race_seen(a, b, self.busy, self.dev):
                    self.qualified.add(key)
                    print('[streams] planted race seen on %s / %s' % (ra, rb))
                    continue
                victim = ra if rb == 'default' else rb
                print('[streams] planted race NOT seen on %s / %s: another stream for %s' % (ra, rb, victim))
                del a, b
                self.replace(victim)
                break
            else:
                for ra, rb in links:      # what the case will run on
                    assert frozenset((self.get(ra).cuda_stream, self.get(rb).cuda_stream)) in self.qualified
                return
        pytest.fail('no streams for %s on which the planted race shows on every pair: two streams that share a '
                    'hardware queue would hide a missing wait' % (links,))


@pytest.fixture(scope='module')
def streams(dev, busy):
    return Streams(dev, busy)


ENQUEUE_MS = {}          # case name -> (host enqueue time, stall), printed at the end of the module


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if ENQUEUE_MS:
        worst = max(ENQUEUE_MS.values())
        print('\n[streams] host enqueue time per case (ms) and stall (ms):')
        for k, (e, s) in sorted(ENQUEUE_MS.items()):
            print('[streams]   %-56s %7.2f %7.0f' % (k, e, s))
        print('[streams] largest enqueue %.2f ms under a stall of %.0f ms' % worst)


# ---------------------------------------------------------------------------------------------
# the data: batches whose images are uploaded per pass, the plain solves, the decoy's buffers
# ---------------------------------------------------------------------------------------------
def raw(t):
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8).copy()


class Data:
    """Of one shape: a TileBatch whose image tensors each pass overwrites (on its pair stream), the
    host images of both pairs pinned, and the plain single-stream results."""

    def __init__(self, shape, dev):
        self.shape, self.dev = shape, dev
        self.host = {}
        for which in ('real', 'decoy'):
            a, b, self.origins, self.s = H.pair(shape, which)
            self.host[which] = (torch.from_numpy(a).pin_memory(), torch.from_numpy(b).pin_memory())
        self.T = len(self.origins)
        a, b = self.host['decoy']
        self.batch = engine.TileBatch(a.to(dev), b.to(dev), self.origins, self.s, self.s, H.WS, NCC, dev)
        self._plain = {}

    def upload(self, which, batch=None):
        """The pair into the batch's images, on the current stream, not blocking the host."""
        batch = batch or self.batch
        batch.img1.copy_(self.host[which][0], non_blocking=True)
        batch.img2.copy_(self.host[which][1], non_blocking=True)

    def plain(self, which, fuse=2, nlev=None, sub_pix=True, keep=False):
        """DevicePyramid(b) + match on the default stream: the bytes every pipelined case must give
        (``keep``: also clones of its stats, stored levels and map, the refill of a later case)."""
        key = (which, fuse, nlev, sub_pix)
        if key not in self._plain:
            torch.cuda.synchronize()
            self.upload(which)
            pyr = engine.DevicePyramid(self.batch, fuse_level2=fuse, build=False).build(nlev=nlev)
            out = pyr.match(sub_pix=sub_pix, nlev=nlev)
            torch.cuda.synchronize()
            bufs = [t.clone() for t in [pyr.stats, out] + pyr.levels if t is not None]
            torch.cuda.synchronize()
            self._plain[key] = (raw(out), out.clone(), bufs)
            del pyr, out
        return self._plain[key][2] if keep else self._plain[key][0]


_DATA = {}


@pytest.fixture(scope='module')
def data(dev):
    def get(shape):
        if shape not in _DATA:
            _DATA[shape] = Data(shape, dev)
        return _DATA[shape]
    yield get
    _DATA.clear()
    _BAND.clear()


REFILL_ROUNDS = 4      # a pool may hold a few free blocks of one size (the decoy pass's, the plain solves')


def refill(owner_streams, bufs):
    """On every owner stream, tensors of the freed sizes with the decoy's data in them, a few of each size
    so that every free block of that size is taken."""
    kept = []
    for s in owner_streams:
        with torch.cuda.stream(s):
            for src in bufs * REFILL_ROUNDS:
                t = torch.empty_like(src)
                t.copy_(src, non_blocking=True)
                kept.append((t, src))
    return kept


def intact(kept):
    """After the synchronize: every refilled tensor still holds the decoy's bytes -- the view of the next
    owner of a block, which a late kernel of the dropped pyramid must not have written."""
    bad = [tuple(t.shape) for t, src in kept
           if not torch.equal(t.reshape(-1).view(torch.uint8), src.reshape(-1).view(torch.uint8))]
    assert not bad, 'tensors allocated after the pyramid was dropped were overwritten: shapes %s' % bad[:4]


# ---------------------------------------------------------------------------------------------
# the scenarios (tests/test_streams_host.py drives the same ones under the model)
# ---------------------------------------------------------------------------------------------
def _pyramid_pass(d, which, st, kw, wait=None, events=None, after_stats=None):
    """One pyramid as a pipelined caller drives it -> its map.  ``after_stats``: called between
    compute_stats and build (a case that holds the pair stream back only then)."""
    pair = st.get('pair')
    own, fuse, cut = kw.get('own', False), kw.get('fuse', 2), kw.get('cut', False)
    ss = st.get('stats') if kw.get('ss') else None
    ls = st.get('level') if kw.get('ls') else None
    n = 3 if cut else None
    with torch.cuda.stream(pair):
        d.upload(which)
    with torch.cuda.stream(st.get('default') if own else pair):
        with torch.cuda.stream(st.get('side') if kw.get('ctor') else None):
            pyr = engine.DevicePyramid(d.batch, stream=pair if own else None, build=False, fuse_level2=fuse,
                                       stats_stream=ss)
        if after_stats is not None:
            pyr.compute_stats()
            after_stats()
        pyr.build(events=events, wait=wait, nlev=n, level_stream=ls)
        out = pyr.match(nlev=n)
        del pyr
    return out


def run_pyramid(d, st, kw, stall_role, busy, stall_ms):
    fuse, n = kw.get('fuse', 2), (3 if kw.get('cut') else None)
    want = d.plain('real', fuse, n)
    bufs = d.plain('decoy', fuse, n, keep=True)
    roles = ['pair'] + (['stats'] if kw.get('ss') else []) + (['level'] if kw.get('ls') else []) + \
        (['default'] if kw.get('own') else [])
    out = _pyramid_pass(d, 'decoy', st, kw)          # the decoy's data into every pool
    del out
    torch.cuda.synchronize()
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if kw.get('wait') else None
    t0 = time.perf_counter()
    if kw.get('ctor'):
        # the stats run at once; the pair stream is held back from the build on, and the level and
        # stats streams have drained when the blocks are taken again
        box = []
        out = _pyramid_pass(d, 'real', st, kw, after_stats=lambda: box.append(Stall(st.get(stall_role), stall_ms, busy)))
        stall = box[0]
        st.get('stats').synchronize()
        st.get('level').synchronize()
    else:
        stall = Stall(st.get(stall_role), stall_ms, busy)
        out = _pyramid_pass(d, 'real', st, kw, wait=stall.marker if kw.get('wait') else None, events=ev)
    kept = refill([st.get(r) for r in roles], bufs)
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    pending = stall.pending()
    torch.cuda.synchronize()
    intact(kept)
    times = None
    if ev is not None:      # H5: the wait completed before events[0], and events[0] <= events[1]
        times = (stall.marker.elapsed_time(ev[0]), ev[0].elapsed_time(ev[1]))
    del kept
    return raw(out), want, enqueue_ms, pending, times


def _refine_pass(d, which, st, kw, coarse):
    pair, side = st.get('pair'), st.get('side')
    own, fuse = kw.get('own', False), kw.get('fuse', 2)
    with torch.cuda.stream(pair):
        d.upload(which)
    with torch.cuda.stream(st.get('default') if own else pair):
        pyr = engine.DevicePyramid(d.batch, stream=pair if own else None, build=kw.get('built', False),
                                   fuse_level2=fuse)
        pyr.compute_stats()
    with torch.cuda.stream(side):
        m = torch.empty_like(coarse)
        m.copy_(coarse, non_blocking=True)          # the map, written on the side stream
    with torch.cuda.stream(st.get('default') if (own or kw.get('current') == 'default') else pair):
        engine.subpix_map_tiles(pyr, m, stream=side)
    del pyr
    return m


def run_refine(d, st, kw, stall_role, busy, stall_ms):
    """dm_match without sub-pixel, then subpix_map_tiles on a second stream: the header states that this
    is dm_match's own sub-pixel step, so the plain solve with sub_pix is the answer."""
    fuse = kw.get('fuse', 2)
    coarse = {}
    for w in ('real', 'decoy'):
        d.plain(w, fuse, sub_pix=False)
        coarse[w] = d._plain[(w, fuse, None, False)][1]
    if ('refine', fuse) not in d._plain:      # the same two calls on one stream
        torch.cuda.synchronize()
        d.upload('real')
        m = coarse['real'].clone()
        engine.subpix_map_tiles(engine.DevicePyramid(d.batch, fuse_level2=fuse), m)
        d._plain[('refine', fuse)] = raw(m)
        del m
    want = d._plain[('refine', fuse)]
    assert np.array_equal(want, d.plain('real', fuse))
    bufs = d.plain('decoy', fuse, keep=True)
    m = _refine_pass(d, 'decoy', st, kw, coarse['decoy'])
    del m
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stall = Stall(st.get(stall_role), stall_ms, busy)
    m = _refine_pass(d, 'real', st, kw, coarse['real'])
    kept = refill([st.get('pair'), st.get('default')], bufs)
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    pending = stall.pending()
    torch.cuda.synchronize()
    intact(kept)
    del kept
    return raw(m), want, enqueue_ms, pending, None


class Band:
    """BandSolver over 7 tiles in 3 chunks; its images are uploaded per pass like a Data batch's."""

    def __init__(self, d):
        a, b = d.host['decoy']
        self.solver = shard.BandSolver(a.to(d.dev), b.to(d.dev), d.origins, d.s, d.s, H.WS, NCC, device=d.dev, chunks=3)
        assert [len(i) for i in self.solver.chunk_idx] == [3, 3, 1]
        self.d = d
        self._plain = {}

    def upload(self, which):
        self.solver.img1.copy_(self.d.host[which][0], non_blocking=True)
        self.solver.img2.copy_(self.d.host[which][1], non_blocking=True)

    def plain(self, which):
        if which not in self._plain:
            torch.cuda.synchronize()
            self.upload(which)
            self._plain[which] = raw(self.solver.solve())
        return self._plain[which]


_BAND = {}


def _band_pass(band, which, st, kw, wait=None, events=None):
    pair = st.get('pair')
    with torch.cuda.stream(pair):
        band.upload(which)
        g = band.solver.start(events=events, wait=wait, level_stream=st.get('level') if kw.get('ls') else None,
                              stats_stream=st.get('stats') if kw.get('ss') else None)
    return g


def _band_result(g, st):
    """ChunkGather.result() under the pair stream: it assembles the chunks with indexed copies, which
    make the host wait for the stream -- so a case calls it only after its marker has been looked at."""
    with torch.cuda.stream(st.get('pair')):
        return g.result()


def run_band(d, st, kw, stall_role, busy, stall_ms):
    if 'band' not in _BAND:
        _BAND['band'] = Band(d)
    band = _BAND['band']
    want = band.plain('real')
    assert np.array_equal(want, d.plain('real'))          # the band's plain solve is the batch's
    if 'bufs' not in _BAND:      # the decoy's stats / levels / maps at the chunks' own sizes (3 tiles and 1)
        torch.cuda.synchronize()
        band.upload('decoy')
        _BAND['bufs'] = []
        for b in (band.solver.batches[0], band.solver.batches[2]):
            pyr = engine.DevicePyramid(b)
            out = pyr.match()
            _BAND['bufs'] += [t.clone() for t in [pyr.stats, out] + pyr.levels if t is not None]
            del pyr, out
        torch.cuda.synchronize()
    bufs = _BAND['bufs']
    res = _band_result(_band_pass(band, 'decoy', st, kw), st)
    del res
    torch.cuda.synchronize()
    evs = []
    roles = ['pair'] + (['stats'] if kw.get('ss') else []) + (['level'] if kw.get('ls') else [])
    t0 = time.perf_counter()
    stall = Stall(st.get(stall_role), stall_ms, busy)
    g = _band_pass(band, 'real', st, kw, wait=stall.marker, events=evs)
    kept = refill([st.get(r) for r in roles], bufs)
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    pending = stall.pending()
    res = _band_result(g, st)
    torch.cuda.synchronize()
    intact(kept)
    assert len(evs) == 3
    times = None
    if stall_role == 'ext':      # ``wait`` holds chunk 0 back; every chunk's events are in order
        times = (stall.marker.elapsed_time(evs[0][0]), min(a.elapsed_time(b) for a, b in evs))
    del kept
    return raw(res), want, enqueue_ms, pending, times


def run_pipeline(d, st, kw, stall_role, busy, stall_ms):
    """Four solves back to back as bench.py's Pipeline drives them, the real pair and the decoy in turn on
    two pair streams: each solve reuses what the one before it released, and must give its own pair's
    plain bytes."""
    if 'second' not in _BAND:
        _BAND['second'] = engine.TileBatch(d.host['decoy'][0].to(d.dev), d.host['decoy'][1].to(d.dev), d.origins,
                                           d.s, d.s, H.WS, NCC, d.dev)
    batches = {'real': d.batch, 'decoy': _BAND['second']}
    want = {w: d.plain(w, 2, 3) for w in ('real', 'decoy')}
    bufs = d.plain('decoy', 2, 3, keep=True)
    torch.cuda.synchronize()
    d.upload('real')
    torch.cuda.synchronize()
    pairs = [st.get('pair'), st.get('pair2')]
    ls = st.get('level') if kw.get('ls') else None
    ss = st.get('stats') if (kw.get('ss') and ls is not None) else None
    roles = ['pair', 'pair2'] + (['level'] if ls is not None else []) + (['stats'] if ss is not None else [])

    def solves(stall_role):
        prev, outs, evs, stall = None, [], [], None
        t0 = time.perf_counter()
        if stall_role is not None:
            stall = Stall(st.get(stall_role), stall_ms, busy)
        for k in range(4):
            which = ('real', 'decoy')[k % 2]
            with torch.cuda.stream(pairs[k % 2]):
                pyr = engine.DevicePyramid(batches[which], build=False, stats_stream=ss)
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                pyr.build(events=ev, wait=prev if ls is None else None, nlev=3, level_stream=ls)
                outs.append((which, pyr.match(nlev=3)))
                del pyr
                prev = ev[1]
                evs.append(ev)
        kept = refill([st.get(r) for r in roles], bufs) if stall is not None else None
        return outs, evs, stall, kept, (time.perf_counter() - t0) * 1e3
    outs, _, _, _, _ = solves(None)          # warm: every pool holds both pairs' buffers
    del outs
    torch.cuda.synchronize()
    outs, evs, stall, kept, enqueue_ms = solves(stall_role)
    pending = stall.pending()
    torch.cuda.synchronize()
    intact(kept)
    for which, out in outs[1:]:
        assert np.array_equal(raw(out), want[which]), 'solve of the %s pair differs from its plain solve' % which
    # the level kernels run one after another: each one's start is not before the end of the one before it
    times = (min(a[1].elapsed_time(b[0]) for a, b in zip(evs, evs[1:])), min(a.elapsed_time(b) for a, b in evs))
    del kept
    return raw(outs[0][1]), want['real'], enqueue_ms, pending, times


RUN = {'pyramid': run_pyramid, 'refine': run_refine, 'band': run_band, 'pipeline': run_pipeline}
def _default(kw):
    """The default stream is part of a case whose pyramid has a stream of its own (torch's current stream is
    then the default one: the parent's blocks came from its pool, and the refill runs there) or is called
    under the default stream after the pair stream (the wait in DevicePyramid._pair)."""
    return [('pair', 'default')] if (kw.get('own') or kw.get('current') == 'default') else []


LINKS = {      # the (held-back, overtaking) pairs of roles a case hands data across
    'pyramid': lambda kw: ([('stats', 'pair')] if kw.get('ss') else []) + ([('level', 'pair')] if kw.get('ls') else []) +
                          ([('stats', 'level')] if kw.get('ss') and kw.get('ls') else []) +
                          ([('ext', 'level' if kw.get('ls') else 'pair')] if kw.get('wait') else []) + _default(kw),
    'refine': lambda kw: [('pair', 'side')] + _default(kw),
    'band': lambda kw: ([('stats', 'pair')] if kw.get('ss') else []) + ([('level', 'pair')] if kw.get('ls') else []) +
                       ([('stats', 'level')] if kw.get('ss') and kw.get('ls') else []) +
                       [('ext', 'level' if kw.get('ls') else 'pair')],
    'pipeline': lambda kw: ([('level', 'pair'), ('level', 'pair2'), ('stats', 'pair'), ('stats', 'pair2'), ('stats', 'level')]
                            if kw.get('ls') else [('pair', 'pair2')]),
}


@pytest.mark.parametrize('shape', sorted(H.SHAPES))
def test_plain_solve_equals_oracle(data, shape):
    """The anchor of every case below is not the code under test: the plain single-stream solve gives
    the oracle's bytes (pinned pow)."""
    d = data(shape)
    nlev = 3 if shape == 'cut64' else None
    got = d.plain('real', 2, nlev)
    want = H.oracle_match(shape, 'real', nlev)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(-1))
    assert not np.array_equal(got, d.plain('decoy', 2, nlev))


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_handoff_under_a_stalled_stream(case, data, streams, busy):
    d = data(case.shape)
    for stall_ms in STALLS_MS:      # the stall grows only while a run proves nothing
        streams.qualify(LINKS[case.kind](case.kw))
        got, want, enqueue_ms, pending, times = RUN[case.kind](d, streams, case.kw, case.stall, busy, stall_ms)
        ENQUEUE_MS[case.name] = (enqueue_ms, stall_ms)
        print('\n[streams] %s: enqueue %.2f ms, stall %.0f ms, marker pending %s, times %s'
              % (case.name, enqueue_ms, stall_ms, pending, times))
        assert np.array_equal(got, want), '%d of %d bytes differ from the plain solve' % (int((got != want).sum()), got.size)
        if pending and stall_ms >= 5 * enqueue_ms:
            break
    assert pending, 'inconclusive: the stall of %.0f ms had ended when the host finished enqueuing (%.1f ms)' \
        % (stall_ms, enqueue_ms)
    assert stall_ms >= 5 * enqueue_ms, 'the stall (%.0f ms) is not 5 x the enqueue time (%.1f ms)' % (stall_ms, enqueue_ms)
    if times is not None:
        assert times[0] >= 0 and times[1] >= 0, times
    assert got.shape == want.shape
    assert np.array_equal(got, want), '%d of %d bytes differ from the plain solve' % (int((got != want).sum()), got.size)


def test_the_stall_without_sleep_is_a_stall(dev):
    """The busy-wait a torch without torch.cuda._sleep gets (a fixed chain of large matrix products) holds
    a stream for about what was asked, and no longer than a stall may last."""
    chain = Busy(dev, sleep=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        e0.record()
        chain(STALL_MS)
        e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    print('\n[streams] the chain asked for %.0f ms took %.1f ms' % (STALL_MS, ms))
    assert 0.5 * STALL_MS <= ms <= STALLS_MS[-1], ms
