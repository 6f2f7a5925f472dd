"""A happens-before checker for the Python code that orders work across streams (engine.DevicePyramid
with ``stats_stream`` / ``level_stream`` / ``wait`` / ``events``, engine.subpix_map_tiles on a second
stream, shard.BandSolver.start): DESIGN.md section 5c holds the ledger of hand-offs, row by row.

For one run the name ``torch`` of engine / shard / _lib is a recording model (as tests/test_guarded_host.py
swaps it for a guarded allocator) and the loaded library is a stand-in that logs every entry as (name,
stream, blocks read, blocks written).  Nothing runs on a device.

  Model     streams with vector clocks.  An operation on stream s ticks s; ``Event.record`` takes a copy
            of the clock, ``wait_event`` / ``wait_stream`` merge one in.  A happened before B iff B's
            clock has reached A's tick on A's stream.
  (a) order a read or write of a block comes after the last write of it, a write also after every read
            since (a missing wait: ``order consumer<-producer``).
  (b) life  when the last reference of a block is dropped (or the run ends), every use of it on a stream
            other than the one whose pool it came from was recorded there (``record_stream``), or the
            pool's stream had already waited for that use -- the caching allocator's rule: a freed
            block is handed out again to work ordered on the pool's stream and after an event on every
            recorded stream (a missing record: ``life block@stream``).
  skip      a set of call keys (``wait:function:consumer<-producer``, ``record:function:block@stream``,
            ``ctx:function:stream``) that the model turns into no-ops: every ledger row has a case that
            plants such an omission, and the checker must name it.

The same file holds the pairs of the GPU half (tests/test_streams_gpu.py): a real pair and a decoy of one
shape whose oracle matches differ in most cells, so a stale read of recycled memory cannot pass by chance.
"""
import collections
import contextlib
import ctypes
import functools
import itertools
import linecache
import os
import re
import sys
import weakref

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

WS = 5
NCC = L.DM_TM_CCOEFF_NORMED
SWAPPED = (engine, shard, L)          # the modules whose ``torch`` is the model for one run


# ---------------------------------------------------------------------------------------------
# read / write sets of the entries the pipelined solve calls, from include/dmstereo.h: the argument
# positions that are device buffers.  'b' stands for the three buffers of the dm_tiles argument.
# ---------------------------------------------------------------------------------------------
def _tiles(ref):
    s = ref._obj
    return [s.d_img1, s.d_img2, s.d_origins]


ENTRIES = {
    # dm_corr_stats(b, d_stats, stream): moments and window operands of the images -> d_stats
    'dm_corr_stats': lambda a: (_tiles(a[0]), [a[1]]),
    # dm_corr_level1(b, d_stats, d_level1, stream): "writes level 1 and the per-patch min/max into d_stats"
    'dm_corr_level1': lambda a: (_tiles(a[0]) + [a[1]], [a[1], a[2]]),
    # dm_corr_level12(b, d_stats, d_level1 or NULL, d_level2, stream)
    'dm_corr_level12': lambda a: (_tiles(a[0]) + [a[1]], [a[1], a[2], a[3]]),
    # dm_corr_volume_ex(b, d_stats, flags, d_l0, stream): the volume and the per-patch min/max
    'dm_corr_volume_ex': lambda a: (_tiles(a[0]) + [a[1]], [a[1], a[3]]),
    # dm_rectify(d_in, n, d_out, stream), dm_rectify_f16 alike
    'dm_rectify': lambda a: ([a[0]], [a[2]]),
    'dm_rectify_f16': lambda a: ([a[0]], [a[2]]),
    # dm_aggregate(d_in, T, h, w, rectify, d_out, stream)
    'dm_aggregate': lambda a: ([a[0]], [a[5]]),
    # dm_match(b, d_stats, d_levels[nlev] (host array), nlev, T, h0, w0, sub_pix, fw, fnum, fmode, d_scratch, d_out, stream)
    'dm_match': lambda a: (_tiles(a[0]) + [a[1]] + list(a[2]), [a[11], a[12]]),
    # dm_subpix_map_tiles(b, d_stats, hm, wm, d_map (in place), stream)
    'dm_subpix_map_tiles': lambda a: (_tiles(a[0]) + [a[1], a[4]], [a[4]]),
}
LEVEL_KERNELS = ('dm_corr_level1', 'dm_corr_level12')


def _addr(p):
    if isinstance(p, ctypes.c_void_p):
        p = p.value
    return int(p) if p else None


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def _caller(skip=()):
    """(function name, frame) of the nearest caller outside this file's plumbing and ``skip``."""
    f = sys._getframe(2)
    while f.f_code.co_name in skip or f.f_code.co_name == '__enter__':      # (contextlib's, around Cuda.stream)
        f = f.f_back
    return f.f_code.co_name, f


class Stream:
    def __init__(self, model, name):
        self.model, self.name = model, name
        self.tick, self.vc = 0, {}
        self.cuda_stream = 0x1000 + 16 * len(model.streams)      # the handle the library is given
        model.streams.append(self)

    def __repr__(self):
        return self.name

    def _merge(self, vc):
        for s, t in vc.items():
            if self.vc.get(s, 0) < t:
                self.vc[s] = t

    def wait_event(self, ev):
        key = 'wait:%s:%s<-%s' % (_caller()[0], self.name, ev.stream.name if ev.stream else 'unrecorded')
        if self.model.call(key) and ev.vc is not None:
            self._merge(ev.vc)

    def wait_stream(self, other):
        key = 'wait:%s:%s<-%s' % (_caller()[0], self.name, other.name)
        if self.model.call(key):
            self._merge(other.vc)

    def synchronize(self):
        self.model.sync()


class Event:
    def __init__(self, model, **kw):
        self.model, self.stream, self.tick, self.vc = model, None, 0, None

    def record(self, stream=None):
        s = stream if stream is not None else self.model.current
        self.stream, self.tick, self.vc = s, s.tick, dict(s.vc)

    def query(self):
        return True

    def synchronize(self):
        self.model.sync()


class Block:
    """One allocation: the unit of both checks.  ``pool`` None: memory the model did not hand out (the
    images of a batch), ordered but never freed."""

    def __init__(self, model, label, base, nbytes, pool):
        self.model, self.label, self.base, self.nbytes, self.pool = model, label, base, nbytes, pool
        self.recorded, self.uses = set(), []          # uses: (stream, tick, entry)
        self.write, self.reads = None, []             # the last write, the reads since
        self.dropped = False

    def __del__(self):
        try:
            self.model.drop(self)
        except Exception:      # (interpreter shutdown)
            pass


class Tensor:
    """What the model hands out for torch.empty & co.: a shape, a dtype and a Block."""

    is_cuda = True

    def __init__(self, block, shape, dtype, device, offset=0):
        self.block, self.shape, self.dtype, self.device, self.offset = block, tuple(shape), dtype, device, offset

    def data_ptr(self):
        return self.block.base + self.offset

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def element_size(self):
        return torch.empty((), dtype=self.dtype).element_size()

    def is_contiguous(self):
        return True

    def contiguous(self):
        return self

    def record_stream(self, stream):
        key = 'record:%s:%s@%s' % (_caller()[0], self.block.label, stream.name)
        if self.block.model.call(key):
            self.block.recorded.add(stream)

    def __getitem__(self, key):
        if key is None:
            return Tensor(self.block, (1,) + self.shape, self.dtype, self.device, self.offset)
        row = self.element_size() * int(np.prod(self.shape[1:], dtype=np.int64))
        if isinstance(key, slice):
            r = range(*key.indices(self.shape[0]))
            assert r.step == 1
            return Tensor(self.block, (len(r),) + self.shape[1:], self.dtype, self.device, self.offset + r.start * row)
        return Tensor(self.block, self.shape[1:], self.dtype, self.device, self.offset + int(key) * row)

    def __setitem__(self, key, value):      # a copy enqueued on the current stream
        m = self.block.model
        m.op('copy', m.current, [value.data_ptr()] if isinstance(value, Tensor) else [], [self.data_ptr()])


class Cuda:
    """What engine / shard / _lib see as torch.cuda."""

    def __init__(self, model):
        self._m = model

    def Stream(self, *a, **kw):
        return self._m.stream('stream%d' % len(self._m.streams))

    def Event(self, *a, **kw):
        return Event(self._m, **kw)

    def current_stream(self, device=None):
        return self._m.current

    @contextlib.contextmanager
    def stream(self, s):
        m = self._m
        if s is None or not m.call('ctx:%s:%s' % (_caller()[0], s.name)):
            yield
            return
        prev, m.current = m.current, s
        try:
            yield
        finally:
            m.current = prev

    def is_available(self):
        return True

    def current_device(self):
        return 0

    def synchronize(self, device=None):
        self._m.sync()


class TorchModel:
    """The name ``torch`` of a swapped module: the real one but for ``cuda`` and the allocations."""

    def __init__(self, model):
        self._m, self.cuda = model, Cuda(model)
        self.Tensor = (torch.Tensor, Tensor)          # isinstance(x, torch.Tensor) holds for both

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device):
        if len(shape) == 1 and not isinstance(shape[0], (int, np.integer)):
            shape = tuple(shape[0])
        name, f = _caller(('_alloc', 'empty', 'empty_like', 'zeros', '_empty_level'))
        line = linecache.getline(f.f_code.co_filename, f.f_lineno)
        got = re.match(r'\s*(?:self\.)?_?(\w+)\s*=[^=]', line)
        label = got.group(1) if got else '%s:%d' % (name, f.f_lineno)
        return self._m.alloc(label, tuple(int(s) for s in shape), dtype or torch.float32, device)

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._alloc(size, dtype, device)

    zeros = empty

    def empty_like(self, t, dtype=None, device=None, **kw):
        return self._alloc(tuple(t.shape), dtype or t.dtype, device or t.device)


class Library:
    """The loaded library: the entries of ENTRIES are logged, dm_stats_bytes answers a constant, and
    ``unsupported`` makes dm_corr_level12 answer DM_ERR_UNSUPPORTED (what it says for a 16 x 16 tile)."""

    def __init__(self, model, unsupported=False):
        self._m, self._unsupported = model, unsupported

    def __getattr__(self, name):
        if name == 'dm_stats_bytes':
            return lambda b: 4096
        if name not in ENTRIES:
            raise AttributeError('%s: no read / write set in ENTRIES' % name)

        def entry(*args):
            if name == 'dm_corr_level12' and self._unsupported:
                return L.DM_ERR_UNSUPPORTED
            reads, writes = ENTRIES[name](args)
            stream = self._m.by_handle[_addr(args[-1])]
            self._m.op(name, stream, reads, writes)
            return L.DM_OK
        return entry


class Model:
    def __init__(self, skip=()):
        self.skip = set(skip)
        self.seen = collections.Counter()             # every call key, skipped or not
        self.streams, self.log, self.violations = [], [], []
        self.default = self.stream('default')
        self.current = self.default
        self.blocks = weakref.WeakValueDictionary()   # base address -> Block
        self.cuda = Cuda(self)
        self.torch = TorchModel(self)
        self._next = 1

    # ---- streams --------------------------------------------------------------------------------
    def stream(self, name):
        return Stream(self, name)

    @property
    def by_handle(self):
        return {s.cuda_stream: s for s in self.streams}

    def call(self, key):
        """Count a wait / record / context call; False when the case plants its omission."""
        self.seen[key] += 1
        return key not in self.skip

    def sync(self):
        """A host synchronize: everything enqueued so far is done before anything enqueued later."""
        for s in self.streams:
            for o in self.streams:
                s._merge(o.vc)

    # ---- memory ---------------------------------------------------------------------------------
    def alloc(self, label, shape, dtype, device):
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        base = (1 << 56) + (self._next << 32)      # (above every address a host tensor can have)
        self._next += 1
        blk = Block(self, label, base, nbytes, self.current)
        self.blocks[base] = blk
        return Tensor(blk, shape, dtype, device)

    def external(self, t, label):
        """A real (host) tensor the model only orders: the images and origins of a TileBatch."""
        blk = Block(self, label, t.data_ptr(), t.numel() * t.element_size(), None)
        self._ext = getattr(self, '_ext', []) + [blk]
        self.blocks[blk.base] = blk
        return blk

    def block(self, p):
        p = _addr(p)
        if p is None:
            return None
        blk = self.blocks.get(p if p < (1 << 56) else p >> 32 << 32)
        assert blk is not None and blk.base <= p <= blk.base + blk.nbytes, 'pointer %#x is no live block' % p
        return blk

    # ---- the log and check (a) --------------------------------------------------------------------
    @staticmethod
    def before(stamp, vc):
        return vc.get(stamp[0], 0) >= stamp[1]

    def op(self, name, stream, reads=(), writes=()):
        stream.tick += 1
        stream.vc[stream] = stream.tick
        stamp, vc = (stream, stream.tick, name), dict(stream.vc)
        rb = [b for b in map(self.block, reads) if b is not None]
        wb = [b for b in map(self.block, writes) if b is not None]
        self.log.append(dict(name=name, stream=stream, tick=stream.tick, vc=vc, reads=[b.label for b in rb],
                             writes=[b.label for b in wb]))
        for b in rb + wb:
            if b.write is not None and not self.before(b.write, vc):
                self.violations.append('order %s<-%s: %s on %s touches %s before %s on %s has written it'
                                       % (stream, b.write[0], name, stream, b.label, b.write[2], b.write[0]))
        for b in wb:
            for r in b.reads:
                if not self.before(r, vc):
                    self.violations.append('order %s<-%s: %s on %s overwrites %s while %s on %s may still read it'
                                           % (stream, r[0], name, stream, b.label, r[2], r[0]))
        for b in rb:
            b.reads.append(stamp)
        for b in wb:
            b.write, b.reads = stamp, []
        for b in set(rb + wb):
            b.uses.append(stamp)
        return len(self.log) - 1

    # ---- check (b) ------------------------------------------------------------------------------
    def drop(self, blk):
        if blk.dropped or blk.pool is None:
            return
        blk.dropped = True
        for s, tick, name in blk.uses:
            if s is not blk.pool and s not in blk.recorded and not self.before((s, tick), blk.pool.vc):
                self.violations.append('life %s@%s: %s comes from the pool of %s, %s used it on %s, and it was freed '
                                       'without record_stream(%s)' % (blk.label, s, blk.label, blk.pool, name, s, s))
                break

    def finish(self):
        """The run ends: whatever is still alive is dropped now, the worst moment."""
        for blk in list(self.blocks.values()):
            self.drop(blk)
        return self.violations

    # ---- H5, H11: where a level kernel sits ---------------------------------------------------------
    def level_ops(self, lo=0, hi=None):
        return [e for e in self.log[lo:hi] if e['name'] in LEVEL_KERNELS]

    def bracket(self, events, wait, lo, stream):
        """events[0] / events[1] bracket the level kernel of log[lo:] on ``stream``, the stream it really
        ran on, and ``wait`` completes before events[0]."""
        ops = self.level_ops(lo)
        assert len(ops) == 1, [e['name'] for e in self.log[lo:]]
        k, (e0, e1) = ops[0], events
        if not (k['stream'] is stream and e0.stream is stream and e1.stream is stream
                and e0.tick < k['tick'] <= e1.tick):
            self.violations.append('bracket %s: events on %s / %s around %s on %s (expected %s)'
                                   % (stream, e0.stream, e1.stream, k['name'], k['stream'], stream))
        if wait is not None and not self.before((wait.stream, wait.tick), e0.vc or {}):
            self.violations.append('bracket %s<-%s: events[0] on %s does not come after the wait event of %s'
                                   % (e0.stream, wait.stream, e0.stream, wait.stream))

    def chained(self, ops):
        """Consecutive level kernels run one after another (serialised by one stream, or by ``wait``)."""
        for a, b in zip(ops, ops[1:]):
            if not self.before((a['stream'], a['tick']), b['vc']):
                self.violations.append('chain %s<-%s: the level kernel on %s does not wait for the one before it on %s'
                                       % (b['stream'], a['stream'], b['stream'], a['stream']))


@contextlib.contextmanager
def modelled(skip=(), unsupported=False):
    """One run under the model: engine / shard / _lib see its torch, L.load() its library."""
    m = Model(skip)
    with pytest.MonkeyPatch.context() as mp:
        for mod in SWAPPED:
            mp.setattr(mod, 'torch', m.torch)
        mp.setattr(L, '_lib', Library(m, unsupported))
        yield m


def _batch(m, T=3, s=32):
    img = torch.zeros((s + WS - 1, T * s + WS - 1), dtype=torch.uint8)
    b = engine.TileBatch(img, img.clone(), [(0, t * s) for t in range(T)], s, s, WS, NCC, device=torch.device('cpu'))
    for t, label in ((b.img1, 'img1'), (b.img2, 'img2'), (b.origins, 'origins')):
        m.external(t, label)
    return b


def _images(b):
    return [b.img1.data_ptr(), b.img2.data_ptr(), b.origins.data_ptr()]


# ---------------------------------------------------------------------------------------------
# the scenarios
# ---------------------------------------------------------------------------------------------
def run_pyramid(fuse=2, unsupported=False, cut=False, ss=False, ls=False, wait=False, own=False, ctor=False, skip=()):
    """One pyramid as a pipelined caller drives it: images uploaded on the pair stream, build with every
    keyword, match, the pyramid dropped, the map read on the pair stream.  ``own``: the pyramid has the
    pair stream as its own (``stream=pair``) and torch's current stream is another one throughout;
    else it has none and the pair stream is current.  ``ctor``: the pyramid (without a stream of its own) is
    constructed while yet another stream is current, and only built and matched under the pair stream."""
    with modelled(skip, unsupported) as m:
        pair, level, stats, ext = m.stream('pair'), m.stream('level'), m.stream('stats'), m.stream('ext')
        b = _batch(m)
        with m.cuda.stream(m.default if own else pair):
            m.op('upload', pair, [], _images(b))
            w = None
            if wait:
                m.op('the level kernel before', ext)
                w = m.cuda.Event()
                w.record(ext)
            with m.cuda.stream(m.stream('other') if ctor else None):
                pyr = engine.DevicePyramid(b, stream=pair if own else None, build=False, fuse_level2=fuse,
                                           stats_stream=stats if ss else None)
            ev, lo = (m.cuda.Event(), m.cuda.Event()), len(m.log)
            n = 3 if cut else None
            pyr.build(events=ev, wait=w, nlev=n, level_stream=level if ls else None)
            out = pyr.match(nlev=n)
            m.bracket(ev, w, lo, level if ls else pair)
            del pyr
            m.op('stitch', pair, [out.data_ptr()])
            del out
        return m.finish(), m.seen


def run_refine(fuse=2, own=False, built=False, current='pair', skip=()):
    """subpix_map_tiles on a second stream (``side``), the map written there just before; the pyramid
    built (``built``) or only its stats, so that mode 2 derives the min / max on demand; then the
    pyramid is dropped and the map read on ``side``.  ``current``: torch's current stream at the call
    of subpix_map_tiles when the pyramid has no stream of its own ('pair': the one it was built under;
    'default': another)."""
    with modelled(skip) as m:
        pair, side = m.stream('pair'), m.stream('side')
        b = _batch(m)
        with m.cuda.stream(m.default if own else pair):
            m.op('upload', pair, [], _images(b))
            pyr = engine.DevicePyramid(b, stream=pair if own else None, build=built, fuse_level2=fuse)
            pyr.compute_stats()
        with m.cuda.stream(side):
            mm = m.torch.empty((b.T, 3, 8, 8), dtype=torch.float64, device=b.device)
        m.op('match_levels', side, [], [mm.data_ptr()])
        with m.cuda.stream(m.default if (own or current == 'default') else pair):
            engine.subpix_map_tiles(pyr, mm, stream=side)
        del pyr
        m.op('read the map', side, [mm.data_ptr()])
        del mm
        return m.finish(), m.seen


def run_band(ss=True, ls=True, wait=True, skip=()):
    """BandSolver.start as bench.py's split solve drives it: 7 tiles of 16 x 16 in 3 chunks on the
    current (pair) stream, the chunks' results assembled and read there."""
    with modelled(skip, unsupported=True) as m:
        pair, level, stats, ext = m.stream('pair'), m.stream('level'), m.stream('stats'), m.stream('ext')
        s, T = 16, 7
        img = torch.zeros((s + WS - 1, T * s + WS - 1), dtype=torch.uint8)
        band = shard.BandSolver(img, img.clone(), [(0, t * s) for t in range(T)], s, s, WS, NCC,
                                device=torch.device('cpu'), chunks=3)
        assert [len(i) for i in band.chunk_idx] == [3, 3, 1]
        for t, label in ((band.img1, 'img1'), (band.img2, 'img2')):
            m.external(t, label)
        for c, b in enumerate(band.batches):
            m.external(b.origins, 'origins%d' % c)
        with m.cuda.stream(pair):
            m.op('upload', pair, [], [band.img1.data_ptr(), band.img2.data_ptr()] + [b.origins.data_ptr() for b in band.batches])
            w = None
            if wait:
                m.op('the level kernel before', ext)
                w = m.cuda.Event()
                w.record(ext)
            evs = []
            g = band.start(events=evs, wait=w, level_stream=level if ls else None, stats_stream=stats if ss else None)
            assert len(evs) == 3 and len(m.level_ops()) == 3
            res = g.result()
            m.op('stitch', pair, [res.data_ptr()])
            lv = m.level_ops()
            if w is not None:      # ``wait`` applies to chunk 0 only, whose events[0] comes after it
                if not m.before((ext, w.tick), evs[0][0].vc):
                    m.violations.append('bracket %s<-ext: chunk 0 does not wait' % evs[0][0].stream)
                assert sum(n for k, n in m.seen.items() if k.startswith('wait:build:') and k.endswith('<-ext')) == 1
            for e, k in zip(evs, lv):
                if not (e[0].stream is k['stream'] and e[0].tick < k['tick'] <= e[1].tick):
                    m.violations.append('bracket %s: a chunk\'s events do not bracket its level kernel' % k['stream'])
            del g, res
        return m.finish(), m.seen


def run_pipeline(ls=True, ss=True, chain=True, skip=()):
    """The pipeline as bench.py drives it (Pipeline.step + Solver.compute): one batch uploaded before a
    synchronize, four solves back to back on two pair streams in turn, every level kernel on one level
    stream and the stats on one stats stream, or, without a level stream, each level kernel waiting
    for the end event of the one before it (``wait``)."""
    with modelled(skip) as m:
        pairs = [m.stream('pair'), m.stream('pair2')]
        level, stats = m.stream('level'), m.stream('stats')
        b = _batch(m)
        m.op('upload', m.default, [], _images(b))
        m.sync()
        prev, held = None, []
        for k in range(4):
            st = pairs[k % 2]
            with m.cuda.stream(st):
                pyr = engine.DevicePyramid(b, build=False, stats_stream=stats if (ss and ls) else None)
                ev, lo = (m.cuda.Event(), m.cuda.Event()), len(m.log)
                w = prev if (not ls and chain) else None
                pyr.build(events=ev, wait=w, nlev=3, level_stream=level if ls else None)
                out = pyr.match(nlev=3)
                m.bracket(ev, w, lo, level if ls else st)
                del pyr
                dmap = m.torch.empty((1, 32, 96), dtype=torch.float64, device=b.device)
                m.op('dm_stitch', st, [out.data_ptr()], [dmap.data_ptr()])
                del out
                held.append(dmap)          # bench.py keeps every solve's maps to compare them afterwards
                prev = ev[1]
        if ls or chain:
            m.chained(m.level_ops())
        m.sync()
        for d in held:
            m.op('compare', m.default, [d.data_ptr()])
        m.sync()
        del held, d, dmap
        return m.finish(), m.seen


RUN = {'pyramid': run_pyramid, 'refine': run_refine, 'band': run_band, 'pipeline': run_pipeline}

# ---------------------------------------------------------------------------------------------
# the ledger: DESIGN.md 5c's rows.  Each case is (scenario, its keywords, the call made a no-op, what
# the checker must then say); the same keywords without the omission must leave nothing to say.
# ---------------------------------------------------------------------------------------------
ALL3 = dict(ss=True, ls=True)
LEDGER = {
    'H1': [('pyramid', dict(ss=True), 'wait:compute_stats:stats<-pair', 'order stats<-pair: dm_corr_stats on stats touches img1'),
           ('pyramid', dict(ALL3, own=True), 'wait:compute_stats:stats<-pair', 'order stats<-pair')],
    'H2': [('pyramid', dict(ss=True), 'wait:compute_stats:pair<-stats', 'order pair<-stats: dm_corr_level12 on pair touches stats'),
           ('pyramid', dict(ss=True, fuse=0), 'wait:compute_stats:pair<-stats', 'order pair<-stats: dm_corr_level1 on pair')],
    'H3': [('pyramid', dict(ALL3), 'wait:build:level<-stats', 'order level<-stats: dm_corr_level12 on level touches stats'),
           ('pyramid', dict(ALL3, fuse=0, own=True), 'wait:build:level<-stats', 'order level<-stats: dm_corr_level1 on level')],
    'H4': [('pyramid', dict(ls=True), 'wait:build:level<-pair', 'order level<-pair: dm_corr_level12 on level touches stats'),
           ('pyramid', dict(ls=True, fuse=1, cut=True), 'wait:build:level<-pair', 'order level<-pair')],
    'H5': [('pyramid', dict(ALL3, wait=True), 'wait:build:level<-ext', 'bracket level<-ext'),
           ('pyramid', dict(wait=True), 'wait:build:pair<-ext', 'bracket pair<-ext'),
           ('pyramid', dict(ls=True, wait=True, unsupported=True), 'wait:build:level<-ext', 'bracket level<-ext')],
    'H6': [('pyramid', dict(ALL3, fuse=0), 'wait:build:pair<-level', 'order pair<-level: dm_aggregate on pair touches l1'),
           ('pyramid', dict(ALL3, fuse=1), 'wait:build:pair<-level', 'order pair<-level: dm_aggregate on pair touches l2'),
           ('pyramid', dict(ALL3, fuse=2), 'wait:build:pair<-level', 'order pair<-level: dm_aggregate on pair touches l2'),
           ('pyramid', dict(ALL3, fuse=2, cut=True), 'wait:build:pair<-level', 'order pair<-level: dm_match on pair touches'),
           ('pyramid', dict(ALL3, fuse=2, unsupported=True), 'wait:build:pair<-level', 'order pair<-level: dm_aggregate on pair touches l1'),
           ('pyramid', dict(ls=True, fuse=2, unsupported=True, cut=True), 'wait:build:pair<-level', 'order pair<-level')],
    'H7': [('pyramid', dict(ALL3), 'record:_pair:stats@pair', 'life stats@pair'),
           ('pyramid', dict(ALL3, ctor=True), 'record:_pair:stats@pair', 'life stats@pair'),
           ('pyramid', dict(ctor=True), 'record:_pair:stats@pair', 'life stats@pair'),
           ('pyramid', dict(ALL3), 'record:build:stats@level', 'life stats@level'),
           ('pyramid', dict(ALL3, fuse=2), 'record:build:l2@pair', 'life l2@pair'),
           ('pyramid', dict(ALL3, fuse=1), 'record:build:l1@pair', 'life l1@pair'),
           ('pyramid', dict(ls=True, fuse=0), 'record:build:l1@pair', 'life l1@pair'),
           ('pyramid', dict(ls=True, fuse=2, unsupported=True), 'record:build:l1@pair', 'life l1@pair')],
    'H8': [('pyramid', dict(own=True), 'ctx:match:pair', 'life out@pair'),
           ('pyramid', dict(own=True), 'ctx:build:pair', 'life nxt@pair'),
           ('pyramid', dict(ALL3, own=True, fuse=0, cut=True), 'ctx:match:pair', 'life out@pair')],
    'H9': [('refine', dict(own=True), 'wait:subpix_map_tiles:side<-pair', 'order side<-pair: dm_subpix_map_tiles on side touches stats'),
           ('refine', dict(own=False), 'wait:subpix_map_tiles:side<-pair', 'order side<-pair: dm_subpix_map_tiles on side touches stats'),
           ('refine', dict(own=False, built=True, fuse=0), 'wait:subpix_map_tiles:side<-pair', 'order side<-pair'),
           ('refine', dict(own=False, current='default'), 'wait:_pair:default<-pair', 'order side<-pair'),
           ('refine', dict(own=True), 'record:subpix_map_tiles:stats@side', 'life stats@side'),
           ('refine', dict(own=False), 'record:subpix_map_tiles:stats@side', 'life stats@side')],
    'H10': [('band', dict(), 'wait:build:pair<-level', 'order pair<-level'),
            ('band', dict(), 'record:build:l1@pair', 'life l1@pair'),
            ('band', dict(), 'record:build:stats@level', 'life stats@level'),
            ('band', dict(), 'wait:build:level<-ext', 'bracket level<-ext'),
            ('band', dict(ss=False, ls=False), 'wait:build:pair<-ext', 'bracket pair<-ext')],
    'H11': [('pipeline', dict(), 'wait:build:pair2<-level', 'order pair2<-level'),
            ('pipeline', dict(), 'record:build:l2@pair', 'life l2@pair'),
            ('pipeline', dict(), 'record:_pair:stats@pair2', 'life stats@pair2'),
            ('pipeline', dict(ls=False), 'wait:build:pair2<-pair', 'chain pair2<-pair'),
            ('pipeline', dict(ls=False), 'wait:build:pair<-pair2', 'chain pair<-pair2')],
}
CASES = [(row, i) for row in LEDGER for i in range(len(LEDGER[row]))]


@pytest.mark.parametrize('row,i', CASES, ids=['%s-%d' % c for c in CASES])
def test_ledger_row_is_ordered_and_its_omission_is_named(row, i):
    scenario, kw, key, says = LEDGER[row][i]
    clean, seen = RUN[scenario](**kw)
    assert clean == [], clean
    assert seen[key] >= 1, 'the run never makes the call %s: %s' % (key, sorted(seen))
    planted, _ = RUN[scenario](skip=[key], **kw)
    assert any(v.startswith(says) for v in planted), (key, planted)


def test_every_combination_build_accepts():
    """fuse_level2 x the UNSUPPORTED fallback x nlev cut / full x stats_stream x level_stream x wait x the
    pyramid's own stream set / None: no violation of (a) or (b), and the events bracket the level kernel
    on the stream it ran on."""
    n = 0
    for fuse, unsupported, cut, ss, ls, wait, own in itertools.product((0, 1, 2), (False, True), (False, True),
                                                                       *[(False, True)] * 4):
        got, _ = run_pyramid(fuse, unsupported, cut, ss, ls, wait, own)
        assert got == [], (fuse, unsupported, cut, ss, ls, wait, own, got)
        n += 1
    assert n == 192
    for fuse, ss, ls in itertools.product((0, 2), (False, True), (False, True)):
        got, _ = run_pyramid(fuse, ss=ss, ls=ls, ctor=True)
        assert got == [], (fuse, ss, ls, 'ctor', got)
    for fuse, own, built, current in itertools.product((0, 1, 2), (False, True), (False, True), ('pair', 'default')):
        got, _ = run_refine(fuse, own, built, current)
        assert got == [], (fuse, own, built, current, got)
    for ss, ls, wait in itertools.product(*[(False, True)] * 3):
        got, _ = run_band(ss, ls, wait)
        assert got == [], (ss, ls, wait, got)
    for ls, ss, chain in itertools.product(*[(False, True)] * 3):
        got, _ = run_pipeline(ls, ss, chain)
        assert got == [], (ls, ss, chain, got)


def test_a_pipeline_without_chaining_is_seen_unchained():
    """The checker's own eye for H11: with neither a level stream nor ``wait`` the level kernels of two
    pair streams are not ordered, and ``chained`` says so."""
    with modelled() as m:
        a, b = m.stream('pair'), m.stream('pair2')
        m.op('dm_corr_level12', a)
        m.op('dm_corr_level12', b)
        m.chained(m.level_ops())
        assert m.violations == ['chain pair2<-pair: the level kernel on pair2 does not wait for the one before it on pair']


def test_model_basics():
    """Clocks, the two checks and the drop of a last reference, on hand-made logs."""
    with modelled() as m:
        a, b = m.stream('a'), m.stream('b')
        with m.cuda.stream(a):
            t = m.torch.empty((4,), dtype=torch.float64, device='cpu')
        assert t.block.label == 't' and t.block.pool is a and t.block.nbytes == 32
        m.op('w', a, [], [t.data_ptr()])
        m.op('r', b, [t.data_ptr()])                       # no wait: (a)
        assert m.violations == ['order b<-a: r on b touches t before w on a has written it']
        ev = m.cuda.Event()
        ev.record(a)
        b.wait_event(ev)
        m.op('r2', b, [t[None].data_ptr()])               # ordered now; used on b, not recorded
        assert len(m.violations) == 1
        m.op('w2', a, [], [t[1:].data_ptr()])              # overwrites while b may still read
        assert m.violations[1].startswith('order a<-b: w2 on a overwrites t while r on b')
        del t                                              # the last reference: (b)
        assert m.violations[-1].startswith('life t@b: t comes from the pool of a, r used it on b')
    with modelled() as m:
        a, b = m.stream('a'), m.stream('b')
        with m.cuda.stream(a):
            t = m.torch.empty(4, dtype=torch.uint8, device='cpu')
            u = m.torch.empty_like(t)
        m.op('r', b, [t.data_ptr(), u.data_ptr()])
        t.record_stream(b)                                 # recorded: free to drop
        a.wait_stream(b)                                   # the pool's stream has waited: free to drop
        del t, u
        assert m.finish() == [] and m.seen['record:test_model_basics:t@b'] == 1
    with modelled(skip=['record:test_model_basics:t@b']) as m:
        a, b = m.stream('a'), m.stream('b')
        with m.cuda.stream(a):
            t = m.torch.empty(4, dtype=torch.uint8, device='cpu')
        m.op('r', b, [t.data_ptr()])
        t.record_stream(b)
        assert m.finish() and m.violations[0].startswith('life t@b')      # alive at the end counts as dropped
    assert engine.torch is torch and shard.torch is torch and L.torch is torch and not isinstance(L._lib, Library)


def test_entries_table_matches_the_header():
    """Every entry of ENTRIES is an entry of the header that takes a stream last, and every entry engine's
    pyramid code calls has a row (an entry without one raises in the model)."""
    from test_guarded_host import stream_entries
    assert set(ENTRIES) <= set(stream_entries())
    src = open(engine.__file__).read()
    body = src[src.index('class DevicePyramid'):src.index('def match_levels')] + \
        src[src.index('def subpix_map_tiles'):src.index('def cal_map')]
    called = set(re.findall(r'\blib\.(dm_[a-z0-9_]+)\(', body)) - {'dm_stats_bytes'}
    assert called and called <= set(ENTRIES), sorted(called - set(ENTRIES))


def test_design_ledger_has_a_case_for_every_row():
    """DESIGN.md 5c's rows and LEDGER's are the same rows; every test the table names exists."""
    txt = open(os.path.join(os.path.dirname(L.HERE), 'DESIGN.md')).read()
    sec = txt[txt.index('### 5c.'):]
    sec = sec[:sec.index('\n## ')]
    rows = re.findall(r'^\| \*\*(H\d+)\*\* \|', sec, flags=re.M)
    assert rows == sorted(set(rows), key=lambda r: int(r[1:])) and set(rows) == set(LEDGER), (rows, sorted(LEDGER))
    assert {'H%d' % k for k in range(1, 12)} <= set(rows)
    import test_streams_gpu as G
    for row in rows:
        assert LEDGER[row], row
        assert any(c.row == row for c in G.CASES), 'no GPU case for %s' % row
    for name in re.findall(r'`(test_[a-z0-9_]+)`', sec):
        assert hasattr(G, name) or name in globals(), name


# ---------------------------------------------------------------------------------------------
# the pairs of the GPU half: a real pair and a decoy of one shape
# ---------------------------------------------------------------------------------------------
SHAPES = {              # name: (tiles, tile side): the smallest shapes that reach each code path
    'mfma32': (3, 32),          # the fused MFMA level kernel (dm_corr_level12)
    'fallback16': (3, 16),      # dm_corr_level12 answers DM_ERR_UNSUPPORTED: dm_corr_level1 + dm_aggregate
    'cut64': (1, 64),           # one tile, nlev cut to 3
    'band16': (7, 16),          # BandSolver: 7 tiles in 3 chunks
}
SEEDS = {'real': (1, 2), 'decoy': (2, -3)}      # (seed, dx) of stereo_pair


def pair(shape, which):
    """(img1, img2, origins, side) of a shape: T tiles side by side in one row."""
    T, s = SHAPES[shape]
    seed, dx = SEEDS[which]
    a, b = stereo_pair(s + WS - 1, T * s + WS - 1, seed=seed, dx=dx)
    return a, b, [(0, t * s) for t in range(T)], s


@functools.lru_cache(maxsize=None)
def oracle_match(shape, which, nlev=None):
    """The oracle's matches (pinned pow) of every tile, float64 [T][3][s][s]; ``nlev``: on the co_map_list
    cut to that many levels."""
    from oracle import oracle as O
    a, b, origins, s = pair(shape, which)
    O.set_pow_mode('pinned')
    try:
        out = []
        for r, c in origins:
            l0 = O.corr_l0(a[r:r + s + WS - 1, c:c + s + WS - 1], b[r:r + s + WS - 1, c:c + s + WS - 1], WS)
            levels, _, _ = O.pyramid(l0)
            out.append(O.match(levels[:nlev] if nlev else levels, sub_pix=True))
        res = np.stack(out)
    finally:
        O.set_pow_mode('libm')
    res.setflags(write=False)
    return res


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_decoy_differs_from_the_real_pair(shape):
    """In every tile the matched position (row, col) of the decoy differs from the real pair's in at
    least half the cells: a solve that read the decoy's recycled stats, levels or maps cannot give the
    real pair's bytes by coincidence."""
    real, decoy = oracle_match(shape, 'real'), oracle_match(shape, 'decoy')
    assert real.shape == decoy.shape == (SHAPES[shape][0], 3, SHAPES[shape][1], SHAPES[shape][1])
    for t in range(len(real)):
        differ = (real[t, :2] != decoy[t, :2]).any(0).mean()
        assert differ >= 0.5, (shape, t, differ)
