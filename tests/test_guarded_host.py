"""Guarded, poisoning allocations for the buffer contract of the C ABI (include/dmstereo.h): a
call writes only inside the buffers it was given, works with a workspace of exactly the bytes its
dm_*_bytes entry reports ("16-byte aligned, contents arbitrary"), and its result does not depend
on bytes outside its inputs.  torch's caching allocator hides all three: it rounds every block
up, aligns it to 512 bytes and very often hands out zeroed memory.

This file holds the helpers (tests/test_guarded_gpu.py runs every entry point under them) and
their own tests on CPU tensors:

  Guarded          the allocator.  Every buffer is a view into a uint8 arena laid out as front
                   guard | payload | back guard; the guards, and the payload of ``empty``, hold a
                   poison byte; ``check()`` asserts that every guard byte still does.
  Guarded.torch    stands in for the name ``torch`` in the modules of the package that allocate
                   (``install``): everything is forwarded to the real module but ``empty``,
                   ``zeros``, ``full`` and their ``*_like`` forms, which come from the allocator
                   with exactly the bytes asked for at an address that is 16-byte aligned and no
                   more.
  Guarded.guarded  a buffer the test itself passes in (an image, a map, a mask, an ``out=``
                   tensor): the same layout at the element's natural alignment only.
  Recorder         wraps the loaded library so that the dm_* entries a case called can be read
                   back.
  stream_entries   the entries of the header that take a stream: the ledger test holds them
                   against the cases of the GPU file.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import _lib as L

POISONS = (0xFF, 0x00)
GUARD_MIN = 64 << 10              # bytes of a guard, at least
TILE_BYTES = 64 * 64 * 8          # one 64 x 64 tile of doubles: "the rest of the tile" past an edge
WORK_ALIGN = 16                   # what the header promises for a workspace, and no more

# the modules of the package that allocate device memory (torch.empty / zeros / full)
ALLOCATING = ('deepmatching_stereo_matching_amd.engine', 'deepmatching_stereo_matching_amd.shard',
              'deepmatching_stereo_matching_amd.postproc', 'deepmatching_stereo_matching_amd.misc.Correlation_map',
              'deepmatching_stereo_matching_amd.misc.sub_pix_cal')

# entries with a stream that no guarded case has to run: self-tests of device helpers, which take
# two plain arrays and no workspace (tests/test_pow_gpu.py, tests/test_f16_num.py run them)
LEDGER_EXEMPT = ('dm_pow14_variant', 'dm_debug_num_tile_f16')


def _modules():
    import importlib
    return [importlib.import_module(m) for m in ALLOCATING]


def guard_bytes(shape, itemsize):
    """Bytes of each guard of a payload of this shape: GUARD_MIN, or one full row of the payload
    plus one 64 x 64 tile of doubles if that is more; a multiple of 64."""
    row = (int(shape[-1]) if len(shape) else 1) * itemsize
    return (max(GUARD_MIN, row + TILE_BYTES) + 63) & ~63


def _size(size, kw):
    if 'size' in kw:
        size = (kw.pop('size'),)
    if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _site(depth):
    f = sys._getframe(depth)
    return '%s:%d' % (os.path.basename(f.f_code.co_filename), f.f_lineno)


class Arena:
    """front guard | payload | back guard in one uint8 tensor ``buf``; the payload is
    buf[lo:lo + nbytes]."""

    def __init__(self, label, buf, lo, nbytes, poison):
        self.label, self.buf, self.lo, self.nbytes, self.poison = label, buf, lo, nbytes, poison

    def payload(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def changed(self):
        """None, or (side, offset): the first guard byte that no longer holds the poison; the
        offset counts from the payload's first byte (negative in the front guard)."""
        for side, g, base in (('front', self.buf[:self.lo], -self.lo),
                              ('back', self.buf[self.lo + self.nbytes:], self.nbytes)):
            bad = g != self.poison
            if bool(bad.any()):
                return side, base + int(bad.nonzero()[0, 0])
        return None


class TorchProxy:
    """The name ``torch`` of an allocating module: the real module except for the allocations."""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        return getattr(torch, name)

    def _new(self, size, kw, fill, default_dtype):
        dtype = kw.pop('dtype', None) or default_dtype
        device = kw.pop('device', None)
        kw.pop('requires_grad', None)
        if kw:
            raise TypeError('guarded allocation does not take %s' % sorted(kw))
        return self._owner.alloc(size, dtype, device, fill=fill, label=_site(3))

    def empty(self, *size, **kw):
        return self._new(_size(size, kw), kw, None, torch.get_default_dtype())

    def zeros(self, *size, **kw):
        return self._new(_size(size, kw), kw, 0, torch.get_default_dtype())

    def full(self, size, fill_value, **kw):
        default = (torch.bool if isinstance(fill_value, bool) else
                   torch.int64 if isinstance(fill_value, (int, np.integer)) else torch.get_default_dtype())
        return self._new(_size((size,), kw), kw, fill_value, default)

    def empty_like(self, t, **kw):
        kw.setdefault('dtype', t.dtype)
        kw.setdefault('device', t.device)
        return self._new(tuple(t.shape), kw, None, t.dtype)

    def zeros_like(self, t, **kw):
        kw.setdefault('dtype', t.dtype)
        kw.setdefault('device', t.device)
        return self._new(tuple(t.shape), kw, 0, t.dtype)


class Guarded:
    def __init__(self, poison):
        assert 0 <= poison <= 255
        self.poison = int(poison)
        self.arenas = []
        self.inputs = []          # (arena, a private copy of the bytes put in): check_inputs()
        self.torch = TorchProxy(self)

    # ---- allocation ---------------------------------------------------------------------------
    def alloc(self, shape, dtype, device=None, fill=None, align=WORK_ALIGN, label=None):
        """A contiguous tensor of ``shape`` and ``dtype`` whose first byte lies at an address a
        with a % (2 * align) == align, exactly numel * itemsize bytes between two guards.
        ``fill`` None: the payload holds the poison; else that value."""
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        nbytes = es * int(np.prod(shape, dtype=np.int64)) if shape else es
        g = guard_bytes(shape, es)
        assert g >= GUARD_MIN and g >= (shape[-1] if shape else 1) * es + TILE_BYTES
        buf = torch.full((g + 2 * align + nbytes + g,), self.poison, dtype=torch.uint8, device=device)
        lo = g + (align - (buf.data_ptr() + g) % (2 * align)) % (2 * align)
        arena = Arena(label or _site(2), buf, lo, nbytes, self.poison)
        self.arenas.append(arena)
        pay = arena.payload()
        if not nbytes:      # (no byte, no address)
            return torch.empty(shape, dtype=dtype, device=buf.device)
        assert pay.data_ptr() % (2 * align) == align and pay.numel() == nbytes
        t = pay.view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        return t

    def guarded(self, array, dtype=None, misalign=None, device=None, label=None):
        """A guarded device copy of ``array`` (a numpy array or a tensor) as ``dtype`` (default:
        its own).  ``misalign``: the payload address a has a % (2 * misalign) == misalign; the
        default is the element size, i.e. the element's natural alignment and no more (float64:
        a % 16 == 8, int32: a % 8 == 4, uint8: an odd address).  The bytes put in are remembered:
        check_inputs() asserts that they are still there."""
        src = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        if dtype is not None:
            src = src.to(dtype)
        es = src.element_size()
        t = self.alloc(src.shape, src.dtype, device, align=misalign or es, label=label or _site(2))
        t.copy_(src)
        self.inputs.append((self.arenas[-1], self.arenas[-1].payload().clone()))
        return t

    def out(self, shape, dtype, device=None, misalign=None, label=None):
        """A guarded ``out=`` tensor at natural alignment, pre-filled with the poison."""
        es = torch.empty((), dtype=dtype).element_size()
        return self.alloc(shape, dtype, device, align=misalign or es, label=label or _site(2))

    def written(self, t):
        """``t`` (a tensor from guarded()) is documented as written by the call: no longer an input."""
        self.inputs = [(a, c) for a, c in self.inputs if a.payload().data_ptr() != t.data_ptr()]

    # ---- checks -------------------------------------------------------------------------------
    def check(self):
        """Every guard byte of every arena still holds the poison (after a synchronize)."""
        for a in self.arenas:
            hit = a.changed()
            assert hit is None, ('buffer %s (%d bytes): the %s guard changed, first at payload offset %d'
                                 % (a.label, a.nbytes, hit[0], hit[1]))

    def check_inputs(self):
        for a, copy in self.inputs:
            bad = a.payload() != copy
            assert not bool(bad.any()), ('input %s (%d bytes) was written, first at byte %d'
                                         % (a.label, a.nbytes, int(bad.nonzero()[0, 0])))


def install(monkeypatch, poison):
    """A Guarded whose proxy replaces ``torch`` in the allocating modules until the test ends."""
    g = Guarded(poison)
    for m in _modules():
        monkeypatch.setattr(m, 'torch', g.torch)
    return g


class Recorder:
    """The loaded library with the names of the dm_* entries called kept in ``calls``."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('dm_'):
            return fn

        def entry(*args):
            self.calls.append(name)
            return fn(*args)
        return entry


def record(monkeypatch):
    rec = Recorder(L.load())
    monkeypatch.setattr(L, '_lib', rec)
    return rec


def stream_entries():
    """The entries of include/dmstereo.h whose last parameter is the stream."""
    txt = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    return sorted(name for name, args in re.findall(r'\b(dm_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;', txt)
                  if re.search(r'void\s*\*\s*stream\s*$', args.strip()))


def raw(t):
    """The bytes of a tensor (or None) as a numpy uint8 array: NaN payloads and -0.0 count."""
    if t is None:
        return None
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().copy()


# ---------------------------------------------------------------------------------------------
# the helpers' own tests (CPU tensors)
# ---------------------------------------------------------------------------------------------
DTYPES = [torch.uint8, torch.int8, torch.int32, torch.float16, torch.float32, torch.float64]


@pytest.mark.parametrize('poison', POISONS)
def test_planted_writes_are_caught_and_named(poison):
    g = Guarded(poison)
    t = g.torch.empty((3, 5), dtype=torch.float64, device='cpu')
    a = g.arenas[0]
    assert a.label.startswith('test_guarded_host.py:')
    g.check()
    other = poison ^ 0x5A
    a.buf[a.lo + a.nbytes] = other                       # one byte just after the payload
    with pytest.raises(AssertionError, match=r'test_guarded_host\.py:\d+ \(120 bytes\): the back guard changed, '
                                             r'first at payload offset 120'):
        g.check()
    a.buf[a.lo + a.nbytes] = poison
    g.check()
    a.buf[a.lo - 1] = other                              # one byte just before it
    with pytest.raises(AssertionError, match=r'the front guard changed, first at payload offset -1'):
        g.check()
    a.buf[a.lo - 1] = poison
    a.buf[0], a.buf[-1] = other, other                   # the far ends of both guards
    with pytest.raises(AssertionError, match=r'front guard changed, first at payload offset -%d' % a.lo):
        g.check()
    a.buf[0] = poison
    with pytest.raises(AssertionError, match=r'back guard changed'):
        g.check()
    a.buf[-1] = poison
    t.fill_(1.5)                                         # the payload is the caller's
    t.view(-1)[-1] = -2.0
    g.check()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[1])
def test_poison_is_visible_through_every_dtype(dtype):
    for poison in POISONS:
        g = Guarded(poison)
        t = g.torch.empty(7, 3, dtype=dtype, device='cpu')
        assert t.dtype == dtype and tuple(t.shape) == (7, 3) and t.is_contiguous()
        assert (raw(t) == poison).all() and raw(t).size == 21 * t.element_size()
        if poison == 0xFF and dtype.is_floating_point:
            assert bool(torch.isnan(t).all())            # all-ones is a NaN in every float format
        elif poison == 0xFF:
            assert bool((t == (255 if dtype == torch.uint8 else -1)).all())
        else:
            assert bool((t == 0).all())
        g.check()


def test_zeros_full_and_like_keep_their_values():
    g = Guarded(0xFF)
    z = g.torch.zeros((), dtype=torch.float64, device='cpu')
    assert z.dim() == 0 and float(z) == 0.0 and g.arenas[-1].nbytes == 8
    z2 = g.torch.zeros((4, 2), dtype=torch.int32, device='cpu')
    assert z2.dtype == torch.int32 and not bool(z2.any())
    f = g.torch.full((2, 3), 2.5, dtype=torch.float32, device='cpu')
    assert bool((f == 2.5).all())
    assert g.torch.full((3,), 7).dtype == torch.int64 and g.torch.zeros(3).dtype == torch.float32
    e = g.torch.empty_like(f)
    assert e.shape == f.shape and e.dtype == f.dtype and bool(torch.isnan(e).all())
    zl = g.torch.zeros_like(z2)
    assert zl.dtype == torch.int32 and zl.shape == z2.shape and not bool(zl.any())
    n = g.torch.empty(0, dtype=torch.uint8, device='cpu')
    assert n.numel() == 0
    g.check()
    assert len(g.arenas) == 8
    # forwarded names are the real ones
    assert g.torch.float64 is torch.float64 and g.torch.Tensor is torch.Tensor and g.torch.cuda is torch.cuda


def test_alignment_and_exact_size():
    g = Guarded(0x00)
    for dtype in DTYPES:
        for shape in [(1,), (5,), (3, 7), (2, 3, 5)]:
            t = g.torch.empty(shape, dtype=dtype, device='cpu')
            a = g.arenas[-1]
            assert t.data_ptr() % 32 == 16, (dtype, shape)                   # 16-byte aligned and no more
            assert a.nbytes == t.numel() * t.element_size()                  # exact to the byte
            assert a.lo >= GUARD_MIN and a.buf.numel() - a.lo - a.nbytes >= GUARD_MIN
    d = g.guarded(np.arange(6, dtype=np.float64).reshape(2, 3))
    i = g.guarded(np.arange(6, dtype=np.int32))
    u = g.guarded(np.arange(35, dtype=np.uint8).reshape(5, 7))
    assert d.data_ptr() % 16 == 8 and i.data_ptr() % 8 == 4 and u.data_ptr() % 2 == 1
    assert u.is_contiguous() and u.stride() == (7, 1) and bool((u.reshape(-1) == torch.arange(35)).all())
    v = g.guarded(np.zeros((4, 32), dtype=np.uint8), misalign=16)           # what a vector path may ask for
    assert v.data_ptr() % 32 == 16
    o = g.out((2, 3), torch.float64)
    assert o.data_ptr() % 16 == 8 and (raw(o) == 0).all()
    w = g.guarded(np.array([1, 0, 1]), dtype=torch.uint8)
    assert w.dtype == torch.uint8 and w.tolist() == [1, 0, 1]
    g.check()


def test_guard_covers_a_row_and_a_tile():
    assert guard_bytes((33, 31), 8) == GUARD_MIN
    assert guard_bytes((), 8) == GUARD_MIN
    for shape, es in [((3, 16384), 8), ((2, 1 << 20), 1), ((100000,), 4)]:
        gb = guard_bytes(shape, es)
        assert gb >= shape[-1] * es + TILE_BYTES and gb >= GUARD_MIN and gb % 64 == 0
    g = Guarded(0xFF)
    t = g.torch.empty((2, 9000), dtype=torch.float64, device='cpu')
    a = g.arenas[0]
    assert a.lo >= 72000 + TILE_BYTES and a.buf.numel() - a.lo - a.nbytes >= 72000 + TILE_BYTES
    assert tuple(t.shape) == (2, 9000)


def test_inputs_are_remembered():
    g = Guarded(0xFF)
    x = g.guarded(np.array([1.0, np.nan, -0.0]))
    y = g.guarded(np.array([3, 4], dtype=np.int32))
    g.check_inputs()
    y[1] = 5
    with pytest.raises(AssertionError, match=r'input test_guarded_host\.py:\d+ \(8 bytes\) was written, first at byte 4'):
        g.check_inputs()
    g.written(y)
    g.check_inputs()
    z = g.guarded(np.zeros(3, dtype=np.uint8), label='test_case.py:12 (the mask)')      # a caller's own name
    z[2] = 1
    with pytest.raises(AssertionError, match=r'input test_case\.py:12 \(the mask\) \(3 bytes\) was written, first at byte 2'):
        g.check_inputs()
    g.written(z)
    x[2] = 0.0                                           # -0.0 -> +0.0: one bit
    with pytest.raises(AssertionError, match='first at byte 23'):
        g.check_inputs()


def test_install_swaps_engine_workspace_and_is_undone(monkeypatch):
    from deepmatching_stereo_matching_amd import engine
    with monkeypatch.context() as mp:
        g = install(mp, 0xFF)
        for m in _modules():
            assert m.torch is g.torch
        w = engine._workspace(100, 'cpu', 'x')
        assert w.dtype == torch.uint8 and w.numel() == 100 and w.data_ptr() % 32 == 16
        assert (raw(w) == 0xFF).all() and g.arenas[-1].label.startswith('engine.py:')
        o = engine._src_out(torch.zeros((2, 3), dtype=torch.float64), None)[1]
        assert bool(torch.isnan(o).all()) and len(g.arenas) == 2
        g.check()
    for m in _modules():
        assert m.torch is torch


def test_every_allocating_module_is_swapped():
    """The allocations of the package all live in the modules install() swaps."""
    pkg = os.path.join(os.path.dirname(L.HERE), 'deepmatching_stereo_matching_amd')
    have = set()
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and re.search(r'\btorch\.(empty|zeros|full)(_like)?\(', open(os.path.join(root, f)).read()):
                rel = os.path.relpath(os.path.join(root, f), os.path.dirname(pkg))[:-3].replace(os.sep, '.')
                have.add(rel)
    assert have <= set(ALLOCATING), sorted(have - set(ALLOCATING))


def test_recorder(monkeypatch):
    with monkeypatch.context() as mp:
        rec = record(mp)
        assert L.load() is rec
        assert L.load().dm_abi_version() == 110
        assert L.load().dm_fill_bytes(1, 4, 4) > 0
        assert rec.calls == ['dm_abi_version', 'dm_fill_bytes']
    assert not isinstance(L.load(), Recorder)


def test_stream_entries_are_known():
    names = stream_entries()
    assert set(names) <= set(L.SIGNATURES)
    assert {'dm_corr_stats', 'dm_match', 'dm_fill_holes', 'dm_lsm_refine', 'dm_shift_matches', 'dm_seq_sum'} <= set(names)
    assert not {'dm_stats_bytes', 'dm_fill_bytes', 'dm_pack_plan', 'dm_gs_schedule', 'dm_level_num_f16'} & set(names)
    # the stream is the last parameter of every entry that has one
    for n in names:
        assert L.SIGNATURES[n][0][-1] is L._P, n


def test_ledger_covers_every_stream_entry():
    """Every entry point that takes a stream is declared by a case of tests/test_guarded_gpu.py; an
    entry added without a guarded case fails here, on the CPU."""
    import test_guarded_gpu as G
    declared = set()
    for case in G.CASES:
        assert case.entries, case.name
        declared |= set(case.entries)
    assert declared <= set(stream_entries()), sorted(declared - set(stream_entries()))
    missing = sorted(set(stream_entries()) - declared - set(LEDGER_EXEMPT))
    assert not missing, 'no guarded case declares %s' % missing
    assert not declared & set(LEDGER_EXEMPT)
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)


def test_volume_entries_reject_a_misaligned_volume():
    """d_l0 of the three volume entries must be 16-byte aligned (include/dmstereo.h: the MFMA volume
    kernels store 16 bytes per lane): DM_ERR_ARG before any HIP call, so this runs without a device
    (the pointers are never followed)."""
    import ctypes
    lib = L.load()
    tiles = L.DmTiles(0x1000, 0x2000, 77, 77, 0x3000, 3, 4, 64, 5, L.DM_TM_CCOEFF_NORMED)
    b, stats = ctypes.byref(tiles), ctypes.c_void_p(0x4000)
    for off in (2, 4, 8):
        bad = ctypes.c_void_p(0x10000 + off)
        for rc in (lib.dm_corr_volume(b, stats, bad, None), lib.dm_corr_volume_f16(b, stats, bad, None),
                   lib.dm_corr_volume_ex(b, stats, 0, bad, None),
                   lib.dm_corr_volume_ex(b, stats, L.DM_VOLUME_F16 | L.DM_VOLUME_MINMAX_KNOWN, bad, None)):
            assert rc == L.DM_ERR_ARG and 'must be 16-byte aligned' in L.last_error()
    with pytest.raises(ValueError, match='16-byte aligned'):
        L.check(lib.dm_corr_volume(b, stats, ctypes.c_void_p(0x10004), None), 'dm_corr_volume')
