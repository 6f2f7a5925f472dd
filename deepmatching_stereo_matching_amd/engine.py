"""Device-resident correlation engine: batches of equally sized tiles -> pyramid -> matches.

This is the layer the reference-surface mirror (``misc/``) and the tile scheduler sit on.
Everything stays in HBM as torch tensors; the HIP library (``_lib``) is called with raw
device pointers on the current torch stream.  Reference call stack it replaces:
``Correlation_map.__call__`` (misc/Correlation_map.py:161-173) ->
``Matching.__call__`` (misc/Matching.py:211-222) -> ``Calc_difference.cal_map``
(misc/Calc_difference.py:26-49), per tile of ``ImageCutSolver`` (misc/image_cut_solver.py).
"""

import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _lib as L

LAM = 1.4
FUSE_DEFAULT = 2   # DevicePyramid level-1/level-2 mode (see its docstring); 2 is fastest on C3


def default_device():
    if not torch.cuda.is_available():
        raise L.DmUnavailable('no HIP device visible: the engine runs on MI355X only')
    return torch.device('cuda', torch.cuda.current_device())


def pyramid_plan(h0, w0):
    """Level count and N_map of Correlation_map._multi_level_correlation_pyramid
    (misc/Correlation_map.py:143-156).  Raises where its _aggregation would (:96-103)."""
    N, it, h, w = 1, 1, h0, w0
    while N < min(h0, w0):
        if h % 2 or w % 2:
            raise ValueError('could not broadcast input array from shape (%d,%d) into shape '
                             '(%d,%d)' % ((h + 1) // 2, (w + 1) // 2, h // 2, w // 2))
        h, w, N, it = h // 2, w // 2, N * 2, it + 1
    return it, N


def to_device_u8(img, device):
    if isinstance(img, torch.Tensor):
        t = img
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(img, dtype=np.uint8)))
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError('images must be 2-D uint8')
    return t.to(device).contiguous()


class TileBatch:
    """T tiles of one image pair: tile t is the (h0+ws-1) x (w0+ws-1) crop at origins[t]."""

    def __init__(self, img1, img2, origins, h0, w0, ws, method, device=None):
        self.device = device or default_device()
        self.img1 = to_device_u8(img1, self.device)
        self.img2 = to_device_u8(img2, self.device)
        if self.img1.shape != self.img2.shape:
            raise ValueError('img1 and img2 must have the same shape')
        org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
        H, W = self.img1.shape
        if ws < 1 or ws % 2 == 0:
            raise ValueError('could not broadcast: window_size must be odd (got %d)' % ws)
        if len(org) == 0 or h0 < 1 or w0 < 1:
            raise ValueError('empty tile batch')
        # the kernels trust these bounds: check them here, on the host
        if org.min() < 0 or (org[:, 0] + h0 + ws - 1).max() > H or (org[:, 1] + w0 + ws - 1).max() > W:
            raise ValueError('tile crop outside the image')
        self.origins_host = org
        self.origins = torch.from_numpy(org.astype(np.int32)).to(self.device).contiguous()
        self.T, self.h0, self.w0, self.ws, self.method = len(org), int(h0), int(w0), int(ws), int(method)
        self.struct = L.DmTiles(self.img1.data_ptr(), self.img2.data_ptr(),
                                self.img1.stride(0), self.img2.stride(0),
                                self.origins.data_ptr(), self.T, self.h0, self.w0,
                                self.ws, self.method)

    @property
    def P(self):
        return self.h0 * self.w0

    def ref(self):
        return ctypes.byref(self.struct)


class DevicePyramid:
    """co_map_list of a TileBatch, resident on the device.

    levels[0] is never stored (the fused kernels do not write level 0; matching evaluates
    it on demand).  ``fuse_level2`` (env DM_FUSE_L2) selects how levels 1-2 are built, on
    shapes the fused level-1/level-2 kernel supports:
      0  dm_corr_level1 writes level 1, dm_aggregate pools it into level 2;
      1  dm_corr_level12 writes levels 1 and 2 in one pass (no level-1 re-read);
      2  dm_corr_level12 writes level 2 only: level 1 stays on chip (levels[1] is None
         until ``level(1)`` asks for it) and matching evaluates it on demand.
    levels[l] for the others are float64 [T][Pl][Pl] tensors.

    Streams (DESIGN.md section 5c has the ledger of every hand-off).  ``stream``: the stream
    every call of this pyramid launches on -- the pair stream; None: the stream that is
    current at each call.  Buffers are allocated from the pair stream's pool whether or not
    it is torch's current stream, so ``DevicePyramid(batch, stream=side)`` may be used while
    another stream is current.  A call made on another pair stream than the call before it (a
    pyramid without a stream of its own, called under two current streams) first waits for
    that earlier stream, and every buffer the pyramid owns is recorded on each stream that
    touches it.  What a call returns (``match``'s map, ``level(k)``, ``volume()``) belongs to
    the pair stream of that call: a caller reading it elsewhere orders and records that read
    itself, as for any torch tensor."""

    def __init__(self, batch, stream=None, build=True, fuse_level2=None, stats_stream=None):
        """stats_stream: optional stream the per-patch stats and window operands
        (dm_corr_stats) are computed on, ahead of this pyramid's own stream -- a caller
        pipelining pairs keeps them off the pair streams, where they would queue behind the
        previous pair's matching."""
        self.b = batch
        self.lib = L.load()
        try:   # a shape the pyramid rejects can still give its level-0 volume (bad_matching.py)
            self._plan = pyramid_plan(batch.h0, batch.w0)
        except ValueError as e:
            self._plan = e
        self.stream = stream
        self._stats_stream = stats_stream
        self._stats_ready = None
        self._home = None      # the pair stream of the latest call: ordered after all work so far
        nbytes = self.lib.dm_stats_bytes(batch.ref())
        # from the stats stream's pool, or the pair stream's; every other stream that touches it
        # is recorded where it does (_pair, build), so the caching allocator reuses it only
        # after their work on it has finished
        with _on(stats_stream if stats_stream is not None else stream):
            self.stats = torch.empty(nbytes, dtype=torch.uint8, device=batch.device)
        if fuse_level2 is None:
            fuse_level2 = int(os.environ.get('DM_FUSE_L2', str(FUSE_DEFAULT)))
        self.fuse_level2 = int(fuse_level2)
        self.levels = [None]
        self._volume = None
        self._have_minmax = False
        self._have_stats = False
        if build:
            self.build()

    def _s(self):
        return L.stream_handle(self.stream)

    def _pair(self):
        """The pair stream of this call (``stream``, or the current one), ordered after the
        pair stream of the call before it when that was another, with the pyramid's buffers
        recorded on it (a no-op on the stream whose pool a buffer came from)."""
        st = self.stream if self.stream is not None else torch.cuda.current_stream()
        if self._home is None or st != self._home:
            if self._home is not None:
                st.wait_stream(self._home)
            for t in [self.stats, self._volume] + self.levels:
                if t is not None:
                    t.record_stream(st)
            self._home = st
        return st

    @property
    def nlev(self):
        """Level count (Correlation_map.iteration); raises the reference's aggregation
        error for shapes whose sides do not halve down to the top level."""
        if isinstance(self._plan, Exception):
            raise self._plan
        return self._plan[0]

    @property
    def N_map(self):
        if isinstance(self._plan, Exception):
            raise self._plan
        return self._plan[1]

    def compute_stats(self):
        st = self._pair()
        if not self._have_stats:
            ss = self._stats_stream
            if ss is not None:
                # forward order: the images / origins may have been written on this pyramid's
                # own stream (a conversion, a non-blocking upload); the stats read them
                ready = torch.cuda.Event()
                ready.record(st)
                ss.wait_event(ready)
            L.check(self.lib.dm_corr_stats(self.b.ref(), L.ptr(self.stats),
                                           L.stream_handle(ss) if ss is not None else self._s()),
                    'dm_corr_stats')
            if ss is not None:
                self._stats_ready = torch.cuda.Event()
                self._stats_ready.record(ss)
                st.wait_event(self._stats_ready)
            self._have_stats = True
        return self

    def _empty_level(self, k):
        b = self.b
        Pk = (b.h0 >> k) * (b.w0 >> k)
        return torch.empty((b.T, Pk, Pk), dtype=torch.float64, device=b.device)

    def _level1(self, stream=None, l1=None):
        if l1 is None:
            self._pair()
            with _on(self.stream):
                l1 = self._empty_level(1)
        sh = L.stream_handle(stream) if stream is not None else self._s()
        L.check(self.lib.dm_corr_level1(self.b.ref(), L.ptr(self.stats), L.ptr(l1), sh),
                'dm_corr_level1')
        self._have_minmax = True
        return l1

    def build(self, events=None, wait=None, nlev=None, level_stream=None):
        """Levels >= 1 up to level ``nlev`` - 1 (default: the full pyramid, as
        Correlation_map always builds it; a smaller ``nlev`` is the k-level pyramid of
        BASELINE configs C2/C3, whose levels above k - 1 Matching never reads).  ``events``:
        optional (start, end) torch.cuda.Event pair recorded around the level-1 (or fused
        level-1/level-2) kernel on this pyramid's stream.  ``wait``: optional event the level
        kernel waits for (the stats run before it) -- a caller pipelining pairs over streams
        passes the previous pair's level-kernel end, so the level kernels run one after
        another while each pair's latency-bound tail (levels >= 3, matching, stitch) overlaps
        the next pair's level kernel.  ``level_stream``: optional stream the level kernel runs
        on (it waits for this pyramid's stats, and this pyramid's stream waits for it): a
        caller that sends every pair's level kernel to one such stream serialises them without
        events, and a pair's stats no longer queue behind the previous pair's tail on a shared
        pair stream.  Building more levels later extends the pyramid."""
        b, lib = self.b, self.lib
        self.compute_stats()
        st = self._pair()
        top = self.nlev if nlev is None else max(1, min(int(nlev), self.nlev))
        if top > 1 and len(self.levels) == 1:
            fused = False
            ls = st
            if level_stream is not None and level_stream != st:
                ls = level_stream
                if self._stats_ready is not None:   # stats on their own stream: wait for them only
                    ls.wait_event(self._stats_ready)
                else:
                    ready = torch.cuda.Event()
                    ready.record(st)
                    ls.wait_event(ready)
                self.stats.record_stream(ls)
            if wait is not None:
                ls.wait_event(wait)
            if events:
                events[0].record(ls)
            # level buffers come from the level stream's pool (st's too when they are one):
            # st's later use of them is recorded, so the caching allocator reuses them only
            # after both streams' work on them
            with torch.cuda.stream(ls):
                l2 = self._empty_level(2) if (self.fuse_level2 and top >= 3) else None
                l1 = self._empty_level(1) if (self.fuse_level2 == 1 or l2 is None) else None
            if ls is not st:
                for t in (l1, l2):
                    if t is not None:
                        t.record_stream(st)
            if l2 is not None:
                rc = lib.dm_corr_level12(b.ref(), L.ptr(self.stats), L.ptr(l1), L.ptr(l2),
                                         L.stream_handle(ls))
                if rc == L.DM_OK:
                    self.levels += [l1, l2]
                    self._have_minmax = True
                    fused = True
                elif rc != L.DM_ERR_UNSUPPORTED:
                    L.check(rc, 'dm_corr_level12')
            if not fused:
                if l1 is None:
                    with torch.cuda.stream(ls):
                        l1 = self._empty_level(1)
                    if ls is not st:
                        l1.record_stream(st)
                self.levels.append(self._level1(ls, l1))
            if events:
                events[1].record(ls)
            if ls is not st:
                done = torch.cuda.Event()
                done.record(ls)
                st.wait_event(done)
        while len(self.levels) < top:
            k = len(self.levels)               # build level k from level k - 1
            h, w = b.h0 >> (k - 1), b.w0 >> (k - 1)
            with _on(self.stream):
                nxt = self._empty_level(k)
            L.check(lib.dm_aggregate(L.ptr(self.levels[k - 1]), b.T, h, w, 1, L.ptr(nxt),
                                     self._s()), 'dm_aggregate')
            self.levels.append(nxt)
        return self

    def level_shape(self, k):
        h, w = self.b.h0 >> k, self.b.w0 >> k
        return (h, w, h, w)

    def _volume_into(self, v, f16):
        """dm_corr_volume_ex into v; once the level kernel (or an earlier volume call) has left
        the per-patch min/max in the stats workspace, the volume kernel reuses them
        (DM_VOLUME_MINMAX_KNOWN) instead of sweeping every window a second time."""
        self.compute_stats()
        flags = (L.DM_VOLUME_F16 if f16 else 0) | (L.DM_VOLUME_MINMAX_KNOWN if self._have_minmax else 0)
        L.check(self.lib.dm_corr_volume_ex(self.b.ref(), L.ptr(self.stats), flags, L.ptr(v), self._s()),
                'dm_corr_volume_ex')
        self._have_minmax = True
        return v

    def volume(self):
        """Level-0 min-max volume (co_map before rectification), float32 [T][P][P]."""
        if self._volume is None:
            b = self.b
            with _on(self.stream):
                v = torch.empty((b.T, b.P, b.P), dtype=torch.float32, device=b.device)
            self._volume = self._volume_into(v, False)
        return self._volume

    def volume_f16(self):
        """The level-0 min-max volume as binary16 (dm_corr_volume_f16, BASELINE config C5's
        fp16 correlation): float16 [T][P][P], each value np.float16 of volume()'s."""
        b = self.b
        with _on(self.stream):
            v = torch.empty((b.T, b.P, b.P), dtype=torch.float16, device=b.device)
        return self._volume_into(v, True)

    def materialized_levels(self, l0_dtype='f32'):
        """co_map_list built the reference's way (misc/Correlation_map.py:132-156): level 0
        stored (float32 ``co_map`` or its fp16 rounding), rectified to float64
        (_rectification, :158-159), then every level by dm_aggregate (_aggregation,
        :89-130).  With 'f32' the levels equal the fused path's bit for bit; 'f16' is the
        C5 fp16-volume variant whose argmax flip rate the tests and bench report.
        Needs T * P^2 * (8 + 2|4) bytes of HBM."""
        b, lib = self.b, self.lib
        v = self.volume_f16() if l0_dtype == 'f16' else self.volume()
        self._pair()
        with _on(self.stream):
            l0 = torch.empty(v.shape, dtype=torch.float64, device=v.device)
        fn = lib.dm_rectify_f16 if l0_dtype == 'f16' else lib.dm_rectify
        L.check(fn(L.ptr(v), v.numel(), L.ptr(l0), self._s()), 'dm_rectify')
        if l0_dtype == 'f16':
            del v
        levels, h, w = [l0], b.h0, b.w0
        for _ in range(1, self.nlev):
            P2 = (h // 2) * (w // 2)
            with _on(self.stream):
                nxt = torch.empty((b.T, P2, P2), dtype=torch.float64, device=b.device)
            L.check(lib.dm_aggregate(L.ptr(levels[-1]), b.T, h, w, 1, L.ptr(nxt), self._s()),
                    'dm_aggregate')
            levels.append(nxt)
            h, w = h // 2, w // 2
        return levels

    def level(self, k):
        """co_map_list[k] as a float64 device tensor [T][Pk][Pk]."""
        if k < 0:
            k += self.nlev
        if not 0 <= k < self.nlev:
            raise IndexError('list index out of range')
        if k > 0:
            if k >= len(self.levels):          # a k-level build: extend it
                self.build(nlev=k + 1)
            if self.levels[k] is None:   # level 1 kept on chip by dm_corr_level12
                self.levels[k] = self._level1()
            return self.levels[k]
        v = self.volume()
        self._pair()
        with _on(self.stream):
            out = torch.empty(v.shape, dtype=torch.float64, device=v.device)
        L.check(self.lib.dm_rectify(L.ptr(v), v.numel(), L.ptr(out), self._s()), 'dm_rectify')
        return out

    def match(self, sub_pix=True, filtering=False, filter_window_size=3, filtering_num=3,
              filtering_mode='median', levels=None, nlev=None):
        """Matching()() for every tile: float64 [T][3][h0][w0] (row, col, score).
        ``levels``: an explicit co_map_list (e.g. materialized_levels()) to match on
        instead of this pyramid's (level 0 then read from memory, not re-derived).
        ``nlev``: match on the first ``nlev`` levels only, the reference's Matching on a
        co_map_list cut to k levels with N_map = 2^(k-1): the descent
        starts at level nlev - 1, one start per cell of that level (Matching.py:80-96)."""
        b = self.b
        n = self.nlev if nlev is None else int(nlev)
        if not 1 <= n <= self.nlev:
            raise IndexError('list index out of range')
        if levels is None:
            if not self._have_minmax:
                self.volume()
            for k in range(len(self.levels), n):
                self.level(k)
            if n == 2 and self.levels[1] is None:   # the top level must be stored
                self.level(1)
        self._pair()
        with _on(self.stream):
            out = torch.empty((b.T, 3, b.h0, b.w0), dtype=torch.float64, device=b.device)
            scratch = torch.empty_like(out)
        if levels is not None:
            ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in levels[:n]])
        else:
            ptrs = (ctypes.c_void_p * n)(*([None] + [None if t is None else t.data_ptr()
                                                      for t in self.levels[1:n]]))
        fnum = int(filtering_num) if filtering else 0
        L.check(self.lib.dm_match(b.ref(), L.ptr(self.stats), ptrs, n, b.T, b.h0, b.w0,
                                  int(bool(sub_pix)), int(filter_window_size), fnum,
                                  1 if filtering_mode == 'median' else 0,
                                  L.ptr(scratch), L.ptr(out), self._s()), 'dm_match')
        return out


def match_levels(levels, sub_pix=True, filtering=False, filter_window_size=3, filtering_num=3,
                 filtering_mode='median', device=None):
    """Matching on an arbitrary (host or device) co_map_list, level 0 materialised."""
    device = device or default_device()
    lib = L.load()
    lv = [torch.as_tensor(np.ascontiguousarray(x) if not isinstance(x, torch.Tensor) else x,
                          dtype=torch.float64).to(device).contiguous() for x in levels]
    h0, w0 = lv[0].shape[:2]
    out = torch.empty((1, 3, h0, w0), dtype=torch.float64, device=device)
    scratch = torch.empty_like(out)
    ptrs = (ctypes.c_void_p * len(lv))(*[t.data_ptr() for t in lv])
    fnum = int(filtering_num) if filtering else 0
    L.check(lib.dm_match(None, None, ptrs, len(lv), 1, h0, w0, int(bool(sub_pix)),
                         int(filter_window_size), fnum, 1 if filtering_mode == 'median' else 0,
                         L.ptr(scratch), L.ptr(out), L.stream_handle()), 'dm_match')
    return out[0]


def subpix_map(level0, match):
    """Matching._sub_pix_cal (Matching.py:177-209) in place on a map that a descent left at a
    level above 0: `match` float64 [3][hm][wm] (device), refined against co_map_list[0]
    (`level0`: [h0][w0][h0][w0], host or device) at patch (i, j) and window (row, col) of each
    entry, as the reference does (dm_subpix_map).  Any entry is accepted and indexed the way
    numpy indexes co_map_list[0] (negative indices wrap, out-of-range ones take the
    reference's except branch)."""
    lib = L.load()
    if not isinstance(match, torch.Tensor) or not match.is_cuda:
        raise ValueError('match must be a device (cuda) tensor: the kernel refines it in place')
    if not match.is_contiguous() or match.dtype != torch.float64 or match.dim() != 3 or match.shape[0] != 3:
        raise ValueError('match must be a contiguous float64 [3][h][w] tensor')
    dev = match.device
    l0 = torch.as_tensor(level0, dtype=torch.float64).to(dev).contiguous()
    if l0.dim() != 4:
        raise ValueError('level 0 must be [h0][w0][h0][w0]')
    h0, w0 = l0.shape[:2]
    _, hm, wm = match.shape
    L.check(lib.dm_subpix_map(L.ptr(l0), 1, h0, w0, hm, wm, L.ptr(match), L.stream_handle()),
            'dm_subpix_map')
    return match


def subpix_map_tiles(pyr, match, stream=None):
    """subpix_map with level 0 on demand (dm_subpix_map_tiles): the five level-0 values an entry
    reads are recomputed from the pyramid's images and statistics, so co_map_list[0] is never
    materialised.  `match`: contiguous float64 device tensor [T][3][hm][wm] (or [3][hm][wm]
    when the batch holds one tile), refined in place.  ``stream``: the stream the refinement runs
    on (None: the pyramid's pair stream); it waits for the pyramid's pair stream when it is another
    one, and the stats workspace is recorded on it.  Like every call of a pyramid this one goes
    through DevicePyramid._pair, ``stream`` given or not: a pyramid without a stream of its own,
    called here under another current stream than at its call before, makes that current stream
    wait for the earlier one (a ``wait_stream`` enqueued on the caller's current stream)."""
    if not isinstance(match, torch.Tensor) or not match.is_cuda:
        raise ValueError('match must be a device (cuda) tensor: the kernel refines it in place')
    m = match if match.dim() == 4 else match[None]
    b = pyr.b
    if not m.is_contiguous() or m.dtype != torch.float64 or m.shape[0] != b.T or m.shape[1] != 3:
        raise ValueError('match must be a contiguous float64 [T][3][h][w] tensor (T = %d)' % b.T)
    if not pyr._have_minmax:   # the per-patch min / max a level kernel or volume leaves in the stats
        pyr.build(nlev=2)
    home = pyr._pair()
    if stream is not None and stream != home:
        stream.wait_stream(home)           # the stats the pyramid's pair stream wrote, whether
        pyr.stats.record_stream(stream)    # it has a stream of its own or ran on the current one
    _, _, hm, wm = m.shape
    L.check(pyr.lib.dm_subpix_map_tiles(b.ref(), L.ptr(pyr.stats), hm, wm, L.ptr(m),
                                        L.stream_handle(stream) if stream is not None else pyr._s()),
            'dm_subpix_map_tiles')
    return match


def cal_map(match, mode, stream=None):
    """Calc_difference.cal_map on a [T][3][h][w] (or [3][h][w]) device tensor."""
    if mode not in L.CAL_MODES:
        raise ValueError(mode)
    m = match if match.dim() == 4 else match[None]
    m = m.contiguous()
    T, _, h, w = m.shape
    out = torch.empty((T, h, w), dtype=torch.float64, device=m.device)
    L.check(L.load().dm_cal_map(L.ptr(m), T, h, w, L.CAL_MODES[mode], L.ptr(out),
                                L.stream_handle(stream)), 'dm_cal_map')
    return out if match.dim() == 4 else out[0]


# ----------------------------------------------------------------------------------------
# tile scheduler (ImageCutSolver semantics, misc/image_cut_solver.py:58-179)
# ----------------------------------------------------------------------------------------
def cut_grid(shape, image_size, stride, window_size):
    """Tile counts and origins in the reference order (j outer, i inner; :62, :103-113)."""
    ex = int((window_size - 1) / 2)
    trimmed = [image_size[i] + 2 * ex for i in range(2)]
    n = [int(np.floor((shape[i] - trimmed[i]) / stride[i])) for i in range(2)]
    if n[0] < 1 or n[1] < 1:
        raise IndexError('list index out of range (no tile fits: image_cut_solver.py:150)')
    org = [(stride[0] * i, stride[1] * j) for j in range(n[1]) for i in range(n[0])]
    return n, np.array(org, dtype=np.int64)


def tile_bytes(h0, w0, level1=True):
    """Device bytes one tile needs inside DevicePyramid + match (levels >= 1, stats, maps).
    ``level1=False``: without the float64 level 1, which the fused level kernel never stores
    (DM_FUSE_L2=2, the default: matching re-derives it) -- 2.1 GB of the 2.3 GB of an S = 256
    tile."""
    nlev, _ = pyramid_plan(h0, w0)
    P = h0 * w0
    total = 6 * 4 * P + 2 * 3 * 8 * P
    h, w = h0, w0
    for k in range(1, nlev):
        h, w = h // 2, w // 2
        if k > 1 or level1:
            total += 8 * (h * w) ** 2
    return total


def level1_stored():
    """Does a DevicePyramid of the current configuration store level 1 (DM_FUSE_L2 != 2)?  The
    fused level kernel (mode 2) keeps it on chip; a shape it does not take (level12_fused)
    stores it anyway, so callers sizing memory for such shapes keep tile_bytes' default."""
    return int(os.environ.get('DM_FUSE_L2', str(FUSE_DEFAULT))) != 2


def build_config():
    """The library's compile-time switches (dm_build_config()) as a dict of ints."""
    cfg = L.load().dm_build_config().decode()
    return {k: int(v) for k, v in (kv.split('=') for kv in cfg.split())}


def level12_fused(h0, w0, ws):
    """Does the fused level kernel (dm_corr_level12) take tiles of this shape, so that a
    DevicePyramid in mode 2 never stores level 1?  The library's own rule, restated:
    mf16_eligible (csrc/dm_mfma.h: h0 % 4 == 0, w0 a power of two in 32 .. 256, ws <= 15) and,
    on the three GW = 4 instances (ws <= 5, w0 = 64 / 128 / 256: launch_level in
    csrc/dm_kernels.hip), cell blocks per tile a multiple of the NB cell blocks a workgroup
    holds -- NB read from the loaded library's build configuration, not assumed."""
    if not (h0 > 0 and h0 % 4 == 0 and w0 in (32, 64, 128, 256) and 1 <= ws <= 15 and ws % 2 == 1):
        return False
    if ws > 5 or w0 == 32:      # GW = 2 instances: one cell block per workgroup
        return True
    nb = build_config()[{64: 'C2_NB', 128: 'C3_NB', 256: 'C5_NB'}[w0]]
    return ((h0 // 4) * (w0 // 4)) % nb == 0


def _on(stream):
    """Run a block with ``stream`` as torch's current stream, so that the library calls
    (launched on the current stream), the copies and the caching allocator's frees are all
    ordered on it."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def solve_tiles(img1, img2, origins, h0, w0, ws, method, sub_pix=True, filtering=False,
                filter_window_size=3, filtering_num=3, filtering_mode='median',
                device=None, mem_budget=None, stream=None):
    """Correlation_map + Matching for every tile; float64 [T][3][h0][w0] device tensor.
    Tiles are processed in chunks that fit ``mem_budget`` bytes of HBM.  Everything,
    allocations included, is ordered on ``stream`` (default: the current stream)."""
    device = device or default_device()
    with _on(stream):
        img1 = to_device_u8(img1, device)
        img2 = to_device_u8(img2, device)
        origins = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
        if mem_budget is None:
            mem_budget = int(os.environ.get('DM_MEM_BUDGET', 64 << 30))
        per = tile_bytes(h0, w0)
        chunk = max(1, min(len(origins), mem_budget // max(per, 1)))
        out = torch.empty((len(origins), 3, h0, w0), dtype=torch.float64, device=device)
        for s in range(0, len(origins), chunk):
            b = TileBatch(img1, img2, origins[s:s + chunk], h0, w0, ws, method, device)
            pyr = DevicePyramid(b)
            out[s:s + len(b.origins_host)] = pyr.match(sub_pix, filtering, filter_window_size,
                                                       filtering_num, filtering_mode)
            del pyr, b
    return out


def bidir_origins(origins, H):
    """Tile origins of a bidirectional solve on the row-stacked pair (solve_tiles_bidir):
    int64 [2T][2], the T origins followed by the same origins with ``H`` (the rows of one
    image) added to the row.  A pure host function."""
    org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([org, org + np.array([int(H), 0], dtype=np.int64)], axis=0)


def stack_pair(img1, img2):
    """(A, Bk) = (img1 over img2, img2 over img1), stacked along rows: tile t of (A, Bk) at
    bidir_origins(...)[t] is the forward crop pair (img1, img2) for t < T and the backward one
    (img2, img1) for t >= T.  Each crop lies inside its own image, so none straddles the seam.
    Tensors stay tensors (on their device), anything else becomes a numpy array."""
    if isinstance(img1, torch.Tensor) or isinstance(img2, torch.Tensor):
        a, b = torch.as_tensor(img1), torch.as_tensor(img2)
        if a.shape != b.shape or a.dim() != 2:
            raise ValueError('img1 and img2 must have the same 2-D shape')
        b = b.to(a.device)
        return torch.cat([a, b], 0), torch.cat([b, a], 0)
    a, b = np.asarray(img1), np.asarray(img2)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError('img1 and img2 must have the same 2-D shape')
    return np.concatenate([a, b], 0), np.concatenate([b, a], 0)


def solve_tiles_bidir(img1, img2, origins, h0, w0, ws, method, sub_pix=True, filtering=False,
                      filter_window_size=3, filtering_num=3, filtering_mode='median',
                      device=None, mem_budget=None, stream=None):
    """solve_tiles in both directions -> (fwd, bwd), each float64 [T][3][h0][w0]: fwd equals
    solve_tiles(img1, img2, ...) and bwd solve_tiles(img2, img1, ...) bit for bit.  Both
    directions go through ONE tile stream of 2T tiles on the row-stacked pair (stack_pair,
    bidir_origins), with solve_tiles' chunking, so every kernel launch covers both
    directions.  The kernels are unchanged: a tile's result depends only on its own crops."""
    device = device or default_device()
    with _on(stream):
        a = to_device_u8(img1, device)
        b = to_device_u8(img2, device)
        if a.shape != b.shape:
            raise ValueError('img1 and img2 must have the same shape')
        A, Bk = stack_pair(a, b)
        org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
        T = len(org)
        both = solve_tiles(A, Bk, bidir_origins(org, a.shape[0]), h0, w0, ws, method, sub_pix, filtering,
                           filter_window_size, filtering_num, filtering_mode, device=device,
                           mem_budget=mem_budget)
    return both[:T], both[T:]


def _fb_pair(fwd, bwd):
    if not (isinstance(fwd, torch.Tensor) and isinstance(bwd, torch.Tensor) and fwd.is_cuda and bwd.is_cuda):
        raise ValueError('fwd and bwd must be device (cuda) tensors')
    if fwd.shape != bwd.shape or fwd.dtype != torch.float64 or bwd.dtype != torch.float64:
        raise ValueError('fwd and bwd must be float64 tensors of one shape')
    f = (fwd if fwd.dim() == 4 else fwd[None]).contiguous()
    b = (bwd if bwd.dim() == 4 else bwd[None]).contiguous()
    if f.dim() != 4 or f.shape[1] != 3:
        raise ValueError('fwd and bwd must be [T][3][h][w] or [3][h][w]')
    return f, b


def fb_check(fwd, bwd, tol, masked=True, stream=None):
    """Forward-backward consistency check (dm_fb_check) of matches fwd (img1 -> img2) and bwd
    (img2 -> img1), float64 device tensors [T][3][h][w] or [3][h][w] -> (err, masked map or
    None).  err [T][h][w]: each cell's distance from where the walk there (fwd, rounded to
    the grid) and back (bwd) returns, NaN for an off-tile or non-finite match.  The masked
    map is fwd with rows 0 and 1 NaN where not err <= tol, the score row unchanged."""
    f, b = _fb_pair(fwd, bwd)
    T, _, h, w = f.shape
    with _on(stream):
        err = torch.empty((T, h, w), dtype=torch.float64, device=f.device)
        m = torch.empty_like(f) if masked else None
        L.check(L.load().dm_fb_check(L.ptr(f), L.ptr(b), T, h, w, float(tol), L.ptr(err), L.ptr(m),
                                     L.stream_handle()), 'dm_fb_check')
    if fwd.dim() == 4:
        return err, m
    return err[0], (m[0] if m is not None else None)


def stitch_fb(fwd, bwd, n, h0, w0, stride, modes, tol, stream=None):
    """stitch(fb_check(fwd, bwd, tol) masked map) in one kernel (dm_stitch_fb) ->
    (d_map, out_map, err): d_map NaN at cells that fail the check, out_map unchanged, err
    [H][W] the stitched round-trip error (NaN where no tile covers)."""
    mode_ids = [L.CAL_MODES[m] for m in modes]
    Hout, Wout = stride[0] * (n[0] - 1) + h0, stride[1] * (n[1] - 1) + w0
    f, b = _fb_pair(fwd, bwd)
    if tuple(f.shape) != (n[0] * n[1], 3, h0, w0):
        raise ValueError('fwd / bwd must be [%d][3][%d][%d]' % (n[0] * n[1], h0, w0))
    with _on(stream):
        dmap = torch.empty((len(modes), Hout, Wout), dtype=torch.float64, device=f.device)
        score = torch.empty((Hout, Wout), dtype=torch.float64, device=f.device)
        err = torch.empty((Hout, Wout), dtype=torch.float64, device=f.device)
        arr = (ctypes.c_int32 * max(1, len(mode_ids)))(*mode_ids)
        L.check(L.load().dm_stitch_fb(L.ptr(f), L.ptr(b), n[0], n[1], h0, w0, stride[0], stride[1], arr,
                                      len(mode_ids), float(tol), L.ptr(dmap), L.ptr(score), L.ptr(err),
                                      L.stream_handle()), 'dm_stitch_fb')
    return dmap, score, err


def merge_rule(rule):
    """The ``merge=`` keyword of ImageCutSolver / shard.solve_image_sharded as a dm_merge_rule."""
    if rule not in L.MERGE_RULES:
        raise ValueError('merge must be one of %s (got %r)' % (', '.join(sorted(L.MERGE_RULES)), rule))
    return L.MERGE_RULES[rule]


def stitch_merge(fwd, bwd, n, h0, w0, stride, modes, tol=None, rule='feather', min_count=1, stream=None):
    """The stitch with every covering tile of a pixel merged instead of the last one kept
    (dm_stitch_merge; include/dmstereo.h has the definition) -> (d_map, out_map, err or None,
    spread, count).  ``rule``: 'last' (stitch / stitch_fb bit for bit), 'center' (the candidate
    deepest inside its tile), 'feather' (edge-distance weighted mean) or 'median'.  ``bwd`` and
    ``tol`` as in stitch_fb: a candidate whose round trip misses the tolerance is not merged;
    ``bwd=None`` merges a one-direction solve (every finite candidate, err is None).  d_map is
    NaN where fewer than ``min_count`` candidates are valid; spread [len(modes)][H][W] is max -
    min of the valid candidates' values, count [H][W] (uint8) their number."""
    mode_ids = [L.CAL_MODES[m] for m in modes]
    rule_id = merge_rule(rule)
    Hout, Wout = stride[0] * (n[0] - 1) + h0, stride[1] * (n[1] - 1) + w0
    if bwd is None:
        if tol is not None:
            raise ValueError('a tolerance needs the backward tiles (bwd)')
        f, b = _fb_pair(fwd, fwd)
        b = None
    else:
        if tol is None:
            raise ValueError('merging both directions needs a tolerance (tol)')
        f, b = _fb_pair(fwd, bwd)
    if tuple(f.shape) != (n[0] * n[1], 3, h0, w0):
        raise ValueError('fwd / bwd must be [%d][3][%d][%d]' % (n[0] * n[1], h0, w0))
    with _on(stream):
        dmap = torch.empty((len(modes), Hout, Wout), dtype=torch.float64, device=f.device)
        score = torch.empty((Hout, Wout), dtype=torch.float64, device=f.device)
        err = torch.empty((Hout, Wout), dtype=torch.float64, device=f.device) if b is not None else None
        spread = torch.empty((len(modes), Hout, Wout), dtype=torch.float64, device=f.device)
        count = torch.empty((Hout, Wout), dtype=torch.uint8, device=f.device)
        arr = (ctypes.c_int32 * max(1, len(mode_ids)))(*mode_ids)
        L.check(L.load().dm_stitch_merge(L.ptr(f), L.ptr(b), n[0], n[1], h0, w0, stride[0], stride[1], arr,
                                         len(mode_ids), float(tol) if b is not None else 0.0, rule_id,
                                         int(min_count), L.ptr(dmap), L.ptr(score), L.ptr(err), L.ptr(spread),
                                         L.ptr(count), L.stream_handle()), 'dm_stitch_merge')
    return dmap, score, err, spread, count


def stitch(match, n, h0, w0, stride, modes, stream=None):
    """ImageCutSolver._execute_matching stitching on the device -> (d_map, out_map)."""
    mode_ids = [L.CAL_MODES[m] for m in modes]
    Hout, Wout = stride[0] * (n[0] - 1) + h0, stride[1] * (n[1] - 1) + w0
    with _on(stream):
        m = match.contiguous()
        dmap = torch.empty((len(modes), Hout, Wout), dtype=torch.float64, device=match.device)
        score = torch.empty((Hout, Wout), dtype=torch.float64, device=match.device)
        arr = (ctypes.c_int32 * max(1, len(mode_ids)))(*mode_ids)
        L.check(L.load().dm_stitch(L.ptr(m), n[0], n[1], h0, w0, stride[0], stride[1], arr,
                                   len(mode_ids), L.ptr(dmap), L.ptr(score), L.stream_handle()),
                'dm_stitch')
    return dmap, score


def stitch_any(fwd, bwd, n, h0, w0, stride, modes, consistency, merge, merge_min_count=1, stitcher=None, merger=None):
    """The stitch that the ``consistency`` and ``merge`` keywords of ImageCutSolver / solve_image_sharded
    select -> the head of chain.Chain.layout as a tuple: stitch_merge with ``merge`` (without its err when
    only one direction was solved), else stitch_fb with ``consistency``, else stitch.  ``fwd``: the solved
    tiles, ``bwd``: those of the other direction, None unless ``consistency`` is set.  ``stitcher`` /
    ``merger`` replace stitch or stitch_fb / stitch_merge (the hooks of solve_image_sharded)."""
    if merge is not None:
        maps = (merger or stitch_merge)(fwd, bwd, n, h0, w0, stride, modes, consistency, merge, merge_min_count)
        return tuple(m for m in maps if m is not None)      # a one-direction merge has no err
    if consistency is not None:
        return (stitcher or stitch_fb)(fwd, bwd, n, h0, w0, stride, modes, consistency)
    return (stitcher or stitch)(fwd, n, h0, w0, stride, modes)


# ---- argument plumbing of the d_map stages below (fill_holes ... lsm_refine) -------------------
def _int_in(x, lo, hi, msg, got=None):
    """int(x) of an int (not a bool) in [lo, hi]; else ValueError(msg % (got or x,))."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(msg % ((x if got is None else got),))
    return int(x)


def _real_in(x, lo, hi, msg, open_lo=False):
    """float(x) of a real (not a bool) in [lo, hi], or (lo, hi] with ``open_lo``; else ValueError(msg % (x,))."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or \
            not ((lo < float(x) if open_lo else lo <= float(x)) and float(x) <= hi):
        raise ValueError(msg % (x,))
    return float(x)


def _maps_shape(maps, msg='maps must be a float64 device (cuda) tensor'):
    """(shape, M, H, W) of a float64 device tensor [H][W] (M = 1) or [M][H][W]; else ValueError."""
    if not (isinstance(maps, torch.Tensor) and maps.is_cuda and maps.dtype == torch.float64):
        raise ValueError(msg)
    if maps.dim() not in (2, 3):
        raise ValueError('maps must be [H][W] or [M][H][W]')
    shape = tuple(maps.shape)
    return (shape,) + ((1,) + shape if maps.dim() == 2 else shape)


def _check_out(out, maps):
    if out is not None and not (isinstance(out, torch.Tensor) and out.device == maps.device and
                                out.dtype == torch.float64 and out.shape == maps.shape and out.is_contiguous()):
        raise ValueError('out must be a contiguous float64 tensor of maps\' shape on its device')


def _src_out(maps, out):
    """(src, out) of a stage: in place (``out`` is ``maps``' memory) the kernel reads ``out``; else a
    contiguous ``maps``, and a new ``out`` if none was given."""
    if out is not None and out.data_ptr() == maps.data_ptr():
        return out, out
    if out is None:
        out = torch.empty(tuple(maps.shape), dtype=torch.float64, device=maps.device)
    return maps.contiguous(), out


def _workspace(nbytes, device, msg):
    """The stage's workspace of ``nbytes`` (its dm_*_bytes entry); 0 bytes: a shape the stage does
    not take, NotImplementedError(msg)."""
    if not nbytes:
        raise NotImplementedError(msg)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _offset(offset):
    """``offset``: an int or (oy, ox) -> (oy, ox)."""
    if isinstance(offset, (tuple, list)):
        if len(offset) != 2:
            raise ValueError('offset must be an int or (oy, ox)')
        oy, ox = offset
    else:
        oy = ox = offset
    msg = 'offset must be an int or (oy, ox) in [-2^30, 2^30] (got %r)'
    return _int_in(oy, -2 ** 30, 2 ** 30, msg, offset), _int_in(ox, -2 ** 30, 2 ** 30, msg, offset)


def _planes_device(d_row, d_col):
    """The device of the two 2-D float64 device planes of one shape; else ValueError."""
    for name, d in (('d_row', d_row), ('d_col', d_col)):
        if not (isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and d.dim() == 2):
            raise ValueError('%s must be a 2-D float64 device (cuda) tensor' % name)
    if d_row.shape != d_col.shape or d_row.device != d_col.device:
        raise ValueError('d_row and d_col must have one shape and device')
    return d_row.device


def fill_iterations(fill):
    """The ``fill=`` keyword of ImageCutSolver / shard.solve_image_sharded as a Jacobi step
    count: an int in [0, 4096] (dm_fill_holes' range)."""
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)):
        raise ValueError('fill must be an int (Jacobi iterations per level) or None')
    if not 0 <= int(fill) <= 4096:
        raise ValueError('fill iterations must be in [0, 4096] (got %r)' % (fill,))
    return int(fill)


def fill_holes(maps, iters=16, out=None, return_holes=False, stream=None):
    """Dense maps from maps with holes (dm_fill_holes): cascadic push-pull with ``iters`` masked
    Jacobi steps per level, deterministic, each map from its own holes.  ``maps``: a float64
    device tensor [H][W] or [M][H][W]; a hole is a non-finite cell (NaN where dm_stitch found
    no tile and where dm_stitch_fb's round trip missed).  Finite cells come out bit-identical;
    the result is finite everywhere unless a whole map is a hole (it is then returned as it
    is).  -> the filled tensor: ``out`` if given (``out=maps`` fills in place), else a new one;
    with ``return_holes`` also the uint8 mask of the cells that were holes."""
    shape, M, H, W = _maps_shape(maps)
    iters = fill_iterations(iters)
    _check_out(out, maps)
    with _on(stream):
        src, out = _src_out(maps, out)
        if maps.numel() == 0:      # no cell, no hole
            holes = torch.empty(shape, dtype=torch.uint8, device=maps.device)
            return (out, holes) if return_holes else out
        lib = L.load()
        work = _workspace(lib.dm_fill_bytes(M, H, W), maps.device,
                          'fill_holes does not take %d maps of %d x %d cells' % (M, H, W))
        holes = torch.empty(shape, dtype=torch.uint8, device=maps.device) if return_holes else None
        L.check(lib.dm_fill_holes(L.ptr(src), M, H, W, int(iters), L.ptr(out), L.ptr(holes), L.ptr(work),
                                  L.stream_handle()), 'dm_fill_holes')
    return (out, holes) if return_holes else out


def speckle_params(speckle):
    """The ``speckle=`` keyword of ImageCutSolver / shard.solve_image_sharded as (max_size,
    max_diff): a pair of an int >= 0 (the largest segment removed, in cells) and a real >= 0
    (the largest difference that joins two neighbours; inf allowed)."""
    if isinstance(speckle, (str, bytes)) or not isinstance(speckle, (tuple, list)) or len(speckle) != 2:
        raise ValueError('speckle must be a (max_size, max_diff) pair or None')
    max_size, max_diff = speckle
    return (_int_in(max_size, 0, 2 ** 31 - 1, 'speckle max_size must be an int >= 0 (got %r)'),
            _real_in(max_diff, 0.0, np.inf, 'speckle max_diff must be a real >= 0 (got %r)'))


def filter_speckles(maps, max_size, max_diff, out=None, return_removed=False, return_sizes=False,
                    return_labels=False, stream=None):
    """Maps without their small segments (dm_filter_speckles), each map on its own.  ``maps``: a
    float64 device tensor [H][W] or [M][H][W].  Two finite 4-neighbours are joined when they
    differ by at most ``max_diff``; every cell of a connected segment of at most ``max_size``
    cells becomes NaN, every other cell is copied bit for bit.  -> the filtered tensor: ``out``
    if given (``out=maps`` filters in place), else a new one; then, as asked for, the uint8
    mask of the cells removed, the size of each cell's segment (0 at holes; an int32 tensor,
    sizes are at most 2^31 - 1) and its int32 label, the smallest linear index of the segment (-1 at holes)."""
    shape, M, H, W = _maps_shape(maps)
    max_size, max_diff = speckle_params((max_size, max_diff))
    _check_out(out, maps)
    with _on(stream):
        src, out = _src_out(maps, out)
        removed = torch.empty(shape, dtype=torch.uint8, device=maps.device) if return_removed else None
        sizes = torch.empty(shape, dtype=torch.int32, device=maps.device) if return_sizes else None
        labels = torch.empty(shape, dtype=torch.int32, device=maps.device) if return_labels else None
        if maps.numel():      # (no cell, no segment)
            lib = L.load()
            work = _workspace(lib.dm_speckle_bytes(M, H, W), maps.device,
                              'filter_speckles does not take %d maps of %d x %d cells' % (M, H, W))
            L.check(lib.dm_filter_speckles(L.ptr(src), M, H, W, max_size, max_diff, L.ptr(out), L.ptr(removed),
                                           L.ptr(sizes), L.ptr(labels), L.ptr(work), L.stream_handle()),
                    'dm_filter_speckles')
    res = (out,) + tuple(t for t in (removed, sizes, labels) if t is not None)
    return res if len(res) > 1 else out


def smooth_params(smooth):
    """The ``smooth=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius,
    sigma_color, sigma_space): an int in [1, 15] (the window is (2 radius + 1)^2 taps) and two
    reals > 0 (inf allowed: a flat weight)."""
    if isinstance(smooth, (str, bytes)) or not isinstance(smooth, (tuple, list)) or len(smooth) != 3:
        raise ValueError('smooth must be a (radius, sigma_color, sigma_space) triple or None')
    radius, sigma_color, sigma_space = smooth
    return (_int_in(radius, 1, 15, 'smooth radius must be an int in [1, 15] (got %r)'),
            _real_in(sigma_color, 0.0, np.inf, 'smooth sigma_color must be a real > 0 (got %r)', open_lo=True),
            _real_in(sigma_space, 0.0, np.inf, 'smooth sigma_space must be a real > 0 (got %r)', open_lo=True))


def bilateral_filter(maps, radius, sigma_color, sigma_space, guide=None, iters=1, fill=False, out=None,
                     return_filled=False, stream=None):
    """Edge-preserving smoothing of maps with holes (dm_bilateral_filter), each map on its own.
    ``maps``: a float64 device tensor [H][W] or [M][H][W].  A cell becomes the mean of the finite
    cells of its (2 radius + 1)^2 window, weighted by exp(-d^2 / (2 sigma_space^2)) of their
    distance and exp(-c^2 / (2 sigma_color^2)) of the difference of the guide; ``guide``: None
    (the map guides itself) or a float64 or uint8 device tensor [H][W] (shared by all maps) or of
    ``maps``' shape; cells where the map or the guide is not finite are left out.  ``iters``
    passes in [1, 64].  Holes (NaN, +-inf) stay bit-identical unless ``fill`` is set (it needs a
    guide): a hole is then filled from the usable cells of its window, if any.  -> the smoothed
    tensor: ``out`` if given (``out=maps`` smooths in place), else a new one; with
    ``return_filled`` also the uint8 mask of the holes that came out finite."""
    shape, M, H, W = _maps_shape(maps)
    radius, sigma_color, sigma_space = smooth_params((radius, sigma_color, sigma_space))
    iters = _int_in(iters, 1, 64, 'iters must be an int in [1, 64] (got %r)')
    flags = 0
    if guide is not None:
        if not (isinstance(guide, torch.Tensor) and guide.device == maps.device and
                guide.dtype in (torch.float64, torch.uint8)):
            raise ValueError('guide must be a float64 or uint8 tensor on maps\' device')
        if tuple(guide.shape) not in (shape, shape[-2:]):
            raise ValueError('guide must be [H][W] or of maps\' shape')
        if guide.dtype == torch.uint8:
            flags |= L.DM_BILAT_GUIDE_U8
    if fill:
        if guide is None:
            raise ValueError('fill needs a guide')
        flags |= L.DM_BILAT_FILL
    _check_out(out, maps)
    with _on(stream):
        src, out = _src_out(maps, out)
        filled = torch.empty(shape, dtype=torch.uint8, device=maps.device) if return_filled else None
        if maps.numel():      # (no cell, nothing to smooth)
            lib = L.load()
            work = _workspace(lib.dm_bilateral_bytes(M, H, W), maps.device,
                              'bilateral_filter does not take %d maps of %d x %d cells' % (M, H, W))
            g = guide.contiguous() if guide is not None else None
            gmaps = M if g is not None and g.dim() == 3 else 1
            L.check(lib.dm_bilateral_filter(L.ptr(src), L.ptr(g), gmaps, M, H, W, radius, bilateral_den(sigma_color),
                                            bilateral_den(sigma_space), int(iters), flags, L.ptr(out),
                                            L.ptr(filled), L.ptr(work), L.stream_handle()), 'dm_bilateral_filter')
    return (out, filled) if return_filled else out


def smooth_guide(img1, exclusive_pix, d_map):
    """The 'image' guide of ``smooth=``: img1[e:e + H, e:e + W] as a uint8 tensor on d_map's
    device, [H][W] d_map's last two sides -- map cell (y, x) is the patch centred at
    (y + e, x + e) of the image."""
    H, W = d_map.shape[-2:]
    e = int(exclusive_pix)
    if np.shape(img1)[0] < e + H or np.shape(img1)[1] < e + W:
        raise ValueError('image %r does not cover the %d x %d map' % (tuple(np.shape(img1)), H, W))
    return to_device_u8(img1, d_map.device)[e:e + H, e:e + W].contiguous()


def bilateral_den(sigma):
    """den_color / den_space of dm_bilateral_filter: 2.0 * sigma**2 as Python evaluates it
    (dm_make_weight's convention); a square beyond the float64 range is inf."""
    try:
        return 2.0 * float(sigma) ** 2
    except OverflowError:
        return float('inf')


def median_params(median):
    """The ``median=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius, iters):
    an int radius in [1, 7] (the window is (2 radius + 1)^2 taps), ``(radius,)`` or ``(radius,
    iters)`` with iters, the number of passes, an int in [1, 64] (default 1)."""
    if isinstance(median, (tuple, list)):
        if not 1 <= len(median) <= 2:
            raise ValueError('median must be a radius, (radius,), (radius, iters) or None')
        radius, iters = median[0], (median[1] if len(median) == 2 else 1)
    else:
        radius, iters = median, 1
    return (_int_in(radius, 1, 7, 'median radius must be an int in [1, 7] (got %r)'),
            _int_in(iters, 1, 64, 'median iters must be an int in [1, 64] (got %r)'))


def median_filter(maps, radius, weight=None, iters=1, min_count=1, fill=False, out=None, return_changed=False,
                  stream=None):
    """Impulse filter of maps with holes (dm_median_filter), each map on its own.  ``maps``: a
    float64 device tensor [H][W] or [M][H][W], or a numpy array of such a shape (it is copied to
    the default device).  A cell becomes the lower median, by the order-preserving key of the
    double, of the finite cells of its (2 radius + 1)^2 window; with ``weight`` -- a float64
    tensor (or array) [H][W], shared by all maps, or of ``maps``' shape -- the weighted lower
    median: the smallest window value at which the weights of the values up to it, summed in
    window order, reach half their total; taps whose weight is not in (0, inf) are left out.
    ``iters`` passes in [1, 64].  A cell with fewer than ``min_count`` usable taps is copied.
    Holes (NaN, +-inf) stay bit-identical unless ``fill`` is set: a hole then receives the median
    of its window.  Every finite output is one of the window's own values, bit for bit.  -> the
    filtered tensor: ``out`` if given (``out=maps`` filters in place), else a new one; with
    ``return_changed`` also the uint8 mask of the cells whose bits changed."""
    if isinstance(maps, np.ndarray):
        if maps.dtype != np.float64:
            raise ValueError('maps must be float64')
        maps = torch.from_numpy(np.ascontiguousarray(maps)).to(default_device())
    shape, M, H, W = _maps_shape(maps, 'maps must be a float64 device (cuda) tensor or a float64 numpy array')
    radius, iters = median_params((radius, iters))
    K = (2 * radius + 1) ** 2
    min_count = _int_in(min_count, 1, K, 'min_count must be an int in [1, %d] (got %%r)' % K)
    if weight is not None:
        if isinstance(weight, np.ndarray):
            if weight.dtype != np.float64:
                raise ValueError('weight must be float64')
            weight = torch.from_numpy(np.ascontiguousarray(weight)).to(maps.device)
        if not (isinstance(weight, torch.Tensor) and weight.device == maps.device and weight.dtype == torch.float64):
            raise ValueError('weight must be a float64 tensor on maps\' device')
        if tuple(weight.shape) not in (shape, shape[-2:]):
            raise ValueError('weight must be [H][W] or of maps\' shape')
    _check_out(out, maps)
    with _on(stream):
        src, out = _src_out(maps, out)
        changed = torch.empty(shape, dtype=torch.uint8, device=maps.device) if return_changed else None
        if maps.numel():      # (no cell, nothing to filter)
            lib = L.load()
            work = _workspace(lib.dm_median_bytes(M, H, W), maps.device,
                              'median_filter does not take %d maps of %d x %d cells' % (M, H, W))
            w = weight.contiguous() if weight is not None else None
            wmaps = M if w is not None and w.dim() == 3 else 1
            L.check(lib.dm_median_filter(L.ptr(src), L.ptr(w), wmaps, M, H, W, radius, int(min_count), iters,
                                         L.DM_MEDIAN_FILL if fill else 0, L.ptr(out), L.ptr(changed), L.ptr(work),
                                         L.stream_handle()), 'dm_median_filter')
    return (out, changed) if return_changed else out


def median_weight(median_weight, maps):
    """The weight plane of ``median=`` for the stitched ``maps`` tuple: None, or with
    'correlation' the stitched out_map (maps[1]), shared by all modes."""
    return maps[1] if median_weight == 'correlation' else None


def photo_params(photo):
    """The ``photo=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius, min_score):
    an int radius in [1, 7] (the window is (2 radius + 1)^2 pixels) -- the final d_map is scored
    -- or ``(radius, min_score)`` with min_score a real in [-1, 1]: the cells that score below it
    are also rejected after the median and before the speckle filter.  min_score is None in the
    first form."""
    if isinstance(photo, (tuple, list)):
        if len(photo) != 2:
            raise ValueError('photo must be a radius, (radius, min_score) or None')
        radius, min_score = photo
        min_score = _real_in(min_score, -1.0, 1.0, 'photo min_score must be a real in [-1, 1] (got %r)')
    else:
        radius, min_score = photo, None
    return _int_in(radius, 1, 7, 'photo radius must be an int in [1, 7] (got %r)'), min_score


def _photo_image(img, device):
    """A 2-D uint8 image as a device tensor whose rows are contiguous (the row stride is kept)."""
    if isinstance(img, torch.Tensor):
        t = img
    else:
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise ValueError('images must be 2-D uint8')
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError('images must be 2-D uint8')
    t = t.to(device)
    if t.numel() and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _pair_images(img1, img2, dev):
    """The pair as _photo_image tensors (a, b) of one shape; else ValueError."""
    a, b = _photo_image(img1, dev), _photo_image(img2, dev)
    if a.shape != b.shape:
        raise ValueError('img1 and img2 must have the same shape')
    return a, b


def _held_planes(d_row, d_col):
    """The two planes as contiguous tensors (a contiguous plane is read from where it is: in place it
    aliases the output, which the kernels allow).  The caller holds them until the launch: a copy must
    not be freed before it."""
    return d_row.contiguous(), d_col.contiguous()


def _plane_mask(mask, d_row):
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.device == d_row.device and
                                 mask.dtype in (torch.uint8, torch.bool) and mask.shape == d_row.shape):
        raise ValueError('mask must be a uint8 or bool tensor of the planes\' shape on their device')


def _plane_out(out, d_row):
    if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 2 and all(
            isinstance(o, torch.Tensor) and o.device == d_row.device and o.dtype == torch.float64 and
            o.shape == d_row.shape and o.is_contiguous() for o in out)):
        raise ValueError('out must be a pair of contiguous float64 tensors of the planes\' shape on their device')


def _rematch(entry, bytes_call, img1, img2, d_row, d_col, offset, mask, out, scalars, return_score, aux_shape, stream,
             unsupported_msg, extra_shape=False):
    """The body of the plane re-matching entries (photo_refine, lsm_refine, sgm_refine), whose C entries
    share one argument layout: the pair, the planes, the map shape and the offset, then the stage's
    ``scalars``, then mask, the two output planes, the score, the int8 plane of ``aux_shape`` (None: not
    asked for), the workspace and the stream.  ``bytes_call(lib, Hi, Wi, H, W)``: the workspace size;
    ``unsupported_msg``: NotImplementedError's text, a template over H, W, Hi, Wi.  ``extra_shape``: for an entry
    that takes one more float64 output between the int8 plane and the workspace (dm_lsm_affine), its shape or
    None (not asked for); the tensor is then a fifth result.
    -> (d_row', d_col', score or None, aux or None[, extra or None])."""
    dev = _planes_device(d_row, d_col)
    oy, ox = _offset(offset)
    _plane_mask(mask, d_row)
    _plane_out(out, d_row)
    H, W = d_row.shape
    with _on(stream):
        a, b = _pair_images(img1, img2, dev)
        o_row, o_col = out if out is not None else (torch.empty((H, W), dtype=torch.float64, device=dev),
                                                    torch.empty((H, W), dtype=torch.float64, device=dev))
        score = torch.empty((H, W), dtype=torch.float64, device=dev) if return_score else None
        aux = torch.empty(aux_shape, dtype=torch.int8, device=dev) if aux_shape is not None else None
        extra = torch.empty(extra_shape, dtype=torch.float64, device=dev) if extra_shape else None
        more = () if extra_shape is False else (L.ptr(extra),)
        if H and W:
            if not a.numel():
                raise ValueError('empty image')
            lib = L.load()
            Hi, Wi = a.shape
            work = _workspace(bytes_call(lib, Hi, Wi, H, W), dev, unsupported_msg % dict(H=H, W=W, Hi=Hi, Wi=Wi))
            m = None if mask is None else mask.to(torch.uint8).contiguous()
            rows, cols = _held_planes(d_row, d_col)
            L.check(getattr(lib, entry)(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), Hi, Wi, L.ptr(rows), L.ptr(cols),
                                        H, W, int(oy), int(ox), *scalars, L.ptr(m), L.ptr(o_row), L.ptr(o_col),
                                        L.ptr(score), L.ptr(aux), *more, L.ptr(work), L.stream_handle()), entry)
    return (o_row, o_col, score, aux) if extra_shape is False else (o_row, o_col, score, aux, extra)


def _plane_stage(fn, img1, img2, d_map, modes, holes, *args, **kw):
    """A plane re-matching stage of the chain on the stitched d_map [len(modes)][H][W], in place: ``fn`` on
    the two elevation planes, of the cells that ``holes`` marks in either (None: every cell).
    -> (d_map, score, the stage's int8 plane[, what else ``fn`` returns])."""
    ir, ic = refine_planes(modes)
    mask = None if holes is None else (holes[ir] | holes[ic])
    res = fn(img1, img2, d_map[ir], d_map[ic], *args, mask=mask, out=(d_map[ir], d_map[ic]), **kw)
    return (d_map,) + tuple(res[2:])


def photo_planes(modes):
    """Indices (row, column) of 'elevation2' and 'elevation' in a degree_map_mode list: the planes
    ``photo=`` reads.  ValueError when one is missing."""
    modes = list(modes)
    if 'elevation' not in modes or 'elevation2' not in modes:
        raise ValueError("photo needs both 'elevation' and 'elevation2' in degree_map_mode (got %r)" % (modes,))
    return modes.index('elevation2'), modes.index('elevation')


def photo_score(img1, img2, d_row, d_col, radius, offset=0, min_score=None, maps=None, out=None,
                return_warped=False, return_rejected=False, stream=None):
    """Photo-consistency of a disparity map (dm_photo_score).  ``img1``, ``img2``: 2-D uint8
    images of one shape, numpy arrays or tensors, host or device; a tensor may be a view with a
    row stride (its rows must be contiguous, else it is copied).  ``d_row``, ``d_col``: float64
    device tensors [H][W], the 'elevation2' and 'elevation' planes.  ``offset``: an int or
    (oy, ox); map cell (y, x) is image pixel (y + oy, x + ox).  A cell's score is the zero-mean
    normalised cross-correlation, in [-1, 1], of the (2 radius + 1)^2 window of img1 around it with
    img2 resampled bilinearly at (y + oy - d_row, x + ox - d_col); NaN where d_row or d_col is not
    finite or a window leaves the image; exactly 0.0 where a window is flat.
    With ``min_score`` (a real in [-1, 1]) ``maps`` -- float64 [H][W] or [M][H][W] on the planes'
    device -- is required: the cells scoring below it become NaN in every plane, all other cells
    keep their bits; the result goes to ``out`` if given (``out=maps`` works in place; d_row and
    d_col may be planes of it), else to a new tensor.
    -> score [H][W]; with ``min_score`` (score, rejected maps); then, when asked for, the warped
    plane (img2 resampled at the centre; NaN outside the image) and the uint8 mask of the
    rejected cells (``return_rejected`` needs ``min_score``) are appended."""
    dev = _planes_device(d_row, d_col)
    radius = photo_params(radius)[0]
    oy, ox = _offset(offset)
    if min_score is not None:
        min_score = photo_params((radius, min_score))[1]
        if not (isinstance(maps, torch.Tensor) and maps.device == dev and maps.dtype == torch.float64 and
                maps.dim() in (2, 3) and maps.shape[-2:] == d_row.shape):
            raise ValueError('min_score needs maps: a float64 tensor [H][W] or [M][H][W] on the planes\' device')
        _check_out(out, maps)
    else:
        if maps is not None or out is not None:
            raise ValueError('maps and out need min_score')
        if return_rejected:
            raise ValueError('return_rejected needs min_score')
    H, W = d_row.shape
    with _on(stream):
        a, b = _pair_images(img1, img2, dev)
        score = torch.empty((H, W), dtype=torch.float64, device=dev)
        warped = torch.empty((H, W), dtype=torch.float64, device=dev) if return_warped else None
        rejected = torch.empty((H, W), dtype=torch.uint8, device=dev) if return_rejected else None
        M = 1
        if min_score is not None:
            M = 1 if maps.dim() == 2 else maps.shape[0]
            # (the planes are read from where they are: in place they alias `out`, which the kernel allows)
            if out is None:
                out = maps.clone(memory_format=torch.contiguous_format)
            elif out.data_ptr() != maps.data_ptr():
                out.copy_(maps)
        if H and W and M:
            if not a.numel():
                raise ValueError('empty image')
            lib = L.load()
            work = _workspace(lib.dm_photo_bytes(M, H, W), dev,
                              'photo_score does not take %d maps of %d x %d cells' % (M, H, W))
            rows, cols = _held_planes(d_row, d_col)
            L.check(lib.dm_photo_score(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), a.shape[0], a.shape[1],
                                       L.ptr(rows), L.ptr(cols), H, W, int(oy), int(ox),
                                       radius, L.DM_PHOTO_REJECT if min_score is not None else 0,
                                       min_score if min_score is not None else 0.0,
                                       L.ptr(out) if min_score is not None else L.ptr(None), M, L.ptr(score),
                                       L.ptr(warped), L.ptr(rejected), L.ptr(work), L.stream_handle()),
                    'dm_photo_score')
    res = (score,) + ((out,) if min_score is not None else ()) + ((warped,) if return_warped else ()) + \
        ((rejected,) if return_rejected else ())
    return res if len(res) > 1 else score


def photo_stage(img1, img2, d_map, modes, photo, offset, reject):
    """One stage of the ``photo=`` chain on the stitched d_map [len(modes)][H][W], in place.
    ``reject``: the rejection after the median -> (d_map, uint8 mask); else the score of the final
    planes -> score."""
    ir, ic = photo_planes(modes)
    if reject:
        _, d, rejected = photo_score(img1, img2, d_map[ir], d_map[ic], photo[0], offset=offset, min_score=photo[1],
                                     maps=d_map, out=d_map, return_rejected=True)
        return d, rejected
    return photo_score(img1, img2, d_map[ir], d_map[ic], photo[0], offset=offset)


def refine_params(refine):
    """The ``refine=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius, search,
    min_gain): ``(radius, search)`` or ``(radius, search, min_gain)`` with an int radius in [1, 7]
    (the window is (2 radius + 1)^2 pixels), an int search in [1, 3] (the candidates are the
    (2 search + 1)^2 integer neighbours) and min_gain a real in [0, 2] (0.0 in the first form): a
    neighbour replaces the cell's own position only if it scores more than min_gain higher."""
    if not isinstance(refine, (tuple, list)) or len(refine) not in (2, 3):
        raise ValueError('refine must be (radius, search), (radius, search, min_gain) or None')
    radius, search = refine[0], refine[1]
    min_gain = refine[2] if len(refine) == 3 else 0.0
    return (_int_in(radius, 1, 7, 'refine radius must be an int in [1, 7] (got %r)'),
            _int_in(search, 1, 3, 'refine search must be an int in [1, 3] (got %r)'),
            _real_in(min_gain, 0.0, 2.0, 'refine min_gain must be a real in [0, 2] (got %r)'))


def refine_planes(modes):
    """photo_planes for ``refine=``: the indices (row, column) of 'elevation2' and 'elevation';
    ValueError when one is missing, or when 'distance' is asked for: a refined cell would make
    that plane stale."""
    if 'distance' in list(modes):
        raise ValueError("refine does not take 'distance' in degree_map_mode: a refined cell would make it stale "
                         '(got %r)' % (list(modes),))
    return photo_planes(modes)


def refine_where(where, fill, keyword='refine_where'):
    """The ``refine_where=`` keyword, and ``lsm_where=`` under its own name: 'filled' (only the cells
    the fill produced; needs ``fill=``) or 'all'."""
    if where not in ('filled', 'all'):
        raise ValueError("%s must be 'filled' or 'all'" % keyword)
    if where == 'filled' and fill is None:
        raise ValueError("%s='filled' needs fill=" % keyword)
    return where


def photo_refine(img1, img2, d_row, d_col, radius, search, offset=0, min_gain=0.0, subpix=True, mask=None,
                 out=None, return_score=False, return_shift=False, stream=None):
    """Local re-matching of a disparity map (dm_photo_refine).  Images, planes, ``offset`` and
    ``radius`` as in photo_score.  Every cell scores the (2 search + 1)^2 integer neighbours of
    the position its disparity claims, search in [1, 3], with photo_score's correlation and moves
    to the best one (ties: the nearest, then the smaller dy, then the smaller dx) if that scores
    more than ``min_gain`` (a real in [0, 2]) above its own position; with ``subpix`` a parabola
    through the winner's scored neighbours refines each axis by at most half a pixel.  A cell
    whose own position wins, a cell that is not finite, whose img1 window leaves the image or
    that has no scored candidate keeps its bits.  ``mask``: a uint8 or bool tensor [H][W] on the
    planes' device; only the cells where it is not 0 are refined.  ``out``: a pair of contiguous
    float64 tensors [H][W] for the two planes (``out=(d_row, d_col)`` works in place when they are
    contiguous), else new tensors.
    -> (d_row', d_col'); then, when asked for, the float64 score of the position kept (NaN for a
    skipped cell) and the int8 shift [2][H][W] (dy, dx) are appended."""
    _planes_device(d_row, d_col)
    radius, search, min_gain = refine_params((radius, search, min_gain))
    res = _rematch('dm_photo_refine', lambda lib, Hi, Wi, H, W: lib.dm_photo_refine_bytes(Hi, Wi, H, W, radius, search),
                   img1, img2, d_row, d_col, offset, mask, out,
                   (radius, search, min_gain, L.DM_REFINE_SUBPIX if subpix else 0), return_score,
                   (2,) + tuple(d_row.shape) if return_shift else None, stream,
                   'photo_refine does not take %(H)d x %(W)d cells on a %(Hi)d x %(Wi)d image')
    return tuple(t for t in res if t is not None)


def refine_stage(img1, img2, d_map, modes, refine, offset, holes=None):
    """The ``refine=`` stage of the chain on the stitched d_map [len(modes)][H][W], in place, after
    the fill and before the smoothing.  ``holes``: the fill's uint8 mask [len(modes)][H][W] --
    only the cells that were filled in the row or in the column plane are refined
    (refine_where='filled') -- or None: every cell.  -> (d_map, score, int8 shift [2][H][W])."""
    return _plane_stage(photo_refine, img1, img2, d_map, modes, holes, refine[0], refine[1], offset=offset,
                        min_gain=refine[2], return_score=True, return_shift=True)


def lsm_params(lsm):
    """The ``lsm=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius, iters,
    max_move): ``(radius, iters)`` or ``(radius, iters, max_move)`` with an int radius in [1, 7]
    (the window is (2 radius + 1)^2 pixels), an int iters in [1, 8] (the least-squares steps) and
    max_move a real in (0, 2] (1.0 in the first form): a cell whose position leaves the square of
    that half-side around its start keeps its input."""
    if not isinstance(lsm, (tuple, list)) or len(lsm) not in (2, 3):
        raise ValueError('lsm must be (radius, iters), (radius, iters, max_move) or None')
    radius, iters = lsm[0], lsm[1]
    max_move = lsm[2] if len(lsm) == 3 else 1.0
    return (_int_in(radius, 1, 7, 'lsm radius must be an int in [1, 7] (got %r)'),
            _int_in(iters, 1, 8, 'lsm iters must be an int in [1, 8] (got %r)'),
            _real_in(max_move, 0.0, 2.0, 'lsm max_move must be a real in (0, 2] (got %r)', open_lo=True))


def lsm_refine(img1, img2, d_row, d_col, radius, iters, offset=0, max_move=1.0, mask=None, out=None,
               return_score=False, return_status=False, stream=None):
    """Least-squares sub-pixel matching of a disparity map (dm_lsm_refine).  Images, planes,
    ``offset`` and ``radius`` as in photo_score.  Every cell linearises img1 around its window and
    solves ``iters`` times, iters in [1, 8], for the shift that best explains the window by img2
    resampled at the current position, gain and offset free; the new position is kept if
    photo_score's correlation there is strictly higher than at the start and no step left the
    square of half-side ``max_move`` (a real in (0, 2]) around the start or the image.  Every other
    cell keeps its bits.  ``mask``: a uint8 or bool tensor [H][W] on the planes' device; only the
    cells where it is not 0 are refined.  ``out``: a pair of contiguous float64 tensors [H][W] for
    the two planes (``out=(d_row, d_col)`` works in place when they are contiguous), else new
    tensors.
    -> (d_row', d_col'); then, when asked for, the float64 score (of the new position of an
    accepted cell, else of the start; NaN for a cell that was not scored) and the int8 status
    [H][W] are appended: ``iters`` accepted, 0 skipped, -1 no texture (a singular system or a flat
    patch), -2 left the image or the square, -3 not better."""
    _planes_device(d_row, d_col)
    radius, iters, max_move = lsm_params((radius, iters, max_move))
    res = _rematch('dm_lsm_refine', lambda lib, Hi, Wi, H, W: lib.dm_lsm_refine_bytes(Hi, Wi, H, W, radius, iters),
                   img1, img2, d_row, d_col, offset, mask, out, (radius, iters, max_move, 0), return_score,
                   tuple(d_row.shape) if return_status else None, stream,
                   'lsm_refine does not take %(H)d x %(W)d cells on a %(Hi)d x %(Wi)d image')
    return tuple(t for t in res if t is not None)


def lsm_stage(img1, img2, d_map, modes, lsm, offset, holes=None):
    """The ``lsm=`` stage of the chain on the stitched d_map [len(modes)][H][W], in place, after the
    refine stage and before the smoothing.  ``holes``: the fill's uint8 mask [len(modes)][H][W] --
    only the cells that were filled in the row or in the column plane are matched
    (lsm_where='filled') -- or None: every cell.  -> (d_map, score, int8 status [H][W])."""
    return _plane_stage(lsm_refine, img1, img2, d_map, modes, holes, lsm[0], lsm[1], offset=offset, max_move=lsm[2],
                        return_score=True, return_status=True)


def lsm_model_params(model):
    """The ``lsm_model=`` keyword of ImageCutSolver / shard.solve_image_sharded as (name, max_shear):
    ``'shift'`` -> ('shift', None), the two-parameter solve of lsm_refine; ``'affine'`` or
    ``('affine', max_shear)`` -> ('affine', max_shear), the six-parameter solve of lsm_affine with
    max_shear a real in (0, 1) (0.5 in the first form).  The parsed tuples are taken as well."""
    if isinstance(model, (tuple, list)) and len(model) == 2 and isinstance(model[0], str):
        name, shear = model
    elif isinstance(model, str):
        name, shear = model, (0.5 if model == 'affine' else None)
    else:
        name = shear = None
    if name == 'shift' and shear is None:
        return 'shift', None
    if name != 'affine':
        raise ValueError("lsm_model must be 'shift', 'affine' or ('affine', max_shear) (got %r)" % (model,))
    shear = _real_in(shear, 0.0, 1.0, 'lsm_model max_shear must be a real in (0, 1) (got %r)', open_lo=True)
    if not shear < 1.0:
        raise ValueError('lsm_model max_shear must be a real in (0, 1) (got %r)' % (model[1],))
    return 'affine', shear


def lsm_affine(img1, img2, d_row, d_col, radius, iters, offset=0, max_move=1.0, max_shear=0.5, mask=None, out=None,
               return_score=False, return_status=False, return_affine=False, stream=None):
    """Affine least-squares matching of a disparity map (dm_lsm_affine, include/dmstereo_lsm.h).
    Arguments as lsm_refine, but ``radius`` in [2, 7].  Every cell solves ``iters`` times for the
    affine warp -- the shift of lsm_refine plus stretch and shear on both axes -- under which img2
    best explains its img1 window: tap (u, v) of the window is sampled at X = px + (1 + a) u + b v,
    Y = py + c u + (1 + d) v.  On a slope of the terrain, where the disparity changes across the
    window, the shift-only solve is biased; this one is not.  The new position is kept if the
    correlation under the final warp is strictly higher than photo_score's at the start and no step
    left the square of half-side ``max_move`` around the start, the image, or |a|, |b|, |c|, |d| <=
    ``max_shear`` (a real in (0, 1)).  Every other cell keeps its bits.
    -> (d_row', d_col'); then, when asked for, the float64 score, the int8 status [H][W] (as
    lsm_refine's; -1 also for a window whose texture cannot carry six parameters) and the float64
    affine values [4][H][W] (a, b, c, d; NaN unless accepted) are appended: -a and -d are the
    disparity gradients along the columns and along the rows."""
    _planes_device(d_row, d_col)
    radius, iters, max_move = lsm_params((radius, iters, max_move))
    if radius < 2:
        raise ValueError('lsm radius must be an int in [2, 7] for the affine model (got %r)' % (radius,))
    max_shear = lsm_model_params(('affine', max_shear))[1]
    res = _rematch('dm_lsm_affine', lambda lib, Hi, Wi, H, W: lib.dm_lsm_affine_bytes(Hi, Wi, H, W, radius, iters),
                   img1, img2, d_row, d_col, offset, mask, out, (radius, iters, max_move, max_shear, 0), return_score,
                   tuple(d_row.shape) if return_status else None, stream,
                   'lsm_affine does not take %(H)d x %(W)d cells on a %(Hi)d x %(Wi)d image',
                   extra_shape=(4,) + tuple(d_row.shape) if return_affine else None)
    return tuple(t for t in res if t is not None)


def lsm_affine_stage(img1, img2, d_map, modes, lsm, offset, holes=None):
    """lsm_stage under lsm_model='affine': ``lsm`` is lsm_params' tuple with max_shear appended.
    -> (d_map, score, int8 status [H][W], float64 affine [4][H][W])."""
    return _plane_stage(lsm_affine, img1, img2, d_map, modes, holes, lsm[0], lsm[1], offset=offset, max_move=lsm[2],
                        max_shear=lsm[3], return_score=True, return_status=True, return_affine=True)


def sgm_params(sgm):
    """The ``sgm=`` keyword of ImageCutSolver / shard.solve_image_sharded as (radius, search, p1, p2,
    paths): ``(radius, search, p1, p2)`` or ``(radius, search, p1, p2, paths)`` with an int radius in
    [1, 7] (the window is (2 radius + 1)^2 pixels), an int search in [1, 3] (the labels are the
    (2 search + 1)^2 integer neighbours), the penalties p1 <= p2 for a step of one pixel and of more
    between neighbouring cells, reals in [0, 16] in units of the score, returned as ints in units
    of 1/1024 (dm_sgm_refine's), and paths 4 or 8 (8 in the first form)."""
    if not isinstance(sgm, (tuple, list)) or len(sgm) not in (4, 5):
        raise ValueError('sgm must be (radius, search, p1, p2), (radius, search, p1, p2, paths) or None')
    paths = sgm[4] if len(sgm) == 5 else 8
    radius = _int_in(sgm[0], 1, 7, 'sgm radius must be an int in [1, 7] (got %r)')
    search = _int_in(sgm[1], 1, 3, 'sgm search must be an int in [1, 3] (got %r)')
    p1 = _real_in(sgm[2], 0.0, 16.0, 'sgm p1 must be a real in [0, 16] (got %r)')
    p2 = _real_in(sgm[3], 0.0, 16.0, 'sgm p2 must be a real in [0, 16] (got %r)')
    if p1 > p2:
        raise ValueError('sgm penalties must satisfy p1 <= p2 (got %r, %r)' % (sgm[2], sgm[3]))
    if isinstance(paths, bool) or not isinstance(paths, (int, np.integer)) or int(paths) not in (4, 8):
        raise ValueError('sgm paths must be 4 or 8 (got %r)' % (paths,))
    return radius, search, int(np.rint(p1 * 1024.0)), int(np.rint(p2 * 1024.0)), int(paths)


def sgm_refine(img1, img2, d_row, d_col, radius, search, p1, p2, paths=8, offset=0, subpix=True, mask=None,
               out=None, return_score=False, return_shift=False, stream=None):
    """Semi-global re-matching of a disparity map (dm_sgm_refine, include/dmstereo_sgm.h).  Images,
    planes, ``offset`` and ``radius`` as in photo_score.  Every cell snaps to the nearest integer
    position and has the (2 search + 1)^2 integer neighbours of it as labels, search in [1, 3]; the
    cost of a label is 1 - photo_score's correlation there in units of 1/1024, and along ``paths``
    (4 or 8) scan directions a step of one pixel between the displacements of neighbouring cells
    costs ``p1``, a larger one ``p2`` (reals in score units, 0 <= p1 <= p2 <= 16).  A cell moves to
    the label with the smallest sum of path costs (ties: the nearest, then the smaller ay, then the
    smaller ax); with ``subpix`` a parabola through the sums of the winner's neighbours refines each
    axis by at most half a pixel.  A cell whose own label wins, a cell that is not finite or that
    has no scored label keeps its bits.  ``mask``: a uint8 or bool tensor [H][W] on the planes'
    device; the cells where it is 0 are anchors: they keep their bits and hold their neighbours to
    their own displacement.  ``out``: a pair of contiguous float64 tensors [H][W] for the two planes
    (``out=(d_row, d_col)`` works in place when they are contiguous), else new tensors.
    -> (d_row', d_col'); then, when asked for, the float64 score of the label kept (NaN for a dead
    cell, an anchor and a cell without a scored label) and the int8 shift [2][H][W] (ay, ax) are
    appended."""
    _planes_device(d_row, d_col)
    return _sgm_rematch(img1, img2, d_row, d_col, sgm_params((radius, search, p1, p2, paths)), offset=offset,
                        subpix=subpix, mask=mask, out=out, return_score=return_score, return_shift=return_shift,
                        stream=stream)


def _sgm_rematch(img1, img2, d_row, d_col, sgm, offset=0, subpix=True, mask=None, out=None, return_score=False,
                 return_shift=False, stream=None):
    """sgm_refine with its parameters as sgm_params' tuple (the penalties as ints in units of 1/1024)."""
    radius, search, q1, q2, paths = sgm
    res = _rematch('dm_sgm_refine', lambda lib, Hi, Wi, H, W: lib.dm_sgm_bytes(H, W, search, paths),
                   img1, img2, d_row, d_col, offset, mask, out,
                   (radius, search, paths, q1, q2, L.DM_SGM_SUBPIX if subpix else 0), return_score,
                   (2,) + tuple(d_row.shape) if return_shift else None, stream,
                   'sgm_refine does not take %(H)d x %(W)d cells')
    return tuple(t for t in res if t is not None)


def sgm_stage(img1, img2, d_map, modes, sgm, offset, holes=None):
    """The ``sgm=`` stage of the chain on the stitched d_map [len(modes)][H][W], in place, after the
    fill and before the refine stage.  ``sgm``: sgm_params' tuple (the penalties in units of
    1/1024).  ``holes``: the fill's uint8 mask [len(modes)][H][W] -- only the cells that were filled
    in the row or in the column plane are matched again, every other cell is an anchor
    (sgm_where='filled') -- or None: every cell.  -> (d_map, score, int8 shift [2][H][W])."""
    return _plane_stage(_sgm_rematch, img1, img2, d_map, modes, holes, sgm, offset=offset, return_score=True,
                        return_shift=True)


# ---- disparity priors (csrc/dm_prior.hip; include/dmstereo.h has the definitions) ----------------
def downsample2(img, device=None, stream=None):
    """The half-resolution image (dm_downsample2): a 2-D uint8 image, a numpy array or a tensor
    (a view with a row stride is read where it is), -> the uint8 device tensor [H // 2][W // 2] of
    (a + b + c + d + 2) >> 2 over each 2 x 2 block; an odd last row or column is dropped."""
    if device is None:
        device = img.device if isinstance(img, torch.Tensor) and img.is_cuda else default_device()
    with _on(stream):
        a = _photo_image(img, device)
        H, W = a.shape
        if H < 2 or W < 2:
            raise ValueError('an image of %d x %d has no 2 x 2 block' % (H, W))
        out = torch.empty((H // 2, W // 2), dtype=torch.uint8, device=device)
        L.check(L.load().dm_downsample2(L.ptr(a), a.stride(0), H, W, L.ptr(out), out.stride(0), L.stream_handle()),
                'dm_downsample2')
    return out


def _tile_shape(h0, w0):
    msg = 'tile sides must be ints in [1, 65536] (got %r)'
    return _int_in(h0, 1, 65536, msg), _int_in(w0, 1, 65536, msg)


def _origins_host(origins):
    """Tile origins as a host int64 array [T][2], T >= 1, none negative; else ValueError."""
    org = np.asarray(origins)
    if org.dtype.kind not in 'iu' or org.size == 0 or org.size % 2:
        raise ValueError('origins must be a non-empty int array [T][2]')
    org = org.astype(np.int64).reshape(-1, 2)
    if org.min() < 0 or org.max() > 2 ** 30:
        raise ValueError('origins must lie in [0, 2^30]')
    return org


def _prior_device(prior, T, device):
    """A prior as a contiguous int32 device tensor [T][2]: an int array or tensor [T][2] (host or
    device; a device tensor is used where it is, without a look at its values)."""
    if isinstance(prior, torch.Tensor):
        if prior.dtype not in (torch.int32, torch.int64) or tuple(prior.shape) != (T, 2):
            raise ValueError('prior must be an int tensor [%d][2]' % T)
        return prior.to(device=device, dtype=torch.int32).contiguous()
    q = np.asarray(prior)
    if q.dtype.kind not in 'iu' or q.shape != (T, 2):
        raise ValueError('prior must be an int array [%d][2]' % T)
    if q.size and np.abs(q.astype(np.int64)).max() > 2 ** 30:
        raise ValueError('prior must lie in [-2^30, 2^30]')
    return torch.from_numpy(np.ascontiguousarray(q.astype(np.int32))).to(device)


def origins_device(origins, device):
    """Tile origins as a contiguous int32 device tensor [T][2]: a host int array (checked and
    uploaded) or such a tensor already on ``device`` (taken as it is: a caller that uploads the
    origins of several solves ahead keeps the copies out of the way of the kernels)."""
    if isinstance(origins, torch.Tensor) and origins.is_cuda:
        if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or not len(origins) or \
                origins.device != device or not origins.is_contiguous():
            raise ValueError('device origins must be a contiguous int32 tensor [T][2] on the planes\' device')
        return origins
    return torch.from_numpy(_origins_host(origins).astype(np.int32)).to(device)


def tile_prior(d_row, d_col, origins, h0, w0, e, scale=2, stream=None):
    """One integer prior per tile from a map of the pair (dm_tile_prior).  ``d_row``, ``d_col``:
    float64 device tensors [Hc][Wc], the 'elevation2' and 'elevation' planes of a map whose cell
    (y, x) sits at pixel (y + e, x + e) of an image ``scale`` (1 or 2) times smaller than the one
    the tiles (``origins`` [T][2], host or device (origins_device), h0 x w0 cells) are cut from.  A
    tile's footprint in the map is
    rows (o_y + e) // scale - e .. (o_y + e + h0 - 1) // scale - e, each end clamped into the map,
    columns alike; over its cells where both planes are finite, the prior is rint(scale * lower
    median) per plane.  A tile without such a cell takes the lower median of the other tiles'
    priors (0 if there is none).  -> (q, valid): int32 [T][2] (row, column) and uint8 [T], 1 for
    the tiles that measured their own prior; both stay on the device, nothing synchronises."""
    dev = _planes_device(d_row, d_col)
    h0, w0 = _tile_shape(h0, w0)
    e = _int_in(e, 0, 65536, 'e must be an int in [0, 65536] (got %r)')
    if isinstance(scale, bool) or scale not in (1, 2):
        raise ValueError('scale must be 1 or 2 (got %r)' % (scale,))
    if d_row.numel() == 0:
        raise ValueError('empty map')
    with _on(stream):
        o = origins_device(origins, dev)
        T = len(o)
        q = torch.empty((T, 2), dtype=torch.int32, device=dev)
        valid = torch.empty((T,), dtype=torch.uint8, device=dev)
        rows, cols = _held_planes(d_row, d_col)
        L.check(L.load().dm_tile_prior(L.ptr(rows), L.ptr(cols), d_row.shape[0],
                                       d_row.shape[1], L.ptr(o), T, h0, w0, e, int(scale), L.ptr(q), L.ptr(valid),
                                       L.stream_handle()), 'dm_tile_prior')
    return q, valid


def pack_grid(T, h0, w0, ws):
    """Where pack_tiles puts its T crops (dm_pack_plan): (origins, Hp, Wp), the host int64 array
    [T][2] of the crops' top-left corners in the packed images and the packed images' shape."""
    gx, Hp, Wp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    L.check(L.load().dm_pack_plan(int(T), int(h0), int(w0), int(ws), ctypes.byref(gx), ctypes.byref(Hp),
                                  ctypes.byref(Wp)), 'dm_pack_plan')
    t = np.arange(int(T), dtype=np.int64)
    org = np.stack([(t // gx.value) * (int(h0) + int(ws) - 1), (t % gx.value) * (int(w0) + int(ws) - 1)], axis=1)
    return org, Hp.value, Wp.value


def pack_tiles(img1, img2, origins, prior, h0, w0, ws, device=None, stream=None):
    """The crop pairs of T tiles with a disparity prior, side by side in a fresh image pair
    (dm_pack_tiles).  Crop t of img1 is cut at origins[t], crop t of img2 at origins[t] - prior[t]
    clamped per axis into the image, so every packed crop pixel is a real pixel.  ``prior``: int
    [T][2] (row, column), host or device, in the units and sign of d_map ('elevation2',
    'elevation').  -> (pack1, pack2, pack_origins, q_eff): the packed uint8 images (one shape,
    contiguous; TileBatch takes them with pack_grid's origins), the device int32 [T][2] places of
    the crops (pack_grid's origins) and the device int32 [T][2] effective priors, origins[t] minus
    the clamped img2 origin.  Nothing synchronises."""
    device = device or default_device()
    h0, w0 = _tile_shape(h0, w0)
    ws = _int_in(ws, 1, 65536, 'window_size must be an int >= 1 (got %r)')
    org = _origins_host(origins)
    T = len(org)
    with _on(stream):
        a, b = _photo_image(img1, device), _photo_image(img2, device)
        if a.shape != b.shape:
            raise ValueError('img1 and img2 must have the same shape')
        H, W = a.shape
        # the kernel trusts these bounds as the solver's do (TileBatch): check them here, on the host
        if (org[:, 0] + h0 + ws - 1).max() > H or (org[:, 1] + w0 + ws - 1).max() > W:
            raise ValueError('tile crop outside the image')
        q = _prior_device(prior, T, device)
        _, Hp, Wp = pack_grid(T, h0, w0, ws)
        o = torch.from_numpy(org.astype(np.int32)).to(device)
        p1 = torch.empty((Hp, Wp), dtype=torch.uint8, device=device)
        p2 = torch.empty((Hp, Wp), dtype=torch.uint8, device=device)
        porg = torch.empty((T, 2), dtype=torch.int32, device=device)
        q_eff = torch.empty((T, 2), dtype=torch.int32, device=device)
        L.check(L.load().dm_pack_tiles(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), H, W, L.ptr(o), L.ptr(q), T,
                                       h0, w0, ws, L.ptr(p1), L.ptr(p2), L.ptr(porg), L.ptr(q_eff),
                                       L.stream_handle()), 'dm_pack_tiles')
    return p1, p2, porg, q_eff


def shift_matches(match, q_eff, stream=None):
    """In place on the matches of a packed solve, a contiguous float64 device tensor
    [T][3][h0][w0] (dm_shift_matches): rows 0 and 1 of tile t minus q_eff[t] (int32 device
    [T][2]), which expresses them in the frame of img1's tile; NaN stays NaN, the score row is
    untouched.  cal_map, stitch and stitch_merge then give global disparities.  -> match."""
    if not (isinstance(match, torch.Tensor) and match.is_cuda and match.dtype == torch.float64 and
            match.dim() == 4 and match.shape[1] == 3 and match.is_contiguous() and match.numel()):
        raise ValueError('match must be a contiguous float64 device tensor [T][3][h0][w0]')
    T, _, h0, w0 = match.shape
    if not (isinstance(q_eff, torch.Tensor) and q_eff.device == match.device and q_eff.dtype == torch.int32 and
            tuple(q_eff.shape) == (T, 2) and q_eff.is_contiguous()):
        raise ValueError('q_eff must be a contiguous int32 tensor [%d][2] on match\'s device' % T)
    with _on(stream):
        L.check(L.load().dm_shift_matches(L.ptr(match), L.ptr(q_eff), T, h0, w0, L.stream_handle()),
                'dm_shift_matches')
    return match


def consistency_tol(tol):
    """A forward-backward tolerance in pixels: a real >= 0."""
    return _real_in(tol, 0.0, np.inf, 'the consistency tolerance must be a real >= 0 (got %r)')


def solve_tiles_prior(img1, img2, origins, prior, h0, w0, ws, method, sub_pix=True, filtering=False,
                      filter_window_size=3, filtering_num=3, filtering_mode='median', device=None,
                      mem_budget=None, stream=None, consistency=None):
    """solve_tiles with one expected disparity per tile -> (match, q_eff), or (match, q_eff, err)
    with ``consistency``.  ``prior``: int [T][2] (row, column), host or device -- a device prior
    (tile_prior's) is never read on the host, so nothing synchronises between it and the solve.
    Per chunk of solve_tiles' chunk loop the crops are packed (pack_tiles: img2's cut at origin -
    prior, clamped into the image), the packed pair is solved by the unchanged path and the
    matches are shifted into the frame of img1's tile (shift_matches), so that match[:, 1] is
    the local match minus q_eff and cal_map / stitch give global disparities.  Packing per chunk
    keeps the extra memory at one chunk's crops: two images of about T_chunk (h0 + ws - 1)
    (w0 + ws - 1) bytes.  match: float64 [T][3][h0][w0]; q_eff: int32 [T][2], the priors that
    took effect after the clamp.  ``consistency``: a tolerance in pixels; the packed pair is then
    solved in both directions (solve_tiles_bidir) and checked per tile, in the local frames,
    before the shift (fb_check): the cells that fail are NaN in rows 0 and 1 of match, err
    [T][h0][w0] is the round-trip error.  A zero prior gives solve_tiles' tiles bit for bit."""
    device = device or default_device()
    tol = None if consistency is None else consistency_tol(consistency)
    h0, w0 = _tile_shape(h0, w0)
    org = _origins_host(origins)
    T = len(org)
    opts = (sub_pix, filtering, filter_window_size, filtering_num, filtering_mode)
    with _on(stream):
        a, b = to_device_u8(img1, device), to_device_u8(img2, device)
        q = _prior_device(prior, T, device)
        if mem_budget is None:
            mem_budget = int(os.environ.get('DM_MEM_BUDGET', 64 << 30))
        chunk = max(1, min(T, mem_budget // max(tile_bytes(h0, w0), 1)))
        out = torch.empty((T, 3, h0, w0), dtype=torch.float64, device=device)
        q_eff = torch.empty((T, 2), dtype=torch.int32, device=device)
        err = torch.empty((T, h0, w0), dtype=torch.float64, device=device) if tol is not None else None
        for s in range(0, T, chunk):
            o = org[s:s + chunk]
            p1, p2, _, qe = pack_tiles(a, b, o, q[s:s + chunk], h0, w0, ws, device=device)
            grid = pack_grid(len(o), h0, w0, ws)[0]
            if tol is None:
                m = solve_tiles(p1, p2, grid, h0, w0, ws, method, *opts, device=device, mem_budget=mem_budget)
            else:
                fwd, bwd = solve_tiles_bidir(p1, p2, grid, h0, w0, ws, method, *opts, device=device,
                                             mem_budget=mem_budget)
                err[s:s + len(o)], m = fb_check(fwd, bwd, tol)
            out[s:s + len(o)] = shift_matches(m, qe)
            q_eff[s:s + len(o)] = qe
            del p1, p2, m
    return (out, q_eff) if tol is None else (out, q_eff, err)


def coarse_params(coarse):
    """The ``coarse=`` keyword of ImageCutSolver as (k, tol): an int k in [1, 4], the number of
    half-resolution levels above the image, or ``(k, tol)`` with tol a real >= 0, the
    forward-backward tolerance of the coarse levels in their own pixels (1.0 in the first form)."""
    if isinstance(coarse, (tuple, list)):
        if len(coarse) != 2:
            raise ValueError('coarse must be a level count k, (k, tol) or None')
        k, tol = coarse
    else:
        k, tol = coarse, 1.0
    return (_int_in(k, 1, 4, 'coarse levels must be an int in [1, 4] (got %r)'),
            _real_in(tol, 0.0, np.inf, 'coarse tol must be a real >= 0 (got %r)'))


def prior_keyword(prior, ntiles):
    """The ``prior=`` keyword of ImageCutSolver -> (kind, value): ('tiles', int64 array
    [ntiles][2]) for a pair of ints (d2, d1) -- one expected ('elevation2', 'elevation') for every
    tile -- or an int array [ntiles][2] in tile order; ('dense', float64 [2][H][W], array or
    tensor) for a float map of the two planes at full resolution (tile_prior(scale=1) turns it
    into tile priors)."""
    if isinstance(prior, torch.Tensor):
        if prior.dtype == torch.float64 and prior.dim() == 3 and prior.shape[0] == 2 and prior.numel():
            return 'dense', prior
        raise ValueError('a tensor prior must be a float64 map [2][H][W]')
    q = np.asarray(prior)
    if q.dtype.kind in 'iu':
        if q.shape == (2,):
            q = np.tile(q.reshape(1, 2), (ntiles, 1))
        if q.shape != (ntiles, 2):
            raise ValueError('an int prior must be (d2, d1) or an array [%d][2] in tile order (got shape %r)'
                             % (ntiles, tuple(q.shape)))
        if np.abs(q.astype(np.int64)).max() > 2 ** 30:
            raise ValueError('prior must lie in [-2^30, 2^30]')
        return 'tiles', q.astype(np.int64)
    if q.dtype.kind == 'f' and q.ndim == 3 and q.shape[0] == 2 and q.size:
        return 'dense', np.ascontiguousarray(q, dtype=np.float64)
    raise ValueError('prior must be (d2, d1), an int array [%d][2] or a float map [2][H][W]' % ntiles)


def coarse_grids(shape, image_size, stride, window_size, k):
    """(tile counts, origins) of the levels 0 .. k of a coarse-to-fine solve: level j is the image
    halved j times (downsample2), cut with the same image_size, stride and window_size by the
    reference's floor rule (cut_grid).  ValueError if the coarsest level holds no tile."""
    shapes = [(int(shape[0]) >> j, int(shape[1]) >> j) for j in range(k + 1)]
    try:      # (the levels shrink: a tile at level k means one at every level)
        return [cut_grid(shp, image_size, stride, window_size) for shp in reversed(shapes)][::-1]
    except IndexError:
        raise ValueError('coarse=%d: no tile at the coarsest level (its %d x %d image holds no %d x %d tile with '
                         'window_size %d)' % (k, shapes[k][0], shapes[k][1], image_size[0], image_size[1],
                                              window_size)) from None


def solve_coarse_to_fine(img1, img2, image_size, stride, ws, method, coarse, sub_pix=True, filtering=False,
                         filter_window_size=3, filtering_num=3, filtering_mode='median', device=None,
                         mem_budget=None, stream=None, consistency=None, trace=None):
    """The tiles of a pair solved with priors from half-resolution solves of the same pair ->
    (match, q_eff, err or None, valid, n, origins): solve_tiles_prior's results for level 0, the
    uint8 [T] flags of the tiles that measured their own prior (tile_prior) and the level-0 tile
    grid (cut_grid).  ``coarse``: k or (k, tol) (coarse_params).  The procedure:
      images L_0 .. L_k, each downsample2 of the one before; the same image_size, stride, ws,
      matching and filtering arguments at every level (ValueError if L_k holds no tile);
      level k is solved with prior 0; every level j >= 1 with consistency=tol, its masked matches
      stitched by the overwriting stitch in modes ('elevation2', 'elevation') -- no merge, no
      chain -- and level j - 1 takes its priors from that map by tile_prior(scale=2);
      level 0 is solved with ``consistency`` (the caller's) and level 1's priors.
    The reachable disparity doubles per level.  The priors stay on the device: nothing
    synchronises between the levels.  ``trace``: a list that receives one dict per level solved,
    coarsest first (level, img1, img2, n, origins, prior, q_eff, match, err, and for a coarse level
    d_map, the stitched pair of planes): the stages' own outputs, for tests."""
    device = device or default_device()
    k, tol = coarse_params(coarse)
    h0, w0 = int(image_size[0]), int(image_size[1])
    e = int((ws - 1) / 2)
    opts = (sub_pix, filtering, filter_window_size, filtering_num, filtering_mode)
    with _on(stream):
        imgs = [(to_device_u8(img1, device), to_device_u8(img2, device))]
        if imgs[0][0].shape != imgs[0][1].shape:
            raise ValueError('img1 and img2 must have the same shape')
        grids = coarse_grids(imgs[0][0].shape, image_size, stride, ws, k)
        for _ in range(k):
            imgs.append((downsample2(imgs[-1][0]), downsample2(imgs[-1][1])))
        prior = torch.zeros((len(grids[k][1]), 2), dtype=torch.int32, device=device)
        valid = None
        org_dev = [origins_device(g[1], device) for g in grids[:k]]      # tile_prior's, uploaded ahead
        for j in range(k, -1, -1):
            n, org = grids[j]
            res = solve_tiles_prior(imgs[j][0], imgs[j][1], org, prior, h0, w0, ws, method, *opts, device=device,
                                    mem_budget=mem_budget, consistency=tol if j else consistency)
            rec = dict(level=j, img1=imgs[j][0], img2=imgs[j][1], n=n, origins=org, prior=prior, q_eff=res[1],
                       match=res[0], err=res[2] if len(res) > 2 else None)
            if j:
                d, _ = stitch(res[0], n, h0, w0, stride, ('elevation2', 'elevation'))
                prior, valid = tile_prior(d[0], d[1], org_dev[j - 1], h0, w0, e, scale=2)
                rec['d_map'] = d
            if trace is not None:
                trace.append(rec)
    n, org = grids[0]
    return res[0], res[1], (res[2] if len(res) > 2 else None), valid, n, org
