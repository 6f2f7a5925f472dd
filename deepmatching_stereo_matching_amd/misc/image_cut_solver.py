"""ImageCutSolver mirror (reference: misc/image_cut_solver.py:26-197).

The reference solves its tiles one after another (``_execute_matching``, :163-175).  Here
all tiles go to the GPU as batches (engine.solve_tiles: one fused level-0/level-1 launch,
one launch per pyramid level and per matching level for the whole batch), and the
stitching -- later tiles overwrite earlier ones, j outer / i inner -- runs in dm_stitch.
Output cells no tile covers are NaN (``np.empty`` garbage in the reference).
"""

import numpy as np
import torch
from PIL import Image

from deepmatching_stereo_matching_amd import _lib as L
from deepmatching_stereo_matching_amd import engine


class ImageCutSolver():
    '''
    小画像に切ってそれぞれdeepmatchingに入れる
    '''

    def __init__(
        self, img1, img2,
        image_size=[32, 32], stride=[32, 32], window_size=5,
        feature_name='cv2.TM_CCOEFF_NORMED', degree_map_mode=['elevation'],
        padding=False,
        sub_pix=True,
        filtering=False,
        filtering_window_size=3,
        filtering_num=3,
        filtering_mode='average',
        consistency=None,
        fill=None,
        merge=None,
        merge_min_count=1,
        speckle=None,
        smooth=None,
        smooth_guide='image',
        median=None,
        median_weight=None,
        photo=None,
        refine=None,
        refine_where='filled'
    ):
        self.img_shape = img1.shape
        assert self.img_shape == img2.shape, '2枚の画像は同じサイズ！'
        self.img1 = img1
        self.img2 = img2
        self.stride = stride
        self.window_size = window_size
        self.degree_map_mode = degree_map_mode
        self.exclusive_pix = int((window_size - 1) / 2)
        self.image_size = image_size
        self.trimed_size = [image_size[i] + 2 * self.exclusive_pix for i in range(2)]
        self.feature_name = feature_name
        if feature_name not in L.METHODS:
            from deepmatching_stereo_matching_amd.misc.Feature_value import Feature_value
            Feature_value(feature_name)  # prints + exits like the reference

        if padding:
            self._padding()

        # loop length
        self.len = [int(np.floor((self.img_shape[i] - self.trimed_size[i]) / self.stride[i])) for i in range(2)]

        self.padding = padding
        self.sub_pix = sub_pix
        self.filtering = filtering
        self.filtering_window_size = filtering_window_size
        self.filtering_num = filtering_num
        self.filtering_mode = filtering_mode
        # forward-backward consistency tolerance in pixels (None: the reference's behaviour)
        self.consistency = consistency
        self.consistency_map = None
        # Jacobi iterations of the hole fill of d_map (engine.fill_holes); None: d_map keeps its NaN
        self.fill = engine.fill_iterations(fill) if fill is not None else None
        self.hole_map = None
        # rule that merges the overlapping tiles of a pixel (engine.stitch_merge); None: the last tile wins
        if merge is not None:
            engine.merge_rule(merge)
        self.merge = merge
        self.merge_min_count = merge_min_count
        self.coverage_map = None
        self.spread_map = None
        # (max_size, max_diff) of the speckle filter of d_map (engine.filter_speckles), run after the
        # stitch and before the fill; None: no segment is removed
        self.speckle = engine.speckle_params(speckle) if speckle is not None else None
        self.speckle_map = None
        # (radius, sigma_color, sigma_space) of the bilateral smoothing of d_map (engine.bilateral_filter),
        # run last: after the stitch, the speckle filter and the fill; None: d_map is not smoothed.
        # smooth_guide: 'image' (img1 under the map's cells, uint8) or 'self' (the map guides itself)
        self.smooth = engine.smooth_params(smooth) if smooth is not None else None
        if smooth_guide not in ('image', 'self'):
            raise ValueError("smooth_guide must be 'image' or 'self'")
        self.smooth_guide = smooth_guide
        # radius, (radius,) or (radius, iters) of the median filter of d_map (engine.median_filter), run
        # immediately after the stitch: impulses go first, then blobs (speckle), holes (fill), smoothing;
        # None: no median.  median_weight: None (unweighted) or 'correlation' (weighted by out_map)
        self.median = engine.median_params(median) if median is not None else None
        if median_weight not in (None, 'correlation'):
            raise ValueError("median_weight must be None or 'correlation'")
        self.median_weight = median_weight
        # radius or (radius, min_score) of the photo-consistency score (engine.photo_score): img2 is
        # resampled where d_map claims the match and correlated with img1 around the cell.  photo_map is
        # the score of the final d_map; with min_score the cells scoring below it are also rejected
        # (NaN in every mode) after the median and before the speckle filter, and photo_reject_map marks
        # them.  Needs both 'elevation' and 'elevation2' in degree_map_mode.  None: nothing is scored
        self.photo = engine.photo_params(photo) if photo is not None else None
        if self.photo is not None:
            engine.photo_planes(degree_map_mode)
        self.photo_map = None
        self.photo_reject_map = None
        # (radius, search) or (radius, search, min_gain) of the local re-matching (engine.photo_refine), run
        # after the fill and before the smoothing: a cell scores the (2 search + 1)^2 integer neighbours of
        # the position it claims and moves to the best one.  refine_where: 'filled' (only the cells the fill
        # produced; needs fill=) or 'all'.  Needs 'elevation' and 'elevation2' and no 'distance' in
        # degree_map_mode.  refine_score_map is the score of the position kept (NaN: not refined),
        # refine_shift_map the int8 shift [2][H][W] (dy, dx).  None: nothing is refined
        self.refine = engine.refine_params(refine) if refine is not None else None
        self.refine_where = refine_where
        if self.refine is not None:
            engine.refine_planes(degree_map_mode)
            engine.refine_where(refine_where, self.fill)
        self.refine_score_map = None
        self.refine_shift_map = None

        self.log_flg = True

    def _padding(self):
        """Reproduces the reference exactly (:73-93): img1 is zero-padded by exclusive_pix
        (and copied in twice), img2 becomes all zeros of the padded size."""
        img1 = self.img1
        ex = self.exclusive_pix
        a = np.zeros([img1.shape[0] + 2 * ex, img1.shape[1] + 2 * ex])
        a[ex:-ex, ex:-ex] = img1
        self.img1 = a.astype(np.uint8)
        self.img2 = np.zeros(a.shape).astype(np.uint8)

    def _cut_and_pool(self):
        '''
        画像を切り出しリストで保存 (crops are views; the batched solver uses the origins)
        '''
        self.img1_sub = []
        self.img2_sub = []
        self.img_index = []
        for j in range(self.len[1]):
            for i in range(self.len[0]):
                r, c = self.stride[0] * i, self.stride[1] * j
                self.img1_sub.append(self.img1[r:r + self.trimed_size[0], c:c + self.trimed_size[1]])
                self.img2_sub.append(self.img2[r:r + self.trimed_size[0], c:c + self.trimed_size[1]])
                self.img_index.append([i, j])

    def _solver(self, solve_image, solve_template):
        """
        小画像に対しdeepmatchingを実施する: one (S+2e)^2 crop pair -> (d_maps, score map),
        as the reference's _solver (:115-142) returns them; solved by the same batched device
        path as _execute_matching (a batch of one tile).
        """
        h0 = np.shape(solve_image)[0] - 2 * self.exclusive_pix
        w0 = np.shape(solve_image)[1] - 2 * self.exclusive_pix
        self._log_pyramid(h0, w0)
        match = engine.solve_tiles(solve_image, solve_template, [[0, 0]], h0, w0, self.window_size,
                                   L.METHODS[self.feature_name], self.sub_pix, self.filtering,
                                   self.filtering_window_size, self.filtering_num,
                                   self.filtering_mode)[0]
        d = np.array([engine.cal_map(match, m).cpu().numpy() for m in self.degree_map_mode])
        return d, match[2].cpu().numpy()

    def _log_pyramid(self, h0, w0):
        if self.log_flg:
            nlev, N = engine.pyramid_plan(h0, w0)
            print('complete to create multi-level correlation pyramid')
            print('pyramid level: {}, N={}'.format(nlev, N))
            self.log_flg = False

    def _execute_matching_device(self):
        """All tiles in batches on the GPU -> (d_map, out_map) device tensors.  The tile grid
        is self.len, counted on the image shape BEFORE _padding (:46,58-62).  Opted in to tile
        sharding (shard.tile_sharding() or DM_SHARD_TILES=1) under a torch.distributed process
        group, the tiles are sharded over its ranks by shard.BandSolver -- the path bench.py's
        c5_split line measures: rank r solves one contiguous band of tiles in chunks, each
        chunk's results gathered to rank 0 behind the compute, rank 0 stitches -- and the maps
        come back on every rank (one broadcast; tile_sharding(result='root'): rank 0 only, the
        others get None).  Every rank must then solve the same pair (shard.broadcast_pair
        sends it from rank 0).  With self.consistency set both branches solve the pair in both
        directions and return a third tensor, the stitched round-trip error (engine.stitch_fb).
        With self.fill set d_map comes back filled (engine.fill_holes) and the uint8 mask of the
        cells that were filled is the last tensor.  With self.merge set the stitch is
        engine.stitch_merge (both directions when self.consistency is set) and the spread and the
        uint8 count of valid candidates follow out_map / the error, before the hole mask.  With
        self.speckle set d_map loses its small segments (engine.filter_speckles) after the stitch
        and before the fill, and the uint8 mask of the cells removed comes immediately before the
        hole mask: (d_map, out_map[, err][, spread, count][, speckles][, holes]).  With self.smooth
        set d_map is smoothed last (engine.bilateral_filter, all modes in one call; holes stay
        holes, self.fill is what fills); no tensor is added.  With self.median set d_map is median
        filtered first, immediately after the stitch and before the speckle filter, the fill and the
        smoothing (engine.median_filter, all modes in one call, in place, weighted by out_map when
        self.median_weight is 'correlation'; holes stay holes); no tensor is added.  With self.photo
        set the final d_map is scored last (engine.photo_score against self.img1 / self.img2, map cell
        (y, x) at pixel (y + e, x + e), e = exclusive_pix) and the float64 score [H][W] is appended
        after every other tensor; with a min_score the cells that score below it are first rejected
        in every mode, after the median and before the speckle filter, and the uint8 mask [H][W] of
        those cells comes immediately before the score.  The chain is stitch -> median -> photo
        reject -> speckle -> fill -> smooth -> photo score, the tuple (d_map, out_map[, err]
        [, spread, count][, speckles][, holes][[, rejected], score]).  With self.refine set the cells
        are matched again locally (engine.photo_refine) after the fill and before the smoothing --
        only the filled ones with refine_where='filled' -- and the float64 score and the int8 shift
        [2][H][W] come immediately before the photo tensors: (d_map, out_map[, err][, spread, count]
        [, speckles][, holes][, refine score, refine shift][[, rejected], score])."""
        from deepmatching_stereo_matching_amd import shard
        n = list(self.len)
        if n[0] < 1 or n[1] < 1:
            raise IndexError('list index out of range')   # img_index[-1] of an empty cut (:150)
        origins = np.array([(self.stride[0] * i, self.stride[1] * j)
                            for j in range(n[1]) for i in range(n[0])], dtype=np.int64)
        h0, w0 = self.image_size
        self._log_pyramid(h0, w0)
        args = (self.img1, self.img2, origins, h0, w0, self.window_size,
                L.METHODS[self.feature_name], self.sub_pix, self.filtering,
                self.filtering_window_size, self.filtering_num, self.filtering_mode)
        if shard.tile_sharding_enabled():
            return shard.solve_image_sharded(self.img1, self.img2, [h0, w0], self.stride, self.window_size,
                                             L.METHODS[self.feature_name], self.degree_map_mode,
                                             self.sub_pix, self.filtering, self.filtering_window_size,
                                             self.filtering_num, self.filtering_mode,
                                             result=shard.shard_result(), grid=(n, origins),
                                             consistency=self.consistency, fill=self.fill,
                                             merge=self.merge, merge_min_count=self.merge_min_count,
                                             speckle=self.speckle, smooth=self.smooth,
                                             smooth_guide=self.smooth_guide, median=self.median,
                                             median_weight=self.median_weight, photo=self.photo,
                                             refine=self.refine, refine_where=self.refine_where)
        if self.merge is not None:
            if self.consistency is not None:
                fwd, bwd = engine.solve_tiles_bidir(*args)
            else:
                fwd, bwd = engine.solve_tiles(*args), None
            maps = engine.stitch_merge(fwd, bwd, n, h0, w0, self.stride, self.degree_map_mode, self.consistency,
                                       self.merge, self.merge_min_count)
            maps = tuple(m for m in maps if m is not None)      # a one-direction merge has no err
        elif self.consistency is not None:
            fwd, bwd = engine.solve_tiles_bidir(*args)
            maps = engine.stitch_fb(fwd, bwd, n, h0, w0, self.stride, self.degree_map_mode, self.consistency)
        else:
            match = engine.solve_tiles(*args)
            maps = engine.stitch(match, n, h0, w0, self.stride, self.degree_map_mode)
        if self.median is not None:
            d = engine.median_filter(maps[0], self.median[0], weight=engine.median_weight(self.median_weight, maps),
                                     iters=self.median[1], out=maps[0])
            maps = (d,) + tuple(maps[1:])
        rejected = None
        if self.photo is not None and self.photo[1] is not None:
            d, rejected = engine.photo_stage(self.img1, self.img2, maps[0], self.degree_map_mode, self.photo,
                                             self.exclusive_pix, True)
            maps = (d,) + tuple(maps[1:])
        if self.speckle is not None:
            d, removed = engine.filter_speckles(maps[0], *self.speckle, out=maps[0], return_removed=True)
            maps = (d,) + tuple(maps[1:]) + (removed,)
        if self.fill is not None:
            d, holes = engine.fill_holes(maps[0], self.fill, out=maps[0], return_holes=True)
            maps = (d,) + tuple(maps[1:]) + (holes,)
        if self.refine is not None:
            d, rscore, rshift = engine.refine_stage(self.img1, self.img2, maps[0], self.degree_map_mode, self.refine,
                                                    self.exclusive_pix,
                                                    maps[-1] if self.refine_where == 'filled' else None)
            maps = (d,) + tuple(maps[1:]) + (rscore, rshift)
        if self.smooth is not None:
            guide = engine.smooth_guide(self.img1, self.exclusive_pix, maps[0]) if self.smooth_guide == 'image' else None
            d = engine.bilateral_filter(maps[0], *self.smooth, guide=guide, out=maps[0])
            maps = (d,) + tuple(maps[1:])
        if self.photo is not None:
            score = engine.photo_stage(self.img1, self.img2, maps[0], self.degree_map_mode, self.photo,
                                       self.exclusive_pix, False)
            maps = tuple(maps) + ((rejected,) if rejected is not None else ()) + (score,)
        return maps

    def _execute_matching(self):
        """
        小画像ごとにマッチングを行い結果を結合
        """
        maps = self._execute_matching_device()
        if self.photo is not None:         # the last tensors: taken off first, the indices below stay as they were
            self.photo_map = maps[-1].cpu().numpy() if maps[-1] is not None else None
            maps = maps[:-1]
            if self.photo[1] is not None:  # the cells rejected for scoring below min_score (before any fill)
                self.photo_reject_map = maps[-1].cpu().numpy().astype(bool) if maps[-1] is not None else None
                maps = maps[:-1]
        if self.refine is not None:        # immediately before the photo tensors: taken off next
            self.refine_shift_map = maps[-1].cpu().numpy() if maps[-1] is not None else None
            self.refine_score_map = maps[-2].cpu().numpy() if maps[-2] is not None else None
            maps = maps[:-2]
        d_map, out_map = maps[0], maps[1]
        # (None on the ranks other than 0 of a sharded solve with tile_sharding(result='root'))
        self.d_map = d_map.cpu().numpy() if d_map is not None else None
        self.out_map = out_map.cpu().numpy() if out_map is not None else None
        if self.consistency is not None:   # [H][W] round-trip error; d_map is NaN where it exceeds the tolerance
            self.consistency_map = maps[2].cpu().numpy() if maps[2] is not None else None
        if self.merge is not None:         # valid candidates per pixel and their max - min, per mode
            k = 3 if self.consistency is not None else 2
            self.spread_map = maps[k].cpu().numpy() if maps[k] is not None else None
            self.coverage_map = maps[k + 1].cpu().numpy() if maps[k + 1] is not None else None
        if self.speckle is not None:       # the cells the speckle filter removed (before any fill)
            k = -2 if self.fill is not None else -1
            self.speckle_map = maps[k].cpu().numpy().astype(bool) if maps[k] is not None else None
        if self.fill is not None:          # d_map is dense; hole_map marks the cells that were filled
            self.hole_map = maps[-1].cpu().numpy().astype(bool) if maps[-1] is not None else None

    def __call__(self):
        self._cut_and_pool()
        self._execute_matching()
        return self.d_map, self.out_map

    @staticmethod
    def image_save(path, arr, threshold=[100, 190]):
        """
        numpy配列を画像として保存 (clamped to threshold, uint8 PNG)
        """
        arr = np.where(arr > threshold[1], threshold[1], arr)
        arr = np.where(arr < threshold[0], threshold[0], arr)
        pil_img = Image.fromarray(arr.astype(np.uint8))
        pil_img.save(path)
