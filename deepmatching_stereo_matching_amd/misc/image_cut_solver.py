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
from deepmatching_stereo_matching_amd import chain, engine


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
        refine_where='filled',
        prior=None,
        coarse=None,
        lsm=None,
        lsm_where='all',
        sgm=None,
        sgm_where='all',
        lsm_model='shift'
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

        if prior is not None and coarse is not None:
            raise ValueError('prior= and coarse= cannot be combined: coarse= measures the priors itself')
        if padding and (prior is not None or coarse is not None):
            raise ValueError('padding=True is not supported with prior= / coarse=: the reference zeroes img2 there')
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
        # rule that merges the overlapping tiles of a pixel (engine.stitch_merge); None: the last tile wins
        if merge is not None:
            engine.merge_rule(merge)
        self.merge = merge
        self.merge_min_count = merge_min_count
        self.coverage_map = None
        self.spread_map = None
        # The post-processing of the stitched d_map (chain.py has the stages and their order); every
        # keyword is kept as parsed, None: the stage is off.
        #   fill: Jacobi iterations of the hole fill; hole_map marks the cells that were filled
        #   speckle: (max_size, max_diff) of the speckle filter; speckle_map marks the cells removed
        #   smooth: (radius, sigma_color, sigma_space) of the bilateral smoothing; smooth_guide: 'image'
        #       (img1 under the map's cells, uint8) or 'self' (the map guides itself)
        #   median: radius, (radius,) or (radius, iters) of the median filter; median_weight: None
        #       (unweighted) or 'correlation' (weighted by out_map)
        #   photo: radius or (radius, min_score) of the photo-consistency score: img2 is resampled where
        #       d_map claims the match and correlated with img1 around the cell.  photo_map is the score of
        #       the final d_map; with min_score the cells scoring below it are also rejected (NaN in every
        #       mode) and photo_reject_map marks them.  Needs 'elevation' and 'elevation2' in degree_map_mode
        #   refine: (radius, search) or (radius, search, min_gain) of the local re-matching: a cell scores the
        #       (2 search + 1)^2 integer neighbours of the position it claims and moves to the best one.
        #       refine_where: 'filled' (only the cells the fill produced; needs fill=) or 'all'.  Needs
        #       'elevation' and 'elevation2' and no 'distance' in degree_map_mode.  refine_score_map is the
        #       score of the position kept (NaN: not refined), refine_shift_map the int8 shift [2][H][W]
        #   lsm: (radius, iters) or (radius, iters, max_move) of the least-squares sub-pixel matching after
        #       the refine stage: a cell solves iters times for the shift that best explains its img1 window
        #       and keeps it if the photo-consistency score rises.  lsm_where: 'all' or 'filled' (needs
        #       fill=).  The modes as for refine.  lsm_score_map is the score of the position kept (NaN: not
        #       scored), lsm_status_map the int8 status [H][W] (iters: accepted, 0: skipped, < 0: kept)
        #   lsm_model: 'shift' (the default), 'affine' or ('affine', max_shear): with 'affine' the lsm stage also
        #       solves for the stretch and shear of the window (engine.lsm_affine; radius >= 2), which removes the
        #       bias of the shift on sloped terrain.  lsm_affine_map is then the float64 [4][H][W] of (a, b, c, d),
        #       NaN unless accepted: -a and -d are the disparity gradients along the columns and the rows
        #   sgm: (radius, search, p1, p2) or (radius, search, p1, p2, paths) of the semi-global re-matching after
        #       the fill and before the refine stage: the cells snap to integer positions and are matched again
        #       together, the (2 search + 1)^2 candidates' costs and a smoothness term (p1 for a step of one pixel
        #       between neighbouring cells, p2 for more, in score units) minimised along 4 or 8 scan directions.
        #       sgm_where: 'all' or 'filled' (needs fill=; every other cell is then a fixed anchor).  The modes as
        #       for refine.  sgm_score_map is the score of the position kept (NaN: not matched), sgm_shift_map the
        #       int8 shift [2][H][W].  Kept as parsed: the penalties in units of 1/1024
        self.chain = chain.Chain(degree_map_mode, fill=fill, speckle=speckle, smooth=smooth, smooth_guide=smooth_guide,
                                 median=median, median_weight=median_weight, photo=photo, refine=refine,
                                 refine_where=refine_where, lsm=lsm, lsm_where=lsm_where, sgm=sgm,
                                 sgm_where=sgm_where, lsm_model=lsm_model)
        self._sgm_given = sgm      # the shard path parses the keyword itself: it gets what this solver was given
        for name in ('fill', 'speckle', 'smooth', 'smooth_guide', 'median', 'median_weight', 'photo', 'refine',
                     'refine_where', 'lsm', 'lsm_where', 'sgm', 'sgm_where', 'lsm_model'):
            setattr(self, name, getattr(self.chain, name))
        self.hole_map = self.speckle_map = self.photo_map = self.photo_reject_map = None
        self.refine_score_map = self.refine_shift_map = None
        self.lsm_score_map = self.lsm_status_map = self.lsm_affine_map = None
        self.sgm_score_map = self.sgm_shift_map = None
        # Disparity priors (engine.solve_tiles_prior): tile t's crop of img2 is cut at its origin minus
        # the expected disparity, so that a match outside the tile's own window of img2 can be found.
        #   prior: (d2, d1) ints, one expected ('elevation2', 'elevation') for every tile, in the units and
        #       sign of d_map; an int array [n0 * n1][2] in tile order (j outer, i inner); or a float map
        #       [2][H][W] of the two planes at full resolution, e.g. an earlier d_map (engine.tile_prior
        #       with scale 1 turns it into tile priors)
        #   coarse: k or (k, tol), 1 <= k <= 4: the priors come from k half-resolution solves of the same
        #       pair (engine.solve_coarse_to_fine), each checked forward-backward at tol (default 1.0)
        # prior_map is then the int32 [n0][n1][2] priors that took effect at level 0 (after the clamp of the
        # crop into the image), prior_valid_map the bool [n0][n1] tiles that measured their own prior (all
        # true for an int prior).  None (both): the reference's behaviour, bit for bit.
        self.prior = engine.prior_keyword(prior, max(self.len[0], 0) * max(self.len[1], 0)) if prior is not None else None
        self.coarse = engine.coarse_params(coarse) if coarse is not None else None
        if (self.prior is not None or self.coarse is not None) and merge is not None and consistency is not None:
            raise ValueError('merge= together with consistency= is not supported with prior= / coarse=: the merge '
                             'checks both directions in one frame, the tiles of a prior are checked in their own')
        self.prior_map = self.prior_valid_map = None
        self._prior_dev = None

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
        With self.merge set the stitch is engine.stitch_merge (both directions when
        self.consistency is set) and the spread and the uint8 count of valid candidates follow
        out_map / the error.  The stitched d_map then runs through self.chain (chain.py: the stages
        that self.fill, self.speckle, self.smooth, self.median, self.photo, self.sgm, self.refine and self.lsm switch on,
        against self.img1 / self.img2 with e = exclusive_pix), which appends the tensors of its
        stages: the tuple is the one chain.Chain.layout names."""
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
                                             refine=self.refine, refine_where=self.refine_where,
                                             lsm=self.lsm, lsm_where=self.lsm_where, lsm_model=self.lsm_model,
                                             sgm=self._sgm_given, sgm_where=self.sgm_where,
                                             prior=self.prior, coarse=self.coarse)
        if self.prior is not None or self.coarse is not None:
            maps = self._stitch_prior(args, n, origins)
        else:
            fwd, bwd = engine.solve_tiles_bidir(*args) if self.consistency is not None else (engine.solve_tiles(*args), None)
            maps = engine.stitch_any(fwd, bwd, n, h0, w0, self.stride, self.degree_map_mode, self.consistency,
                                     self.merge, self.merge_min_count)
        return self.chain.run(maps, self.img1, self.img2, self.exclusive_pix, self.consistency, self.merge)

    def _stitch_prior(self, args, n, origins):
        """The stitched maps of a solve with priors (self.prior or self.coarse) -> the head of the chain's
        layout.  Level 0 is engine.solve_tiles_prior: with self.consistency the tiles are checked per tile in
        their local frames (engine.fb_check), then shifted, then stitched in one direction, and the error is
        the overwriting stitch of the per-tile error; with self.merge the shifted tiles are merged as a
        one-direction solve.  The effective priors stay on the device (self._prior_dev) until the maps are
        fetched."""
        img1, img2, _, h0, w0, ws, method = args[:7]
        opts = args[7:]
        if self.coarse is not None:
            match, q_eff, err, valid, _, _ = engine.solve_coarse_to_fine(img1, img2, [h0, w0], self.stride, ws, method,
                                                                         self.coarse, *opts,
                                                                         consistency=self.consistency)
        else:
            kind, prior = self.prior
            valid = None
            if kind == 'dense':
                d = torch.as_tensor(prior).to(engine.default_device())
                prior, valid = engine.tile_prior(d[0], d[1], origins, h0, w0, self.exclusive_pix, scale=1)
            res = engine.solve_tiles_prior(img1, img2, origins, prior, h0, w0, ws, method, *opts,
                                           consistency=self.consistency)
            match, q_eff, err = res[0], res[1], (res[2] if len(res) > 2 else None)
        self._prior_dev = (q_eff, valid)
        maps = engine.stitch_any(match, None, n, h0, w0, self.stride, self.degree_map_mode, None, self.merge,
                                 self.merge_min_count)
        if err is not None and self.merge is None:      # the stitch of a tile's score row, fed with the error
            maps += (engine.stitch(torch.stack([err, err, err], 1), n, h0, w0, self.stride, ['elevation'])[1],)
        return maps

    # attribute: (entry of chain.Chain.layout, a uint8 mask that is kept as bool)
    _MAPS = {'d_map': ('d_map', False), 'out_map': ('out_map', False),
             'consistency_map': ('err', False),        # round-trip error; d_map is NaN where it exceeds the tolerance
             'spread_map': ('spread', False),          # max - min of the valid candidates of a pixel, per mode
             'coverage_map': ('count', False),         # their number
             'speckle_map': ('speckles', True),        # the cells the speckle filter removed (before any fill)
             'hole_map': ('holes', True),              # d_map is dense; the cells that were filled
             'sgm_score_map': ('sgm_score', False), 'sgm_shift_map': ('sgm_shift', False),
             'refine_score_map': ('refine_score', False), 'refine_shift_map': ('refine_shift', False),
             'lsm_score_map': ('lsm_score', False), 'lsm_status_map': ('lsm_status', False),
             'lsm_affine_map': ('lsm_affine', False),
             'photo_reject_map': ('rejected', True),   # the cells scoring below min_score (before any fill)
             'photo_map': ('score', False)}

    def _execute_matching(self):
        """
        小画像ごとにマッチングを行い結果を結合
        """
        maps = dict(zip(self.chain.names(self.consistency, self.merge), self._execute_matching_device()))
        for attr, (name, mask) in self._MAPS.items():
            t = maps.get(name)      # absent: the stage is off; None: off rank 0 with tile_sharding(result='root')
            a = t.cpu().numpy() if t is not None else None
            setattr(self, attr, a.astype(bool) if mask and a is not None else a)
        if self._prior_dev is not None:
            q_eff, valid = self._prior_dev
            n0, n1 = self.len
            self.prior_map = np.ascontiguousarray(q_eff.cpu().numpy().reshape(n1, n0, 2).transpose(1, 0, 2))
            self.prior_valid_map = np.ones((n0, n1), dtype=bool) if valid is None else \
                np.ascontiguousarray(valid.cpu().numpy().astype(bool).reshape(n1, n0).T)

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
