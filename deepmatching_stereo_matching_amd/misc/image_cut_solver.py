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
        merge=None,
        merge_min_count=1,
        prior=None,
        coarse=None,
        **keywords
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
        # rule that merges the overlapping tiles of a pixel (engine.stitch_merge); None: the last tile wins
        if merge is not None:
            engine.merge_rule(merge)
        self.merge = merge
        self.merge_min_count = merge_min_count
        # The post-processing of the stitched d_map: chain.py declares the stages, their keywords (which arrive
        # here as **keywords), their order and the *_map attributes their tensors land in.  Every keyword is kept
        # as parsed (None: the stage is off); every *_map is None until the solve.
        self.chain = chain.Chain(degree_map_mode, **keywords)
        for name in chain.keywords():
            setattr(self, name, getattr(self.chain, name))
        for o in chain.outputs():
            setattr(self, o.attr, None)
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
        its keywords switch on, against self.img1 / self.img2 with e = exclusive_pix), which appends the
        tensors of its stages: the tuple is the one chain.Chain.layout names.  The sharded branch is handed
        self.chain itself, so no keyword is parsed a second time."""
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
                                             consistency=self.consistency, merge=self.merge,
                                             merge_min_count=self.merge_min_count, prior=self.prior,
                                             coarse=self.coarse, chain=self.chain)
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

    def _execute_matching(self):
        """
        小画像ごとにマッチングを行い結果を結合
        """
        maps = dict(zip(self.chain.names(self.consistency, self.merge), self._execute_matching_device()))
        for o in chain.outputs():
            t = maps.get(o.name)      # absent: the stage is off; None: off rank 0 with tile_sharding(result='root')
            a = t.cpu().numpy() if t is not None else None
            setattr(self, o.attr, a.astype(bool) if o.mask and a is not None else a)
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
