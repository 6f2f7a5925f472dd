"""The whole chain of chain.py on the device against its nine engine calls written out: every stage on, the affine
lsm model.  This pins the arguments of every engine call that the table of chain.py makes."""

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import engine
from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_chain_table import ATTRS, BOOL, GEO, ON, PMODES

pytestmark = pytest.mark.gpu


def test_solver_equals_the_nine_engine_calls():
    a, b = stereo_pair(40, 40, seed=1, dx=2)
    kw = dict(degree_map_mode=list(PMODES), **GEO)
    base = ImageCutSolver(a, b, **kw)      # the tiles solved and stitched, once
    d, out_map = [t.clone() for t in base._execute_matching_device()]
    H, W = out_map.shape
    e, row, col = 2, 1, 0      # 'elevation2' is the row plane, 'elevation' the column plane

    d = engine.median_filter(d, 1, weight=out_map, iters=2, out=d)
    _, d, rejected = engine.photo_score(a, b, d[row], d[col], 2, offset=e, min_score=0.75, maps=d, out=d,
                                        return_rejected=True)
    d, speckles = engine.filter_speckles(d, 4, 1.0, out=d, return_removed=True)
    d, holes = engine.fill_holes(d, 16, out=d, return_holes=True)
    filled = holes[row] | holes[col]
    _, _, sgm_score, sgm_shift = engine.sgm_refine(a, b, d[row], d[col], 2, 2, 2.0, 8.0, paths=8, offset=e,
                                                   mask=filled, out=(d[row], d[col]), return_score=True,
                                                   return_shift=True)
    _, _, refine_score, refine_shift = engine.photo_refine(a, b, d[row], d[col], 2, 1, offset=e, min_gain=0.0,
                                                           mask=filled, out=(d[row], d[col]), return_score=True,
                                                           return_shift=True)
    _, _, lsm_score, lsm_status, lsm_affine = engine.lsm_affine(a, b, d[row], d[col], 2, 3, offset=e, max_move=1.0,
                                                                max_shear=0.5, mask=None, out=(d[row], d[col]),
                                                                return_score=True, return_status=True,
                                                                return_affine=True)
    guide = torch.from_numpy(a).to(d.device)[e:e + H, e:e + W].contiguous()
    d = engine.bilateral_filter(d, 2, 0.5, 2.0, guide=guide, out=d)
    score = engine.photo_score(a, b, d[row], d[col], 2, offset=e)

    want = dict(d_map=d, out_map=out_map, speckles=speckles, holes=holes, sgm_score=sgm_score, sgm_shift=sgm_shift,
                refine_score=refine_score, refine_shift=refine_shift, lsm_score=lsm_score, lsm_status=lsm_status,
                lsm_affine=lsm_affine, rejected=rejected, score=score)
    solver = ImageCutSolver(a, b, **ON, **kw)
    assert solver.chain.names(None, None) == [n for n in ATTRS if n in want]
    solver()
    for name, attr in ATTRS.items():
        got = getattr(solver, attr)
        if name not in want:      # err, spread, count: neither consistency= nor merge=
            assert got is None, attr
            continue
        w = want[name].cpu().numpy()
        w = w.astype(bool) if attr in BOOL else w
        assert got.dtype == w.dtype and got.shape == w.shape, attr
        assert got.tobytes() == w.tobytes(), attr      # bit for bit, NaNs included
    assert (H, W) == (16, 16) and solver.lsm_affine_map.shape == (4, 16, 16) and solver.sgm_shift_map.dtype == np.int8
