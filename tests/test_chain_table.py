"""The table of chain.py: every stage is declared once, and Chain, ImageCutSolver and shard.solve_image_sharded
take their keywords, hooks, layout and attributes from it.  CPU only: host hooks, the oracle as tile solver and a
host stitcher."""

import numpy as np
import pytest
import torch

from deepmatching_stereo_matching_amd import chain as chain_mod
from deepmatching_stereo_matching_amd import engine, shard
from deepmatching_stereo_matching_amd.misc.image_cut_solver import ImageCutSolver
from deepmatching_stereo_matching_amd.synthetic import stereo_pair

from test_fill_host import _host_stitch, _oracle_tiles

PMODES = ('elevation', 'elevation2')
GEO = dict(image_size=[16, 16], stride=[12, 16], window_size=5)
ON = dict(median=(1, 2), median_weight='correlation', photo=(2, 0.75), speckle=(4, 1.0), fill=16,
          sgm=(2, 2, 2.0, 8.0), sgm_where='filled', refine=(2, 1), refine_where='filled', lsm=(2, 3), lsm_where='all',
          lsm_model='affine', smooth=(2, 0.5, 2.0), smooth_guide='image')
KEYS = ('median', 'photo', 'speckle', 'fill', 'sgm', 'refine', 'lsm', 'smooth')
NAMES = ['d_map', 'out_map', 'err', 'spread', 'count', 'speckles', 'holes', 'sgm_score', 'sgm_shift', 'refine_score',
         'refine_shift', 'lsm_score', 'lsm_status', 'lsm_affine', 'rejected', 'score']
ATTRS = {'d_map': 'd_map', 'out_map': 'out_map', 'err': 'consistency_map', 'spread': 'spread_map',
         'count': 'coverage_map', 'speckles': 'speckle_map', 'holes': 'hole_map', 'sgm_score': 'sgm_score_map',
         'sgm_shift': 'sgm_shift_map', 'refine_score': 'refine_score_map', 'refine_shift': 'refine_shift_map',
         'lsm_score': 'lsm_score_map', 'lsm_status': 'lsm_status_map', 'lsm_affine': 'lsm_affine_map',
         'rejected': 'photo_reject_map', 'score': 'photo_map'}
BOOL = {'speckle_map', 'hole_map', 'photo_reject_map'}


@pytest.fixture(scope='module')
def pair():
    return stereo_pair(40, 40, seed=1, dx=2)


def recorders(calls):
    """The eight hooks as recorders of (stage, number of arguments) that return correctly shaped arrays."""
    def plane(name, aux):
        def hook(*args):
            calls.append((name, len(args)))
            row, col = np.asarray(args[2]), np.asarray(args[3])
            more = aux[:len(args) - 8]      # lsmer: the affine planes only under the affine model's ten arguments
            return (row, col, np.zeros(row.shape)) + tuple(np.zeros(lead + row.shape, dt) for lead, dt in more)
        return hook

    def photo(img1, img2, d_row, d_col, radius, e, min_score, maps):
        calls.append(('photo', 8))
        score = np.ones(np.shape(d_row))
        return score if min_score is None else (score, maps, np.zeros(np.shape(d_row), np.uint8))

    def masked(name):
        def hook(d, *args):
            calls.append((name, 1 + len(args)))
            return d, np.zeros(np.shape(d), np.uint8)
        return hook

    def same(name):
        def hook(d, *args):
            calls.append((name, 1 + len(args)))
            return d
        return hook

    return dict(medianer=same('median'), photoer=photo, speckler=masked('speckle'), filler=masked('fill'),
                sgmer=plane('sgm', [((2,), np.int8)]), refiner=plane('refine', [((2,), np.int8)]),
                lsmer=plane('lsm', [((), np.int8), ((4,), np.float64)]), smoother=same('smooth'))


# the calls of one run with every stage on, lsm_model='affine': (stage, arguments) as chain.py documents the hooks
CALLS = [('median', 4), ('photo', 8), ('speckle', 3), ('fill', 2), ('sgm', 11), ('refine', 9), ('lsm', 10),
         ('smooth', 5), ('photo', 8)]


def test_layout_pinned():
    """(a) names() and layout() of every stage on, literally, for consistency and merge set or not."""
    c = chain_mod.Chain(PMODES, **ON)
    f64, u8, i8 = torch.float64, torch.uint8, torch.int8
    want = {'d_map': ((2, 5, 7), f64), 'out_map': ((5, 7), f64), 'err': ((5, 7), f64), 'spread': ((2, 5, 7), f64),
            'count': ((5, 7), u8), 'speckles': ((2, 5, 7), u8), 'holes': ((2, 5, 7), u8), 'sgm_score': ((5, 7), f64),
            'sgm_shift': ((2, 5, 7), i8), 'refine_score': ((5, 7), f64), 'refine_shift': ((2, 5, 7), i8),
            'lsm_score': ((5, 7), f64), 'lsm_status': ((5, 7), i8), 'lsm_affine': ((4, 5, 7), f64),
            'rejected': ((5, 7), u8), 'score': ((5, 7), f64)}
    assert list(want) == NAMES
    for consistency in (None, 1.0):
        for merge in (None, 'feather'):
            absent = (['err'] if consistency is None else []) + (['spread', 'count'] if merge is None else [])
            names = [n for n in NAMES if n not in absent]
            assert c.names(consistency, merge) == names
            assert c.layout(5, 7, consistency, merge) == [(n,) + want[n] for n in names]
    off = chain_mod.Chain(PMODES)
    assert off.names(None, None) == ['d_map', 'out_map']
    assert off.layout(5, 7, None, None) == [('d_map', (2, 5, 7), f64), ('out_map', (5, 7), f64)]


def _run(c, hooks, H=9, W=11, e=2):
    a, b = stereo_pair(H + 2 * e, W + 2 * e, seed=4, dx=2)
    return c.run((np.zeros((2, H, W)), np.ones((H, W))), a, b, e, None, None, **hooks)


def test_run_order_pinned():
    """(b) one Chain.run calls the hooks in the order of the stages, each with its documented arguments; a stage
    whose keyword is off is not called."""
    calls = []
    hooks = recorders(calls)
    c = chain_mod.Chain(PMODES, **ON)
    got = _run(c, hooks)
    assert calls == CALLS
    assert len(got) == len(c.names(None, None)) == 13
    for key in KEYS:
        kw = dict(ON, **{key: None})
        if key == 'fill':
            kw.update(sgm_where='all', refine_where='all')
        del calls[:]
        got = _run(chain_mod.Chain(PMODES, **kw), hooks)
        assert calls == [x for x in CALLS if x[0] != key], key
        assert len(got) == len(chain_mod.Chain(PMODES, **kw).names(None, None))
    del calls[:]
    _run(chain_mod.Chain(PMODES, **dict(ON, photo=2, lsm_model='shift')), hooks)      # no reject pass, nine arguments
    assert calls == [('lsm', 9) if x[0] == 'lsm' else x for x in CALLS[:1] + CALLS[2:]]
    del calls[:]
    assert len(_run(chain_mod.Chain(PMODES), hooks)) == 2 and calls == []
    with pytest.raises(TypeError, match='prober'):
        _run(c, dict(hooks, prober=None))


def test_attribute_map(pair):
    """(c) every layout name has exactly one ImageCutSolver attribute and back; a fresh solver has them all None."""
    outs = chain_mod.outputs()
    assert [o.name for o in outs] == NAMES
    assert {o.name: o.attr for o in outs} == ATTRS and len({o.attr for o in outs}) == len(outs) == 16
    assert {o.attr for o in outs if o.mask} == BOOL
    s = ImageCutSolver(*pair, degree_map_mode=list(PMODES), **GEO, **ON)
    assert all(getattr(s, attr, 0) is None for attr in ATTRS.values())
    parsed = chain_mod.Chain(PMODES, **ON)
    assert list(chain_mod.keywords()) == ['median', 'median_weight', 'photo', 'speckle', 'fill', 'sgm', 'sgm_where',
                                          'refine', 'refine_where', 'lsm', 'lsm_where', 'lsm_model', 'smooth',
                                          'smooth_guide']
    for name in chain_mod.keywords():
        assert getattr(s, name) == getattr(s.chain, name) == getattr(parsed, name), name
    assert s.photo == (2, 0.75) and s.sgm == (2, 2, 2048, 8192, 8) and s.lsm_model == ('affine', 0.5) and s.fill == 16
    assert chain_mod.hooks() == ['medianer', 'photoer', 'speckler', 'filler', 'sgmer', 'refiner', 'lsmer', 'smoother']


SHARDED = shard.solve_image_sharded      # the function itself, whatever a test patches the name with


def _sharded(a, b, **kw):
    return SHARDED(a, b, GEO['image_size'], GEO['stride'], 5, 5, PMODES, solver=_oracle_tiles,
                                     stitcher=_host_stitch, **kw)


def _host_path(monkeypatch, hooks):
    """ImageCutSolver's sharded path on the host: sharding on, and solve_image_sharded given the oracle as tile
    solver, the host stitcher and the hooks beside what the solver hands it.  -> the list of what it was handed."""
    handed = []

    def forward(*args, **kwargs):
        handed.append(kwargs)
        got = SHARDED(*args, solver=_oracle_tiles, stitcher=_host_stitch, **hooks, **kwargs)
        return tuple(torch.as_tensor(np.asarray(t)) for t in got)      # as the device path returns them

    monkeypatch.setattr(shard, 'tile_sharding_enabled', lambda: True)
    monkeypatch.setattr(shard, 'solve_image_sharded', forward)
    return handed


@pytest.mark.parametrize('kw', [dict(photo=2), dict(ON, photo=2)], ids=['photo', 'all'])
def test_hand_off(pair, kw, monkeypatch):
    """(d) the sharded path receives the solver's own Chain and no chain keyword, and solves with it.  Before the
    chain was handed over, the parsed keywords were parsed again, and photo=2 raised ValueError('photo min_score must
    be a real in [-1, 1] (got None)') here."""
    calls = []
    hooks = recorders(calls)
    s = ImageCutSolver(*pair, degree_map_mode=list(PMODES), **GEO, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(shard, 'tile_sharding_enabled', lambda: True)
        mp.setattr(shard, 'solve_image_sharded', lambda *args, **kwargs: calls.append(kwargs))
        s._execute_matching_device()
    assert calls[0]['chain'] is s.chain
    assert not set(calls[0]) & (set(chain_mod.keywords()) | set(chain_mod.hooks()))
    del calls[:]
    names = s.chain.names(None, None)
    got = _sharded(*pair, chain=s.chain, **hooks)
    assert isinstance(got, tuple) and len(got) == len(names) == (3 if kw == dict(photo=2) else 12)
    assert calls == ([('photo', 8)] if kw == dict(photo=2) else CALLS[:1] + CALLS[2:])
    handed = _host_path(monkeypatch, hooks)
    s._cut_and_pool()
    s._execute_matching()
    assert handed[0]['chain'] is s.chain and np.array_equal(s.photo_map, np.ones((16, 16)))
    assert all((getattr(s, ATTRS[n]) is not None) == (n in names) for n in NAMES)
    with pytest.raises(ValueError, match='chain='):
        _sharded(*pair, chain=s.chain, photo=2)
    with pytest.raises(ValueError, match='chain='):
        _sharded(*pair, chain=s.chain, lsm_model='shift')
    with pytest.raises(ValueError, match='modes'):
        SHARDED(*pair, GEO['image_size'], GEO['stride'], 5, 5, ('elevation2', 'elevation'), solver=_oracle_tiles,
                stitcher=_host_stitch, chain=s.chain)


def test_a_stage_is_one_declaration(pair, monkeypatch):
    """(e) a made-up stage added to the table, and to nothing else, is taken by all three entry points."""
    def run(st, c, v, r):
        v['probe_mask'] = r.prober(v['d_map'], c.probe)

    probe = chain_mod.Stage('probe', (('probe', None, lambda v: None if v is None else int(v)),), 'prober', (run,),
                            (chain_mod.Out('probe_mask', (), torch.uint8, 'probe_map', True),))
    a, b = pair
    kw = dict(degree_map_mode=list(PMODES), **GEO)
    def unknown(bad):      # not in the table: TypeError naming it, from each entry point
        with pytest.raises(TypeError, match="'%s'" % bad):
            chain_mod.Chain(PMODES, **{bad: 1})
        with pytest.raises(TypeError, match="'%s'" % bad):
            ImageCutSolver(a, b, **{bad: 1}, **kw)
        with pytest.raises(TypeError, match="'%s'" % bad):
            _sharded(a, b, **{bad: 1})

    unknown('probe')
    monkeypatch.setattr(chain_mod, 'RUN', chain_mod.RUN + (probe,))
    monkeypatch.setattr(chain_mod, 'LAYOUT', chain_mod.LAYOUT + (probe,))
    unknown('probe2')
    with pytest.raises(TypeError, match="'prober2'"):
        _sharded(a, b, probe=1, prober2=None)
    c = chain_mod.Chain(PMODES, probe=1, photo=2)
    assert c.probe == 1 and c.names(None, None) == ['d_map', 'out_map', 'score', 'probe_mask']
    assert c.layout(5, 7, None, None)[-1] == ('probe_mask', (5, 7), torch.uint8)
    assert chain_mod.Chain(PMODES).probe is None
    s = ImageCutSolver(a, b, probe=1, **kw)
    assert s.probe == 1 and s.probe_map is None
    seen = []

    def hook(d, value):
        seen.append(value)
        return np.full(np.shape(d)[-2:], 3, np.uint8)

    calls = []
    got = _sharded(a, b, probe=1, prober=hook, fill=4, filler=recorders(calls)['filler'])
    assert seen == [1] and calls == [('fill', 2)] and len(got) == 4      # d_map, out_map, holes, probe_mask
    assert np.array_equal(got[3], np.full((16, 16), 3, np.uint8))
    _host_path(monkeypatch, dict(prober=hook))
    s._cut_and_pool()
    s._execute_matching()
    assert seen == [1, 1] and s.probe_map.dtype == bool and s.probe_map.shape == (16, 16) and s.probe_map.all()


PARSERS = ('fill_iterations', 'speckle_params', 'smooth_params', 'median_params', 'photo_params', 'refine_params',
           'lsm_params', 'lsm_model_params', 'sgm_params')


def test_parsing_happens_once(pair, monkeypatch):
    """(f) building an ImageCutSolver and running its sharded path hands every keyword's value to its parser once."""
    seen = []
    for name in PARSERS:
        def counted(value, name=name, parse=getattr(engine, name)):
            seen.append(name)
            return parse(value)
        monkeypatch.setattr(engine, name, counted)
    kw = dict(ON, photo=2)
    s = ImageCutSolver(*pair, degree_map_mode=list(PMODES), **GEO, **kw)
    _host_path(monkeypatch, recorders([]))
    s._cut_and_pool()
    s._execute_matching()
    assert s.lsm_affine_map.shape == (4, 16, 16) and s.photo_map is not None
    assert sorted(seen) == sorted(PARSERS)
