"""CPU: the shapes of tests/clump_shape_cases.py.  The C oracle's clump against the host model of the reference's
loop and against the unmodified reference (tests/golden/clump_shapes.npz), and the census of each walk: the
conditions below are what makes the shapes reach every step of the device walker (the run blocks of the nine
runnable masks beyond one register tile, the bulk dead-end test's second iteration, spill and refill of the stack
window, the cap inside a run, one-pixel pieces of a cut component, bitmaps of one to three words per row, the
global-bitmap walker under SHEPSEG_DFS_POOL=1, the counter hand-out under SHEPSEG_DFS_PER_WG=1), so the shapes
cannot be thinned without a failure here."""
import hashlib
import os
import re

import numpy as np
import pytest

import clump_shape_cases as cs
from conftest import ROOT

_cache = {}


def walker_constant(name):
    """a #define of the walker's launch (pyshepseg_amd/csrc/clump.h)"""
    with open(os.path.join(ROOT, 'pyshepseg_amd', 'csrc', 'clump.h')) as f:
        return int(re.search(r'^#define %s (\d+)u' % name, f.read(), flags=re.M).group(1))


def model(name, four):
    """(labels, next id, census) of the host model, computed once per (shape, connectivity)"""
    if (name, four) not in _cache:
        _cache[(name, four)] = cs.replay_census(cs.make(name), four)
    return _cache[(name, four)]


def census4(name):
    return model(name, True)[2]


@pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])
@pytest.mark.parametrize('name', cs.MODEL_SHAPES)
def test_oracle_equals_host_model(name, four, oracle):
    lab, nxt, _cen = model(name, four)
    seg, onxt = oracle.clump(cs.make(name), 0, four, 1)
    assert onxt == nxt
    assert np.array_equal(seg, lab)


@pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])
@pytest.mark.parametrize('name', cs.SHAPES)
def test_oracle_equals_reference(name, four, oracle, golden):
    g = golden('clump_shapes')
    key = '%s/%d/' % (name, 4 if four else 8)
    seg, nxt = oracle.clump(cs.make(name), 0, four, 1)
    assert seg.dtype == np.uint32 and nxt == int(g[key + 'next'])
    if key + 'labels' in g:
        assert np.array_equal(seg, g[key + 'labels'])
    assert hashlib.sha256(np.ascontiguousarray(seg).tobytes()).digest() == g[key + 'sha256'].tobytes()


def test_golden_holds_every_shape_and_the_whole_arrays(golden):
    g = golden('clump_shapes')
    for name in cs.SHAPES:
        for c in (4, 8):
            assert '%s/%d/next' % (name, c) in g and g['%s/%d/sha256' % (name, c)].shape == (32,)
    for key in ('percolation/4', 'lattice3/4', 'rect_widths/4', 'percolation8/8'):
        lab = g[key + '/labels']
        assert lab.dtype == np.uint32 and lab.shape == cs.make(key.split('/')[0]).shape
        assert hashlib.sha256(lab.tobytes()).digest() == g[key + '/sha256'].tobytes()


def test_shapes_and_padding():
    want = {'percolation': (300, 330), 'percolation8': (300, 330), 'serp_h1': (260, 200), 'serp_v1': (200, 260),
            'strips_v2': (220, 210), 'strips_h2': (210, 220), 'strips_h2_low': (222, 230),
            'strips_h3_mid': (221, 230), 'strips_v2_up': (230, 222), 'lattice3': (230, 230),
            'comb_up': (200, 260), 'comb_down': (200, 260), 'rings': (241, 241), 'rect_widths': (345, 284),
            'many_big': (1717, 1700)}
    assert set(want) == set(cs.SHAPES)
    for name, shape in want.items():
        cl = cs.make(name)
        assert cl.shape == shape and cl.dtype == np.int32 and cl.flags.c_contiguous and cl.min() >= 0
        if name != 'many_big':
            assert cs.padded(cl).size <= 120000         # a GPU case stays a fraction of a second
    cl = cs.make('rect_widths')
    p = cs.padded(cl)
    assert p.shape == (347, 284 + 35) and p.dtype == np.int32
    assert np.array_equal(p[1:-1, 33:-2], cl)
    assert not p[0].any() and not p[-1].any() and not p[:, :33].any() and not p[:, -2:].any()
    assert np.array_equal(cs.make('serp_v1'), cs.make('serp_h1').T)
    assert np.array_equal(cs.make('strips_h2'), cs.make('strips_v2').T)


def test_percolation8_is_cut_only_8_connected():
    cl = cs.make('percolation8')
    assert cs.components(cl, False)[1][1:].max() >= cs.BIG
    assert cs.components(cl, True)[1][1:].max() < cs.BIG
    assert model('percolation8', False)[2]['capped'] >= 1 and census4('percolation8')['capped'] == 0


def test_every_mask_is_popped_and_15_never():
    pops = np.sum([census4(n)['pops'] for n in cs.MODEL_SHAPES], axis=0)
    assert pops.shape == (16,)
    for m in range(1, 15):
        assert pops[m] >= 100, (m, int(pops[m]))
    # a popped pixel has a visited pusher, and a seed has no unvisited member above or to its left
    assert pops[15] == 0
    pops8 = np.sum([model(n, False)[2]['pops'] for n in cs.MODEL_SHAPES], axis=0)
    assert pops8.shape == (9,) and pops8[8] == 0 and (pops8[:6] >= 100).all()


def test_streaks_longer_than_a_register_tile_for_every_runnable_mask():
    over = np.sum([census4(n)['over62'] for n in cs.MODEL_SHAPES], axis=0)
    for m in cs.RUNNABLE:
        assert over[m] >= 20, (m, int(over[m]))
    # and the shape that carries each of them keeps doing so
    for m, name in ((1, 'serp_h1'), (2, 'serp_v1'), (3, 'rect_widths'), (4, 'serp_h1'), (6, 'strips_h2_low'),
                    (8, 'serp_v1'), (9, 'strips_v2'), (12, 'strips_h2'), (14, 'strips_h3_mid')):
        assert census4(name)['over62'][m] >= 20, (m, name)


def test_dead_runs_iterate_the_bulk_test():
    assert census4('strips_h2')['dead_over64'] >= 50
    assert census4('strips_h3_mid')['longest'][0] >= 400


def test_stack_depths_spill_and_refill():
    assert census4('percolation')['depth'] >= 1500
    assert census4('lattice3')['depth'] >= 1500
    assert census4('rect_widths')['depth'] >= 4000
    assert 512 < census4('strips_v2_up')['depth'] < 2 * 512        # just above one window


def test_cap_inside_a_streak_and_capped_pieces():
    assert census4('rect_widths')['capped_in_streak'] >= 5
    for name in cs.MODEL_SHAPES:
        if name.startswith(('strips_', 'serp_')):
            assert census4(name)['capped_in_streak'] >= 1, name
        four = name != 'percolation8'
        assert model(name, four)[2]['capped'] >= 1, name


def test_one_pixel_pieces_inside_a_cut_component():
    assert cs.singles_in_cut(cs.make('lattice3'), True, census4('lattice3')) >= 1


def test_many_big_holds_289_cut_components(oracle):
    cl = cs.make('many_big')
    assert np.array_equal(cl[::101, ::100], (np.arange(289).reshape(17, 17)) % 7 + 1)     # no two blocks touch alike
    seg, nxt = oracle.clump(cl, 0, True, 1)
    sizes = np.bincount(seg.ravel())[1:]
    assert nxt == 2 * 289 + 1 and (sizes == 10001).sum() == 289 and (sizes == 99).sum() == 289
    # with one walker per workgroup (SHEPSEG_DFS_PER_WG=1) the launch is short of walkers: the counter hands out the rest
    assert 289 > walker_constant('DFS_MAX_BLOCKS')


@pytest.mark.parametrize('name', cs.MODEL_SHAPES)
def test_bitmap_geometry(name):
    four = name != 'percolation8'
    words = cs.bitmap_words(cs.make(name), four)
    gran = walker_constant('DFS_GRAN_WORDS')
    assert gran == 512 and walker_constant('DFS_POOL_GRANS_DEFAULT') == 34
    assert words and max(words) > gran                 # a pool of one granule: the global-bitmap walker
    assert max(words) <= 34 * gran                     # the default pool: the LDS walker
    if name == 'rect_widths':                          # one, two and three words per row, either side of a boundary
        boxes = cs.cut_components(cs.make(name), True)
        assert [c1 - c0 + 3 for (_r0, _r1, c0, c1, _n) in boxes] == [32, 33, 64, 65, 96]
        assert len(words) == 5
