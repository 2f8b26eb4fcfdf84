"""GPU: neighbours.mergeSimilarSegments against its definition in numpy (tests/similar_cases.py).  The link model is a
boolean per entry; groups, recode, the contracted table by the graph route and by the raster route, the histogram and
the recoded raster are integers and compared with numpy.array_equal, as tests/test_gpu_merge.py compares them.  Every
case asserts what it is for (links and non-links both occur, a tie occurs, ...) so that none passes empty."""
import functools

import numpy as np
import pytest

import merge_cases as mc
import neighbour_cases as nc
import similar_cases as sc
from test_gpu_merge import assert_groups, assert_table

pytestmark = pytest.mark.gpu
FOURS = [True, False]


@functools.lru_cache(maxsize=None)
def tabled(name, four):
    """(seg, S, the table by neighbour_cases): computed once, shared, left unchanged"""
    seg = {'example': lambda: nc.EXAMPLE, 'mosaic': mc.mosaic, 'star': nc.hot_segment,
           'row_descending': lambda: mc.line_raster(mc.line_descending(), False),
           'column_permuted': lambda: mc.line_raster(mc.line_permuted(), True),
           'drawn': lambda: nc.random_labels((65, 129), 40, 11),
           'drawn_wide': lambda: nc.random_labels((129, 129), 1000, 13)}[name]()
    S = int(seg.max())
    return (seg, S, nc.reference_neighbours(seg, four, S))


def check(name, four, columns, withRaster=True, nb=None, **rule):
    """mergeSimilarSegments of a case against the model: (result, model)"""
    from pyshepseg_amd import neighbours
    (seg, S, table) = tabled(name, four)
    model = sc.reference_similar(table, columns, **rule)
    if nb is None:
        nb = neighbours.findSegmentNeighbours(seg, four, maxSegId=S)
    kwargs = dict(rule)
    if 'keys' in kwargs:
        kwargs['keyColumn'] = kwargs.pop('keys')
    res = neighbours.mergeSimilarSegments(nb, columns, segfile=seg if withRaster else None, **kwargs)
    assert_groups(res, model)
    assert res.neighbours.residentSerial == neighbours.residentTableSerial()
    if withRaster:
        assert_table(res.neighbours, mc.raster_route(seg, four, model), model.maxSegId, 'raster route')
        assert res.segimg.dtype == np.uint32 and np.array_equal(res.segimg, model.recode[seg])
        assert np.array_equal(res.hist, np.bincount(model.recode[seg].ravel(), minlength=model.maxSegId + 1))
    if rule.get('segSize') is not None:
        assert np.array_equal(res.hist, model.hist)
    return (res, model)


def both_occur(model):
    (cand, link) = (model.rule.candidate, model.rule.link)
    assert link.any() and (cand & ~link).any(), 'links and non-links must both occur'


# ---- (a) the examples by hand -------------------------------------------------------------------------------------
COLUMN = np.array([0, 10, 13, 20], dtype=np.float64)
TIE = np.array([0, 10, 13, 16], dtype=np.float64)
PAIR = [np.array([0, 1, 4, 100], dtype=np.float64), np.array([0, 1, 5, 100], dtype=np.float64)]
HAND = [
    ('at_3', [COLUMN], dict(maxDistance=3), [0, 1, 1, 2]),
    ('chain_7', [COLUMN], dict(maxDistance=7), [0, 1, 1, 1]),
    ('below_3', [COLUMN], dict(maxDistance=2.999), [0, 1, 2, 3]),
    ('mutual', [COLUMN], dict(mutualNearest=True), [0, 1, 1, 2]),
    ('mutual_cut', [COLUMN], dict(mutualNearest=True, maxDistance=2), [0, 1, 2, 3]),
    ('mutual_tie', [TIE], dict(mutualNearest=True), [0, 1, 1, 2]),
    ('pair_at_5', PAIR, dict(maxDistance=5), [0, 1, 1, 2]),
    ('pair_below_5', PAIR, dict(maxDistance=np.nextafter(5.0, 0)), [0, 1, 2, 3]),
]


@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('name,columns,rule,recode', HAND, ids=[h[0] for h in HAND])
def test_example_by_hand(name, columns, rule, recode, four):
    (res, model) = check('example', four, columns, **rule)
    assert res.recode.tolist() == recode and res.maxSegId == max(recode)
    if name == 'mutual_tie':
        assert model.rule.best.tolist() == [0, 2, 1, 2]         # the tie of row 2 went to the smaller id


# ---- (b) a real table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('C,dtype', [(1, np.float64), (3, np.float64), (8, np.float64), (3, np.float32), (3, np.int16)],
                         ids=['c1', 'c3', 'c8', 'c3_float32', 'c3_int16'])
def test_mosaic(C, dtype, four):
    (seg, S, table) = tabled('mosaic', four)
    columns = sc.integer_columns(S, C, 100 + C, dtype=dtype)
    assert all(col.dtype == dtype for col in columns)
    (dist, frac) = sc.quarter_to_three_quarters(table, columns)
    assert 0.25 <= frac <= 0.75
    (res, model) = check('mosaic', four, columns, maxDistance=dist)
    both_occur(model)
    assert 1 < res.maxSegId < S


@pytest.mark.parametrize('four', FOURS)
def test_mosaic_real_values_and_mutual(four):
    """real-valued columns (no two distances tie) under both rules"""
    (seg, S, table) = tabled('mosaic', four)
    rng = np.random.default_rng(8)
    columns = [rng.uniform(-1.0, 1.0, size=S + 1) for _ in range(6)]
    (a, b, w) = sc.entries(table)
    dist = float(np.sqrt(np.median(sc.distance2(columns, a, b))))
    (res, model) = check('mosaic', four, columns, maxDistance=dist)
    both_occur(model)
    (res, model) = check('mosaic', four, columns, mutualNearest=True)
    both_occur(model)
    assert set(res.groupSize[1:].tolist()) == {1, 2}


@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('mutual', [False, True], ids=['threshold', 'mutual'])
def test_many_rows_per_piece_and_many_pieces(mutual, four):
    """1000 rows of some 60 entries over some 30 workgroups; integer columns, so many rows tie at their smallest d2"""
    (seg, S, table) = tabled('drawn_wide', four)
    assert 20 * sc.MRG_PIECE < len(table[1]) < 150000
    columns = sc.integer_columns(S, 3, 71, top=6)
    (dist, frac) = sc.quarter_to_three_quarters(table, columns)
    assert 0.25 <= frac <= 0.75
    (res, model) = check('drawn_wide', four, columns, maxDistance=dist, mutualNearest=mutual)
    both_occur(model)
    if mutual:
        assert (sc.ties_per_row(table, model.rule) > 1).sum() > 100


# ---- (c) the 4097-long lines ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('name,order', [('row_descending', mc.line_descending), ('column_permuted', mc.line_permuted)])
def test_line_is_one_chain(name, order, four):
    (seg, S, table) = tabled(name, four)
    assert len(table[1]) > 2 * sc.MRG_PIECE
    column = sc.position_column(order())
    (res, model) = check(name, four, [column], maxDistance=1)
    assert res.maxSegId == 1 and res.groupSize.tolist() == [0, mc.LINE] and res.links == mc.LINE - 1
    # the two ends of the chain are 4096 apart, and one step less breaks every link
    assert check(name, four, [column], maxDistance=np.nextafter(1.0, 0), withRaster=False)[0].maxSegId == mc.LINE


@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('name,order', [('row_descending', mc.line_descending), ('column_permuted', mc.line_permuted)])
def test_line_ties_go_to_the_smaller_id(name, order, four):
    (seg, S, table) = tabled(name, four)
    line = np.asarray(order(), dtype=np.int64)
    (res, model) = check(name, four, [sc.position_column(line)], mutualNearest=True)
    # every inner segment has its two neighbours at distance 1: best is the smaller of the two
    best = model.rule.best
    assert np.array_equal(best[line[1:-1]], np.minimum(line[:-2], line[2:]))
    assert (best[line[0]], best[line[-1]]) == (line[1], line[-2])
    both_occur(model)
    assert res.links == int(((best[best[line]] == line)).sum()) // 2 >= 1


# ---- (d) one row longer than the hook's piece ----------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('tie', [False, True], ids=['best_in_last_piece', 'tie_with_first_piece'])
def test_star_row_over_workgroups(tie, four):
    (seg, S, table) = tabled('star', four)
    (offsets, nbrs, lens) = table
    hub = 1
    (r0, r1) = (int(offsets[hub]), int(offsets[hub + 1]))
    assert r1 - r0 > 4 * sc.MRG_PIECE
    (first, last) = (int(nbrs[r0 + 5]), int(nbrs[r1 - 3]))
    assert (r0 + 5) // sc.MRG_PIECE == 0 and (r1 - 3) // sc.MRG_PIECE == (r1 - 1) // sc.MRG_PIECE >= 4
    column = sc.star_column(S, hub, [first, last] if tie else [last])
    (res, model) = check('star', four, [column], mutualNearest=True)
    assert model.rule.best[hub] == (first if tie else last)
    assert res.links == 1 and res.recode[first if tie else last] == res.recode[hub] == 1
    assert res.recode[last if tie else first] != 1
    # the threshold rule on the same row: both near ids and nothing else
    (res, model) = check('star', four, [sc.star_column(S, hub, [first, last])], maxDistance=5, withRaster=False)
    assert res.links == 2 and res.groupSize[1] == 3


# ---- (e) ignored values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('kind', ['nan', 'value', 'both', 'one_of_three'])
def test_ignored_values(kind, four):
    (seg, S, table) = tabled('drawn', four)
    rng = np.random.default_rng(21)
    columns = sc.integer_columns(S, 3 if kind == 'one_of_three' else 1, 22, top=6)
    holes = rng.choice(np.arange(1, S + 1), size=S // 4, replace=False)
    rule = dict(maxDistance=2)
    hit = columns[-1]
    withNan = holes[::2] if kind != 'value' else holes[:0]
    withValue = holes[1::2] if kind != 'nan' else holes[:0]
    hit[withNan] = np.nan
    if len(withValue):
        hit[withValue] = -7
        rule['ignoreValue'] = -7
    (res, model) = check('drawn', four, columns, **rule)
    both_occur(model)
    bad = sc.ignored_ids(columns, rule.get('ignoreValue'))
    assert np.array_equal(np.flatnonzero(bad), np.sort(np.concatenate([withNan, withValue]))) and bad.any()
    # an id with a hole is alone in its group, and without the holes some of them would have merged
    assert (res.groupSize[res.recode[np.flatnonzero(bad)]] == 1).all()
    filled = [np.where(sc.ignored_ids([col], rule.get('ignoreValue')), 3.0, col) for col in columns]
    assert sc.reference_similar(table, filled, maxDistance=2).maxSegId < model.maxSegId
    (res, model) = check('drawn', four, columns, withRaster=False, mutualNearest=True, ignoreValue=rule.get('ignoreValue'))
    assert (model.rule.best[bad] == 0).all() and (res.groupSize[res.recode[np.flatnonzero(bad)]] == 1).all()


# ---- (f) sizes, minBorder, keys -----------------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
@pytest.mark.parametrize('mutual', [False, True], ids=['threshold', 'mutual'])
def test_sizes_min_border_and_keys(mutual, four):
    from pyshepseg_amd import neighbours
    (seg, S, table) = tabled('drawn', four)
    # ids without pixels: the table gets five rows behind the largest label, and two labels are wiped from the raster
    seg = seg.copy()
    seg[(seg == 7) | (seg == 23)] = 0
    S = S + 5
    table = nc.reference_neighbours(seg, four, S)
    size = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64)
    assert (size[1:] == 0).sum() == 7
    columns = sc.integer_columns(S, 2, 31, top=6)
    keys = np.random.default_rng(32).integers(0, 3, size=S + 1).astype(np.int8)
    minBorder = int(np.median(table[2]))
    assert table[2].min() < minBorder <= table[2].max()
    rule = dict(maxDistance=4, mutualNearest=mutual, keys=keys, ignoreKey=2, minBorder=minBorder, segSize=size)
    model = sc.reference_similar(table, columns, **rule)
    plain = sc.link_model(table, columns, maxDistance=4, mutualNearest=mutual)
    both_occur(model)
    # each of the three conditions removes links the distance alone would make
    for without in ('keys', 'minBorder'):
        fewer = dict(rule)
        fewer.pop(without)
        if without == 'keys':
            fewer.pop('ignoreKey')
        assert sc.link_model(table, columns, **fewer).candidate.sum() > model.rule.candidate.sum()
    assert plain.candidate.sum() > model.rule.candidate.sum()
    nb = neighbours.findSegmentNeighbours(seg, four, maxSegId=S)
    res = neighbours.mergeSimilarSegments(nb, columns, maxDistance=4, mutualNearest=mutual, keyColumn=keys, ignoreKey=2,
                                          minBorder=minBorder, segSize=size, segfile=seg)
    assert_groups(res, model)
    assert (res.recode[size == 0] == 0).all() and np.array_equal(res.hist, model.hist)
    assert np.array_equal(res.segimg, model.recode[seg])
    assert_table(res.neighbours, mc.raster_route(seg, four, model), model.maxSegId, 'raster route')
    assert (keys[res.representative[1:]][res.groupSize[1:] > 1] != 2).all()


# ---- (g) mutual pairs cut by a threshold ---------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
def test_mutual_nearest_with_a_threshold(four):
    (seg, S, table) = tabled('mosaic', four)
    columns = sc.integer_columns(S, 2, 41, top=12)
    free = sc.link_model(table, columns, mutualNearest=True)
    dist = int(np.sqrt(np.median(free.d2[free.link])))
    (res, model) = check('mosaic', four, columns, mutualNearest=True, maxDistance=dist)
    cut = free.link & ~model.rule.link
    assert cut.any() and model.rule.link.any(), 'the threshold must cut some mutual pairs and keep some'
    assert np.array_equal(free.best, model.rule.best)
    ties = sc.ties_per_row(table, free)
    assert (ties > 1).any(), 'integer columns: some row has two candidates at its smallest distance'


# ---- (h) resident and uploaded ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mutual', [False, True], ids=['threshold', 'mutual'])
def test_hand_built_table_equals_resident(mutual):
    from pyshepseg_amd import neighbours
    (seg, S, table) = tabled('mosaic', True)
    columns = sc.integer_columns(S, 3, 51)
    rule = dict(maxDistance=sc.quarter_to_three_quarters(table, columns)[0], mutualNearest=mutual)
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    (resident, model) = check('mosaic', True, columns, withRaster=False, nb=nb, **rule)
    assert resident.timings['uploaded'] is False
    byHand = neighbours.SegmentNeighbours(*[x.copy() for x in table], S, True)
    (uploaded, model) = check('mosaic', True, columns, withRaster=False, nb=byHand, **rule)
    assert uploaded.timings['uploaded'] is True
    for name in ('recode', 'representative', 'groupSize'):
        assert np.array_equal(getattr(resident, name), getattr(uploaded, name))
    both_occur(model)


# ---- two rounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', FOURS)
def test_two_rounds(four):
    """merge, carry exact columns to the groups, merge the groups' table on them: the model run twice, and the two
    recodes composed give the second raster"""
    from pyshepseg_amd import neighbours
    import aggregate_cases as ac
    (seg, S, table) = tabled('mosaic', four)
    size = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64)
    columns = [col.astype(np.int64) for col in sc.integer_columns(S, 2, 61)]
    dist = sc.quarter_to_three_quarters(table, columns, segSize=size)[0]
    nb = neighbours.findSegmentNeighbours(seg, four, maxSegId=S)
    first = neighbours.mergeSimilarSegments(nb, columns, maxDistance=dist, segSize=size, segfile=seg)
    model1 = sc.reference_similar(table, columns, maxDistance=dist, segSize=size)
    assert_groups(first, model1)
    out = neighbours.aggregateToGroups(first, [(columns[0], [('lo', 'min'), ('hi', 'max')]), (columns[1], [('total', 'sum')])],
                                       weights=size)
    ref0 = ac.reference_aggregate(model1.recode, model1.maxSegId, columns[0], weights=size)
    ref1 = ac.reference_aggregate(model1.recode, model1.maxSegId, columns[1], weights=size)
    want = {'lo': ref0['min'], 'hi': ref0['max'], 'total': ref1['sum']}
    for name in want:
        assert out[name].dtype == want[name].dtype and np.array_equal(out[name], want[name]), name
    assert out['total'].dtype == np.int64
    second_columns = [out['lo'], out['hi'], out['total']]
    dist2 = sc.quarter_to_three_quarters(model1.table, second_columns, segSize=model1.hist)[0]
    second = neighbours.mergeSimilarSegments(first.neighbours, second_columns, maxDistance=dist2, segSize=first.hist,
                                             segfile=first.segimg)
    assert second.timings['uploaded'] is False
    model2 = sc.reference_similar(model1.table, [want['lo'], want['hi'], want['total']], maxDistance=dist2,
                                  segSize=model1.hist)
    both_occur(model2)
    assert_groups(second, model2)
    assert 1 < second.maxSegId < first.maxSegId < S
    assert np.array_equal(second.recode[first.recode][seg], second.segimg)
    assert np.array_equal(model2.recode[model1.recode][seg], second.segimg)
