"""The numpy model of the distributed merge (merge_dist_cases): its shares assemble to the definition's contracted
table, its counts add up, and the cases tests/test_gpu_merge_dist.py runs reach what they are meant to reach."""
import numpy as np
import pytest

import merge_cases as mc
import merge_dist_cases as MD
import similar_cases as sc
from pyshepseg_amd import distributed, neighbours

MRG_PIECE = sc.MRG_PIECE
Err = neighbours.PyShepSegNeighboursError


def caseByName(name):
    return [c for c in mc.CASES if c.name == name][0]


def built(name, four=True, keys=None):
    """(seg, S, keys, segSize, table, link per entry, the definition's Model) of a merge_cases case"""
    case = caseByName(name)
    (seg, S, k, size, table) = mc.build(case, four)
    if keys is not None:
        k = keys(S)
    link = MD.key_links(table, k, case.ignoreKey, case.minBorder, size)
    ref = mc.reference_merge(table, k, case.ignoreKey, case.minBorder, size)
    return (seg, S, k, size, table, link, ref)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


NAMES = ['column_permuted', 'through_a_third', 'star_alternating', 'row_descending', 'no_segments', 'one_segment',
         'drawn_large_ignore', 'half_planes_300', 'half_planes_301', 'mosaic']


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_shares_assemble_to_the_definition_and_counts_add_up(name, world):
    (_seg, S, _k, size, table, link, ref) = built(name)
    m = MD.model(table, link, world, size)
    g = m['groups']
    assert g.maxSegId == ref.maxSegId and same(g.recode, ref.recode) and same(g.representative, ref.representative)
    got = MD.assembled(m['ranks'], g.maxSegId)
    for (x, y) in zip(got, ref.table):
        assert same(x, y)
    assert sum(r['links'] for r in m['ranks']) == ref.links
    assert sum(r['records_entries'] for r in m['ranks']) == ref.recordsSorted
    for (rank, r) in enumerate(m['ranks']):
        assert r['idRange'] == distributed.idRange(rank, world, g.maxSegId)
        assert r['records_home'] + r['records_sent'] == r['records_local'] <= r['records_entries']
        assert r['forest_pairs'] <= r['links']
    if world == 1:
        assert m['ranks'][0]['records_sent'] == 0 == m['ranks'][0]['records_picked']
        assert m['ranks'][0]['forest_pairs'] == S - g.maxSegId - int((g.recode[1:] == 0).sum())


def test_the_union_of_the_forests_is_needed_when_all_keys_are_equal():
    (_seg, S, _k, _size, table, link, ref) = built('column_permuted')
    assert S == 4097 and ref.maxSegId == 1
    for (world, pairs) in ((2, [3089, 1007]), (3, [2288, 1367, 441])):
        m = MD.model(table, link, world)
        assert [r['forest_pairs'] for r in m['ranks']] == pairs
        assert MD.groups_no_rank_holds_whole(m) == 1        # (the one group: skipping the union splits it)


def test_groups_that_no_rank_holds_whole_with_two_keys():
    (_seg, S, _k, _size, table, link, ref) = built('column_permuted', keys=lambda S: np.arange(S + 1) % 2)
    sizes = ref.groupSize[1:]
    assert ref.maxSegId == 2013 and int((sizes >= 2).sum()) == 1015 and int(sizes.max()) == 12
    for (world, pairs, split) in ((2, [1569, 515], 199), (3, [1187, 665, 232], 285)):
        m = MD.model(table, link, world)
        assert [r['forest_pairs'] for r in m['ranks']] == pairs
        assert MD.groups_no_rank_holds_whole(m) == split


def test_one_and_two_join_only_through_three_whose_links_two_ranks_hold():
    (_seg, S, _k, _size, table, link, ref) = built('through_a_third')
    m = MD.model(table, link, 3)
    assert S == 3 and ref.maxSegId == 1 and [r['forest_pairs'] for r in m['ranks']] == [0, 1, 1]
    assert [r['pairs'].tolist() for r in m['ranks']] == [[], [[3, 1]], [[3, 2]]]


@pytest.mark.parametrize('world,split', [(2, (5624, 5626)), (3, (3748, 7502))])
def test_the_hub_row_is_one_ranks_and_the_others_still_get_their_rows(world, split):
    (_seg, S, _k, _size, table, link, ref) = built('star_alternating')
    assert S == 22501 and ref.maxSegId == 11251
    m = MD.model(table, link, world)
    hub = m['ranks'][0]
    (lo, hi) = distributed.idRange(0, world, S)
    rows = np.diff(table[0])[lo:hi]
    assert int(rows.max()) == 22500 and -(-22500 // MRG_PIECE) == 11
    assert (hub['links'], hub['records_local']) == (11250, 11250)
    assert (hub['records_home'], hub['records_sent']) == split
    for r in m['ranks'][1:]:
        assert r['links'] == 0 and r['forest_pairs'] == 0 and r['entries'] > 0


def test_argument_errors_come_before_any_collective():
    share = neighbours.SegmentNeighboursShare((0, 4), 3, True, None, None, None, None)
    with pytest.raises(Err, match='keyColumn has 3 rows'):
        distributed.mergeRule(share, np.zeros(3, dtype=np.int64))
    with pytest.raises(Err, match='minBorder must be at least 1'):
        distributed.mergeRule(share, np.zeros(4, dtype=np.int64), minBorder=0)
    with pytest.raises(Err, match='needs mutualNearest=True'):
        distributed.mergeRule(share, distanceColumns=[np.zeros(4)])
    with pytest.raises(Err, match='share must be a SegmentNeighboursShare'):
        distributed.mergeSegmentsDistributed(None, None, object(), np.zeros(4, dtype=np.int64))
    with pytest.raises(Err, match='outfile needs dres'):
        distributed.mergeSegmentsDistributed(None, None, share, np.zeros(4, dtype=np.int64), outfile='x.npy')
