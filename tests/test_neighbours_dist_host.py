"""The distributed neighbour table without a GPU: the numpy model of its split over the ranks
(neighbours_dist_helpers.model) against the table's definition, the conditions under which the cases reach the paths
they are meant for, and everything the entry points refuse before they touch the device."""
import numpy as np
import pytest

import neighbour_cases as NC
import neighbours_dist_helpers as D
from pyshepseg_amd import distributed, neighbours


class FixedComm(object):
    """a communicator whose allgather_obj answers with what the other ranks are said to have sent"""
    onDevice = True

    def __init__(self, rank, others):
        (self.rank, self.others, self.world) = (rank, others, len(others))

    def allgather_obj(self, obj):
        out = list(self.others)
        out[self.rank] = obj
        return out


@pytest.mark.parametrize('name', D.CASE_NAMES)
def test_model_shares_assemble_to_the_reference(name):
    (_name, seg, S, cuts, four) = D.caseByName(name)
    m = D.model(seg, cuts, S, four)
    want = NC.reference_neighbours(seg, four, S)
    got = D.assembled(m['ranks'], S)
    for (w, g) in zip(want, got):
        assert w.dtype == g.dtype and w.tobytes() == g.tobytes()
    for r in m['ranks']:
        assert r['records_home'] + r['records_sent'] == r['records_local']


@pytest.mark.parametrize('name', D.CASE_NAMES)
def test_reach_conditions(name):
    (_name, seg, S, cuts, four) = D.caseByName(name)
    D.assertReach(name, D.model(seg, cuts, S, four), S)


def test_overlapping_output_rows_are_refused_before_the_device():
    for rank in range(2):
        comm = FixedComm(rank, [(0, 120, None, 50, 190, True), (100, 203, None, 50, 190, True)])
        with pytest.raises(neighbours.PyShepSegNeighboursError, match='SHEPSEG_SHARD=rows'):
            distributed.deviceNeighbours(None, comm, 0, 203, 190, comm.others[rank][:2], 50)


def test_rows_nobody_holds_are_refused_before_the_device():
    comm = FixedComm(0, [(0, 100, None, 50, 190, True), (110, 203, None, 50, 190, True)])
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='rows 100..110'):
        distributed.deviceNeighbours(None, comm, 0, 203, 190, (0, 100), 50)


def test_a_bad_max_seg_id_on_one_rank_is_raised_on_the_others():
    comm = FixedComm(0, [None, (100, 203, 'maxSegId must be an integer (got None)', None, 190, True)])
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='maxSegId'):
        distributed.deviceNeighbours(None, comm, 0, 203, 190, (0, 100), 50)


def _share():
    r = D.model(NC.EXAMPLE, [0, 2, 3], 3, True)['ranks'][1]
    cols = {'numNeighbours': np.zeros(4, dtype=np.int64), 'borderLength': np.zeros(4, dtype=np.int64)}
    return neighbours.SegmentNeighboursShare(r['idRange'], 3, True, r['offsets'], r['neighbours'], r['borderLengths'], cols)


def test_neighbours_of_an_id_outside_the_share():
    sh = _share()
    assert sh.idRange == (2, 4)
    assert sh.neighboursOf(2)[0].tolist() == [1, 3] and sh.neighboursOf(3)[1].tolist() == [2, 2]
    for bad in (0, 1, 4, -1):
        with pytest.raises(neighbours.PyShepSegNeighboursError, match='share'):
            sh.neighboursOf(bad)


def test_reduce_arguments_are_refused_before_any_collective():
    sh = _share()
    col = np.arange(4, dtype=np.float64)
    comm = FixedComm(0, [None, None])
    comm.allgather_obj = None                   # (any collective would fail the test)
    for (sel, kw) in (([(col[:3], [('x', 'mean')])], {}), ([(col, [('x', 'median')])], {}), ([], {}),
                      ([(col, [('x', 'mean')])], dict(ignoreValue='no'))):
        with pytest.raises(neighbours.PyShepSegNeighboursError):
            distributed.reduceOverNeighboursDistributed(None, comm, sh, sel, **kw)
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='SegmentNeighboursShare'):
        distributed.reduceOverNeighboursDistributed(None, comm, object(), [(col, [('x', 'mean')])])


def test_unequal_column_lengths_between_the_ranks_are_refused_before_the_device():
    sh = _share()
    col = np.arange(4, dtype=np.float64)
    other = (4, [(5, 0, [4])], None, -9999.0)      # the other rank's table has maxSegId 4 and a column of 5 values
    comm = FixedComm(0, [None, other])
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='different columns'):
        distributed.reduceOverNeighboursDistributed(None, comm, sh, [(col, [('x', 'mean')])])


def test_gather_refuses_shares_that_do_not_partition_the_ids():
    sh = _share()
    comm = FixedComm(1, [None, None])
    comm.allgather_obj = lambda mine: [mine, mine]
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='partition'):
        distributed.gatherSegmentNeighbours(comm, sh)
