"""Helpers of tests/test_merge_dist_host.py and tests/test_gpu_merge_dist.py (no tests here): a numpy model of how the
distributed merge (distributed.deviceMerge) splits its work over the ranks.

The model follows the definition, not the kernels.  The table is sharded by id: rank r holds the rows of
distributed.idRange(r, world, S) and OWNS their entries a < b, so every such entry of the whole table has one owner.
A rank's links are the links among the entries it owns; its forest is their connected components over all ids; it
sends one pair (i, smallest id of i's local component) for every id that is not that smallest id.  The groups are the
components of all ranks' links (merge_cases.components through similar_cases.groups_from_links).  The entries a < b a
rank owns whose ends lie in different groups are its records; its distinct (lo, hi) pairs among them stay home when
both new ids lie in the rank's share idRange(r, world, M) of the NEW ids and travel otherwise; a rank picks, from all
travelling records, those with an end in its new share; its new share table is those rows of the contracted table."""
import numpy as np

import merge_cases as mc
import similar_cases as sc


def key_links(table, keys, ignoreKey=None, minBorder=1, segSize=None):
    """the key rule's link per entry of the table (merge_cases.reference_merge's rule)"""
    (a, b, w) = sc.entries(table)
    S = len(table[0]) - 2
    keys = np.asarray(keys).astype(np.int64)
    vertex = np.ones(S + 1, dtype=bool)
    vertex[0] = False
    if segSize is not None:
        vertex &= np.asarray(segSize) > 0
    link = (keys[a] == keys[b]) & (w >= minBorder) & vertex[a] & vertex[b]
    if ignoreKey is not None:
        link &= keys[a] != ignoreKey
    return link


def share_rows(table, lo, hi):
    """(offsets from 0, neighbours, borderLengths) of the rows lo .. hi - 1 of a table"""
    (offsets, nbrs, lens) = table
    (x, y) = (int(offsets[lo]), int(offsets[hi]))
    return (offsets[lo:hi + 1] - x, nbrs[x:y], lens[x:y])


def model(table, link, world, segSize=None, mutual=False):
    """What every rank of the distributed merge should hold and report, from the whole table and the link per entry.
    Returns a dict: 'groups' (similar_cases.groups_from_links of the whole table), 'ranks' = per rank a dict with
    links, forest_pairs, pairs (the (id, root) pairs, sorted by id), local (the rank's component labels),
    records_entries, records_local, records_home, records_sent, records_picked, entries, idRange (of the new ids),
    offsets, neighbours, borderLengths; 'exchange_bytes'."""
    from pyshepseg_amd import distributed
    (a, b, w) = sc.entries(table)
    S = len(table[0]) - 2
    g = sc.groups_from_links(table, link, segSize)
    M = g.maxSegId
    (ra, rb) = (g.recode[a].astype(np.int64), g.recode[b].astype(np.int64))
    keep = (ra != rb) & (ra != 0) & (rb != 0)
    ranks = []
    for r in range(world):
        (lo, hi) = distributed.idRange(r, world, S)
        own = (a >= lo) & (a < hi) & (a < b) & (a != 0)
        mine = own & link
        local = mc.components(S + 1, a[mine], b[mine])
        moved = np.flatnonzero(local != np.arange(S + 1))
        rec = own & keep
        (plo, phi) = (np.minimum(ra[rec], rb[rec]), np.maximum(ra[rec], rb[rec]))
        (u, inv) = np.unique((plo.astype(np.uint64) << np.uint64(32)) | phi.astype(np.uint64), return_inverse=True)
        tot = np.zeros(len(u), dtype=np.int64)
        np.add.at(tot, inv.reshape(-1), w[rec])
        (ulo, uhi) = ((u >> np.uint64(32)).astype(np.int64), (u & np.uint64(0xFFFFFFFF)).astype(np.int64))
        (nlo, nhi) = distributed.idRange(r, world, M)
        home = (ulo >= nlo) & (ulo < nhi) & (uhi >= nlo) & (uhi < nhi)
        ranks.append(dict(links=int(mine.sum()), forest_pairs=len(moved), pairs=np.stack([moved, local[moved]], axis=1),
                          local=local, records_entries=int(rec.sum()), records_local=len(u), records_home=int(home.sum()),
                          records_sent=int((~home).sum()), idRange=(nlo, nhi), trav=(ulo[~home], uhi[~home], tot[~home])))
    (tlo, thi) = (np.concatenate([m['trav'][0] for m in ranks]), np.concatenate([m['trav'][1] for m in ranks]))
    for m in ranks:
        (nlo, nhi) = m['idRange']
        m['records_picked'] = int((((tlo >= nlo) & (tlo < nhi)) | ((thi >= nlo) & (thi < nhi))).sum())
        (m['offsets'], m['neighbours'], m['borderLengths']) = share_rows(g.table, nlo, nhi)
        m['entries'] = len(m['neighbours'])
    exchange = 8 * sum(m['forest_pairs'] for m in ranks) + 16 * sum(m['records_sent'] for m in ranks)
    return dict(groups=g, ranks=ranks, exchange_bytes=exchange + (8 * (S + 1) if mutual else 0))


INFO_KEYS = ('links', 'forest_pairs', 'records_entries', 'records_local', 'records_home', 'records_sent',
             'records_picked', 'entries')


def info_of(m, rank):
    """what deviceMerge's ``info`` of a rank should be, without 'deviceMs'"""
    out = {k: m['ranks'][rank][k] for k in INFO_KEYS}
    out['exchange_bytes'] = m['exchange_bytes']
    return out


def assembled(ranks, M):
    """(offsets, neighbours, borderLengths) of the whole contracted table from the ranks' new shares, in id order"""
    offsets = np.zeros(M + 2, dtype=np.int64)
    base = 0
    for m in ranks:
        (lo, hi) = m['idRange']
        offsets[lo:hi + 1] = base + m['offsets']
        base += int(m['offsets'][-1])
    return (offsets, np.concatenate([m['neighbours'] for m in ranks]), np.concatenate([m['borderLengths'] for m in ranks]))


def groups_no_rank_holds_whole(m):
    """how many groups of two or more members are the component of no single rank's own forest"""
    g = m['groups']
    count = 0
    members = np.argsort(g.recode, kind='stable')
    bounds = np.searchsorted(g.recode[members], np.arange(1, g.maxSegId + 2))
    for k in range(g.maxSegId):
        ids = members[bounds[k]:bounds[k + 1]]
        if len(ids) >= 2 and not any(len(np.unique(r['local'][ids])) == 1 for r in m['ranks']):
            count += 1
    return count
