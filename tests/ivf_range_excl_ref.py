"""float64 numpy reference of radad_ivf_range_search_excl / _excl_pq (no GPU): the exact range search restricted to the ADMISSIBLE rows
of the probed lists.

Built on tests/ivf_range_ref.py: probed_keys() gives every query its (ids, keys) over the probed lists; filter_batch() / filter_pq()
drop the ids whose tag the batch-wide set, or the query's own live tags (ivf_excl_pq_ref.live_tags: the first clamp(count, 0, m)
entries of its row, any order, repeats allowed), exclude; ivf_range_ref.members() then cuts at the radius as it does for the plain
search.  So the margin members() reports is taken over the ADMISSIBLE probed rows: an excluded row next to the boundary decides
nothing.
"""
import numpy as np

import ivf_range_ref as RR
from ivf_excl_pq_ref import live_tags


def filter_batch(pk, tags, excl):
    """pk without the ids whose tag is in `excl` (one set for the batch; None / empty: pk as it is)"""
    tags = np.asarray(tags, np.int64)
    if excl is None or len(excl) == 0:
        return list(pk)
    excl = np.asarray(excl, np.int64).reshape(-1)
    out = []
    for ids, keys in pk:
        keep = ~np.isin(tags[ids], excl)
        out.append((ids[keep], keys[keep]))
    return out


def filter_pq(pk, tags, qtags, counts=None):
    """pk without, for query j, the ids whose tag is among query j's live tags (qtags None or zero columns wide: pk as it is)"""
    tags = np.asarray(tags, np.int64)
    if qtags is None:
        return list(pk)
    qtags = np.asarray(qtags, np.int64).reshape(len(pk), -1)
    out = []
    for j, (ids, keys) in enumerate(pk):
        keep = ~np.isin(tags[ids], live_tags(qtags, counts, j))
        out.append((ids[keep], keys[keep]))
    return out


def members_batch(pk, tags, excl, radius, M):
    return RR.members(filter_batch(pk, tags, excl), radius, M)


def members_pq(pk, tags, qtags, counts, radius, M):
    return RR.members(filter_pq(pk, tags, qtags, counts), radius, M)


def brute_batch(db, q, tags, excl, radius, M):
    """the same over every row of the store: what nprobe == nlist must give"""
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64).reshape(-1, db.shape[1])
    all_ids = np.arange(len(db), dtype=np.int64)
    pk = [(all_ids, ((db - q[i][None, :]) ** 2).sum(1)) for i in range(len(q))]
    return members_batch(pk, tags, excl, radius, M)


def brute_pq(db, q, tags, qtags, counts, radius, M):
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64).reshape(-1, db.shape[1])
    all_ids = np.arange(len(db), dtype=np.int64)
    pk = [(all_ids, ((db - q[i][None, :]) ** 2).sum(1)) for i in range(len(q))]
    return members_pq(pk, tags, qtags, counts, radius, M)
