"""The numpy model of the per-query exclusion-aware search (tests/excl_per_query_ref.py) on the CPU: against a plain numpy brute
force; equal sets for every query reduce to expected_excluding; the shard model equals the whole-store model; and the conditions
the GPU tests (tests/test_gpu_knn_excl_per_query.py) rest on, asserted on the designed stores as the model derives them.  The last
test checks that the library declares, binds and wires what the model describes."""
import os

import numpy as np
import pytest

from exclusion_ref import crowded, expected_exact, expected_excluding
import excl_per_query_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(db, tags, qtags, qcnt, q, k, metric):
    """plain numpy: float64 keys of every row, the excluded rows masked, (key, id) order"""
    db64, q64 = db.astype(np.float64), q.astype(np.float64)
    if metric == "COSINE":
        db64 = db64 / np.linalg.norm(db64, axis=1, keepdims=True)
        q64 = q64 / np.linalg.norm(q64, axis=1, keepdims=True)
    qtags, cnt = P.clamp_counts(qtags, qcnt)
    I = np.full((len(q), k), -1, np.int64)
    D = np.full((len(q), k), np.nan)
    for j in range(len(q)):
        key = ((db64 - q64[j]) ** 2).sum(axis=1) if metric == "L2" else -(db64 @ q64[j])
        ok = np.flatnonzero(~np.isin(tags, qtags[j, :cnt[j]]))
        order = ok[np.lexsort((ok, key[ok]))][:k]
        I[j, :len(order)] = order
        D[j, :len(order)] = key[order] if metric == "L2" else -key[order]
    return D, I


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_model_against_brute_force(metric):
    db, q, tags, qtags, qcnt, rows = P.mutual(700, 16, 3, 6101)
    ed, ei = P.expected_pq(db, tags, qtags, qcnt, q, 5, metric)
    bd, bi = _brute(db, tags, qtags, qcnt, q, 5, metric)
    np.testing.assert_array_equal(ei, bi)
    np.testing.assert_allclose(ed, bd, rtol=1e-9, atol=1e-9)
    # counts: above m = m, negative = 0, and only the first cnt tags count
    cnt = np.array([0, 1, 100, -3] * 6, np.int32)
    ed, ei = P.expected_pq(db, tags, qtags, cnt, q, 5, metric)
    bd, bi = _brute(db, tags, qtags, np.clip(cnt, 0, qtags.shape[1]), q, 5, metric)
    np.testing.assert_array_equal(ei, bi)
    # few admissible rows: everything but three rows excluded for query 0 through duplicates and any order
    db2, q2, tags2 = db[:40], q[:2], tags[:40]
    qt = np.stack([np.concatenate([tags2[3:][::-1], tags2[3:5]]), np.concatenate([tags2[:39], tags2[:0]])[:39]])
    _, i2 = P.expected_pq(db2, tags2, qt, None, q2, 5, metric)
    assert sorted(i2[0, :3]) == [0, 1, 2] and np.all(i2[0, 3:] == -1)
    assert i2[1, 0] == 39 and np.all(i2[1, 1:] == -1)


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_equal_sets_reduce_to_the_batch_form(metric):
    db, q, tags, excl, which = crowded(4001, 32, 24, 8, 12, 6201, extra_excl=16)
    assert len(excl) <= 64 * 2
    excl = excl[:64]
    qtags = np.tile(excl[::-1], (len(q), 1))                                     # any order
    ed, ei = expected_excluding(db, tags, excl, q, 5, metric)
    pd, pi = P.expected_pq(db, tags, qtags, None, q, 5, metric)
    np.testing.assert_array_equal(pi, ei)
    np.testing.assert_allclose(pd, ed, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(P.expected_exact_pq(db, tags, qtags, None, q, 5, 15, metric),
                                  expected_exact(db, tags, excl, q, 5, 15, metric))
    # nothing excluded: the plain oracle
    from oracle import radad_oracle as O
    _, oi = O.knn(db, q, 5, metric)
    np.testing.assert_array_equal(P.expected_pq(db, tags, qtags, np.zeros(len(q), np.int32), q, 5, metric)[1], oi)
    np.testing.assert_array_equal(P.expected_pq(db, tags, np.zeros((len(q), 0), np.int64), None, q, 5, metric)[1], oi)


def _shards_equal_whole(store, k, k_fetch, metric, sizes):
    db, q, tags, qtags, qcnt = store[:5]
    K, I, unproved = P.sharded_search_excluding_pq(db, tags, qtags, qcnt, q, k, k_fetch, metric, sizes)
    ed, ei = P.expected_pq(db, tags, qtags, qcnt, q, k, metric)
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    np.testing.assert_allclose(K[f], ed[f], rtol=1e-12, atol=1e-12)
    assert np.all(np.isnan(K[~f]))
    return unproved


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("sizes", [[2500, 2500, 1000], [7, 3000, 2993]])
def test_shard_model_equals_whole_store_model(sizes, metric):
    for store, k_fetch in ((P.mutual(6000, 64, 5, 9402), 10), (P.per_file(6000, 64, 40, 3, 13, 9301), 7)):
        _shards_equal_whole(store, 5, k_fetch, metric, sizes)
        # k_fetch 6 per shard: some queries stay unproved across the shards and the second half runs (the GPU shard test's setting)
        assert _shards_equal_whole(store, 5, 6, metric, sizes).any()
    # one shard: the certificate is the single-handle one
    s = P.nearest(3000, 64, 19, 9501)
    u = _shards_equal_whole(s, 5, 15, "L2", [3000])
    np.testing.assert_array_equal(u.astype(bool), P.expected_exact_pq(s[0], s[2], s[3], s[4], s[1], 5, 15, "L2"))


# ---- the conditions the GPU tests rest on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("n", [20000, 6000])
def test_mutual_store_is_what_the_gpu_tests_need(n, metric):
    """results are planted rows: the float64 gap between adjacent admissible ranks 1 .. k + 1 is >= 1e-6 (an fp32 cosine query
    normalisation moves the difference of two keys by about 3e-8 here: 30x); some queries are listed, their number is no multiple of 8
    (a tail group runs), and the eight identical queries of a group get several different id lists"""
    db, q, tags, qtags, qcnt, rows = P.mutual(n, 64, 5, 9402)
    k, k_fetch = 5, 10
    assert np.all(q.reshape(5, 8, 64) == q.reshape(5, 8, 64)[:, :1])             # eight identical queries per group
    gap = P.adjacent_gap(db, tags, qtags, qcnt, q, k, metric)
    listed = P.expected_exact_pq(db, tags, qtags, qcnt, q, k, k_fetch, metric)
    _, ei = P.expected_pq(db, tags, qtags, qcnt, q, k, metric)
    distinct = [len({tuple(r) for r in ei[8 * g:8 * g + 8]}) for g in range(5)]
    print(f"mutual n={n} {metric}: gap {gap:.2e}, listed {int(listed.sum())} of 40, distinct id lists per group {distinct}")
    assert gap >= 1e-6
    assert listed.sum() > 8 and listed.sum() % 8 != 0
    assert min(distinct) >= 2
    assert np.all(np.isin(ei, rows))                                              # the results are the planted rows
    for j in range(40):
        assert not np.isin(tags[ei[j]], qtags[j]).any()


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("n", [20000, 6000])
def test_per_file_store_is_what_the_gpu_tests_need(n, metric):
    """no tag is carried by more than c = 3 rows and a query lists m = 1: k_fetch = k + m c = 8 proves every query; at k_fetch 7 the
    three own-file rows leave 4 < 5 admissible hits for exactly the owning queries"""
    db, q, tags, qtags, qcnt, which = P.per_file(n, 64, 40, 3, 13, 9301)
    assert np.bincount((tags - 11) // 7).max() == 3 and len(set(which)) == 13
    assert not P.expected_exact_pq(db, tags, qtags, qcnt, q, 5, 8, metric).any()
    listed = P.expected_exact_pq(db, tags, qtags, qcnt, q, 5, 7, metric)
    np.testing.assert_array_equal(np.flatnonzero(listed), np.sort(which))
    _, ei = P.expected_pq(db, tags, qtags, qcnt, q, 5, metric)
    for j in which:
        assert not np.isin(tags[ei[j]], qtags[j]).any()


def test_nearest_store_is_what_the_gpu_tests_need():
    """every query excludes its own 20 nearest rows: all 19 are listed whenever k_fetch - 20 < k"""
    db, q, tags, qtags, qcnt, oi = P.nearest(3000, 64, 19, 9501)
    for k, k_fetch in ((5, 15), (130, 140), (1024, 1024)):
        assert P.expected_exact_pq(db, tags, qtags, qcnt, q, k, k_fetch, "L2").all()
    _, ei = P.expected_pq(db, tags, qtags, qcnt, q, 5, "L2")
    for j in range(19):
        assert not np.isin(ei[j], oi[j]).any()


def test_library_declares_and_binds_the_per_query_forms():
    hdr = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert "#define RADAD_EXCL_PQ_MAX_TAGS 64" in hdr
    assert "int radad_knn_search_excl_pq(" in hdr and "int radad_knn_search_excl_pq_begin(" in hdr
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.config import Config
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex, HipIVFFlatIndex, VectorDatabase
    assert _lib.EXCL_PQ_MAX_TAGS == 64
    for cls, names in ((HipFlatIndex, ("search_excluding_per_query", "search_excluding_per_query_begin", "sharded_excluding_per_query")),
                       (VectorDatabase, ("search_excluding_per_query",))):
        for name in names:
            assert callable(getattr(cls, name))
    assert Config().exclusion_scope == "batch"
    with pytest.raises(ValueError, match="IVF"):
        HipIVFFlatIndex.search_excluding_per_query(None)
    import torch
    calls = []

    def local(q, k, qt, qc, kf):
        calls.append((tuple(q.shape), k, qt.tolist(), qc, kf))
        return torch.zeros((len(q), k), dtype=torch.float64), torch.zeros((len(q), k), dtype=torch.int64)
    s = ShardedSearch(None, 0, local_search_excluding_per_query=local)           # world == 1: the one-piece call
    d, i = s.search_excluding(torch.zeros((2, 8)), 4, query_tags_local=torch.tensor([[3], [9]]), k_fetch=14)
    assert d.dtype == torch.float32 and calls == [((2, 8), 4, [[3], [9]], None, 14)]
    with pytest.raises(ValueError, match="not both"):
        s.search_excluding(torch.zeros((2, 8)), 4, torch.tensor([1]), query_tags_local=torch.tensor([[3], [9]]))
    with pytest.raises(ValueError):
        ShardedSearch(None, 0).search_excluding(torch.zeros((2, 8)), 4, query_tags_local=torch.tensor([[3], [9]]))
