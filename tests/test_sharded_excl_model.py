"""The numpy model of the sharded exclusion-aware search (tests/sharded_excl_ref.py: begin, certificate across shards, finish, merge)
against expected_excluding over the WHOLE store -- the certificate is sound and the exact pass completes it -- on crowded stores at
G = 1, 2, 3, 8 and on the four designed stores, each with its condition asserted on the inputs.  The last test checks that the
library declares, binds and wires what the model describes."""
import numpy as np
import pytest

from exclusion_ref import crowded, expected_exact, expected_excluding
import sharded_excl_ref as M


def _sizes(n, G):
    q, r = divmod(n, G)
    return [q + (1 if g < r else 0) for g in range(G)]


def _check(db, q, tags, excl, k, k_fetch, metric, sizes):
    K, I, unproved = M.sharded_search_excluding(db, tags, excl, q, k, k_fetch, metric, sizes)
    ed, ei = expected_excluding(db, tags, excl, q, k, metric)
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    # (float64 sums over a shard and over the whole store may differ in the last bits: BLAS blocks them differently)
    np.testing.assert_allclose(K[f], ed[f], rtol=1e-12, atol=1e-12)
    assert np.all(np.isnan(K[~f]))
    return unproved


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_crowded_stores(G, metric):
    db, q, tags, excl, which = crowded(4001, 32, 24, 8, 30, 7100 + G)
    unproved = _check(db, q, tags, excl, 5, 15, metric, _sizes(4001, G))
    if G == 1:                                              # one shard: the certificate is the single-handle one
        np.testing.assert_array_equal(unproved.astype(bool), expected_exact(db, tags, excl, q, 5, 15, metric))
    # a query the whole store's k_fetch hits prove is proved by the shards too (each shard's list reaches at least as far)
    assert not np.any(unproved.astype(bool) & ~expected_exact(db, tags, excl, q, 5, 15, metric))


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_a_duplicates_in_one_shard(metric):
    sizes = [1500, 1500]
    db, q, tags, excl, which = M.store_a(sizes, 32, 24, 8, 30, 7201)
    rows = np.flatnonzero(np.isin(tags, excl))
    assert rows.max() < sizes[0] and len(rows) == 8 * 30                     # every excluded duplicate lies in shard 0
    unproved = _check(db, q, tags, excl, 5, 15, metric, sizes)
    assert np.all(unproved[which] == 1)                                       # 30 excluded duplicates fill shard 0's 15 hits


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_b_one_shard_mostly_excluded(metric):
    sizes, k = [1500, 1500], 5
    db, q, tags, excl, planted = M.store_b(sizes, 32, 24, k, 7301)
    gone = np.isin(tags, excl)
    assert 0.89 < gone[:1500].mean() <= 0.9 and not gone[1500:].any()
    assert planted.min() >= 1500 and planted.shape == (24, k)
    _, oi = expected_excluding(db, tags, excl, q, k, metric)
    np.testing.assert_array_equal(np.sort(oi, 1), np.sort(planted, 1))        # the planted rows ARE every query's neighbours
    alone = expected_exact(db[:1500], tags[:1500], excl, q, k, 15, metric)   # the per-shard rule on shard 0 alone
    assert alone.sum() > 0
    unproved = _check(db, q, tags, excl, k, 15, metric, sizes)
    assert unproved.sum() == 0                                                # the global certificate lists nobody


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_c_small_shard_and_shard_without_admissible_rows(metric):
    sizes = [1000, 8, 300]
    db, q, tags, excl, gone = M.store_c(sizes, 32, 24, 7401)
    assert sizes[1] < 15 and gone[1008:].all() and not gone[1000:1008].any() and 0 < gone[:1000].sum() < 1000
    _check(db, q, tags, excl, 5, 15, metric, sizes)
    _check(db, q, tags, excl, 5, 15, metric, [8, 1000, 300])                  # ... and the small shard first
    K, I, FK, FI = M.shard_begin(db[1000:1008], tags[1000:1008], excl, q, 5, 15, metric, 1000)
    np.testing.assert_array_equal(FI, I[:, 4])                                # 8 admissible rows: the frontier is the 5th survivor
    _check(db, q, tags, excl, 10, 15, metric, sizes)
    K, I, FK, FI = M.shard_begin(db[1000:1008], tags[1000:1008], excl, q, 10, 15, metric, 1000)
    assert np.all(FI == -1) and np.all(np.isnan(FK))                          # k = 10: its 8 hits are all it has, nothing unseen
    K, I, FK, FI = M.shard_begin(db[1008:], tags[1008:], excl, q, 5, 15, metric, 1008)
    assert np.all(I == -1) and np.all(FI >= 1008)                             # no survivor, and rows beyond its 15 hits


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_d_everything_excluded(metric):
    sizes = [700, 600]
    db, q, tags, excl, _ = M.store_d(sizes, 32, 24, 7501)
    assert np.isin(tags, excl).all()
    K, I, unproved = M.sharded_search_excluding(db, tags, excl, q, 5, 15, metric, sizes)
    assert np.all(I == -1) and np.all(np.isnan(K)) and np.all(unproved == 1)
    _check(db, q, tags, excl, 5, 15, metric, sizes)


def test_ties_go_to_the_lower_id_across_shards():
    db, q, tags, _, _ = crowded(600, 16, 6, 0, 0, 7601, extra_excl=0)
    rows = np.array([3, 150, 299, 301, 450, 599])
    db[rows] = q[0] + np.float32(1e-3)                                        # six bit-identical rows at rank 1, three per shard
    excl = np.unique(tags[rows[[1, 3]]])
    _check(db, q, tags, excl, 3, 4, "L2", [300, 300])
    K, I, _ = M.sharded_search_excluding(db, tags, excl, q, 3, 4, "L2", [300, 300])
    np.testing.assert_array_equal(I[0], [3, 299, 450])


def test_the_library_declares_and_binds_the_sharded_form():
    """fails without the feature: the C ABI, its bindings and the Python surface of the model above"""
    import inspect
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib, sharded
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex
    for name in ("radad_knn_search_excl_begin", "radad_knn_search_excl_finish", "radad_excl_merge_certify"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    for name in ("search_excluding_begin", "search_excluding_finish", "excl_merge_certify"):
        assert hasattr(HipFlatIndex, name)
    assert "excluding" in inspect.signature(sharded.ShardedSearch.__init__).parameters
    assert "local_search_excluding" in inspect.signature(sharded.ReplicatedSearch.__init__).parameters
    idx = HipFlatIndex.__new__(HipFlatIndex)
    with pytest.raises(ValueError, match="no exclusion-aware search was begun"):
        idx.search_excluding_finish()
