"""CPU: the designed store of the per-query search on the certified tile scan (tests/excl_scan_pq_ref.speakers) has the properties
tests/test_gpu_knn_excl_scan_pq.py relies on, for every shape, store kind and metric used there, in plain float64 numpy and against
the oracle:
  * every crowd row outranks its owning query's k-th ADMISSIBLE neighbour -- so a floor that counted crowd rows would lie above every
    admissible row, and a scan that let them through to the re-rank would return them;
  * adjacent admissible ranks 1 .. k + 1 are at least 1e-4 apart (excl_per_query_ref.adjacent_gap, the oracle's keys): comparing ids
    exactly does not hinge on a near-tie;
  * a bystander's top k lies inside the crowd its neighbour queries exclude.
And the wiring: the Python surface of the new call exists, and the refusing wrappers name the right call."""
import numpy as np
import pytest

import excl_per_query_ref as P
import excl_scan_pq_ref as S

K_OF = {"grid": 10, "c1500": 10, "c5000": 10, "two_phase": 100, "shards": 10}


def test_the_store_is_what_its_docstring_says():
    db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["grid"])
    c = S.SHAPES["grid"]["c"]
    assert db.dtype == np.float32 and q.dtype == np.float32 and db.shape == (20480, 64) and q.shape == (300, 64)
    for s in range(4):
        assert np.all(tags[info["crowd"][s]] == S.SPEAKER_TAG0 + s) and len(np.unique(info["crowd"][s])) == c
        assert len(np.unique(tags[info["near"][s]])) == info["ladder"] and not np.isin(tags[info["near"][s]], qtags).any()
    assert (tags >= S.SPEAKER_TAG0).sum() == 4 * c
    own = info["owner"]
    assert np.array_equal(qcnt, own.astype(np.int32)) and np.array_equal(qtags[:, 0], S.SPEAKER_TAG0 + info["speaker"])
    for prefix in (40, 300):                                                    # both kinds at every centre, in every batch the tests form
        for s in range(4):
            at = info["speaker"][:prefix] == s
            assert (own[:prefix] & at).sum() >= 2 and (~own[:prefix] & at).sum() >= 1
    # the crowd is spread over the whole store: both sides of any phase boundary, and inside a 1 / 16 sample
    assert (info["crowd"] < 20480 // 8).any() and (info["crowd"] >= 20480 // 8).any()
    db5, _, _, _, qcnt5, info5 = S.speakers(**S.SHAPES["c5000"])
    assert qcnt5.sum() == 8 and info5["owner"][:8].all() and not info5["owner"][8:].any()


@pytest.mark.parametrize("metric", ["L2", "COSINE", "IP"])
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_properties_the_gpu_tests_rely_on(name, kind, metric):
    db, q, tags, qtags, qcnt, info = S.shape(name, kind)
    k = K_OF[name]
    p = S.store_properties(db, q, tags, qtags, qcnt, info, k, metric)
    print(name, kind, metric, p)
    assert p["crowd_outranks"], p
    assert p["bystanders_inside"], p
    assert p["min_gap"] >= 1e-4, p
    if name == "two_phase":
        first = 131072                                                          # rows of the scan's first phase (the plan check prints it)
        assert (info["crowd"] < first).any(axis=1).all() and (info["crowd"] >= first).any(axis=1).all()
        assert (info["crowd"] < S.TWO_PHASE_ROWS // 8).any(axis=1).all()


@pytest.mark.parametrize("metric", ["L2", "COSINE", "IP"])
@pytest.mark.parametrize("name", ["grid", "c1500"])
def test_adjacent_gap_by_the_oracle(name, metric):
    """the same gap from the oracle the GPU tests compare against (40 queries: every speaker's owners and bystanders)"""
    db, q, tags, qtags, qcnt, info = S.shape(name)
    gap = P.adjacent_gap(db, tags, qtags[:40], qcnt[:40], q[:40], K_OF[name], metric)
    assert gap >= 1e-4, gap
    ed, ei = P.expected_pq(db, tags, qtags[:40], qcnt[:40], q[:40], K_OF[name], metric)
    for j in range(40):
        s = info["speaker"][j]
        pool = info["near"][s] if info["owner"][j] else info["crowd"][s]
        assert np.isin(ei[j], pool).all()                                       # owners: near rows only; bystanders: the crowd
        assert info["owner"][j] == (not np.isin(ei[j], info["crowd"][s]).any())


def test_the_python_surface():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import Config, HipFlatIndex, HipIVFFlatIndex, VectorDatabase
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    assert Config().exclusion_per_query_in_scan is False
    for cls in (HipFlatIndex, VectorDatabase):
        assert callable(getattr(cls, "search_excluding_per_query_in_scan"))
    with pytest.raises(ValueError, match="search_probed_excluding_per_query"):
        HipIVFFlatIndex.search_excluding_per_query_in_scan(None)
    with pytest.raises(ValueError, match="search_excluding_per_query_in_scan"):
        ShardedSearch.search_excluding_per_query_in_scan(None)
