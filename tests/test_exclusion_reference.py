"""The reference the exclusion-aware search is tested against (tests/exclusion_ref.py), itself checked where it can run: the
`valid[...]` remapping of the oracle over the admissible rows and the derived number of exact-pass queries, on a 200-row example,
against a direct masked float64 sort."""
import numpy as np
import pytest

from exclusion_ref import crowded, expected_exact, expected_excluding


def _direct(db, tags, excl, q, k, metric):
    """masked float64 sort over the whole store: (ids [nq,k] with -1 padding, keys, order of ALL rows per query)"""
    x, y = q.astype(np.float64), db.astype(np.float64)
    if metric == "COSINE":
        x = x / (np.sqrt((x * x).sum(1)) + 1e-12)[:, None]
        y = y / (np.sqrt((y * y).sum(1)) + 1e-12)[:, None]
    d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1) if metric == "L2" else -(x @ y.T)
    order = np.lexsort((np.broadcast_to(np.arange(len(db)), d.shape), d), axis=1)      # (distance, id)
    bad = np.isin(tags, excl)
    ids = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        keep = order[j][~bad[order[j]]][:k]
        ids[j, :len(keep)] = keep
    return ids, order, bad


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("k,k_fetch", [(5, 15), (5, 5), (12, 40)])
def test_reference_matches_masked_sort(metric, k, k_fetch):
    db, q, tags, excl, which = crowded(200, 16, 10, 4, 20, 4242, extra_excl=10)
    tags = tags // 2 * 2                                    # two rows per tag: a dropped tag takes both
    excl = np.unique(tags[np.isin(tags, excl // 2 * 2)])
    ids, order, bad = _direct(db, tags, excl, q, k, metric)
    D, I = expected_excluding(db, tags, excl, q, k, metric)
    np.testing.assert_array_equal(I, ids)
    assert not np.isin(tags[I[I >= 0]], excl).any()
    assert np.all(np.isnan(D[I < 0])) and np.all(np.isfinite(D[I >= 0]))
    # the derived count: fewer than k admissible rows among the first k_fetch of the full order
    want = np.array([(~bad[order[j][:k_fetch]]).sum() < k for j in range(len(q))])
    got = expected_exact(db, tags, excl, q, k, k_fetch, metric)
    np.testing.assert_array_equal(got, want)
    assert got[which].all() or k_fetch > 20                 # 20 excluded near-duplicates crowd out a list of <= 20


def test_reference_padding_and_id_base():
    db, q, tags, _, _ = crowded(200, 16, 6, 2, 10, 77, extra_excl=0)
    excl = np.unique(tags[3:])                              # three admissible rows
    D, I = expected_excluding(db, tags, excl, q, 5, "L2", id_base=1000)
    assert set(I[0, :3].tolist()) == {1000, 1001, 1002} and np.all(I[:, 3:] == -1) and np.all(np.isnan(D[:, 3:]))
    assert expected_exact(db, tags, excl, q, 5, 15, "L2").all()
    # a store smaller than k_fetch: the list has unfilled slots, nothing takes the exact pass
    assert not expected_exact(db[:8], tags[:8], excl, q, 5, 15, "L2").any()
    D0, I0 = expected_excluding(db, tags, None, q, 5, "L2")
    assert np.all(I0 >= 0) and np.all(np.diff(D0, axis=1) >= 0)
