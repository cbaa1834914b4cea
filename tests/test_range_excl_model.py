"""CPU: what the designed stores of tests/test_gpu_knn_range_excl.py (tests/range_excl_ref.py) must be, from plain float64 numpy -- so
that a failure on the GPU is the library's and not the data's:
  * the two references agree (the masked range_ref.expected_range and a walk over the (query, row) pairs);
  * no designed store has a boundary row among its admissible rows, except the integer stores;
  * every query meant to stay on the tile route has at most BAND_CAP = 2048 rows whose key reaches the threshold lowered by
    range_ref.EPS_MODEL -- in the per-query mode counted over ALL rows, because the scan emits a query's excluded rows too; in the
    batch mode over the admissible rows, because a NaN bias keeps the others out of the buffers;
  * the queries meant to overflow have more than 4096 rows the scan must emit;
  * in at least half of the queries of the graded stores the exclusion changes the answer: a call that ignored the tags would fail."""
import numpy as np
import pytest

import range_excl_ref as X
import range_ref as R


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            c = X.case(name)
            c["adm"] = X.admissible(c)
            c["key"] = R.keys(c["db"], c["q"], c["metric"])
            cache[name] = c
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name", X.CASES)
def test_the_designed_store(cases, name):
    c = cases(name)
    db, q, metric, adm, key = c["db"], c["q"], c["metric"], c["adm"], c["key"]
    nq = len(q)
    counts, ids, keys, boundary = X.expected_range_excl(db, q, c["radius"], metric, c["M"], adm, key=key)
    plain = R.expected_range(db, q, c["radius"], metric, c["M"], key=key)
    inside = R.within(key, c["radius"], metric)
    np.testing.assert_array_equal(counts, (inside & adm).sum(axis=1))
    assert (counts <= plain[0]).all()
    f = ids >= 0
    assert adm[np.nonzero(f)[0], ids[f]].all(), "an excluded row in a slot"
    over = np.zeros(nq, bool)
    over[c["overflow"]] = True
    if name.startswith("integer"):
        assert (boundary & adm).any(axis=1).sum() >= nq // 2, "admissible rows that hit the integer radius exactly, for most queries"
    else:
        assert not boundary.any(), f"{int(boundary.sum())} boundary rows"
    if c["route"] == "tile":
        e = R.EPS_MODEL[metric]
        band = key <= np.float64(c["radius"]) + e if metric == "L2" else key >= np.float64(c["radius"]) - e
        emitted = (band & adm if c["mode"] == "batch" else band).sum(axis=1)            # what the scan may emit
        sure = (inside & adm if c["mode"] == "batch" else inside).sum(axis=1)           # what it must emit
        assert (emitted[~over] <= R.BAND_CAP).all(), f"a tile-route query with {int(emitted[~over].max())} rows in the band"
        assert (sure[over] > R.BUFFER).all(), "a query meant to overflow that may fit"
    # what each case is for
    base = name[:-len("_batch")] if name.endswith("_batch") else name
    if c["mode"] == "pq" and (base.startswith("graded") or base == "centred"):
        live = X.live_counts(c["q_cnt"], nq, X.M_TAGS)
        want = np.array([R.COUNTS[j % 4] - (len(c["info"]["planted_in"][j][0::2]) if live[j] else 0) for j in range(nq)])
        np.testing.assert_array_equal(counts, want)
        np.testing.assert_array_equal(live, [0 if j % 16 == 8 else 4 if j % 16 == 7 else j % 4 for j in range(nq)])
        assert (counts != plain[0]).sum() >= nq // 2, "the exclusion changes too few answers"
        assert c["q_tags"][6, 0] == c["q_tags"][6, 1] == X.own(6)
        assert ((c["q_cnt"] < 0) | (c["q_cnt"] > X.M_TAGS)).sum() >= 2
    if c["mode"] == "batch" and base != "all_excluded":
        assert (counts != plain[0]).sum() >= nq // 4 and counts.sum() > 0
        assert (np.diff(c["excl"]) > 0).all()
    if base == "crowd_fits":
        assert counts[0] == 40 and plain[0][0] == 1540 and nq == 299 and len(c["overflow"]) == 0
        assert (c["row_tags"] == X.own(0)).sum() >= 1500
    if base == "crowd_overflows":
        assert (c["row_tags"] == X.own(299)).sum() == 5000 and nq == 300
        if c["mode"] == "pq":
            assert counts[299] == 5 and counts[0] == 40
        else:
            assert X.own(0) in c["excl"] and X.own(299) not in c["excl"] and counts[299] > R.BUFFER and 0 < counts[0] < 40
    if base == "truncation":
        assert counts[0] == 300 and plain[0][0] == 500 and c["M"] == 16
        worst_excluded = key[0, c["info"]["planted_in"][0][300:]].min()
        assert (keys[0, :16] < worst_excluded).all(), "the excluded rows rank better than every admissible row"
    if base == "everything":
        assert nq == 17 and (counts == adm.sum(axis=1)).all() and (counts < len(db)).any() and (counts > R.BUFFER).all()
    if base == "all_excluded":
        assert (counts == 0).all() and (ids == -1).all() and np.isnan(keys).all() and plain[0].sum() > 0
    if base.startswith("integer"):
        info = c["info"]
        rows = np.concatenate([[info["best"]], info["copies"][1:]])            # the first copy is excluded by query 0
        np.testing.assert_array_equal(ids[0, :len(rows)], rows)
        assert len(set(keys[0, :len(rows)])) == 1 and plain[1][0, 1] == info["copies"][0]
        assert counts.max() > c["M"] and counts.min() > 0


@pytest.mark.parametrize("name", ["graded_cosine", "graded_l2", "graded_ip", "integer_ip", "integer_l2", "truncation", "crowd_overflows",
                                  "graded_cosine_batch", "crowd_overflows_batch", "exact_small_store", "exact_small_store_batch"])
def test_the_reference_against_a_per_row_walk(cases, name):
    c = cases(name)
    sel = np.unique(np.concatenate([np.arange(min(4, len(c["q"]))), [min(6, len(c["q"]) - 1)], c["overflow"][:1]])).astype(np.int64)
    M = c["M"]
    counts, ids, key, _ = X.expected_range_excl(c["db"], c["q"][sel], c["radius"], c["metric"], M, c["adm"][sel], id_base=1000)
    if c["mode"] == "batch":
        bc, bi, bk = X.brute_range_excl(c["db"], c["q"][sel], c["radius"], c["metric"], M, c["row_tags"], excl=c["excl"], id_base=1000)
    else:
        bc, bi, bk = X.brute_range_excl(c["db"], c["q"][sel], c["radius"], c["metric"], M, c["row_tags"], q_tags=c["q_tags"][sel],
                                        q_cnt=None if c["q_cnt"] is None else c["q_cnt"][sel], id_base=1000)
    np.testing.assert_array_equal(counts, bc)
    np.testing.assert_array_equal(ids, bi)
    f = ids >= 0
    np.testing.assert_allclose(key[f], bk[f], rtol=1e-12, atol=1e-12)
    assert np.isnan(key[~f]).all() and np.isnan(bk[~f]).all()
