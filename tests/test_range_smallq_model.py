"""CPU: what the designed stores of tests/test_gpu_knn_range_smallq.py (tests/range_smallq_ref.py) must be, from plain float64 numpy --
so that a failure on the GPU is the library's and not the data's:
  * the counts are the planted ones, nothing random comes near a threshold;
  * no row lies within 1e-9 of its radius (the nearest are the knife rows: 1e-5 of cosine, 2e-5 of squared distance);
  * crowd queries apart, no query has more than range_ref.BAND_CAP rows within EPS_MODEL of the threshold: its 4096-entry buffer
    cannot overflow while the scan's eps stays below EPS_MODEL; the crowd query has more rows within the radius than a buffer holds.

Checked here (band max: most rows of one query within EPS_MODEL of the threshold; the crowd query apart):
  knife_cos16  80   min |key - radius| 1.0e-5        knife_l2  80   2.0e-5        ip1       60   >= 5e-3
  centred16    81   >= 5e-3                          many9    302   >= 5e-3       crowd5  5000 (query 0, as intended)   >= 5e-3"""
import numpy as np
import pytest

import range_excl_ref as X
import range_ref as R
import range_smallq_ref as S


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = S.case(name)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name", S.MODEL_CASES)
def test_the_designed_store(cases, name):
    c = cases(name)
    db, q, metric = c["db"], c["q"], c["metric"]
    assert len(db) == R.N_ROWS and len(q) <= 16 and db.shape[1] % 64 == 0
    counts, ids, key, boundary = R.expected_range(db, q, c["radius"], metric, c["M"])
    band, inside = R.band_counts(db, q, c["radius"], metric)
    allkeys = R.keys(db, q, metric)
    gap = np.abs(allkeys - np.float64(c["radius"])).min()
    print(f"{name}: counts {counts.tolist()} band max {int(band.max())} min |key - radius| {gap:.3e}")
    np.testing.assert_array_equal(inside, counts)
    np.testing.assert_array_equal(counts, c["counts"])                       # exactly the planted rows
    assert not boundary.any() and gap > 1e-9, f"{int(boundary.sum())} boundary rows, nearest {gap:.3e}"
    over = np.zeros(len(q), bool)
    over[c["overflow"]] = True
    assert (band[~over] <= R.BAND_CAP).all(), f"a query with {int(band[~over].max())} rows within EPS_MODEL of the threshold"
    assert (counts[over] > R.BUFFER).all()
    for j in range(len(q)):
        np.testing.assert_array_equal(np.sort(np.flatnonzero(R.within(allkeys[j], c["radius"], metric))), np.sort(c["info"]["planted_in"][j]))
    assert (band - counts >= 1)[~over].all()                                 # rows planted just outside sit in the band
    if name.startswith("knife"):
        assert gap < 5e-5                                                    # rows that only the float64 re-rank can tell apart
    else:
        assert gap >= 5e-3 - 1e-6                                            # the nearest level is 5e-3 away, the rows are rounded to fp32


def test_the_boundary_copies(cases):
    c = cases("knife_cos16")
    d, src = S.with_boundary_copies(c)
    counts = R.expected_range(d["db"], d["q"], d["radius"], "COSINE", 64)[0]
    base = np.array(c["counts"])
    # the nine overwritten rows were random rows or other queries' planted rows: query 3 gains nine, nobody gains any
    assert counts[3] == base[3] + len(S.BOUNDARY_ROWS) - len(set(S.BOUNDARY_ROWS) & set(c["info"]["planted_in"][3].tolist()))
    assert (np.delete(counts, 3) <= np.delete(base, 3)).all()
    n = R.N_ROWS
    assert n % 16 == 5 and n - 6 == (n // 16) * 16 - 1                       # the last full step's last row; the last step holds 5 rows
    assert -(-n // S.ROWS_PER_WAVE) % 4 == 3                                  # the last workgroup's fourth wave starts beyond the store


def test_the_exclusion_tags(cases):
    """every second planted in-row of query j carries 10 + j: excluding that tag halves (rounding up) what query j finds, and no
    other query loses a row"""
    c = cases("knife_cos16")
    tags = S.tags_by_query(c)
    base = np.array(c["counts"])
    for j in (1, 2, 3):
        adm = X.admissible_batch(tags, np.array([10 + j], np.int64), 16)
        counts = X.expected_range_excl(c["db"], c["q"], c["radius"], "COSINE", 64, adm)[0]
        want = base.copy()
        want[j] = base[j] // 2
        np.testing.assert_array_equal(counts, want)
