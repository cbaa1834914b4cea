"""CPU: what the designed stores of the range-search GPU tests (tests/range_ref.py) must be, from plain float64 numpy -- so that a
failure on the GPU is the library's and not the data's:
  * no boundary rows (a key within 1e-9 of the radius could fall either way on the device), except on the integer stores, whose keys
    are exact in any order of summation and where rows that HIT the radius are the point;
  * every query meant for the tile route has at most BAND_CAP = 2048 rows whose key reaches the threshold lowered by EPS_MODEL, so a
    4096-entry candidate buffer cannot overflow while the scan's eps stays below EPS_MODEL;
  * every query meant to overflow has more than 4096 rows within the radius;
  * the reference agrees with a second implementation that walks the (query, row) pairs one by one."""
import numpy as np
import pytest

import range_ref as R


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.case(name)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name", R.CASES)
def test_the_designed_store(cases, name):
    c = cases(name)
    db, q, metric = c["db"], c["q"], c["metric"]
    counts, ids, key, boundary = R.expected_range(db, q, c["radius"], metric, c["M"])
    band, inside = R.band_counts(db, q, c["radius"], metric)
    np.testing.assert_array_equal(inside, counts)
    over = np.zeros(len(q), bool)
    over[c["overflow"]] = True
    if name.startswith("integer"):
        assert boundary.any(axis=1).sum() >= len(q) // 2, "rows that hit the integer radius exactly, for most queries"
        assert boundary.sum() >= 3 * len(q)
    else:
        assert not boundary.any(), f"{int(boundary.sum())} boundary rows"
    if c["route"] == "tile":
        assert (band[~over] <= R.BAND_CAP).all(), f"a query with {int(band[~over].max())} rows within EPS_MODEL of the threshold"
        assert (counts[over] > R.BUFFER).all()
    # what each case is for
    if name.startswith("graded") or name == "centred":
        want = np.array([R.COUNTS[j % 4] for j in range(len(q))])
        np.testing.assert_array_equal(counts, want)                          # exactly the planted rows, nothing random
        for j in (1, 2, 3):
            np.testing.assert_array_equal(np.sort(ids[j, :counts[j]]), np.sort(c["info"]["planted_in"][j]))
        assert (band - counts >= 1).all()                                    # rows planted just outside sit in the band
    if name == "truncation":
        assert counts[0] == 300 and c["M"] == 16
    if name == "overflow":
        assert (counts[c["overflow"]] == 5000).all() and (counts[~over] <= 12).all()
    if name == "nothing":
        assert (counts == 0).all()
    if name == "everything":
        assert (counts == len(db)).all() and len(q) == 17
    if name.startswith("integer"):
        info = c["info"]
        assert counts.max() > c["M"] and counts.min() > 0                    # some lists are cut, none is empty
        rows = np.concatenate([[info["best"]], info["copies"]])
        np.testing.assert_array_equal(ids[0, :len(rows)], rows)              # the duplicates of query 0's best row, in id order
        assert len(set(key[0, :len(rows)])) == 1
        for r in (c["radius"] - 1, c["radius"] + 1):                         # moving the radius by one moves the rows that hit it
            c2 = R.expected_range(db, q, r, metric, c["M"])[0]
            admitting = (r > c["radius"]) == (metric == "L2")               # towards more rows: the ones that hit the radius come in
            moved = (c2 - counts) if admitting else (counts - c2)
            assert (moved >= (boundary.sum(axis=1) if admitting else 0)).all() and moved.sum() > 0


@pytest.mark.parametrize("name", ["graded_cosine", "graded_l2", "graded_ip", "integer_ip", "integer_l2", "truncation", "overflow"])
def test_the_reference_against_a_per_row_walk(cases, name):
    c = cases(name)
    sel = np.unique(np.concatenate([np.arange(min(4, len(c["q"]))), c["overflow"][:1]])).astype(np.int64)
    M = c["M"]
    counts, ids, key, _ = R.expected_range(c["db"], c["q"][sel], c["radius"], c["metric"], M, id_base=1000)
    bc, bi, bk = R.brute_range(c["db"], c["q"][sel], c["radius"], c["metric"], M, id_base=1000)
    np.testing.assert_array_equal(counts, bc)
    np.testing.assert_array_equal(ids, bi)
    f = ids >= 0
    np.testing.assert_allclose(key[f], bk[f], rtol=1e-12, atol=1e-12)
    assert np.isnan(key[~f]).all() and np.isnan(bk[~f]).all()
