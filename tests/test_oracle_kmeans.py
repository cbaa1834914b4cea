"""The float64 k-means restatement of oracle/radad_oracle.py (kmeans_init, kmeans_assign, kmeans_step) on hand-made cases.
No GPU: tests/test_gpu_ivf_build.py holds radad_ivf_train / radad_ivf_add against these."""
import numpy as np
import pytest

from conftest import c_knn
from oracle import radad_oracle as O


@pytest.fixture(params=["numpy", "c"])
def knn_fn(request, knn_oracle_lib):
    return None if request.param == "numpy" else (lambda db, q, k: c_knn(knn_oracle_lib, db, q, k, "L2"))


def test_init_picks_the_strided_rows():
    rows = np.arange(10, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)
    assert O.kmeans_init(rows, 5)[:, 0].tolist() == [0, 2, 4, 6, 8]              # n a multiple of nlist
    assert O.kmeans_init(rows, 4)[:, 0].tolist() == [0, 2, 5, 7]                 # (c * 10) // 4, not c * (10 // 4)
    assert O.kmeans_init(rows, 10)[:, 0].tolist() == list(range(10))             # n == nlist
    assert O.kmeans_init(rows[:3], 8)[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]  # n < nlist: rows repeat
    assert O.kmeans_init(rows[4:5], 3)[:, 0].tolist() == [4, 4, 4]               # n == 1
    assert O.kmeans_init(rows, 4).dtype == np.float32 and O.kmeans_init(rows, 4).shape == (4, 4)


def test_two_obvious_clusters(knn_fn):
    rows = np.array([[0, 0], [0, 2], [10, 0], [10, 4], [2, 0]], np.float32)
    cent = np.array([[1, 1], [9, 1]], np.float32)
    new, assign, counts = O.kmeans_step(rows, cent, knn_fn)
    assert assign.tolist() == [0, 0, 1, 1, 0] and assign.dtype == np.int32
    assert counts.tolist() == [3, 2]
    np.testing.assert_array_equal(new, np.array([[2 / 3, 2 / 3], [10, 2]], np.float64))
    assert new.dtype == np.float64


def test_a_tie_goes_to_the_lower_id(knn_fn):
    cent = np.array([[4, 0], [0, 0], [2, 0], [0, 0]], np.float32)                 # 1 and 3 identical; row [1, 0] between 1 and 2
    rows = np.array([[0, 0], [1, 0], [3, 0], [0, 0.5]], np.float32)
    assert O.kmeans_assign(rows, cent, knn_fn).tolist() == [1, 1, 0, 1]
    new, assign, counts = O.kmeans_step(rows, cent, knn_fn)
    assert counts.tolist() == [1, 3, 0, 0]
    np.testing.assert_array_equal(new[3], cent[3].astype(np.float64))             # the higher of two equal centroids stays empty, unmoved
    np.testing.assert_array_equal(new[1], [1 / 3, 0.5 / 3])


def test_an_empty_cluster_keeps_its_centroid_bit_for_bit(knn_fn):
    odd = np.float32(0.1)                                                         # not a float64-round number
    cent = np.array([[0, 0], [100, odd], [1, 1]], np.float32)
    rows = np.array([[0, 0.25], [1, 1.5], [0.25, 0]], np.float32)
    new, assign, counts = O.kmeans_step(rows, cent, knn_fn)
    assert counts.tolist() == [2, 0, 1]
    assert new[1, 1] == np.float64(odd) and new[1, 0] == 100.0
    assert new[1].astype(np.float32).tobytes() == cent[1].tobytes()
    np.testing.assert_array_equal(new[0], [0.125, 0.125])


def test_fewer_rows_than_lists(knn_fn):
    rows = np.array([[1, 0], [0, 1], [5, 5]], np.float32)
    cent = O.kmeans_init(rows, 7)                                                 # rows 0 0 0 1 1 2 2
    np.testing.assert_array_equal(cent, rows[[0, 0, 0, 1, 1, 2, 2]])
    new, assign, counts = O.kmeans_step(rows, cent, knn_fn)
    assert assign.tolist() == [0, 3, 5]
    assert counts.tolist() == [1, 0, 0, 1, 0, 1, 0]
    np.testing.assert_array_equal(new, cent.astype(np.float64))


def test_assign_is_float64_where_float32_cannot_tell(knn_fn):
    """two centroids whose distances to the row differ by one part in 1e9: a float32 evaluation of 2 q.c - |c|^2 calls it a tie"""
    x = np.full((1, 8), 1000.0, np.float32)
    cent = np.full((2, 8), 1000.0, np.float32)
    cent[0, 0] += np.float32(1.0)                                                 # distance 1
    cent[1, 0] -= np.float32(1.0) - np.float32(2.0 ** -14)                        # distance (1 - 2^-14)^2: nearer
    assert O.kmeans_assign(x, cent, knn_fn).tolist() == [1]
