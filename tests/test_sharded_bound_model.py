"""The numpy model of the bounded sharded search (tests/sharded_bound_ref.py) against the float64 oracle over the WHOLE store, and the
designed stores S1-S6 against what they were designed for: the gap of S2, the tie groups of S3 at the cut, the small shards of S4
that must contribute.  CPU only; tests/test_gpu_sharded_bound.py searches the same stores on the device."""
import numpy as np
import pytest

from oracle import radad_oracle as O
import sharded_bound_ref as M

KS = (1, 4, 7, 10, 128)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name, metric):
        if (name, metric) not in cache:
            db, q, sizes, info = M.STORES[name]()
            stored = O.stored_rows(db, metric, name in M.F16).astype(np.float32)
            qq = O.stored_rows(q, "COSINE") if metric == "COSINE" else q          # (the prepared query: radad_rownorm's value)
            cache[(name, metric)] = (M.Model(stored, qq, metric, sizes), stored, qq, info)
        return cache[(name, metric)]
    yield get
    cache.clear()


def _oracle_ids(stored, qq, k, metric):
    if metric == "L2":
        return O.knn_exact_l2_chunked(stored, qq, k)
    return O.knn(stored, qq, k, "IP")


@pytest.mark.parametrize("name,metric", [(n, m) for n in ("S1", "S2", "S4") for m in ("L2", "COSINE", "IP")]
                         + [("S5", "L2"), ("S6", "COSINE"), ("S6", "L2")])
def test_model_is_the_oracle_of_the_whole_store(models, name, metric):
    m, stored, qq, _ = models(name, metric)
    od, oi = _oracle_ids(stored, qq, max(KS), metric)
    for k in KS:
        ms, mi = m.topk(k)
        np.testing.assert_array_equal(mi, oi[:, :k])
        np.testing.assert_allclose(-ms if metric == "L2" else ms, od[:, :k], rtol=1e-12, atol=1e-12)
        # the union over the shards of must_return is the oracle top k, and no id is claimed twice
        for j in range(m.nq):
            parts = [m.must_return(g, k)[j] for g in range(len(m.sizes))]
            assert sorted(np.concatenate(parts).tolist()) == sorted(oi[j, :k].tolist())
        _bound_is_tight(m, k)


def _bound_is_tight(m, k):
    kth, tb = m.kth(k), m.tightest_bound(k)
    assert tb.dtype == np.float32
    assert np.all(tb.astype(np.float64) <= kth)
    assert np.all(np.nextafter(tb, np.float32(np.inf)).astype(np.float64) > kth)        # within one float32 ulp of it


def test_bound_of_a_store_with_fewer_than_k_rows():
    db, q, _, _ = M.s4(8)
    m = M.Model(db[-7:], q, "L2", [3, 4])
    assert np.all(np.isfinite(m.tightest_bound(7))) and np.all(m.tightest_bound(8) == -np.inf)
    assert m.topk(10)[1].shape == (8, 7) and m.shard_topk(1, 10).shape == (8, 4)
    assert np.all(m.shard_topk(1, 10) >= 3)


@pytest.mark.parametrize("metric,gap", [("COSINE", 0.2), ("L2", 10.0), ("IP", 10.0)])
def test_s2_gap(models, metric, gap):
    """the 10-th best score of every query lies in shard 1, far above anything shards 0 and 2 hold"""
    m, _, _, rows = models("S2", metric)
    for k in (1, 10):
        kth = m.kth(k)
        far = np.maximum(m.shard_sorted(0)[:, 0], m.shard_sorted(2)[:, 0])
        assert (kth - far).min() >= gap, (k, kth.min(), far.max())
        for g in (0, 2):
            assert all(len(x) == 0 for x in m.must_return(g, k))
    assert np.array_equal(np.sort(m.topk(M.S2_PLANTED)[1], 1), rows)


@pytest.mark.parametrize("metric", ["L2", "COSINE", "IP"])
@pytest.mark.parametrize("k", [4, 7])
def test_s3_cut_falls_inside_a_tie_group(models, metric, k):
    m, _, _, (tied, first, second) = models("S3", metric)
    ms, mi = m.topk(k + 1)
    assert np.all(ms[tied, k - 1] == ms[tied, k])                    # rank k and rank k + 1 hold equal float64 keys
    for c, j in enumerate(tied):
        assert len(set(m.S[j, first[c]])) == 1 and len(set(m.S[j, second[c]])) == 1
        groups = sorted([(m.S[j, first[c][0]], np.sort(first[c])), (m.S[j, second[c][0]], np.sort(second[c]))], key=lambda t: -t[0])
        assert groups[0][0] > groups[1][0] > m.sorted[j, 9]           # the nine copies are the query's nine best rows
        want = np.concatenate([groups[0][1], groups[1][1]])[:k]       # group by group, the lower id first
        np.testing.assert_array_equal(mi[j, :k], want)
        got = np.concatenate([m.must_return(g, k)[j] for g in range(3)])
        assert sorted(got.tolist()) == sorted(want.tolist())
        assert sum(len(m.must_return(g, k)[j]) > 0 for g in range(3)) >= 2      # the tie is decided ACROSS shards
    _bound_is_tight(m, k)


@pytest.mark.parametrize("metric", ["L2", "COSINE", "IP"])
def test_s4_small_shards_contribute(models, metric):
    m, _, _, rows = models("S4", metric)
    for g in (1, 2, 3):
        owners = [j for j in range(m.nq) if rows[j, 0] >= m.bases[g] and rows[j, 0] < m.bases[g + 1]]
        assert len(owners) >= 2
        for k in (1, 10):
            mr = m.must_return(g, k)                                  # k = 1: one of the three; k = 10: all three
            assert all(len(set(rows[j]) & set(mr[j].tolist())) == min(k, 3) for j in owners), (g, k)
    assert m.sizes[3] < 10 and np.all(np.isfinite(m.tightest_bound(10)))


def test_host_kth_largest_ranks_nan_lowest():
    x = np.array([[[1.0, np.nan]], [[-np.inf, 0.5]]], np.float32)     # G = 2, nq = 1, kk = 2
    assert [float(M.host_kth_largest(x, k)[0]) for k in (1, 2, 3, 4)] == [1.0, 0.5, -np.inf, -np.inf]


def test_global_bound_on_host_tensors_ranks_nan_lowest():
    """HipFlatIndex.global_bound on CPU tensors takes torch.topk, which ranks NaN highest; the kernel it stands in for ranks it lowest
    (include/radad_hip.h, radad_kth_largest).  -inf and +inf stay what they are."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 9, 10)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = np.nan
    x[rng.random(x.shape) < 0.1] = -np.inf
    x[rng.random(x.shape) < 0.05] = np.inf
    x[:, 1, :] = np.nan
    x[0, 2, :] = -np.inf
    for k in (1, 5, 10):
        got = HipFlatIndex.global_bound(torch.from_numpy(x), k).numpy()
        assert np.array_equal(got, M.host_kth_largest(x, k)), k
    assert HipFlatIndex.global_bound(torch.from_numpy(x), 1)[1] == -np.inf
