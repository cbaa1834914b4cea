"""GPU parity of the inverted-file flat index (vector_db_index_type == "IVF", vector_database.py:65-70,124-128,174-181).
faiss' k-means cannot be reproduced bit for bit (and faiss is absent), so training is checked through its invariants and
the SEARCH is checked exactly: given the centroids and list assignments the index holds, results must equal the float64
oracle restricted to the probed lists."""
import numpy as np
import pytest

from conftest import c_knn
from oracle import radad_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu


def _clustered(n, dim, n_clusters, seed):
    centers = synth.rows(0, n_clusters, dim, seed) * np.float32(3.0)
    which = (np.arange(n) * 7919) % n_clusters
    return (centers[which] + synth.rows(0, n, dim, seed + 1)).astype(np.float32)


@pytest.mark.parametrize("n,dim,nlist,nq,k,nprobe", [(20000, 64, 64, 100, 5, 8), (30000, 512, 128, 300, 15, 32),
                                                     (5000, 96, 64, 3, 10, 64), (8000, 5376, 64, 20, 15, 4)])
def test_ivf_search_matches_oracle(gpu, knn_oracle_lib, n, dim, nlist, nq, k, nprobe):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    db = _clustered(n, dim, 50, 5001)
    q = _clustered(nq, dim, 50, 5003)
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    assert not idx.is_trained and idx.ntotal == 0
    idx.train(db[: min(n, 10000)])
    assert idx.is_trained
    idx.add(db[: n // 2])
    idx.add(db[n // 2:])
    assert idx.ntotal == n
    cent, assign = idx.centroids(), idx.assignments()
    assert cent.shape == (nlist, dim) and assign.shape == (n,) and np.isfinite(cent).all()
    # every row sits in the list of its nearest centroid: the float64 argmin (the lower id on a tie), at every dim
    np.testing.assert_array_equal(assign, O.kmeans_assign(db, cent, lambda c, x, kk: c_knn(knn_oracle_lib, c, x, kk, "L2")))
    idx.nprobe = nprobe
    D, I = idx.search(q, k)
    od, oi = O.ivf_search(db, assign, cent, q, k, nprobe)
    np.testing.assert_array_equal(I, oi)
    fin = np.isfinite(od)
    np.testing.assert_allclose(D[fin], od[fin], rtol=1e-6, atol=1e-5)
    assert np.all(np.isinf(D[~fin]))
    # probing every list == exact search
    idx.nprobe = nlist
    D, I = idx.search(q[:10], k)
    od, oi = O.knn(db, q[:10], k, "L2")
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(idx.reconstruct(123), db[123], rtol=0, atol=0)


@pytest.mark.parametrize("dim,nprobe,k", [(32, 8, 10), (32, 64, 26), (1056, 8, 10), (1056, 16, 26)])
def test_ivf_search_matches_oracle_at_the_narrowest_and_a_wide_no_plane_width(gpu, dim, nprobe, k):
    """dim 32 is the smallest radad_ivf_create takes; 1056 = 64 * 16 + 32 has no f16 plane route (dim % 64 == 32): both search on the
    fp32 list scan.  The rows are a tail_store (tests/knn_width_ref.py): per query 1100 decoys that equal it except in ONE vec4 column
    group -- first, last, the first of the partial 64-column step, an interior one -- so a list scan that mishandles that group ranks
    them first; a correct one has nothing to reject."""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    import knn_width_ref as W
    n, nlist, nq = 8000, 64, 20
    db, q, info = W.tail_store(dim, n, nq, 26, 5201)
    assert info["centres"] == len(W.column_groups(dim)) >= 3
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    idx.train(db)
    idx.add(db[: n // 2])
    idx.add(db[n // 2:])
    cent, assign = idx.centroids(), idx.assignments()
    idx.nprobe = nprobe
    D, I = idx.search(q, k)
    info_s = idx.last_search_info()
    assert info_s["scan"] == "f32_lists", info_s
    assert info_s["rejected"] == 0, info_s
    od, oi = O.ivf_search(db, assign, cent, q, k, nprobe)
    np.testing.assert_array_equal(I, oi)
    fin = np.isfinite(od)
    assert fin[:, 0].all()
    np.testing.assert_allclose(D[fin], od[fin], rtol=1e-6, atol=1e-5)
    assert np.all(np.isinf(D[~fin]))
    if nprobe == nlist:                                   # every list probed: the centre's own neighbours, in order
        s, _ = W.scores64(db, info["centre_rows"], "L2")
        np.testing.assert_array_equal(I, W.topk64(s, k)[info["centre_of"]])


def test_ivf_kmeans_improves_and_is_deterministic(gpu):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    db = _clustered(6000, 64, 20, 6001)

    def cost(cent):
        d2 = ((db[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1)
        return d2.min(1).mean()
    a = R.HipIVFFlatIndex(64, 64, gpu.index or 0, niter=0); a.train(db)
    b = R.HipIVFFlatIndex(64, 64, gpu.index or 0, niter=10); b.train(db)
    c = R.HipIVFFlatIndex(64, 64, gpu.index or 0, niter=10); c.train(db)
    assert cost(b.centroids()) < 0.8 * cost(a.centroids())            # Lloyd iterations reduce the quantisation error
    np.testing.assert_array_equal(b.centroids(), c.centroids())      # deterministic (no atomics in the update)


def test_vector_database_ivf_mode(gpu, tmp_path):
    """the reference's IVF branch end to end: nlist = max(64, ivf_nlist), train on add, nprobe from config, save/load"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, vector_db_path=str(tmp_path / "ivf"), vector_db_index_type="IVF", vector_db_nprobe=16)
    cfg.ivf_nlist = 32                                               # max(64, 32) -> 64 lists (vector_database.py:67-68)
    vdb = R.VectorDatabase(cfg)
    db = _clustered(12000, 128, 40, 7001)
    vdb.add_vectors(db, [f"f{i}.wav" for i in range(len(db))], [0] * len(db), {})
    assert isinstance(vdb.index, R.HipIVFFlatIndex) and vdb.index.nlist == 64 and vdb.index.is_trained and vdb.index.ntotal == 12000
    q = _clustered(40, 128, 40, 7003)
    D, I = vdb.search_batch(q, k=10)
    assert vdb.index.nprobe == 16
    od, oi = O.ivf_search(db, vdb.index.assignments(), vdb.index.centroids(), q, 10, 16)
    np.testing.assert_array_equal(I, oi)
    exact_d, exact_i = O.knn(db, q, 10, "L2")
    recall = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(I, exact_i)])
    assert recall > 0.9                                              # clustered data, 16 of 64 lists probed
    vdb.save()
    # the rows travel as a native flat snapshot (streamed, never a host array of the store), the centroids in a sidecar
    import os
    with open(vdb.db_path, "rb") as f:
        assert f.read(8) == b"RADADKNN"
    assert os.path.exists(vdb.db_path + ".ivf.npz")
    v2 = R.VectorDatabase(cfg)
    v2.load()
    assert v2.index.ntotal == 12000
    np.testing.assert_array_equal(v2.search_batch(q, k=10)[1], I)
    np.testing.assert_array_equal(v2.index.centroids(), vdb.index.centroids())
    np.testing.assert_array_equal(v2.index.assignments(), vdb.index.assignments())
    for i in (0, 1, 5999, 11999):
        np.testing.assert_array_equal(v2.index.reconstruct(i), db[i])


@pytest.mark.parametrize("k", [40, 100])
def test_ivf_large_k_is_answered_by_the_exact_scan(gpu, k):
    """faiss takes k up to 2048 (vector_database.py:169-181).  The list scan holds k + 6 <= 32 candidates per (query, list); above
    k = 26 the index answers with the exact search over the same rows (ids in insertion order): the float64 brute force itself"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    n, dim, nlist, nq = 30000, 128, 64, 50
    db = _clustered(n, dim, 50, 5101)
    q = _clustered(nq, dim, 50, 5103)
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    idx.train(db[:10000])
    idx.add(db)
    idx.nprobe = 4
    D, I = idx.search(q, k)
    od, oi = O.knn(db, q, k, "L2")
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        idx.search(q, 129)


@pytest.mark.parametrize("hi_scan,nq", [(1, 1), (1, 40), (1, 700), (0, 40), (2, 40), (2, 3)])
def test_ivf_list_scan_variants_agree_with_the_oracle(gpu, hi_scan, nq):
    """the certified f16 list scan (default), the fp32 list scan alone (hi_scan 0), and the fp32 pass behind the f16 scan when the
    certificate rejects (hi_scan 2 declares every query rejected): the same float64 oracle restricted to the probed lists; one query
    (lists split over several workgroups), a few tasks per list, and lists probed by more than 16 queries (several tasks per list)"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    n, dim, nlist, k, nprobe = 40000, 256, 96, 15, 12
    db = _clustered(n, dim, 60, 5201)
    q = _clustered(nq, dim, 60, 5203)
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, hi_scan=hi_scan)
    idx.train(db[:10000])
    idx.add(db)
    idx.nprobe = nprobe
    D, I = idx.search(q, k)
    info = idx.last_search_info()
    assert info["scan"] == ("f32_lists" if hi_scan == 0 else "hi_lists"), info
    if hi_scan == 2:
        assert info["rejected"] == nq, info
    elif hi_scan == 1:
        assert info["rejected"] <= max(1, nq // 20), info           # the certificate holds on ordinary data
    od, oi = O.ivf_search(db, idx.assignments(), idx.centroids(), q, k, nprobe)
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-6, atol=1e-5)
    # rows appended afterwards: the list-major plane is gathered again
    extra = _clustered(3000, dim, 60, 5205)
    idx.add(extra)
    db2 = np.concatenate([db, extra])
    D, I = idx.search(q, k)
    od, oi = O.ivf_search(db2, idx.assignments(), idx.centroids(), q, k, nprobe)
    np.testing.assert_array_equal(I, oi)


def test_ivf_long_lists_take_several_chunks(gpu):
    """lists of more than 256 rows (the scan's chunk): the k best of a list are carried from chunk to chunk for the admission bound"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    n, dim, nlist, nq, k, nprobe = 30000, 128, 16, 50, 20, 5
    db = _clustered(n, dim, 8, 5301)
    q = _clustered(nq, dim, 8, 5303)
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    idx.train(db[:10000])
    idx.add(db)
    idx.nprobe = nprobe
    D, I = idx.search(q, k)
    assert idx.last_search_info()["scan"] == "hi_lists"
    od, oi = O.ivf_search(db, idx.assignments(), idx.centroids(), q, k, nprobe)
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("seed", [0, 1])
def test_ivf_fuzz_against_the_oracle(gpu, seed):
    """bounded random sweep over the IVF search: dims with and without an f16 plane (dim % 64), one query to a few thousand, k from 1 to
    26, nprobe from 1 to every list, more lists than rows per list (empty lists), skewed lists; ids == the float64 oracle restricted to
    the probed lists, every time"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    rng = np.random.default_rng(100 + seed)
    for case in range(6):
        dim = int(rng.choice([64, 96, 128, 320, 512]))
        nlist = int(rng.choice([16, 50, 128, 300]))
        n = int(rng.choice([3000, 20000, 45000]))
        nq = int(rng.choice([1, 2, 16, 17, 100, 1500]))
        k = int(rng.choice([1, 5, 15, 26]))
        nprobe = int(rng.choice([1, 3, 8, nlist]))
        n_clusters = int(rng.choice([3, 40, 400]))
        db = _clustered(n, dim, n_clusters, 6000 + 10 * seed + case)
        q = _clustered(nq, dim, n_clusters, 6500 + 10 * seed + case)
        idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, niter=int(rng.choice([0, 3])))
        idx.train(db[: min(n, 8000)])
        idx.add(db)
        idx.nprobe = nprobe
        D, I = idx.search(q, k)
        info = idx.last_search_info()
        what = dict(seed=seed, case=case, dim=dim, nlist=nlist, n=n, nq=nq, k=k, nprobe=nprobe, n_clusters=n_clusters, info=info)
        assert info["scan"] == ("hi_lists" if dim % 64 == 0 else "f32_lists"), what
        od, oi = O.ivf_search(db, idx.assignments(), idx.centroids(), q, k, min(nprobe, nlist))
        np.testing.assert_array_equal(I, oi, err_msg=str(what))
        fin = np.isfinite(od)
        np.testing.assert_allclose(D[fin], od[fin], rtol=1e-6, atol=1e-5, err_msg=str(what))


@pytest.fixture(scope="module")
def exact_launches_case(gpu):
    """4096 rows of dim 64 under 256 centroids that are rows of the store, every list probed at k = 26 with every query declared
    rejected (hi_scan 2): k_ivf_exact answers the batch, 1260 queries per launch (256 x 26 x 16 B of partial lists each, 128 MiB per
    launch).  The store, the queries, the index and the float64 oracle over the whole store, made once and released with the module."""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    n, dim, nlist, k = 4096, 64, 256, 26
    db, q = synth.rows(0, n, dim, 5401), synth.rows(0, 1300, dim, 5403)
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, hi_scan=2)
    idx.set_centroids(db[:: n // nlist])
    idx.add(db)
    idx.nprobe = nlist
    tags = np.arange(n, dtype=np.int64)
    excl = np.sort(np.random.default_rng(5405).choice(n, n // 100, replace=False)).astype(np.int64)
    keep = np.flatnonzero(~np.isin(tags, excl))
    fd, fi = O.knn(db[keep], q, k, "L2")
    yield dict(idx=idx, q=q, k=k, plain=O.knn(db, q, k, "L2"), tags=tags, excl=excl, filtered=(fd, keep[fi]))


@pytest.mark.parametrize("nq,filtered", [(1260, False), (1261, False), (1300, False), (1300, True)])
def test_ivf_exact_list_scan_in_more_than_one_launch(gpu, exact_launches_case, nq, filtered):
    """the rejected queries' partial lists exceed the budget of one launch of k_ivf_exact from 1261 queries on: 1260 is one launch,
    1261 and 1300 are two, the second with 1 and 40 live slots; unfiltered, and with 1 % of the rows excluded"""
    import torch
    c = exact_launches_case
    idx, q, k = c["idx"], c["q"][:nq], c["k"]
    if filtered:
        qd, td, ed = (torch.from_numpy(a).to(gpu) for a in (q, c["tags"], c["excl"]))
        D, I = (t.cpu().numpy() for t in idx.search_probed_excluding(qd, k, td, ed))
        od, oi = c["filtered"]
        assert not np.isin(I, c["excl"]).any()
    else:
        D, I = idx.search(q, k)
        od, oi = c["plain"]
    info = idx.last_search_info()
    assert info["scan"] == "hi_lists" and info["rejected"] == nq and info["exact"] == nq, info
    np.testing.assert_array_equal(I, oi[:nq])
    np.testing.assert_allclose(D, od[:nq], rtol=1e-6, atol=1e-5)
