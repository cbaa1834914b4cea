"""GPU parity: libradad_hip.so's store + brute-force top-k against the float64 oracle.
Bar: neighbour ids bit-exact (ties -> lower id), distances within 1e-4 absolute on unit-norm data /
1e-4 relative on raw L2 (fp32 cannot do better than ~2e-7 relative on |x|^2 ~ 512)."""
import os

import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu


def _mk(gpu, metric, dim, id_base=0, **options):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    return HipFlatIndex(dim, m, gpu.index or 0, id_base, **options)


def _check(D, I, od, oi, metric, unit):
    np.testing.assert_array_equal(I, oi)
    if unit:
        np.testing.assert_allclose(D, od, rtol=0, atol=1e-4)      # north_star: 1e-4 absolute on unit-norm data
    else:
        np.testing.assert_allclose(D, od, rtol=1e-6, atol=1e-6)   # raw data: distances are float64 re-scored, so ~1 ulp


def _assert_separated(od, D):
    """the final order comes from a float64 re-rank, so ids must match the oracle whenever the oracle itself has no
    exact tie between different rows (ties are covered by test_knn_ties_break_to_lower_id)"""
    assert O.rank_gaps(od).min() > 0, "the seed produced an exact float64 tie; pick another seed"


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("n,nq,dim,k", [(10000, 16, 512, 15), (3001, 129, 256, 10), (777, 1, 64, 5), (50000, 300, 512, 10)])
def test_knn_matches_oracle(gpu, metric, n, nq, dim, k):
    db = synth.rows(0, n, dim, 4321)
    q = synth.rows(0, nq, dim, 977)
    # plant near-duplicates of each query so that top-k is not trivial
    for j in range(nq):
        for c in range(3):
            db[(j * 7 + c * 131) % n] = q[j] + np.float32(0.05 * (c + 1)) * synth.rows(j * 3 + c, 1, dim, 55)[0]
    idx = _mk(gpu, metric, dim)
    idx.add(db[: n // 2])
    idx.add(db[n // 2:])                    # append path: two batches
    assert idx.ntotal == n
    D, I = idx.search(q, k)
    od, oi = O.knn(db, q, k, metric)
    _check(D, I, od, oi, metric, unit=(metric == "COSINE"))
    _assert_separated(od, D)


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("n,nq,dim,k", [(3000, 40, 5376, 15),      # the reference's own D (7 x 768) and k_search = K + 10
                                        (4000, 130, 100, 12),      # dim not a multiple of 32: generic kernel, K tail
                                        (6000, 70, 64, 40),        # k + margin > 32: lists in the partial arrays
                                        (2500, 9, 96, 30),         # small batch with k too large for the streaming kernel
                                        (5000, 16, 2048, 10),      # streaming kernel at its largest dim
                                        (5000, 3, 4096, 10)])      # small batch, dim beyond the streaming kernel
@pytest.mark.parametrize("split", [1, 0])
def test_knn_kernel_variants(gpu, split, metric, n, nq, dim, k):
    """dispatch branches of radad_knn_search on small stores: fp32 tile kernel with register lists (16/32), generic tile
    kernel, streaming small-batch kernel -- each followed by the certified float64 re-rank (the hi_plane option only matters for
    stores of >= 16384 rows: test_knn_wide_kernel)"""
    db = synth.rows(0, n, dim, 1001)
    q = synth.rows(0, nq, dim, 1002)
    for j in range(nq):
        db[(j * 13 + 5) % n] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 1003)[0]
    idx = _mk(gpu, metric, dim)
    idx.add(db)
    D, I = idx.search(q, k)
    od, oi = O.knn(db, q, k, metric)
    _check(D, I, od, oi, metric, unit=(metric == "COSINE"))


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("n,nq,dim,k,f16", [(40000, 257, 128, 10, False),   # ragged query tile
                                            (40000, 700, 512, 15, False),   # reference k_search = 15: 16-entry lists + certificate
                                            (33000, 130, 64, 24, False),    # one K step per tile
                                            (33000, 300, 64, 10, True),     # fp16 store through the same kernel
                                            (33000, 140, 64, 15, True),     # fp16 store, k = 15
                                            (1000, 513, 128, 3, False)])    # too few rows for the certified scan: fp32 tile kernel
def test_knn_wide_kernel(gpu, metric, n, nq, dim, k, f16):
    """> 16 queries on >= 16384 rows: the certified 256 x 256 tile scan on the f16 matrix pipe (knn_hi.inc) -- f16 hi plane
    of an fp32 store (per-row power-of-two scales, one scale for cosine), or the fp16 store itself.  It only filters; ids
    must still equal the float64 oracle."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    db = synth.rows(0, n, dim, 2001)
    q = synth.rows(0, nq, dim, 2002)
    # rows of very different magnitude (the per-row scale has to cope) -- not for cosine, where rows are normalised anyway
    if metric != "COSINE" and not f16:
        db *= np.exp2(np.arange(n) % 23 - 11).astype(np.float32)[:, None]
        q *= np.exp2(np.arange(nq) % 7 - 3).astype(np.float32)[:, None]
    for j in range(nq):
        db[(j * 17 + 3) % n] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 2003)[0]
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    idx = HipFlatIndex(dim, m, 0, 0, store_f16=f16)
    idx.add(db[: n // 3])
    D0, I0 = idx.search(q, k)                      # builds the split copy of the first third
    idx.add(db[n // 3:])                           # appended rows: only they are split on the next search
    D, I = idx.search(q, k)
    # judged on the rows AS STORED (normalised / rounded to fp16 by the add kernel): reconstruct is bit-exact
    import torch
    rec = idx.reconstruct_batch(torch.arange(n, device=gpu)).cpu().numpy()
    om = "IP" if metric == "COSINE" else metric
    qq = q.astype(np.float64)
    if metric == "COSINE":
        qq = qq / np.sqrt((qq ** 2).sum(1))[:, None]           # ranking does not depend on the query's scale
    od, oi = O.knn(rec, qq, k, om)
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-5, atol=1e-5)
    od3, oi3 = O.knn(rec[: n // 3], qq, k, om)
    np.testing.assert_array_equal(I0, oi3)
    # (rows scaled over 2^22 make the per-store error bound useless for the small rows: the certificate rejects many queries,
    # they go through the exact kernel and the next searches stay on the fp32 kernels -- still exact, asserted above)
    scaled = metric != "COSINE" and not f16
    if not scaled:
        assert idx.last_launch()["block_threads"] == (512 if n >= 33000 else 256)


def test_knn_wide_kernel_equals_fp32_tile_kernel(gpu):
    """hi_plane=0 (radad_knn_set_option) keeps an fp32 store on the fp32 tile kernel; both paths return identical ids and
    distances (the float64 re-rank decides both)."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    n, nq, dim, k = 20000, 400, 256, 10
    db = synth.rows(0, n, dim, 2101)
    q = synth.rows(0, nq, dim, 2102)
    res = []
    for flag in (1, 0):
        idx = HipFlatIndex(dim, _lib.METRIC_L2, 0, 0, hi_plane=flag)
        idx.add(db)
        res.append(idx.search(q, k) + (idx.last_launch()["block_threads"],))
    assert (res[0][2], res[1][2]) == (512, 256)
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0], res[1][0])


def test_knn_empty_store(gpu):
    idx = _mk(gpu, "L2", 32)
    D, I = idx.search(synth.rows(0, 3, 32, 1), 4)
    assert np.all(I == -1) and np.all(np.isinf(D)) and idx.ntotal == 0


def test_knn_device_tensors_and_reconstruct(gpu):
    import torch
    n, dim, k = 5000, 128, 8
    db = synth.rows(0, n, dim, 11)
    q = synth.rows(0, 40, dim, 12)
    idx = _mk(gpu, "COSINE", dim)
    idx.add_device(torch.from_numpy(db).to(gpu))
    D, I = idx.search_device(torch.from_numpy(q).to(gpu), k)
    od, oi = O.knn(db, q, k, "COSINE")
    _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, "COSINE", True)
    # reconstruct returns the STORED (normalised) row (pipeline.py:503), zeros for id -1
    ids = torch.tensor([[0, 17, -1], [4999, 5000, 3]], device=gpu)
    rec = idx.reconstruct_batch(ids).cpu().numpy()
    nd, bound = O.stored_rows_err(db)              # the float64 value and the bound derived from the kernel's arithmetic (a few ulp)
    for got, r in ((rec[0, 0], 0), (rec[0, 1], 17), (rec[1, 0], 4999), (idx.reconstruct(3), 3)):
        assert np.all(np.abs(got - nd[r]) <= bound[r]), f"row {r}"
    assert np.all(rec[0, 2] == 0) and np.all(rec[1, 1] == 0)


def test_knn_ties_break_to_lower_id(gpu):
    dim = 64
    base = synth.rows(0, 200, dim, 3)
    db = np.concatenate([base, base[:50], base[:50]])          # every row of base[:50] appears three times
    for metric in ("L2", "IP"):
        idx = _mk(gpu, metric, dim)
        idx.add(db)
        D, I = idx.search(base[:50], 3)
        if metric == "L2":
            want = np.stack([np.arange(50), 200 + np.arange(50), 250 + np.arange(50)], 1)
            np.testing.assert_array_equal(I, want)
            assert np.all(D < 1e-3)
        else:
            od, oi = O.knn(db, base[:50], 3, "IP")
            np.testing.assert_array_equal(I, oi)


def test_knn_k_larger_than_ntotal_and_small_stores(gpu):
    dim = 32
    db = synth.rows(0, 5, dim, 8)
    q = synth.rows(0, 3, dim, 9)
    for metric in ("L2", "IP"):
        idx = _mk(gpu, metric, dim)
        idx.add(db)
        D, I = idx.search(q, 8)
        od, oi = O.knn(db, q, 5, metric)
        np.testing.assert_array_equal(I[:, :5], oi)
        assert np.all(I[:, 5:] == -1)                       # faiss fills missing results with -1
        assert np.all(np.isinf(D[:, 5:])) and np.all((D[:, 5:] > 0) == (metric == "L2"))


def test_knn_id_base_and_merge_equals_unsharded(gpu):
    """two shards with global ids + radad_topk_merge == one store (the multi-GPU path on one GPU)"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge, shard_bounds
    n, dim, k, nq = 9001, 128, 10, 37
    db = synth.rows(0, n, dim, 21)
    q = synth.rows(0, nq, dim, 22)
    for metric in ("L2", "COSINE"):
        parts_d, parts_i = [], []
        for r in range(3):
            lo, hi = shard_bounds(n, 3, r)
            idx = _mk(gpu, metric, dim, id_base=lo)
            idx.add(db[lo:hi])
            d, i = idx.search_device(torch.from_numpy(q).to(gpu), k)
            parts_d.append(d); parts_i.append(i)
        md, mi = hip_merge(idx.metric, torch.stack(parts_d), torch.stack(parts_i), k)
        od, oi = O.knn(db, q, k, metric)
        _check(md.cpu().numpy(), mi.cpu().numpy(), od, oi, metric, unit=(metric == "COSINE"))


def test_sharded_f64_merge_with_certified_lists(gpu):
    """the multi-GPU path on one GPU at k = 15 (certified scan inside every shard): three shards with global ids, float64 keys
    merged by radad_topk_merge_f64 == one store; one query's neighbours are 30 adjacent rows of a single shard (the 16-entry
    chunk lists of rounds 1-2 had to send that query to the exact kernel; the emit-mode scan lists them all and certifies it)"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge, shard_bounds
    n, dim, k, nq = 90000, 64, 15, 200
    db = synth.rows(0, n, dim, 5021)
    q = synth.rows(0, nq, dim, 5022)
    for t in range(30):
        db[40010 + t] = q[11] + np.float32(0.02 + 0.001 * t) * synth.rows(t, 1, dim, 5023)[0]
    keys, ids, rechecked = [], [], 0
    for r in range(3):
        lo, hi = shard_bounds(n, 3, r)
        idx = _mk(gpu, "L2", dim, id_base=lo)
        idx.add(db[lo:hi])
        d, i, k64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
        rechecked += idx.last_launch()["rechecked_queries"]
        keys.append(k64); ids.append(i)
    assert rechecked == 0
    md, mi = hip_merge(idx.metric, torch.stack(keys), torch.stack(ids), k)
    od, oi = O.knn(db, q, k, "L2")
    np.testing.assert_array_equal(mi.cpu().numpy(), oi)
    np.testing.assert_allclose(md.cpu().numpy(), od, rtol=1e-5, atol=1e-5)


def test_knn_save_load_roundtrip(gpu, tmp_path):
    dim = 64
    db = synth.rows(0, 1234, dim, 31)
    q = synth.rows(0, 9, dim, 32)
    for metric in ("L2", "COSINE"):
        a = _mk(gpu, metric, dim)
        a.add(db)
        p = str(tmp_path / f"{metric}.bin")
        a.save(p)
        b = _mk(gpu, metric, dim)
        b.load(p)
        assert b.ntotal == 1234
        Da, Ia = a.search(q, 6)
        Db, Ib = b.search(q, 6)
        np.testing.assert_array_equal(Ia, Ib)
        np.testing.assert_array_equal(Da, Db)
    with pytest.raises(OSError):
        _mk(gpu, "L2", 32).load(p)          # dim mismatch


def test_knn_argument_errors(gpu):
    with pytest.raises(ValueError):
        _mk(gpu, "L2", 30)                   # dim must be a multiple of 4
    idx = _mk(gpu, "L2", 32)
    idx.add(synth.rows(0, 10, 32, 1))
    with pytest.raises(ValueError):
        idx.search(synth.rows(0, 2, 32, 1), 0)
    with pytest.raises(ValueError):
        idx.search(synth.rows(0, 2, 16, 1), 3)


def test_vector_database_surface(gpu, tmp_path):
    """VectorDatabase mirrors vector_database.py: index types, cosine normalisation, k clamp, empty DB, save/load."""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, vector_db_path=str(tmp_path / "vdb"), vector_db_index_type="IP", vector_add_batch_size=300)
    vdb = R.VectorDatabase(cfg)
    with pytest.raises(ValueError):
        vdb.search_batch(np.zeros((1, 8), np.float32))          # vector_database.py:160-161
    db = synth.rows(0, 1000, 64, 41)
    paths = [f"/d/f{i}.wav" for i in range(1000)]
    vdb.add_vectors(db, paths, list(range(1000)), {"speaker_id": [f"s{i % 7}" for i in range(1000)]})
    assert vdb.index.ntotal == 1000 and len(vdb.vector_paths) == 1000 and vdb.vector_metadata["speaker_id"][999] == "s5"
    q = synth.rows(0, 4, 64, 42)
    D, I = vdb.search_batch(q, k=5)
    od, oi = O.knn(db, q, 5, "COSINE")
    assert D.dtype == np.float32 and I.dtype == np.int64
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, atol=1e-4)
    d1, i1 = vdb.search(q[0], k=5)                               # 1-D query (vector_database.py:164-165,185-188)
    np.testing.assert_array_equal(i1, oi[0])
    assert vdb.search_batch(q, k=5000)[1].shape == (4, 1000)     # k clamped to ntotal (:169)
    vdb.save()
    v2 = R.VectorDatabase(cfg)
    v2.load()
    assert v2.index.ntotal == 1000 and v2.vector_paths == paths
    np.testing.assert_array_equal(v2.search_batch(q, k=5)[1], oi)
    cfg.vector_db_index_type = "bogus"
    with pytest.raises(ValueError):
        R.VectorDatabase(cfg).create_index(8)                   # vector_database.py:72


def test_filter_topk_kernel(gpu, tmp_path):
    """radad_filter_topk == the exclusion loop of pipeline.py:491-515 on ids"""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    cfg = R.Config()
    cfg.update(device=gpu, vector_db_path=str(tmp_path / "v"))
    vdb = R.VectorDatabase(cfg)
    n = 50
    paths = [f"/a/b/f{i % 40}.wav" for i in range(n)]          # f0..f9 appear twice: duplicates of a basename share a tag
    vdb.add_vectors(synth.rows(0, n, 32, 3), paths, [i % 2 for i in range(n)], {})
    assert vdb.row_tags_device().cpu().tolist() == [path_tag(p) for p in paths]
    assert path_tag("/x/y/f3.wav") == path_tag("f3.wav") != path_tag("f4.wav")
    idxs = torch.tensor([[3, 43, 7, -1, 9, 12], [0, 1, 2, 3, 4, 5], [40, 41, 42, 43, 44, 45]], device=gpu)
    dists = torch.arange(18, dtype=torch.float32, device=gpu).reshape(3, 6)
    excl = torch.tensor(sorted({path_tag("f3.wav"), path_tag("f9.wav"), path_tag("f1.wav")}), device=gpu)
    d, i = vdb.filter_hits(dists, idxs, 3, excl)
    assert i.cpu().tolist() == [[7, 12, -1], [0, 2, 4], [40, 42, 44]]          # row 43 is f3.wav again; -1 is skipped
    dd = d.cpu().numpy()
    assert dd[0, 0] == 2 and dd[0, 1] == 5 and np.isnan(dd[0, 2]) and dd[1].tolist() == [6, 8, 10]
    d, i = vdb.filter_hits(dists, idxs, 4, None)                                # no exclusion set
    assert i.cpu().tolist()[0] == [3, 43, 7, 9]
    d, i = vdb.filter_hits(dists[:, :0], idxs[:, :0], 2, excl)                  # no hits at all -> padding
    assert i.cpu().tolist() == [[-1, -1]] * 3 and bool(torch.isnan(d).all())


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("n,nq,dim,k", [(20000, 200, 512, 10),     # fp16 MFMA tile kernel (dim % 64 == 0), 16-entry lists
                                        (9000, 129, 256, 20),      # 32-entry lists
                                        (5000, 7, 512, 10),        # small batch on an fp16 store: tile kernel
                                        (4000, 60, 96, 10),        # dim % 64 != 0: decoded to fp32 while staging
                                        (4000, 60, 128, 40)])      # k too large for register lists: generic kernel
def test_fp16_store(gpu, metric, n, nq, dim, k):
    """config.use_float16 (vector_database.py:80): rows rounded to fp16 on add; ranking = float64 over the DECODED rows
    with the fp32 queries, so ids must equal the oracle run on exactly those rows"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    lib = _lib.load()
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    db = synth.rows(0, n, dim, 2001)
    q = synth.rows(0, nq, dim, 2002)
    for j in range(nq):
        db[(j * 17 + 3) % n] = q[j] + np.float32(0.2) * synth.rows(j, 1, dim, 2003)[0]
    idx = HipFlatIndex(dim, m, gpu.index or 0, store_f16=True)
    idx.add(db[: n // 3])
    idx.add_device(torch.from_numpy(db[n // 3:]).to(gpu))
    stored = idx.reconstruct_batch(torch.arange(n, device=gpu)).cpu().numpy()          # decoded fp16 rows
    assert np.array_equal(stored, stored.astype(np.float16).astype(np.float32))         # every value is an fp16 number
    if metric == "COSINE":      # one fp16 rounding (2^-11 relative, 2^-25 absolute among the subnormals) of a value within the model's bound
        exact, bound = O.stored_rows_err(db)
        assert np.all(np.abs(stored - exact) <= bound + 2.0 ** -11 * (np.abs(exact) + bound) + 2.0 ** -25)
    else:                       # round-to-nearest-even of the input, bit for bit (tests/test_gpu_store_contents.py has the tie cases)
        np.testing.assert_array_equal(stored, O.stored_rows(db, metric, f16=True).astype(np.float32))
    qt = torch.from_numpy(q).to(gpu)
    if metric == "COSINE":
        qn = torch.empty_like(qt)
        _lib.check(lib.radad_rownorm(qt.data_ptr(), qn.data_ptr(), nq, dim, gpu.index or 0, _lib.stream_ptr(gpu)))
        q_used = qn.cpu().numpy()
    else:
        q_used = q
    D, I = idx.search(q, k)
    od, oi = O.knn(stored, q_used, k, "L2" if metric == "L2" else "IP")
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(idx.reconstruct(5), stored[5], rtol=0, atol=0)


def test_fp16_store_save_load_and_config(gpu, tmp_path):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, vector_db_path=str(tmp_path / "vdb16"), vector_db_index_type="L2", use_float16=True)
    vdb = R.VectorDatabase(cfg)
    db = synth.rows(0, 3000, 64, 2101)
    vdb.add_vectors(db, [f"f{i}.wav" for i in range(3000)], [0] * 3000, {})
    assert vdb.index.store_f16
    q = synth.rows(0, 20, 64, 2102)
    D, I = vdb.search_batch(q, k=7)
    vdb.save()
    v2 = R.VectorDatabase(cfg)
    v2.load()
    D2, I2 = v2.search_batch(q, k=7)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)
    cfg.use_float16 = False
    v3 = R.VectorDatabase(cfg)
    v3.load()                                   # dtype mismatch is logged and leaves the store empty (log-and-degrade)
    assert v3.index is None or v3.index.ntotal == 0


def test_load_store_written_in_faiss_flat_layout(gpu, tmp_path):
    """VectorDatabase.load() also accepts `faiss_index.bin` in faiss' IndexFlat on-disk layout (the file the reference
    writes, vector_database.py:203).  faiss is absent here, so this only round-trips our own writer of that layout."""
    import pickle
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import read_faiss_flat, write_faiss_flat
    cfg = R.Config()
    cfg.update(device=gpu, vector_db_path=str(tmp_path / "ref_vdb"), vector_db_index_type="L2")
    db = synth.rows(0, 2000, 64, 3001)
    os.makedirs(cfg.vector_db_path, exist_ok=True)
    write_faiss_flat(os.path.join(cfg.vector_db_path, "faiss_index.bin"), db, "L2")
    m, d, rows = read_faiss_flat(os.path.join(cfg.vector_db_path, "faiss_index.bin"))
    assert (m, d) == ("L2", 64) and np.array_equal(rows, db)
    paths = [f"p{i}.wav" for i in range(2000)]
    with open(os.path.join(cfg.vector_db_path, "metadata.pkl"), "wb") as f:       # the reference's metadata (vector_database.py:205-213)
        pickle.dump({"paths": paths, "labels": [0] * 2000, "metadata": {}, "index_type": "L2", "dimension": 64}, f)
    vdb = R.VectorDatabase(cfg)
    vdb.load()
    assert vdb.index.ntotal == 2000 and vdb.vector_paths == paths
    q = synth.rows(0, 11, 64, 3002)
    D, I = vdb.search_batch(q, k=6)
    od, oi = O.knn(db, q, 6, "L2")
    np.testing.assert_array_equal(I, oi)
    with pytest.raises(ValueError):
        read_faiss_flat(os.path.join(cfg.vector_db_path, "metadata.pkl"))


@pytest.mark.parametrize("store_f16", [False, True])
def test_snapshot_loaded_as_row_shards(gpu, tmp_path, store_f16):
    """one snapshot file, loaded as 3 row shards (each handle reads only its byte range, global ids via
    id_base); merged shard results == the single-store search; whole-file load == original rows bit for bit."""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge, shard_bounds
    n, d, k = 5003, 96, 7
    rows = torch.from_numpy(synth.rows(0, n, d, 808)).to(gpu)
    q = torch.from_numpy(synth.rows(0, 33, d, 809)).to(gpu)
    full = R.HipFlatIndex(d, _lib.METRIC_L2, device=0, store_f16=store_f16)
    full.add_device(rows)
    path = str(tmp_path / "store.radad")
    full.save(path)
    info = R.HipFlatIndex.snapshot_info(path)
    assert info == {"d": d, "metric": _lib.METRIC_L2, "store_f16": store_f16, "ntotal": n}
    assert os.path.getsize(path) == 32 + n * d * (2 if store_f16 else 4)
    D0, I0, K0 = full.search_device(q, k, return_f64=True)
    again = R.HipFlatIndex(d, _lib.METRIC_L2, device=0, store_f16=store_f16)
    again.load(path)
    ids = torch.arange(n, device=gpu)
    assert torch.equal(again.reconstruct_batch(ids), full.reconstruct_batch(ids))
    parts = [R.HipFlatIndex.load_shard(path, r, 3, device=0) for r in range(3)]
    assert [p.ntotal for p in parts] == [hi - lo for lo, hi in (shard_bounds(n, 3, r) for r in range(3))]
    res = [p.search_device(q, k, return_f64=True) for p in parts]
    Dm, Im = hip_merge(_lib.METRIC_L2, torch.stack([r[2] for r in res]), torch.stack([r[1] for r in res]), k)
    assert torch.equal(Im, I0)
    np.testing.assert_allclose(Dm.cpu().numpy(), D0.cpu().numpy(), rtol=1e-6)
    lo, hi = shard_bounds(n, 3, 1)
    assert torch.equal(parts[1].reconstruct_batch(torch.arange(lo, hi, device=gpu)), full.reconstruct_batch(torch.arange(lo, hi, device=gpu)))
    with pytest.raises(ValueError, match="outside the snapshot"):
        again.load(path, n - 5, 6)
    empty = R.HipFlatIndex(d, _lib.METRIC_L2, device=0, store_f16=store_f16)
    empty.load(path, 17, 0)
    assert empty.ntotal == 0
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 4)
    with pytest.raises(OSError, match="truncated"):
        again.load(path)


def test_load_into_used_store_refreshes_split_copy(gpu, tmp_path):
    """load() replaces the rows of a store that has already scanned a large batch (its f16 hi plane exists and the
    capacity suffices, so nothing is reallocated): the plane must follow the new rows."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    n, nq, dim, k = 20000, 300, 128, 10
    a_rows, b_rows = synth.rows(0, n, dim, 3101), synth.rows(0, n, dim, 3102)
    q = synth.rows(0, nq, dim, 3103)
    src = HipFlatIndex(dim, _lib.METRIC_IP, 0, 0)
    src.add(b_rows)
    path = str(tmp_path / "b.radad")
    src.save(path)
    idx = HipFlatIndex(dim, _lib.METRIC_IP, 0, 0)
    idx.add(a_rows)
    Da, Ia = idx.search(q, k)                               # builds the split copy of A
    np.testing.assert_array_equal(Ia, O.knn(a_rows, q, k, "IP")[1])
    idx.load(path)                                          # same size, same capacity: rows replaced in place
    Db, Ib = idx.search(q, k)
    np.testing.assert_array_equal(Ib, O.knn(b_rows, q, k, "IP")[1])
    assert idx.last_launch()["block_threads"] == 512


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_knn_truncated_lists_recheck(gpu, metric):
    """queries whose best rows are CLUSTERED in the store (30 near-duplicates stored contiguously -- a clip's augmentations, a
    speaker's utterances).  Rounds 1-2 kept 16 candidates per store chunk: such a query used up its chunk's list, could not be
    certified and went through the exact float64 kernel.  The emit-mode scan lists every row at or above the floor wherever it
    sits: all queries are certified, none takes the exact kernel."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    n, nq, dim, k = 60000, 300, 64, 15
    db = synth.rows(0, n, dim, 4101)
    q = synth.rows(0, nq, dim, 4102)
    clustered = [3, 77, 150, 299]
    bases = [1030, 6000, 11010, 16130]                      # each cluster inside one 256-row chunk of the scan
    for c, j in enumerate(clustered):                       # 30 consecutive rows around query j
        base = bases[c]
        for t in range(30):
            db[base + t] = q[j] + np.float32(0.02 + 0.001 * t) * synth.rows(base + t, 1, dim, 4103)[0]
    m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
    idx = HipFlatIndex(dim, m, 0, 0)
    idx.add(db)
    D, I = idx.search(q, k)
    info = idx.last_launch()
    assert info["block_threads"] == 512
    assert info["rechecked_queries"] == 0, info
    od, oi = O.knn(db, q, k, metric)
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-5, atol=1e-5)
    for c, j in enumerate(clustered):
        assert set(I[j]) <= set(range(bases[c], bases[c] + 30))
    D10, I10 = idx.search(q, 10)
    np.testing.assert_array_equal(I10, oi[:, :10])
    assert idx.last_launch()["rechecked_queries"] <= len(clustered) + 12


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("f16", [False, True])
def test_small_batch_on_the_f16_plane(gpu, metric, f16):
    """<= 16 queries on a store of >= 16384 rows stream the f16 plane (k_knn_hi_smallq) and are certified like the tile scan; the
    same store with the plane switched off (hi_plane=0 at creation) streams the fp32 rows: both are the float64 brute force."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    n, dim, k = 40000, 128, 15
    db = synth.rows(0, n, dim, 8801)
    q = synth.rows(0, 16, dim, 8802)
    for j in range(16):
        db[(j * 2003 + 9) % n] = q[j] + np.float32(0.03) * synth.rows(j, 1, dim, 8803)[0]
    idx = HipFlatIndex(dim, m, 0, store_f16=f16)
    idx.add(db)
    ref = HipFlatIndex(dim, m, 0, store_f16=f16, hi_plane=0)
    ref.add(db)
    for nq in (1, 5, 16):
        D, I = idx.search(q[:nq], k)
        assert idx.last_launch()["scan_kind"] == "hi_smallq"
        Dr, Ir = ref.search(q[:nq], k)
        assert ref.last_launch()["scan_kind"] in ("f32_smallq", "f16_tile")
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_allclose(D, Dr, rtol=1e-6, atol=1e-6)
        assert idx.last_launch()["certificate"]["queries"] == nq
    import torch
    stored = idx.reconstruct_batch(torch.arange(n, device=gpu)).cpu().numpy().astype(np.float32)
    if metric == "COSINE":
        qt = torch.from_numpy(q).to(gpu); qo = torch.empty_like(qt)
        _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), qo.data_ptr(), 16, dim, 0, _lib.stream_ptr(gpu)))
        _, oi = O.knn(stored, qo.cpu().numpy(), k, "IP")
    else:
        _, oi = O.knn(stored, q, k, metric)
    np.testing.assert_array_equal(idx.search(q, k)[1], oi)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_full_size_properties(gpu, metric):
    """BASELINE's store size (1 M x 512) through size-independent properties: every stored row retrieves ITSELF first (distance 0 /
    similarity 1), lists are sorted, ids are distinct and in range, a second search gives the same bits, and the certificate
    rejects nothing on this data."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    lib = _lib.load()
    n, dim, k, nq = 1_000_000, 512, 10, 2048
    m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
    rows = torch.empty((n, dim), device=gpu)
    _lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, n, dim, 777, 0, _lib.stream_ptr(gpu)))
    idx = HipFlatIndex(dim, m, 0)
    idx.reserve(n)
    idx.add_device(rows)
    pick = (torch.arange(nq, device=gpu) * 487 + 13) % n
    q = rows[pick].contiguous()
    del rows
    D, I = idx.search_device(q, k)
    info = idx.last_launch()
    assert info["scan_kind"] == "hi_tile" and info["certificate"]["rejected"] == 0, info
    assert torch.equal(I[:, 0], pick)
    if metric == "L2":
        assert float(D[:, 0].abs().max()) < 1e-6 and bool((D[:, 1:] >= D[:, :-1]).all())
    else:
        assert float((D[:, 0] - 1).abs().max()) < 1e-5 and bool((D[:, 1:] <= D[:, :-1]).all())
    assert int(I.min()) >= 0 and int(I.max()) < n
    srt = I.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())                      # distinct ids per query
    D2, I2 = idx.search_device(q, k)
    assert torch.equal(I2, I) and torch.equal(D2, D)


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("k", [40, 64, 128])
def test_large_k_stays_on_the_certified_f16_scan(gpu, metric, k):
    """faiss accepts k up to 2048 (vector_database.py:169-181); up to k = 128 the certified f16 tile scan serves it (its candidate
    buffers are sized from k; rounds 1-2 fell to the 8x slower fp32 kernels above k = 26).  ids == the float64 brute force."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    n, nq, dim = 50000, 200, 512
    db = synth.rows(0, n, dim, 9101)
    q = synth.rows(0, nq, dim, 9102)
    for j in range(nq):                                     # 60 near-duplicates per query, 20 of them adjacent in the store
        for t in range(40):
            db[(j * 211 + t * 1237 + 3) % n] = q[j] + np.float32(0.02 + 0.002 * t) * synth.rows(j * 64 + t, 1, dim, 9103)[0]
    for j in range(0, nq, 10):
        for t in range(20):
            db[(j * 97 + 40000 + t) % n] = q[j] + np.float32(0.03 + 0.002 * t) * synth.rows(j * 64 + 40 + t, 1, dim, 9103)[0]
    m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
    idx = HipFlatIndex(dim, m, 0, 0)
    idx.add(db)
    D, I = idx.search(q, k)
    info = idx.last_launch()
    assert info["scan_kind"] == "hi_tile" and info["certificate"]["rejected"] <= nq // 100, info
    import torch
    stored = idx.reconstruct_batch(torch.arange(n, device=gpu)).cpu().numpy()
    qq = q
    if metric == "COSINE":        # the ranking is defined on the queries as the index normalises them (fp32, vector_database.py:166);
        qt = torch.from_numpy(q).to(gpu); qo = torch.empty_like(qt)           # checked against float64 numpy to 1e-6
        _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), qo.data_ptr(), nq, dim, 0, _lib.stream_ptr(gpu)))
        qq = qo.cpu().numpy()
        np.testing.assert_allclose(qq, q.astype(np.float64) / np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None], rtol=0, atol=1e-6)
    od, oi = O.knn(stored, qq, k, "IP" if metric == "COSINE" else "L2")
    assert O.rank_gaps(od).min() > 0
    np.testing.assert_array_equal(I, oi)
    np.testing.assert_allclose(D, od, rtol=1e-5, atol=1e-5)


def test_searches_alternating_between_streams_share_the_workspace_safely(gpu):
    """one handle, two streams, searches enqueued alternately without any host synchronisation in between: they share the handle's
    workspace, so a search on another stream than the previous one must wait for it (an event recorded behind the previous stream
    when the next search arrives; none at all on one stream).  Results == the same searches done one at a time; flat and IVF."""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    n, dim, k = 60000, 128, 10
    db = torch.from_numpy(synth.rows(0, n, dim, 9101)).to(gpu)
    qs = [torch.from_numpy(synth.rows(0, nq, dim, 9110 + i)).to(gpu) for i, nq in enumerate((300, 1, 700, 16, 40, 1000))]
    flat = HipFlatIndex(dim, _lib.METRIC_L2, 0)
    flat.add_device(db)
    ivf = R.HipIVFFlatIndex(dim, 64, 0)
    ivf.train(db[:10000].cpu().numpy())
    ivf.add(db.cpu().numpy())
    ivf.nprobe = 8
    for index in (flat, ivf):
        want = []
        for q in qs:
            D, I = index.search_device(q, k)
            want.append((D.clone(), I.clone()))
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
        for rep in range(3):
            got = []
            for i, q in enumerate(qs):
                with torch.cuda.stream(streams[(i + rep) & 1]):
                    got.append(index.search_device(q, k))
            torch.cuda.synchronize()
            for (D, I), (Dw, Iw) in zip(got, want):
                assert torch.equal(I, Iw) and torch.equal(D, Dw)
