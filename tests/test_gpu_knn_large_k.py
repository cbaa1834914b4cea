"""Flat searches with 128 < k <= RADAD_KNN_MAX_K = 1024 against the float64 C oracle (oracle/knn_oracle.c) over the rows AS STORED.

The reference hands any k to an exact faiss flat search (vector_database.py:163-181); so must this build.  Above k = 128 the
certified f16 scans do not run: the fp32 tile kernels filter, the float64 re-rank decides, the per-query certificate checks that
no unlisted row can reach the k-th, and the exact float64 kernel searches the queries it rejects.  Every case checks ids (exact),
fp32 distances (1e-5) and, where asked for, the float64 keys (1e-12 relative), and that the search was certified."""
import os

import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

def _mk(metric, dim, f16=False, id_base=0):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    return HipFlatIndex(dim, m, 0, id_base, store_f16=f16)


def _stored(idx, n, gpu):
    import torch
    out = []
    for r0 in range(0, n, 1 << 17):
        ids = torch.arange(idx.id_base + r0, idx.id_base + min(n, r0 + (1 << 17)), device=gpu)
        out.append(idx.reconstruct_batch(ids).cpu().numpy())
    return np.concatenate(out) if out else np.zeros((0, idx.d), np.float32)


def _gpu_unit(q, gpu):
    """the queries normalised by the library's own fp32 row normalisation (what a cosine search ranks with)"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    qt = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(gpu)
    qo = torch.empty_like(qt)
    _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), qo.data_ptr(), qt.shape[0], qt.shape[1], 0, _lib.stream_ptr(gpu)))
    return qo.cpu().numpy()


def _oracle(lib, stored, q, k, metric, gpu, id_base=0):
    """(od, oi, qq): float64 brute force over the stored rows; qq = the fp32 queries the oracle ranked with"""
    from conftest import c_knn
    qq = _gpu_unit(q, gpu) if metric == "COSINE" else np.ascontiguousarray(q, np.float32)
    od, oi = c_knn(lib, stored, qq, k, "L2" if metric == "L2" else "IP", id_base)
    return od, oi, qq


def _check(D, I, od, oi, stored, qq, metric, id_base=0, K64=None, ctx=None):
    """ids equal to the oracle's (cosine: or equal float64 score multisets within 1e-7, as test_gpu_fuzz does); fp32 distances
    to 1e-5; float64 keys to 1e-12 relative; unfilled slots -1 / +-inf"""
    D, I = np.asarray(D), np.asarray(I)
    filled = oi >= 0
    ok = np.array_equal(I, oi)
    if not ok and metric == "COSINE":
        sc = lambda ids, j: np.sort(stored[ids[ids >= 0] - id_base].astype(np.float64) @ qq[j].astype(np.float64))[::-1]
        ok = np.array_equal(I < 0, ~filled) and all(np.allclose(sc(I[j], j), sc(oi[j], j), rtol=0, atol=1e-7) for j in range(len(I)))
    assert ok, dict(ctx or {}, bad_rows=np.flatnonzero((I != oi).any(1))[:10].tolist())
    np.testing.assert_allclose(D[filled], od[filled], rtol=1e-5, atol=1e-5)
    tail = np.inf if metric == "L2" else -np.inf
    assert np.all(D[~filled] == tail) and np.all(I[~filled] == -1)
    if K64 is not None:
        K64 = np.asarray(K64)
        same = I == oi
        scale = max(1.0, float(np.abs(od[filled]).max())) if filled.any() else 1.0
        np.testing.assert_allclose(K64[same & filled], od[same & filled], rtol=1e-12, atol=1e-12 * scale)
        assert np.all(K64[~filled] == tail)


def _certified(idx, nq):
    info = idx.last_launch()
    assert info["certificate"]["queries"] == nq, info
    return info


# ---- (a) plain parity grid -----------------------------------------------------------------------------------------------------
_GRID_N, _GRID_DIM, _GRID_NQ, _GRID_K = 50000, 512, 300, 1024


@pytest.fixture(scope="module")
def grid_store(gpu, knn_oracle_lib):
    """one store per (metric, store dtype) and the oracle's top 1024 of 300 queries over it; smaller k and batches are prefixes"""
    cache = {}

    def get(metric, f16):
        if (metric, f16) not in cache:
            db = synth.rows(0, _GRID_N, _GRID_DIM, 8101)
            q = synth.rows(0, _GRID_NQ, _GRID_DIM, 8102)
            for j in range(0, _GRID_NQ, 3):                       # a planted near neighbour for every third query
                db[(j * 157 + 5) % _GRID_N] = q[j] + np.float32(0.05) * synth.rows(j, 1, _GRID_DIM, 8103)[0]
            idx = _mk(metric, _GRID_DIM, f16)
            idx.add(db)
            stored = _stored(idx, _GRID_N, gpu)
            od, oi, qq = _oracle(knn_oracle_lib, stored, q, _GRID_K, metric, gpu)
            cache[(metric, f16)] = (idx, stored, q, od, oi, qq)
        return cache[(metric, f16)]
    yield get
    cache.clear()


@pytest.mark.parametrize("nq", [300, 16, 1])
@pytest.mark.parametrize("k", [129, 200, 512, 1024])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_large_k_parity_grid(gpu, grid_store, metric, f16, k, nq):
    import torch
    idx, stored, q, od, oi, qq = grid_store(metric, f16)
    od, oi, qq = od[:nq, :k], oi[:nq, :k], qq[:nq]
    if metric != "COSINE":
        assert O.rank_gaps(od).min() > 0                          # ids are decidable (cosine: the score fallback of _check)
    D, I, K64 = idx.search_device(torch.from_numpy(q[:nq]).to(gpu), k, return_f64=True)
    info = _certified(idx, nq)
    # above k = 128 the fp32 tile kernels filter (the f16 scans and the streaming kernels are tuned for k <= 128)
    assert info["scan_kind"] == "f32_tile", info
    _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, stored, qq, metric, K64=K64.cpu().numpy(),
           ctx=dict(metric=metric, f16=f16, k=k, nq=nq, info=info))


# ---- (b) the cancellation store ------------------------------------------------------------------------------------------------
def _cancellation_store(n, nq, dim, offset, seed):
    """rows and queries c + 0.05 N(0, 1) around one common c ~ U(offset, 2 offset) per coordinate (un-normalised embeddings share a
    large common component): an fp32 ranking by 2 q.y - |y|^2 cancels ~|c|^2 and loses the neighbours' gaps"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(offset, 2 * offset, dim)
    db = (c + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    q = (c + 0.05 * rng.standard_normal((nq, dim))).astype(np.float32)
    return db, q


@pytest.fixture(scope="module")
def cancellation_store(gpu, knn_oracle_lib):
    n, nq, dim = 20000, 400, 128
    db, q = _cancellation_store(n, nq, dim, 20.0, 8201)
    idx = _mk("L2", dim)
    idx.add(db)
    od, oi, _ = _oracle(knn_oracle_lib, db, q, 1024, "L2", gpu)
    return idx, db, q, od, oi


@pytest.mark.parametrize("k,nq", [(129, 64), (512, 64), (1024, 64), (1024, 400)])
def test_large_k_cancellation_store_is_certified(gpu, cancellation_store, k, nq):
    """the fp32 filter's error here is far larger than the gaps between neighbours: the certificate must see it and send the
    queries to the exact kernel (until this was fixed, the k + 6 best fp32 candidates were re-ranked unchecked and every query
    lost true neighbours).  400 rejected queries at k = 1024 take several launches of the exact kernel (its partial lists are
    bounded per launch)."""
    import torch
    idx, db, q, od, oi = cancellation_store
    q, od, oi = q[:nq], od[:nq], oi[:nq]
    D, I, K64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
    info = _certified(idx, nq)
    assert info["certificate"]["rejected"] > 0, info
    _check(D.cpu().numpy(), I.cpu().numpy(), od[:, :k], oi[:, :k], db, q, "L2", K64=K64.cpu().numpy(), ctx=dict(k=k, info=info))


# ---- (c) ties and edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_large_k_exact_copies_straddling_rank_k(gpu, knn_oracle_lib, metric):
    """100 closer rows, then 300 exact copies of one row at ranks 100-399 of query 3: the top 200 holds the copies of the LOWEST
    ids (the header's tie rule), with a large id base"""
    import torch
    n, nq, dim, k, base = 50000, 40, 128, 200, 12345678901
    db = synth.rows(0, n, dim, 8301)
    q = synth.rows(0, nq, dim, 8302)
    close = [45000 + 7 * t for t in range(100)]
    for t, r in enumerate(close):
        db[r] = q[3] + np.float32(0.02) * synth.rows(t, 1, dim, 8303)[0]
    dup = q[3] + np.float32(0.05) * synth.rows(0, 1, dim, 8304)[0]
    if metric == "IP":                                            # copies score below the closer rows for inner product too
        for r in close:
            db[r] = q[3] * np.float32(1.5)
        db[close] += np.float32(0.01) * synth.rows(0, 100, dim, 8305)
    copies = [1001 + 131 * t for t in range(300)]
    db[copies] = dup
    idx = _mk(metric, dim, id_base=base)
    idx.add(db)
    D, I, K64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
    _certified(idx, nq)
    stored = _stored(idx, n, gpu)
    od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu, id_base=base)
    I = I.cpu().numpy()
    _check(D.cpu().numpy(), I, od, oi, stored, qq, metric, id_base=base, K64=K64.cpu().numpy())
    got = [i - base for i in I[3] if i - base in set(copies)]
    assert got == copies[:100], got[:5]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_large_k_near_duplicate_bands(gpu, knn_oracle_lib, metric, f16):
    """test_gpu_certificate's bands at k = 256: 700 near-ties straddling rank k of query 33 (more than the re-rank takes: exact
    kernel) and 100 adjacent exact copies at the top of query 7"""
    import torch
    n, nq, dim, k = 50000, 80, 64, 256
    db = synth.rows(0, n, dim, 7101)
    q = synth.rows(0, nq, dim, 7102)
    near = q[33] + np.float32(0.05) * synth.rows(1, 1, dim, 7103)[0]
    for t in range(700):
        row = near.copy()
        row[t % dim] += np.float32(3e-4 * ((t * 7) % 11 - 5))
        db[(t * 67 + 11) % n] = row
    dup = q[7] + np.float32(0.05) * synth.rows(0, 1, dim, 7103)[0]
    db[20000:20100] = dup
    idx = _mk(metric, dim, f16)
    idx.add(db)
    D, I, K64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
    info = _certified(idx, nq)
    assert info["certificate"]["rejected"] >= 1, info
    stored = _stored(idx, n, gpu)
    od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu)
    I = I.cpu().numpy()
    _check(D.cpu().numpy(), I, od, oi, stored, qq, metric, K64=K64.cpu().numpy(), ctx=dict(info=info))
    assert list(I[7][:100]) == list(range(20000, 20100))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_large_k_beyond_ntotal(gpu, knn_oracle_lib, metric, f16):
    """k = 1024 over 700 rows: all 700 in order, then id -1 with +inf (L2) / -inf (IP, cosine), as faiss fills"""
    import torch
    n, nq, dim, k, base = 700, 33, 96, 1024, 12345678901
    db = synth.rows(0, n, dim, 8401)
    q = synth.rows(0, nq, dim, 8402)
    idx = _mk(metric, dim, f16, id_base=base)
    idx.add(db)
    D, I, K64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
    _certified(idx, nq)
    stored = _stored(idx, n, gpu)
    od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu, id_base=base)
    assert np.all(oi[:, n:] == -1)
    _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, stored, qq, metric, id_base=base, K64=K64.cpu().numpy())


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_large_k_append_between_searches(gpu, knn_oracle_lib, metric):
    """k = 300: half the rows, search, the rest, search -- each against the store as it stood"""
    import torch
    n, nq, dim, k = 30000, 70, 256, 300
    db = synth.rows(0, n, dim, 8501)
    q = synth.rows(0, nq, dim, 8502)
    for j in range(nq):
        db[(j * 421 + 9) % n] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 8503)[0]
    idx = _mk(metric, dim)
    for n_now in (n // 2, n):
        idx.add(db[idx.ntotal:n_now])
        D, I = idx.search_device(torch.from_numpy(q).to(gpu), k)
        _certified(idx, nq)
        stored = _stored(idx, n_now, gpu)
        od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu)
        _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, stored, qq, metric, ctx=dict(n_now=n_now))


# ---- (d) bf16 queries on an fp16 store (BASELINE config 5's form) ----------------------------------------------------------------
def test_large_k_bf16_queries_on_fp16_store(gpu, knn_oracle_lib):
    import torch
    n, nq, dim, k = 60000, 300, 256, 256
    db = synth.rows(0, n, dim, 8601)
    q = synth.rows(0, nq, dim, 8602)
    for j in range(nq):
        db[(j * 193 + 7) % n] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 8603)[0]
    idx = _mk("COSINE", dim, f16=True)
    idx.add(db)
    qb = torch.from_numpy(q).to(gpu).to(torch.bfloat16)
    D, I, K64 = idx.search_device(qb, k, return_f64=True)
    _certified(idx, nq)
    D2, I2 = idx.search_device(qb.float(), k)
    assert torch.equal(I, I2) and torch.equal(D, D2)
    stored = _stored(idx, n, gpu)
    od, oi, qq = _oracle(knn_oracle_lib, stored, qb.float().cpu().numpy(), k, "COSINE", gpu)
    _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, stored, qq, "COSINE", K64=K64.cpu().numpy())


# ---- (e) sharded on one GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [200, 1024])
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_large_k_sharded_two_half_search(gpu, knn_oracle_lib, metric, k):
    """three row shards with global id bases: search_begin -> global_bound (G k = 600 on the selection kernel, 3072 on its torch
    fallback) -> search_finish(global bound, float64 keys) -> hip_merge == the unsharded oracle"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge, shard_bounds
    n, dim, nq, G = 36001, 128, 90, 3
    db = synth.rows(0, n, dim, 8701)
    q = synth.rows(0, nq, dim, 8702)
    for t in range(40):                                           # one query's neighbours crowd a single shard
        db[20010 + t] = q[11] + np.float32(0.02 + 0.001 * t) * synth.rows(t, 1, dim, 8703)[0]
    qd = torch.from_numpy(q).to(gpu)
    shards, stored = [], []
    for r in range(G):
        lo, hi = shard_bounds(n, G, r)
        idx = _mk(metric, dim, id_base=lo)
        idx.add(db[lo:hi])
        shards.append(idx)
        stored.append(_stored(idx, hi - lo, gpu))
    lbs = torch.stack([s.search_begin(qd, k) for s in shards])
    glb = HipFlatIndex.global_bound(lbs, k)
    keys, ids = [], []
    for s in shards:
        _, i, k64 = s.search_finish(glb, return_f64=True)
        _certified(s, nq)
        keys.append(k64); ids.append(i)
    md, mi = hip_merge(shards[0].metric, torch.stack(keys), torch.stack(ids), k)
    stored = np.concatenate(stored)
    od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu)
    _check(md.cpu().numpy(), mi.cpu().numpy(), od, oi, stored, qq, metric)


# ---- (f) the pipeline boundary: top_k = 120 with exclude_self searches k = 130 ---------------------------------------------------
def test_large_k_retrieve_similar_vectors(gpu, tmp_path):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, feature_dim=64, tpp_levels=[1, 2, 4], top_k=120, vector_db_index_type="L2",
               vector_db_path=str(tmp_path / "vdb"))
    pipe = R.HotPathPipeline(cfg)
    D = pipe.tpp.get_output_dim()
    n, nq = 20000, 48
    db = synth.rows(0, n, D, 8801)
    q = synth.rows(0, nq, D, 8802)
    own = [(j * 401 + 13) % n for j in range(nq)]
    for j, r in enumerate(own):                                   # every query is stored (its own basename) and has close neighbours
        db[r] = q[j]
        for t in range(3):
            db[(r + 1 + t) % n] = q[j] + np.float32(0.01 * (t + 1)) * synth.rows(t, 1, D, 8803 + j)[0]
    db_paths = [f"/train/f{i}.wav" for i in range(n)]
    labels = [float(i % 2) for i in range(n)]
    pipe.vector_db.add_vectors(db, db_paths, labels, {"speaker_id": ["s"] * n})
    query_paths = [f"/query/f{r}.wav" for r in own]
    qd = torch.from_numpy(q).to(gpu)
    vec, lbl, rp, dist = pipe.retrieve_similar_vectors(qd, query_paths=query_paths, exclude_self=True, return_info=True,
                                                       return_distances=True)
    assert pipe.vector_db.index.last_launch()["certificate"]["queries"] == nq
    K = cfg.top_k
    od, oi = O.knn(db, q, K + 10, "L2")
    ov, ol, op, odist = O.retrieve_postprocess(od, oi, db, db_paths, labels, K, D, query_paths=query_paths, exclude_self=True)
    assert rp == op
    assert all(os.path.basename(x) != f"f{own[j]}.wav" for j, row in enumerate(rp) for x in row)
    np.testing.assert_array_equal(lbl.cpu().numpy(), ol)
    np.testing.assert_allclose(dist.cpu().numpy(), odist, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(vec.cpu().numpy(), ov)


# ---- (g) bounded fuzz --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [101, 102])
def test_fuzz_knn_large_k(gpu, knn_oracle_lib, seed):
    """test_fuzz_knn's dims, store sizes, batch sizes, id bases and append patterns at k in {129, 130, 257, 600, 1024}"""
    import torch
    rng = np.random.default_rng(seed)
    for case in range(10):
        metric = ["L2", "IP", "COSINE"][rng.integers(3)]
        dim = int(rng.choice([32, 64, 96, 128, 256, 512, 100, 36]))
        n = int(rng.choice([1, 17, 255, 256, 257, 1000, 4097, 20000, 70001]))
        nq = int(rng.choice([1, 16, 17, 33, 128, 129, 255, 256, 257, 600]))
        k = int(rng.choice([129, 130, 257, 600, 1024]))
        f16 = bool(rng.integers(4) == 0)
        id_base = int(rng.choice([0, 0, 12345678901]))
        db = synth.rows(0, n, dim, 19000 + 100 * seed + case)
        q = synth.rows(0, nq, dim, 19500 + 100 * seed + case)
        if rng.integers(2) and not f16 and metric != "COSINE":
            db *= np.exp2(rng.integers(-10, 10, size=n)).astype(np.float32)[:, None]
        for j in range(min(nq, 50)):
            db[(j * 31 + 7) % n] = q[j] + np.float32(0.05) * synth.rows(j, 1, dim, 19900 + case)[0]
        idx = _mk(metric, dim, f16, id_base)
        cut = int(rng.integers(0, n + 1))
        if cut:
            idx.add(db[:cut])
        if cut and rng.integers(2):
            idx.search(q[: min(nq, 300)], min(k, cut))             # a search between the appends
        if cut < n:
            idx.add(db[cut:])
        D, I, K64 = idx.search_device(torch.from_numpy(q).to(gpu), k, return_f64=True)
        ctx = dict(seed=seed, case=case, metric=metric, dim=dim, n=n, nq=nq, k=k, f16=f16, id_base=id_base, cut=cut)
        info = _certified(idx, nq)
        ctx["info"] = info
        stored = _stored(idx, n, gpu)
        od, oi, qq = _oracle(knn_oracle_lib, stored, q, k, metric, gpu, id_base)
        _check(D.cpu().numpy(), I.cpu().numpy(), od, oi, stored, qq, metric, id_base, K64=K64.cpu().numpy(), ctx=ctx)
