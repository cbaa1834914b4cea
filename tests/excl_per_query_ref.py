"""Reference of the exclusion-aware search with one exclusion set PER QUERY (HipFlatIndex.search_excluding_per_query,
radad_knn_search_excl_pq), shared by its GPU tests and checked on the CPU by tests/test_excl_per_query_model.py.  Built like
tests/exclusion_ref.py on the float64 oracle over the rows AS STORED: per query, the oracle over the rows whose tag is not among
the query's first `cnt` tags; the queries the certificate cannot prove, derived from the oracle's top-k_fetch over the whole store;
the shard halves (certify / merge / bases_of are tests/sharded_excl_ref.py's); and three designed stores.
Order everywhere: (float64 key in the metric's order, lower id)."""
import numpy as np

from oracle import radad_oracle as O
from oracle import synth
from sharded_excl_ref import bases_of, certify, merge


def clamp_counts(qtags, qcnt):
    """-> (qtags int64 [nq, m], counts int64 [nq] in [0, m]); qcnt None = m for every query"""
    qtags = np.asarray(qtags, np.int64)
    qtags = qtags.reshape(len(qtags), -1)
    m = qtags.shape[1]
    cnt = np.full(len(qtags), m, np.int64) if qcnt is None else np.clip(np.asarray(qcnt, np.int64), 0, m)
    return qtags, cnt


def expected_pq(stored, tags, qtags, qcnt, q, k, metric, id_base=0):
    """(D float64 [nq,k], I int64 [nq,k]): per query the k best rows whose tag is not among the first cnt of the query's tags, by
    the float64 oracle over those rows alone; id -1 / distance NaN where fewer than k such rows exist"""
    tags = np.asarray(tags, np.int64)
    qtags, cnt = clamp_counts(qtags, qcnt)
    stored = np.asarray(stored)
    nq = len(q)
    D = np.full((nq, k), np.nan, np.float64)
    I = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        valid = np.flatnonzero(~np.isin(tags, qtags[j, :cnt[j]]))
        if len(valid):
            od, oi = O.knn(stored[valid], q[j:j + 1], k, metric)
            D[j, :od.shape[1]] = od[0]
            I[j, :oi.shape[1]] = valid[oi[0]] + id_base
    return D, I


def _admitted(tags, oi, qtags, cnt):
    """bool like oi: the hit's tag is not among its query's tags"""
    return np.stack([~np.isin(tags[oi[j]], qtags[j, :cnt[j]]) for j in range(len(oi))]) if len(oi) else np.zeros(oi.shape, bool)


def expected_exact_pq(stored, tags, qtags, qcnt, q, k, k_fetch, metric):
    """bool [nq]: the queries that must take the exact pass -- the store holds at least k_fetch rows and the oracle's top-k_fetch
    over the WHOLE store holds fewer than k rows admissible for that query"""
    tags = np.asarray(tags, np.int64)
    qtags, cnt = clamp_counts(qtags, qcnt)
    if len(stored) < k_fetch:
        return np.zeros(len(q), bool)
    _, oi = O.knn(stored, q, k_fetch, metric)
    return _admitted(tags, oi, qtags, cnt).sum(axis=1) < k


def shard_begin_pq(stored, tags, qtags, qcnt, q, k, k_fetch, metric, id_base=0):
    """one shard's first half, as sharded_excl_ref.shard_begin with the per-query admission test"""
    tags = np.asarray(tags, np.int64)
    qtags, cnt = clamp_counts(qtags, qcnt)
    nq, n = len(q), len(stored)
    K, I = np.full((nq, k), np.nan), np.full((nq, k), -1, np.int64)
    FK, FI = np.full(nq, np.nan), np.full(nq, -1, np.int64)
    if n == 0:
        return K, I, FK, FI
    kf, whole = min(k_fetch, n), k_fetch > n
    od, oi = O.knn(stored, q, kf, metric)
    adm = _admitted(tags, oi, qtags, cnt)
    for j in range(nq):
        s = np.flatnonzero(adm[j])[:k]
        K[j, :len(s)], I[j, :len(s)] = od[j, s], oi[j, s] + id_base
        if len(s) == k:
            FK[j], FI[j] = od[j, s[-1]], oi[j, s[-1]] + id_base
        elif not whole:
            FK[j], FI[j] = od[j, kf - 1], oi[j, kf - 1] + id_base
    return K, I, FK, FI


def shard_finish_pq(stored, tags, qtags, qcnt, q, k, metric, id_base, K, I, flags):
    """the flagged queries' rows become the shard's exact admissible top k; the others stay"""
    K, I = K.copy(), I.copy()
    f = np.flatnonzero(flags)
    if len(f):
        qtags, cnt = clamp_counts(qtags, qcnt)
        K[f], I[f] = expected_pq(stored, tags, qtags[f], cnt[f], q[f], k, metric, id_base)
    return K, I


def sharded_search_excluding_pq(stored, tags, qtags, qcnt, q, k, k_fetch, metric, sizes):
    """the whole search over contiguous row shards of `sizes` rows -> (keys [nq,k], ids [nq,k], unproved [nq])"""
    b = bases_of(sizes)
    tags = np.asarray(tags, np.int64)
    parts = [(stored[b[g]:b[g + 1]], tags[b[g]:b[g + 1]], int(b[g])) for g in range(len(sizes))]
    begun = [shard_begin_pq(s, t, qtags, qcnt, q, k, k_fetch, metric, base) for s, t, base in parts]
    K, I, FK, FI = (np.stack([x[c] for x in begun]) for c in range(4))
    md, mi, unproved = certify(metric, K, I, FK, FI)
    if unproved.any():
        done = [shard_finish_pq(s, t, qtags, qcnt, q, k, metric, base, K[g], I[g], unproved) for g, (s, t, base) in enumerate(parts)]
        md, mi = merge(metric, np.stack([x[0] for x in done]), np.stack([x[1] for x in done]), k)
    return md, mi, unproved


def adjacent_gap(stored, tags, qtags, qcnt, q, k, metric):
    """the smallest float64 gap between adjacent admissible ranks 1 .. k + 1 over all queries (NaN slots skipped)"""
    D, _ = expected_pq(stored, tags, qtags, qcnt, q, k + 1, metric)
    g = np.abs(np.diff(D, axis=1))
    return float(np.nanmin(g))


# ---- designed stores: (db, q, tags, qtags [nq, m], qcnt [nq], info) ------------------------------------------------------------------
def per_file(n, dim, nq, c, n_own, seed):
    """files of c rows each share a tag; n_own evenly spaced queries own one file each: its c rows are the query + 1e-3 noise, and the
    query excludes that file's tag (count 1); the other queries exclude nothing (count 0).  info = the owning queries"""
    rng = np.random.default_rng(seed)
    db = synth.rows(0, n, dim, seed)
    q = synth.rows(0, nq, dim, seed + 1)
    tags = (np.arange(n, dtype=np.int64) // c) * 7 + 11
    files = rng.choice(n // c, n_own, replace=False)
    which = (np.arange(n_own) * max(1, nq // n_own)) % nq
    qtags = np.zeros((nq, 1), np.int64)
    qcnt = np.zeros(nq, np.int32)
    for f, j in zip(files, which):
        db[f * c:f * c + c] = q[j] + 1e-3 * rng.standard_normal((c, dim))
        qtags[j, 0] = tags[f * c]
        qcnt[j] = 1
    return db, q, tags, qtags, qcnt, which


def mutual(n, dim, n_groups, seed, n_dups=16, width=8, noise=0.1):
    """eight IDENTICAL queries per group; n_dups planted rows near the group's vector; query 8 g + i excludes `width` of them, a
    window that moves with i: the queries of one exact-pass group have the same vector and different admissible sets.
    info = the planted rows [n_groups, n_dups]"""
    rng = np.random.default_rng(seed)
    db = synth.rows(0, n, dim, seed)
    v = synth.rows(0, n_groups, dim, seed + 1)
    q = np.repeat(v, 8, axis=0)
    tags = np.arange(n, dtype=np.int64) * 7 + 11
    rows = rng.choice(n, n_groups * n_dups, replace=False).reshape(n_groups, n_dups)
    for g in range(n_groups):
        db[rows[g]] = v[g] + noise * rng.standard_normal((n_dups, dim))
    qtags = np.zeros((8 * n_groups, width), np.int64)
    for g in range(n_groups):
        for i in range(8):
            qtags[8 * g + i] = tags[rows[g][(i + np.arange(width)) % n_dups]]
    return db, q, tags, qtags, np.full(8 * n_groups, width, np.int32), rows


def nearest(n, dim, nq, seed, depth=20, metric="L2"):
    """random rows and queries; query j excludes the tags of its own `depth` nearest rows (the oracle's); m = depth.  info = those
    rows [nq, depth]"""
    db = synth.rows(0, n, dim, seed)
    q = synth.rows(0, nq, dim, seed + 1)
    tags = np.arange(n, dtype=np.int64) * 7 + 11
    _, oi = O.knn(db, q, depth, metric)
    return db, q, tags, tags[oi].copy(), np.full(nq, depth, np.int32), oi
