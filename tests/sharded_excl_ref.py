"""numpy model of the exclusion-aware search over G row shards (ShardedSearch.search_excluding: radad_knn_search_excl_begin ->
radad_excl_merge_certify -> radad_knn_search_excl_finish -> radad_topk_merge_f64), built from the float64 oracle per shard and
tests/exclusion_ref.py, and the designed stores its tests search.  Order everywhere: (float64 key in the metric's order, lower id).
tests/test_sharded_excl_model.py checks it against expected_excluding over the whole store."""
import numpy as np

from exclusion_ref import expected_excluding
from oracle import radad_oracle as O
from oracle import synth


def bases_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def shard_begin(stored, tags, excl, q, k, k_fetch, metric, id_base=0):
    """one shard's first half -> (K f64 [nq,k], I i64 [nq,k], FK f64 [nq], FI i64 [nq]): the first <= k admissible of the shard's
    top-k_fetch (-1 / NaN padded) and the frontier: the k-th survivor; else the last of the k_fetch hits; else (the hits are all the
    shard has) -1 / NaN"""
    tags, excl = np.asarray(tags, np.int64), np.asarray([] if excl is None else excl, np.int64)
    nq, n = len(q), len(stored)
    K, I = np.full((nq, k), np.nan), np.full((nq, k), -1, np.int64)
    FK, FI = np.full(nq, np.nan), np.full(nq, -1, np.int64)
    if n == 0:
        return K, I, FK, FI
    kf, whole = min(k_fetch, n), k_fetch > n
    od, oi = O.knn(stored, q, kf, metric)
    adm = ~np.isin(tags[oi], excl)
    for j in range(nq):
        s = np.flatnonzero(adm[j])[:k]
        K[j, :len(s)], I[j, :len(s)] = od[j, s], oi[j, s] + id_base
        if len(s) == k:
            FK[j], FI[j] = od[j, s[-1]], oi[j, s[-1]] + id_base
        elif not whole:
            FK[j], FI[j] = od[j, kf - 1], oi[j, kf - 1] + id_base
    return K, I, FK, FI


def merge(metric, K, I, k):
    """[G, nq, k] lists -> merged ([nq,k] keys, [nq,k] ids), id -1 last, padding -1 / NaN"""
    md, mi = O.merge_topk(list(K), list(I), k, "L2" if metric == "L2" else "IP")
    return np.where(mi < 0, np.nan, md), mi


def certify(metric, K, I, FK, FI):
    """-> (merged keys, merged ids, unproved int32 [nq]): proved iff for every shard with a frontier (id >= 0) the merged list holds
    k entries and its last is the frontier entry or ranks ahead of it"""
    G, nq, k = K.shape
    md, mi = merge(metric, K, I, k)
    sgn = 1.0 if metric == "L2" else -1.0                    # smaller sgn * key ranks ahead
    unproved = np.zeros(nq, np.int32)
    for j in range(nq):
        for g in range(G):
            if FI[g, j] < 0:
                continue
            full = mi[j, k - 1] >= 0
            a, b = sgn * md[j, k - 1], sgn * FK[g, j]
            if not (full and (a < b or (a == b and mi[j, k - 1] <= FI[g, j]))):
                unproved[j] = 1
    return md, mi, unproved


def shard_finish(stored, tags, excl, q, k, metric, id_base, K, I, flags):
    """the flagged queries' rows become the shard's exact admissible top k; the others stay"""
    K, I = K.copy(), I.copy()
    f = np.flatnonzero(flags)
    if len(f):
        K[f], I[f] = expected_excluding(stored, tags, excl, q[f], k, metric, id_base)
    return K, I


def sharded_search_excluding(stored, tags, excl, q, k, k_fetch, metric, sizes):
    """the whole search over contiguous row shards of `sizes` rows -> (keys [nq,k], ids [nq,k], unproved [nq])"""
    b = bases_of(sizes)
    tags = np.asarray(tags, np.int64)
    parts = [(stored[b[g]:b[g + 1]], tags[b[g]:b[g + 1]], int(b[g])) for g in range(len(sizes))]
    begun = [shard_begin(s, t, excl, q, k, k_fetch, metric, base) for s, t, base in parts]
    K, I, FK, FI = (np.stack([x[c] for x in begun]) for c in range(4))
    md, mi, unproved = certify(metric, K, I, FK, FI)
    if unproved.any():
        done = [shard_finish(s, t, excl, q, k, metric, base, K[g], I[g], unproved) for g, (s, t, base) in enumerate(parts)]
        md, mi = merge(metric, np.stack([x[0] for x in done]), np.stack([x[1] for x in done]), k)
    return md, mi, unproved


def own_flags(I, FI):
    """[nq] bool: the queries a shard's own rule lists (k_excl_compact): its list is short and rows are unseen"""
    return (I[:, -1] < 0) & (FI >= 0)


# ---- designed stores: (db, q, tags, excl sorted, info) over shards of `sizes` rows -------------------------------------------------
def _base(sizes, dim, nq, seed):
    n = int(np.sum(sizes))
    return synth.rows(0, n, dim, seed), synth.rows(0, nq, dim, seed + 1), np.arange(n, dtype=np.int64) * 7 + 11


def store_a(sizes, dim, nq, n_crowded, n_dups, seed):
    """crowding near-duplicates (excluded) of the first n_crowded evenly spaced queries, ALL in shard 0; info = those queries"""
    rng = np.random.default_rng(seed)
    db, q, tags = _base(sizes, dim, nq, seed)
    rows = rng.choice(int(sizes[0]), n_crowded * n_dups, replace=False)
    which = (np.arange(n_crowded) * max(1, nq // n_crowded)) % nq
    for c, j in enumerate(which):
        r = rows[c * n_dups:(c + 1) * n_dups]
        db[r] = q[j] + np.float32(1e-3) * rng.standard_normal((n_dups, dim)).astype(np.float32)
    return db, q, tags, np.unique(tags[rows]), which


def store_b(sizes, dim, nq, k, seed):
    """about 90 % of shard 0 excluded; shard 1 holds k planted admissible near rows per query; info = the planted rows [nq, k]"""
    rng = np.random.default_rng(seed)
    db, q, tags = _base(sizes, dim, nq, seed)
    b = bases_of(sizes)
    gone = rng.choice(int(sizes[0]), int(0.9 * sizes[0]), replace=False)
    planted = b[1] + rng.choice(int(sizes[1]), nq * k, replace=False).reshape(nq, k)
    for j in range(nq):
        # (0.1: near enough to be every query's neighbours, far enough apart that their order does not hang on the last bits of a
        # cosine store's fp32 row norms -- these rows are RESULTS, unlike the excluded duplicates of store_a)
        db[planted[j]] = q[j] + np.float32(0.1) * rng.standard_normal((k, dim)).astype(np.float32)
    return db, q, tags, np.unique(tags[gone]), planted


def store_c(sizes, dim, nq, seed):
    """the LAST shard has no admissible row (all its tags excluded) plus 32 excluded rows elsewhere; the caller makes one shard
    smaller than k_fetch through `sizes`; info = the exclusion mask over rows"""
    rng = np.random.default_rng(seed)
    db, q, tags = _base(sizes, dim, nq, seed)
    b = bases_of(sizes)
    gone = np.concatenate([np.arange(b[-2], b[-1]), rng.choice(int(b[-2]), min(32, int(b[-2]) // 2), replace=False)])
    excl = np.unique(tags[gone])
    return db, q, tags, excl, np.isin(tags, excl)


def store_d(sizes, dim, nq, seed):
    """everything excluded"""
    db, q, tags = _base(sizes, dim, nq, seed)
    return db, q, tags, np.unique(tags), None
