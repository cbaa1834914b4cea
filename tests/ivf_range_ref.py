"""float64 numpy reference of radad_ivf_range_search (no GPU): the exact range search restricted to the probed lists.

Given the centroids and list assignments an index holds, the probes of a query are the `nprobe` centroids nearest to it
(oracle.radad_oracle.knn, float64, (distance, id) order); its MEMBERS are the rows of those lists whose float64 key
sum((q - y)^2) is < radius, strictly, ordered by (key, insertion id).  The radius is a float32 on the C side and compared as a
double: the reference rounds it the same way.

probed_keys() does the expensive part once per (store, queries, nprobe); members() cuts it at a radius, so a test that tries several
radii shares one pass.  ivf_range() is the two together.
"""
import numpy as np

from oracle import radad_oracle as O


def probed_keys(db, assign, centroids, q, nprobe):
    """per query (ids int64 ascending, keys float64) of the rows of its probed lists"""
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q.reshape(1, -1)
    assign = np.asarray(assign)
    _, probes = O.knn(centroids, q, min(int(nprobe), len(centroids)), "L2")
    out = []
    for i in range(len(q)):
        cand = np.flatnonzero(np.isin(assign, probes[i])).astype(np.int64)
        keys = ((db[cand] - q[i][None, :]) ** 2).sum(1) if len(cand) else np.zeros((0,), np.float64)
        out.append((cand, keys))
    return out


def members(pk, radius, M):
    """-> (counts int32 [nq], ids int64 [nq, M] (-1), keys float64 [nq, M] (NaN), margin float64 [nq]):
    margin[i] = min |key - radius| / radius over the probed rows of query i (inf: no probed row, or an infinite radius) -- how far the
    nearest row is from the boundary, i.e. whether membership is decidable in float64 whatever the order of summation"""
    r = float(np.float32(radius))
    nq = len(pk)
    counts = np.zeros((nq,), np.int32)
    ids = np.full((nq, M), -1, np.int64)
    keys = np.full((nq, M), np.nan, np.float64)
    margin = np.full((nq,), np.inf, np.float64)
    for i, (cand, k) in enumerate(pk):
        inside = k < r
        counts[i] = int(inside.sum())
        c, kk = cand[inside], k[inside]
        order = np.lexsort((c, kk))[:M]
        ids[i, :len(order)] = c[order]
        keys[i, :len(order)] = kk[order]
        if len(k) and np.isfinite(r) and r != 0.0:
            margin[i] = float(np.min(np.abs(k - r)) / abs(r))
    return counts, ids, keys, margin


def ivf_range(db, assign, centroids, q, radius, nprobe, M):
    return members(probed_keys(db, assign, centroids, q, nprobe), radius, M)


def brute_range(db, q, radius, M):
    """the same over every row: what nprobe == nlist must give"""
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q.reshape(1, -1)
    all_ids = np.arange(len(db), dtype=np.int64)
    return members([(all_ids, ((db - q[i][None, :]) ** 2).sum(1)) for i in range(len(q))], radius, M)


def radius_between(pk, query, rank):
    """a float32 radius midway between the keys of ranks `rank` - 1 and `rank` (0-based, ascending) of one query's probed rows: exactly
    `rank` members for that query, the boundary as far from both as the data allows"""
    k = np.sort(pk[query][1])
    return float(np.float32(0.5 * (k[rank - 1] + k[rank])))
