"""numpy model of the bounded two-half search over G row shards (radad_knn_search_begin -> k-th largest of the G k lower bounds ->
radad_knn_search_finish(global_lb) -> radad_topk_merge_f64) and the designed stores its tests search.  Everything is float64 from the
rows AS STORED and the queries AS PREPARED (cosine: after radad_rownorm), and works on SCORES, larger is better: q.y for inner product
and cosine, -sum (q - y)^2 for L2 -- summed as written, never formed as 2 q.y - |y|^2.  Order everywhere: (score descending, lower
id).  tests/test_sharded_bound_model.py checks the model and the stores' designs on the CPU; tests/test_gpu_sharded_bound.py runs the
device code against them."""
import numpy as np

from oracle import synth

DIM = 64


def bases_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scores(stored, qq, metric):
    """exact score of every (query, row) pair -> float64 [nq, n]"""
    y = np.asarray(stored).astype(np.float64)
    q = np.asarray(qq).astype(np.float64)
    out = np.empty((len(q), len(y)))
    for j in range(len(q)):          # (row by row, no BLAS: bit-identical rows get bit-identical scores wherever they are stored)
        out[j] = -((q[j][None, :] - y) ** 2).sum(1) if metric == "L2" else (y * q[j][None, :]).sum(1)
    return out


class Model:
    """the whole store's scores, cut into contiguous shards of `sizes` rows; ids are global (a shard's id_base is its first row)"""

    def __init__(self, stored, qq, metric, sizes):
        self.metric, self.sizes, self.bases = metric, list(sizes), bases_of(sizes)
        assert len(stored) == self.bases[-1]
        self.S = scores(stored, qq, metric)
        ids = np.broadcast_to(np.arange(self.S.shape[1], dtype=np.int64), self.S.shape)
        self.order = np.lexsort((ids, -self.S), axis=1)          # per query: every row, best first, lower id first among equals
        self.sorted = np.take_along_axis(self.S, self.order, 1)

    @property
    def nq(self):
        return self.S.shape[0]

    def topk(self, k):
        """the oracle over the whole store -> (scores [nq, min(k, n)], ids)"""
        return self.sorted[:, :k], self.order[:, :k]

    def kth(self, k):
        """exact global k-th best score per query; -inf where the store has fewer than k rows"""
        return self.sorted[:, k - 1].copy() if k <= self.S.shape[1] else np.full(self.nq, -np.inf)

    def tightest_bound(self, k):
        """float32 [nq]: the largest float32 that is <= the exact global k-th best score -- the hardest valid bound search_finish can
        be given"""
        kth = self.kth(k)
        with np.errstate(over="ignore"):
            f = kth.astype(np.float32)
        up = f.astype(np.float64) > kth
        f[up] = np.nextafter(f[up], np.float32(-np.inf))
        return f

    def shard_sorted(self, g):
        """shard g's own exact scores per query, best first -> float64 [nq, n_g]"""
        return -np.sort(-self.S[:, self.bases[g]:self.bases[g + 1]], axis=1)

    def shard_topk(self, g, k):
        """shard g's own top k -> global ids [nq, min(k, n_g)]"""
        lo, hi = self.bases[g], self.bases[g + 1]
        s = self.S[:, lo:hi]
        ids = np.broadcast_to(np.arange(lo, hi, dtype=np.int64), s.shape)
        return np.take_along_axis(ids, np.lexsort((ids, -s), axis=1)[:, :k], 1)

    def must_return(self, g, k):
        """per query the ids of the global oracle top k that lie in shard g -> list of nq int64 arrays (in the oracle's order)"""
        _, oi = self.topk(k)
        lo, hi = self.bases[g], self.bases[g + 1]
        return [row[(row >= lo) & (row < hi)] for row in oi]

    def score_of(self, j, ids):
        return self.S[j, ids]


def host_kth_largest(lb_all, k):
    """[G, nq, kk] float32 -> [nq]: the k-th largest of a query's G kk values, NaN ranking lowest (radad_kth_largest's rule)"""
    x = np.asarray(lb_all, np.float32)
    x = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    flat = np.transpose(x, (1, 0, 2)).reshape(x.shape[1], -1)
    return -np.sort(-flat, axis=1)[:, k - 1]


# ---- designed stores: (db float32 [n, DIM], q float32 [nq, DIM], sizes, info) ------------------------------------------------------
EVEN = (16640, 16640, 16640)            # three shards, each just above the 16 384 rows the certified f16 scans ask for
UNEVEN = (40000, 9000, 3000, 7)         # f16 tile scan, fp32 tile kernel, dense kernel, a shard with fewer than k rows
S2_PLANTED = 15                         # rows planted per query in shard 1 (k + 5 at k = 10)


def _noise(t, seed):
    return synth.rows(t, 1, DIM, seed)[0]


def s1(nq=40):
    """even shards, one planted neighbour per query, spread over the shards; info = the planted rows [nq]"""
    n = sum(EVEN)
    db, q = synth.rows(0, n, DIM, 9101), synth.rows(0, nq, DIM, 9102)
    rows = np.array([(j * 16661 + 5) % n for j in range(nq)])      # (16661 = a shard + 21: consecutive queries in consecutive shards)
    for j, r in enumerate(rows):
        db[r] = q[j] + np.float32(0.05) * _noise(j, 9103)
    return db, q, EVEN, rows


def s2(nq=40):
    """one shard holds everything: S2_PLANTED rows q + (0.02 + 0.002 t) noise per query, all in shard 1; info = those rows [nq, 15]"""
    db, q = synth.rows(0, sum(EVEN), DIM, 9901), synth.rows(0, nq, DIM, 9902)
    rows = EVEN[0] + np.arange(nq)[:, None] * 32 + np.arange(S2_PLANTED)[None, :]
    for j in range(nq):
        for t in range(S2_PLANTED):
            db[rows[j, t]] = q[j] + np.float32(0.02 + 0.002 * t) * _noise(t, 9903 + j)
    return db, q, EVEN, rows


def s3(nq=42):
    """ties across the shard boundaries: for every third query its nearest planted row has 6 bit-identical copies, 2 in each shard,
    and its next-nearest 3, one in each shard: the cuts k = 4 and k = 7 fall inside a group of equal float64 keys.
    info = (tied queries, copies of the nearest [n_tied, 6], copies of the next [n_tied, 3])"""
    db, q = synth.rows(0, sum(EVEN), DIM, 9301), synth.rows(0, nq, DIM, 9302)
    b = bases_of(EVEN)
    tied = np.arange(0, nq, 3)
    first = np.empty((len(tied), 6), np.int64)
    second = np.empty((len(tied), 3), np.int64)
    for c, j in enumerate(tied):
        near = q[j] + np.float32(0.05) * _noise(j, 9303)
        nxt = q[j] + np.float32(0.08) * _noise(j, 9304)
        # (the two copies of a shard far apart: different row tiles of the scan; the order of the ids is not that of the planting)
        first[c] = [b[g] + (977 * c + 13 + 8000 * h) % EVEN[g] for g in range(3) for h in range(2)]
        second[c] = [b[g] + (1409 * c + 4001 + 111 * g) % EVEN[g] for g in (2, 0, 1)]
        db[first[c]] = near
        db[second[c]] = nxt
    assert len(np.unique(np.concatenate([first.ravel(), second.ravel()]))) == first.size + second.size
    return db, q, EVEN, (tied, first, second)


def s4(nq=40):
    """uneven shards that run different scan kernels.  Query j has three planted neighbours in shard j % 4 (the 7-row shard: the
    first two such queries only); info = planted rows [nq, 3], -1 where none"""
    n = sum(UNEVEN)
    db, q = synth.rows(0, n, DIM, 9401), synth.rows(0, nq, DIM, 9402)
    b = bases_of(UNEVEN)
    rows = np.full((nq, 3), -1, np.int64)
    for j in range(nq):
        g = j % 4
        if g == 3 and j // 4 >= 2:
            continue
        for t in range(3):
            r = b[g] + ((j // 4) * 3 + t if g == 3 else (j * 211 + 97 * t + 3) % UNEVEN[g])
            db[r] = q[j] + np.float32(0.05 + 0.01 * t) * _noise(t, 9403 + j)
            rows[j, t] = r
    assert len(np.unique(rows[rows >= 0])) == (rows >= 0).sum()
    return db, q, UNEVEN, rows


def s5():
    """S1 with a batch of 12 queries: the small-batch scans"""
    db, q, sizes, rows = s1()
    return db, q[:12].copy(), sizes, rows[:12]


STORES = {"S1": s1, "S2": s2, "S3": s3, "S4": s4, "S5": s5, "S6": s1}     # S6: S1 on an fp16 store
F16 = {"S6"}
