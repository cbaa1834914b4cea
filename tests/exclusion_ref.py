"""Reference of the exclusion-aware search (HipFlatIndex.search_excluding), shared by its GPU tests and checked on the CPU by
tests/test_exclusion_reference.py: the float64 oracle over the rows that are NOT excluded, the number of queries the certificate
cannot prove (derived from the oracle's top-k_fetch over the whole store), and the "crowded" stores the tests search."""
import numpy as np

from oracle import radad_oracle as O
from oracle import synth


def expected_excluding(stored, tags, excl, q, k, metric, id_base=0):
    """(D float64 [nq,k], I int64 [nq,k]): the k best rows whose tag is not in `excl`, by the float64 oracle over those rows alone;
    id -1 / distance NaN where fewer than k such rows exist"""
    tags = np.asarray(tags, np.int64)
    excl = np.asarray([] if excl is None else excl, np.int64)
    valid = np.flatnonzero(~np.isin(tags, excl))
    nq = len(q)
    D = np.full((nq, k), np.nan, np.float64)
    I = np.full((nq, k), -1, np.int64)
    if len(valid):
        od, oi = O.knn(np.asarray(stored)[valid], q, k, metric)
        D[:, :od.shape[1]] = od
        I[:, :oi.shape[1]] = valid[oi] + id_base
    return D, I


def expected_exact(stored, tags, excl, q, k, k_fetch, metric):
    """bool [nq]: the queries that must take the exact pass -- the oracle's top-k_fetch over the WHOLE store has no unfilled slot
    (the store holds at least k_fetch rows) and fewer than k of its entries are outside `excl`"""
    tags = np.asarray(tags, np.int64)
    excl = np.asarray([] if excl is None else excl, np.int64)
    if len(stored) < k_fetch:
        return np.zeros(len(q), bool)
    _, oi = O.knn(stored, q, k_fetch, metric)
    return (~np.isin(tags[oi], excl)).sum(axis=1) < k


def crowded(n, dim, nq, n_crowded, n_dups, seed, extra_excl=64, tags=None):
    """random rows and queries; the first n_crowded of `nq` evenly spaced queries get n_dups near-duplicates each (query + 1e-3 noise)
    at random rows; those rows' tags and the tags of extra_excl further random rows form the exclusion set.
    -> (db, q, tags, excl sorted, crowded query indices)"""
    rng = np.random.default_rng(seed)
    db = synth.rows(0, n, dim, seed)
    q = synth.rows(0, nq, dim, seed + 1)
    tags = (np.arange(n, dtype=np.int64) * 7 + 11) if tags is None else np.asarray(tags, np.int64)
    rows = rng.choice(n, n_crowded * n_dups + extra_excl, replace=False)
    which = (np.arange(n_crowded) * max(1, nq // max(n_crowded, 1))) % nq
    for c, j in enumerate(which):
        r = rows[c * n_dups:(c + 1) * n_dups]
        db[r] = q[j] + np.float32(1e-3) * rng.standard_normal((n_dups, dim)).astype(np.float32)
    return db, q, tags, np.unique(tags[rows]), which
