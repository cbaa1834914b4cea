"""The float64 numpy reference of the certified range search among the rows a query does not exclude (radad_knn_range_search_excl /
_excl_pq, HipFlatIndex.range_search_excluding / _per_query) and the designed stores of tests/test_gpu_knn_range_excl.py, checked on the
CPU by tests/test_range_excl_model.py.

The reference is range_ref.expected_range restricted to the admissible rows: the key of every (query, row) pair the query excludes is
replaced by a value that passes no strict test, everything else -- keys, membership, order, padding -- is range_ref's.
brute_range_excl restates the contract one pair at a time and shares only the strict compare with it.

Admissibility, one set per query: row r is admissible for query j iff row_tags[r] is not among the first clamp(q_cnt[j], 0, m)
entries of q_tags[j] (q_cnt None: m).  One set for the batch: iff row_tags[r] is not in the set.

Tags of the designed stores (range_ref.graded): every row carries a tag, 1_000_000 + row unless said otherwise.  For query j every
SECOND planted-in row (the first, third, ...) and the nearest row planted just outside the radius carry own(j) = 10 + j.  Query j
lists m = 4 tags of which the first j % 4 are live: own(j) in one of the live slots, tags no row carries (ABSENT + ...) in the others;
a query with no live slot lists own(j) in every slot and excludes nothing.  Two stored counts lie outside [0, m] (the clamp), and
query 6 lists own(6) twice."""
import functools

import numpy as np

import range_ref as R

M_TAGS = 4
ROW_TAG0 = 1_000_000
ABSENT = 5_000_000_000                   # tags no row carries
N_ROWS, EPS_MODEL, BUFFER, BAND_CAP, COUNTS = R.N_ROWS, R.EPS_MODEL, R.BUFFER, R.BAND_CAP, R.COUNTS


def own(j):
    return 10 + int(j)


# ---- admissibility and the reference ----------------------------------------------------------------------------------------------------
def live_counts(q_cnt, nq, m):
    return np.full(nq, m, np.int64) if q_cnt is None else np.clip(np.asarray(q_cnt, np.int64), 0, m)


def admissible_pq(row_tags, q_tags, q_cnt):
    """bool [nq, n]"""
    q_tags = np.asarray(q_tags, np.int64).reshape(len(q_tags), -1)
    nq, m = q_tags.shape
    live = live_counts(q_cnt, nq, m)
    adm = np.ones((nq, len(row_tags)), bool)
    for j in range(nq):
        if live[j]:
            adm[j] = ~np.isin(row_tags, q_tags[j, :live[j]])
    return adm


def admissible_batch(row_tags, excl, nq):
    a = np.ones(len(row_tags), bool) if excl is None or len(excl) == 0 else ~np.isin(row_tags, excl)
    return np.broadcast_to(a, (nq, len(row_tags)))


def expected_range_excl(stored, q, radius, metric, M, adm, id_base=0, key=None):
    """range_ref.expected_range over the admissible rows -> (counts, ids, keys, boundary); boundary covers admissible rows only"""
    key = R.keys(stored, q, metric) if key is None else key
    never = np.float64(np.inf) if metric == "L2" else -np.float64(np.inf)          # passes no strict test, at any radius
    return R.expected_range(stored, q, radius, metric, M, id_base, key=np.where(adm, key, never))


def brute_range_excl(stored, q, radius, metric, M, row_tags, q_tags=None, q_cnt=None, excl=None, id_base=0):
    """the contract one (query, row) pair at a time; per-query sets (q_tags, q_cnt) or one set for the batch (excl)"""
    nq = len(q)
    counts = np.zeros(nq, np.int32)
    ids = np.full((nq, M), -1, np.int64)
    out = np.full((nq, M), np.nan, np.float64)
    r = float(radius)
    batch = set(int(t) for t in excl) if excl is not None else None
    for j in range(nq):
        if batch is not None:
            mine = batch
        else:
            m = len(q_tags[j])
            c = m if q_cnt is None else max(0, min(int(q_cnt[j]), m))
            mine = set(int(t) for t in q_tags[j][:c])
        x = np.asarray(q[j], np.float64)
        if metric == "COSINE":
            x = x / np.sqrt(np.dot(x, x))
        hits = []
        for row in range(len(stored)):
            if int(row_tags[row]) in mine:
                continue
            y = np.asarray(stored[row], np.float64)
            if metric == "COSINE":
                y = y / np.sqrt(np.dot(y, y))
            if metric == "L2":
                k = float(np.dot(x - y, x - y))
                if k < r:
                    hits.append((k, row))
            else:
                k = float(np.dot(x, y))
                if k > r:
                    hits.append((-k, row))
        hits.sort()
        counts[j] = len(hits)
        for s, (k, row) in enumerate(hits[:M]):
            ids[j, s] = row + id_base
            out[j, s] = k if metric == "L2" else -k
    return counts, ids, out


def band_counts(stored, q, radius, metric):
    """rows per query the scan may EMIT (key within EPS_MODEL of the threshold), excluded rows included: range_ref.band_counts"""
    return R.band_counts(stored, q, radius, metric)[0]


# ---- tags of the designed stores --------------------------------------------------------------------------------------------------------
def graded_tags(db, q, radius, metric, info, own_rows=None):
    """-> (row_tags int64 [n], q_tags int64 [nq, 4], q_cnt int32 [nq]).  own_rows: {query: rows that carry its own tag} instead of
    every second planted-in row, for the queries it names."""
    n, nq = len(db), len(q)
    row_tags = ROW_TAG0 + np.arange(n, dtype=np.int64)
    key = R.keys(db, q, metric)
    inside = R.within(key, radius, metric)
    for j in range(nq):
        rows = np.asarray(info["planted_in"].get(j, ()), np.int64)
        mine = rows[0::2] if own_rows is None or j not in own_rows else np.asarray(own_rows[j], np.int64)
        row_tags[mine] = own(j)
        outside = np.flatnonzero(~inside[j])                                    # the nearest row planted just outside
        near = outside[np.argmin(key[j, outside]) if metric == "L2" else np.argmax(key[j, outside])]
        if row_tags[near] >= ROW_TAG0:
            row_tags[near] = own(j)
    q_tags = ABSENT + np.arange(nq * M_TAGS, dtype=np.int64).reshape(nq, M_TAGS)
    q_cnt = np.zeros(nq, np.int32)
    for j in range(nq):
        c = j % 4
        q_cnt[j] = c
        if c == 0:
            q_tags[j, :] = own(j)                                               # no live slot: listed, not excluded
        else:
            q_tags[j, (j // 4) % c] = own(j)
    if nq > 6:
        q_tags[6, :2] = own(6)                                                  # (two live slots) the same tag twice
    for j in range(nq):                                                         # stored counts outside [0, m]: the device clamps
        if j % 16 == 7:
            q_cnt[j] = 9                                                        # -> 4: the fourth slot (a tag no row carries) is live too
        if j % 16 == 8:
            q_cnt[j] = -3                                                       # -> 0
    return row_tags, q_tags, q_cnt


def batch_set(row_tags, fraction=0.4, seed=99):
    """an ascending set: `fraction` of the distinct tags of the store"""
    tags = np.unique(row_tags)
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(tags, int(round(fraction * len(tags))), replace=False)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _crowd_store():
    """one store for crowd_fits and crowd_overflows: query 0 has 1540 rows within the radius of which 1500 carry its own tag; query 299
    has 5005 of which 5000 carry its own tag"""
    db, q, info = R.graded("COSINE", seed=8100, many=(0, 1540), crowds=(299,), crowd_rows=5005)
    r0, r299 = info["planted_in"][0], info["planted_in"][299]
    keep0 = r0[np.linspace(0, len(r0) - 1, 40).astype(np.int64)]
    keep299 = r299[np.linspace(0, len(r299) - 1, 5).astype(np.int64)]
    own_rows = {0: np.setdiff1d(r0, keep0), 299: np.setdiff1d(r299, keep299)}
    row_tags, q_tags, q_cnt = graded_tags(db, q, 0.9, "COSINE", info, own_rows)
    q_cnt[0] = 1
    q_tags[0, 0] = own(0)                                                        # (query 0 would have no live slot: j % 4 == 0)
    return db, q, info, row_tags, q_tags, q_cnt


def integer_tags(db, q, info, seed=8500):
    """tags from a pool of 7 (100 .. 106): query j excludes 100 + j % 7 and a tag no row carries.  Of the duplicates of query 0's best
    row the first copy is excluded by query 0, the original and the other copies are not."""
    rng = np.random.default_rng(seed)
    row_tags = 100 + rng.integers(0, 7, len(db)).astype(np.int64)
    row_tags[info["best"]] = 101
    row_tags[info["copies"]] = 102
    row_tags[info["copies"][0]] = 100
    nq = len(q)
    q_tags = np.stack([100 + np.arange(nq) % 7, ABSENT + np.arange(nq)], axis=1).astype(np.int64)
    return row_tags, q_tags, None


def case(name):
    """the designed cases -> range_ref.case's dict plus mode ("pq" / "batch"), row_tags, q_tags + q_cnt or excl, and overflow: the
    queries designed to EMIT more than the buffer holds (excluded rows included in the per-query mode, never in the batch mode)"""
    mode = "pq"
    base = name
    if name.endswith("_batch"):
        mode, base = "batch", name[:-len("_batch")]
    c = dict(name=name, M=64, route="tile", overflow=np.zeros(0, np.int64), kind="uncentred", mode=mode)
    if base in ("graded_cosine", "graded_l2", "graded_ip", "graded_dim128", "centred", "graded_f16", "graded_bf16", "exact_nq3", "exact_dim36",
                "exact_small_store", "exact_plane_off"):
        c.update(R.case(base))
        c["name"], c["mode"] = name, mode
        c["row_tags"], c["q_tags"], c["q_cnt"] = graded_tags(c["db"], c["q"], c["radius"], c["metric"], c["info"])
    elif base in ("integer_ip", "integer_l2"):
        c.update(R.case(base))
        c["name"], c["mode"] = name, mode
        c["row_tags"], c["q_tags"], c["q_cnt"] = integer_tags(c["db"], c["q"], c["info"])
    elif base in ("crowd_fits", "crowd_overflows"):
        db, q, info, row_tags, q_tags, q_cnt = _crowd_store()
        nq = 299 if base == "crowd_fits" else 300
        c.update(metric="COSINE", db=db, q=q[:nq], radius=0.9, info=info, row_tags=row_tags, q_tags=q_tags[:nq], q_cnt=q_cnt[:nq])
        if base == "crowd_overflows" and mode == "pq":
            c["overflow"] = np.array([299])                                      # (one set for the batch: its 5000 rows are never emitted)
    elif base == "truncation":
        db, q, info = R.graded("COSINE", nq=17, seed=8600, many=(0, 500))        # levels ascend along planted_in[0]: the last 200 rank best
        own_rows = {0: info["planted_in"][0][300:]}
        row_tags, q_tags, q_cnt = graded_tags(db, q, 0.9, "COSINE", info, own_rows)
        q_cnt[0] = 1
        q_tags[0, 0] = own(0)
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, M=16, row_tags=row_tags, q_tags=q_tags, q_cnt=q_cnt)
    elif base in ("everything", "all_excluded"):
        e = R.case("everything" if base == "everything" else "graded_cosine")
        c.update(e)
        c["name"], c["mode"] = name, mode
        full = R.case("nothing")                                                 # the store of "everything" with all its queries
        tags = graded_tags(full["db"], full["q"], 0.9, "COSINE", full["info"]) if base == "everything" else \
            graded_tags(c["db"], c["q"], c["radius"], c["metric"], c["info"])
        c["row_tags"], c["q_tags"], c["q_cnt"] = tags[0], tags[1][:len(c["q"])], tags[2][:len(c["q"])]
        if base == "all_excluded":
            c["mode"] = "batch"
    else:
        raise KeyError(name)
    if c["mode"] == "batch":
        c["excl"] = np.unique(c["row_tags"]) if base == "all_excluded" else batch_set(c["row_tags"])
        if base == "crowd_overflows":
            # query 0's crowd is in the set (never emitted), query 299's is not: its 5000 rows overflow the buffer and the exact pass
            # answers it among the rows the bitmap admits
            c["excl"] = np.union1d(np.setdiff1d(c["excl"], [own(299)]), [own(0)]).astype(np.int64)
            c["overflow"] = np.array([299])
    return c


def admissible(c):
    if c["mode"] == "batch":
        return admissible_batch(c["row_tags"], c["excl"], len(c["q"]))
    return admissible_pq(c["row_tags"], c["q_tags"], c["q_cnt"])


PQ_TILE = ("graded_cosine", "graded_l2", "graded_ip", "centred", "graded_f16", "graded_bf16", "graded_dim128", "integer_ip", "integer_l2",
           "crowd_fits", "crowd_overflows", "truncation", "everything")
BATCH_TILE = ("graded_cosine_batch", "graded_l2_batch", "centred_batch", "graded_f16_batch", "crowd_overflows_batch", "all_excluded")
EXACT = ("exact_nq3", "exact_dim36", "exact_small_store", "exact_plane_off")
CASES = PQ_TILE + BATCH_TILE + EXACT + tuple(n + "_batch" for n in EXACT)
