"""The float64 model of the IVF search with one exclusion set per query (radad_ivf_search_excl_pq) and the designed cases of
tests/test_gpu_ivf_excl_pq.py.  No GPU: tests/test_ivf_excl_pq_model.py asserts what makes each case the case it claims to be.

The model is the existing oracle on each query's own ADMISSIBLE rows: for query j, O.ivf_search(db[adm_j], assign[adm_j], ...) with the
ids mapped back through flatnonzero(adm_j) (monotone: ties still go to the lower id), adm_j = the rows whose tag is not among the first
clamp(counts[j], 0, m) entries of qtags[j].  The gap conditions of tests/test_gpu_ivf_adversarial.py (assert_gaps) are asserted per
query on that query's admissible rows, so "ids are equal" is a fair demand of the device."""
import numpy as np

from oracle import radad_oracle as O
from oracle import synth
from test_gpu_ivf_adversarial import KS, _blobs, assert_gaps, cpu_assign

KMAX = max(KS)
_CASES = {}


def live_tags(qtags, counts, j):
    """the tags query j really excludes: the first clamp(counts[j], 0, m) entries of its row (counts None = all m)"""
    qtags = np.asarray(qtags, np.int64).reshape(len(qtags), -1)
    m = qtags.shape[1]
    c = m if counts is None else int(min(max(int(counts[j]), 0), m))
    return qtags[j, :c]


def expected_pq(db, assign, cent, q, k, nprobe, tags, qtags, counts=None, what=""):
    """(float64 distances, ids) [nq, k + 1] of the model, the gap conditions asserted per query on its own admissible rows.  Queries
    with the same vector and the same set of live tags share one oracle call."""
    nq = len(q)
    od = np.full((nq, k + 1), np.inf)
    oi = np.full((nq, k + 1), -1, np.int64)
    done = {}
    for j in range(nq):
        live = np.unique(live_tags(qtags, counts, j))
        key = (q[j].tobytes(), live.tobytes())
        if key not in done:
            adm = ~np.isin(tags, live)
            keep = np.flatnonzero(adm)
            if len(keep) == 0:
                done[key] = (np.full(k + 1, np.inf), np.full(k + 1, -1, np.int64))
            else:
                d, i = assert_gaps(db[adm], assign[adm], cent, q[j:j + 1], k, nprobe, what=f"{what} query {j}")
                done[key] = (d[0], np.where(i[0] >= 0, keep[np.clip(i[0], 0, None)], -1))
        od[j], oi[j] = done[key]
    return od, oi


def list_major(assign, nlist):
    """(offsets [nlist + 1], position of every row): a row's list-major position is its list's offset plus its rank by insertion id
    inside the list (the stable counting sort of the index)"""
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int64)
    order = np.argsort(assign, kind="stable")
    pos = np.empty(len(assign), np.int64)
    pos[order] = np.arange(len(assign))
    return off, pos


def _base(dim, n=6000, nlist=24, seed=9951, nq=300):
    cent, db = _blobs(n, dim, nlist, seed)
    q = (cent[(np.arange(nq) * 5) % nlist] + synth.rows(0, nq, dim, seed + 4)).astype(np.float32)
    return db, cent, q


def _near(rng, v, n, dim, scale=1e-3):
    return (v + np.float32(scale) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)


# ---- 1. twins in one task -----------------------------------------------------------------------------------------------------------
def case_twins(dim):
    """40 bitwise-equal copies of one query, every copy with another set (m = 2).  Copy 0 excludes its 20 planted near-copies (tag A),
    copy 1 nothing (count 0), copy 2 the 20 rows planted around ANOTHER query (tag B), copy c > 2 the single row 100 + c"""
    rng = np.random.default_rng(9961 + dim)
    db, cent, q = _base(dim)
    tags = np.arange(len(db), dtype=np.int64)
    A, B = 1_000_000, 1_000_001
    at = rng.choice(np.arange(1000, len(db)), 40, replace=False)
    db[at[:20]] = _near(rng, q[3], 20, dim)
    db[at[20:]] = _near(rng, q[4], 20, dim)
    tags[at[:20]] = A
    tags[at[20:]] = B
    copies = 40
    qq = np.repeat(q[3:4], copies, axis=0)
    qtags = np.full((copies, 2), -9, np.int64)
    counts = np.full(copies, 2, np.int32)
    qtags[0] = (A, A)
    counts[1] = 0
    qtags[1] = (A, B)                      # (beyond the count: ignored)
    qtags[2] = (-9, B)
    for c in range(3, copies):
        qtags[c] = (100 + c, -9)
    return dict(db=db, cent=cent, q=qq, tags=tags, qtags=qtags, counts=counts, nprobe=3, planted_a=np.sort(at[:20]), planted_b=np.sort(at[20:]))


# ---- 2. crowded leave-one-out -------------------------------------------------------------------------------------------------------
def case_loo(dim):
    """20 near-copies of each of the queries 3 .. 10 under that query's own tag; every query excludes its own tag only (m = 1).  Query
    11 sits next to query 3: query 3's planted rows stay admissible for it and are its nearest neighbours"""
    rng = np.random.default_rng(9971 + dim)
    db, cent, q = _base(dim)
    q[11] = _near(rng, q[3], 1, dim, 5e-3)[0]
    tags = np.arange(len(db), dtype=np.int64)
    planted = np.arange(3, 11)
    at = rng.choice(len(db), 8 * 20, replace=False).reshape(8, 20)
    for j, rows in zip(planted, at):
        db[rows] = _near(rng, q[j], 20, dim)
        tags[rows] = 1_000_000 + j
    qtags = (1_000_000 + np.arange(len(q), dtype=np.int64)).reshape(-1, 1)
    return dict(db=db, cent=cent, q=q, tags=tags, qtags=qtags, counts=None, nprobe=3, planted=planted, at=at)


# ---- 3. position coverage -----------------------------------------------------------------------------------------------------------
def case_positions(dim):
    """40 near-copies of query 3 on a run of 40 consecutive list-major positions of its home list that straddles a multiple of 256 (and
    so of 64), every row under a tag of its own.  42 bitwise-equal queries: copy 0 excludes all 40 rows (m = 40), copy 1 nothing, copy
    2 + i row i of the run only.  by_list: the tag of a row is its list; copy 0 excludes its home list, copy 1 a list it does not probe"""
    rng = np.random.default_rng(9981 + dim)
    db, cent, q = _base(dim)
    nlist = len(cent)
    assign = cpu_assign(db, cent)
    off, pos = list_major(assign, nlist)
    # a query whose home list holds a multiple of 256 with 20 positions of the list on either side
    run = None
    for j in range(len(q)):
        home = int(O.knn(cent, q[j:j + 1], 1, "L2")[1][0, 0])
        for P in range(256, len(db), 256):
            if off[home] <= P - 20 and P + 20 <= off[home + 1]:
                run = (j, home, P)
                break
        if run:
            break
    assert run, "no list holds a multiple of 256 with 20 rows on either side: pick another seed"
    j, home, P = run
    rows = np.flatnonzero((pos >= P - 20) & (pos < P + 20))          # ascending ids = ascending positions inside one list
    db[rows] = _near(rng, q[j], 40, dim)
    tags = np.arange(len(db), dtype=np.int64)
    tags[rows] = 5_000_000 + np.arange(40)
    copies = 42
    qq = np.repeat(q[j:j + 1], copies, axis=0)
    qtags = np.full((copies, 40), -9, np.int64)
    counts = np.ones(copies, np.int32)
    qtags[0] = 5_000_000 + rng.permutation(40)
    counts[0] = 40
    counts[1] = 0
    for i in range(40):
        qtags[2 + i, 0] = 5_000_000 + i
    other = int(O.knn(cent, q[j:j + 1], nlist, "L2")[1][0, -1])       # the farthest list: never probed at nprobe 3
    list_qtags = np.array([[home], [other]], np.int64)
    return dict(db=db, cent=cent, q=qq, tags=tags, qtags=qtags, counts=counts, nprobe=3, rows=rows, home=home, P=P, other=other,
                list_qtags=list_qtags)


def case_long(dim):
    """lists longer than 256 rows (split over several workgroups for nq = 1 and 17): tags are the row ids, every query excludes the 40
    rows nearest to it (m = 40), so its answer starts at rank 41 -- positions anywhere in the shares"""
    db, cent, q = _base(dim, n=30000, nlist=8, seed=9991, nq=17)
    return dict(db=db, cent=cent, q=q, tags=np.arange(len(db), dtype=np.int64), counts=None, nprobe=3)


# ---- 4. the set's shape -------------------------------------------------------------------------------------------------------------
def case_shapes(dim):
    """tags are the row ids; `top` = every query's true 12 nearest rows (plain oracle).  m = 64: the live part of a row lists the
    query's top 3 in any order, twice, among tags no row has; the entries BEYOND the count are the ranks 4 .. 12 and must be ignored.
    counts cycle through 0, a negative one, one above m (all 64 entries live: they hold the top 5 and fillers) and 9"""
    rng = np.random.default_rng(9995 + dim)
    db, cent, q = _base(dim, nq=120)
    assign = cpu_assign(db, cent)
    _, top = O.ivf_search(db, assign, cent, q, 12, 3)
    assert (top >= 0).all()
    m = 64
    qtags = np.empty((len(q), m), np.int64)
    counts = np.empty(len(q), np.int32)
    for j in range(len(q)):
        kind = j % 4
        row = -1 - rng.integers(0, 1 << 40, m)                      # tags no row has (negative)
        if kind == 2:
            counts[j] = 100
            row[rng.choice(m, 10, replace=False)] = np.repeat(top[j, :5], 2)
        else:
            counts[j] = (0, -3, 0, 9)[kind]
            live = np.concatenate([top[j, :3], top[j, :3], row[:3]])
            row[:9] = rng.permutation(live)
            row[9:18] = top[j, 3:12]
        qtags[j] = row
    one = top[:, :1].copy()                                         # m = 1: every query excludes its nearest row
    return dict(db=db, cent=cent, q=q, tags=np.arange(len(db), dtype=np.int64), qtags=qtags, counts=counts, one=one, top=top, nprobe=3,
                assign=assign)


_BUILDERS = {"twins": case_twins, "loo": case_loo, "positions": case_positions, "long": case_long, "shapes": case_shapes}


def case(name, dim):
    """the inputs of a case and the model's answers for k = 26 (every smaller k is a prefix), the gap conditions asserted"""
    key = (name, dim)
    if key in _CASES:
        return _CASES[key]
    c = _BUILDERS[name](dim)
    db, cent, q, tags, nprobe = c["db"], c["cent"], c["q"], c["tags"], c["nprobe"]
    assign = c["assign"] = c.get("assign", cpu_assign(db, cent))
    what = f"{name} dim {dim}"
    if name == "long":
        _, top = O.ivf_search(db, assign, cent, q, 40, nprobe)
        c["qtags"] = top.copy()
    c["od"], c["oi"] = expected_pq(db, assign, cent, q, KMAX, nprobe, tags, c["qtags"], c["counts"], what)
    if name in ("loo", "shapes"):
        c["plain"] = assert_gaps(db, assign, cent, q, KMAX, nprobe, what=what + " unfiltered")
    if name == "shapes":
        c["od_null"], c["oi_null"] = expected_pq(db, assign, cent, q, KMAX, nprobe, tags, c["qtags"], None, what + " NULL counts")
        c["od_one"], c["oi_one"] = expected_pq(db, assign, cent, q, KMAX, nprobe, tags, c["one"], None, what + " m = 1")
    if name == "positions":
        ltags = assign.astype(np.int64)
        for npb in (1, 3):
            c[f"list{npb}"] = expected_pq(db, assign, cent, q[:2], 15, npb, ltags, c["list_qtags"], None, what + f" home list excluded, nprobe {npb}")
        c["ltags"] = ltags
    _CASES[key] = c
    return c
