"""The float64 numpy reference of the certified range search (radad_knn_range_search / HipFlatIndex.range_search) and the designed
stores of tests/test_gpu_knn_range.py, checked on the CPU by tests/test_range_model.py.

Membership is STRICT on the float64 key, as faiss's range_search: squared L2 distance < radius, inner product / cosine > radius.
The device sums a key in another order than numpy, so a row whose key lies within 1e-9 max(1, |radius|) of the radius -- a
BOUNDARY row -- may fall either way; the designed stores have none, except the integer store, whose keys are exact in any order.

Planted rows: for a unit query direction qd, a row  a qd + w u  (u a unit vector orthogonal to qd) has inner product a with qd and,
when a^2 + w^2 = 1, cosine a and squared distance 2 - 2 a.  Random unit rows in 64 dimensions have cosines of standard deviation
1 / 8 with anything, so nothing random comes near a threshold of 0.9: who is within the radius is decided by the planting.

EPS_MODEL: what the tests assume the scan's error bound eps(q) stays below on these stores (fp16 operands, relative 2^-11, on scores
of magnitude <= 2: a few 1e-3).  Generous guesses; the GPU tests measure eps (threshold minus the floor the scan ran with) and fail,
naming the constant, when it is larger.  A query of the tile route must not have more than BAND_CAP rows whose key reaches the
threshold lowered by EPS_MODEL: then its 4096-entry candidate buffer cannot overflow."""
import numpy as np

N_ROWS = 16640 + 37                      # 65 whole 256-row tiles and a partial one
EPS_MODEL = {"IP": 0.02, "COSINE": 0.02, "L2": 0.05}
BUFFER = 4096                            # entries of a query's candidate buffer on the tile route
BAND_CAP = 2048
IN_LEVELS = (0.99, 0.95, 0.92, 0.905)    # planted within a radius of 0.9 ...
OUT_LEVELS = (0.895, 0.88)               # ... and just outside it
COUNTS = (0, 1, 5, 40)                   # rows planted within the radius of query j: COUNTS[j % 4]


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _perp(rng, qd, count):
    u = rng.standard_normal((count, len(qd)))
    u -= np.outer(u @ qd, qd)
    return unit(u)


def plant(rng, qd, along, perp=None):
    """[len(along), dim]: rows  along[i] qd + perp[i] u_i  for the unit direction qd (perp None: sqrt(1 - along^2), unit rows)"""
    along = np.asarray(along, np.float64)
    perp = np.sqrt(1.0 - along * along) if perp is None else np.asarray(perp, np.float64)
    return along[:, None] * qd + perp[:, None] * _perp(rng, qd, len(along))


def keys(stored, q, metric):
    """float64 keys [nq, n] as the library reports them: squared distance (L2: smaller is better), inner product (IP), cosine over
    rows and queries normalised in float64 (COSINE; the GPU tests hand in the rows as stored and the device's normalised queries
    under "IP" instead)"""
    d, x = np.asarray(stored, np.float64), np.asarray(q, np.float64)
    if metric == "COSINE":
        d, x = unit(d), unit(x)
    if metric == "L2":
        return np.stack([((xj - d) ** 2).sum(axis=1) for xj in x])           # sum (q - y)^2: no cancellation
    return x @ d.T


def within(key, radius, metric):
    return key < np.float64(radius) if metric == "L2" else key > np.float64(radius)


def expected_range(stored, q, radius, metric, M, id_base=0, key=None):
    """-> (counts int32 [nq], ids int64 [nq, M], keys float64 [nq, M], boundary bool [nq, n]): per query the exact number of rows
    within the radius, its best min(count, M) ordered by (key, lower id), -1 / NaN in the other slots; boundary: rows whose key is
    within 1e-9 max(1, |radius|) of the radius (an infinite radius has none).  key: keys(stored, q, metric), when the caller has them"""
    key = keys(stored, q, metric) if key is None else key
    inside = within(key, radius, metric)
    nq = len(key)
    counts = inside.sum(axis=1).astype(np.int32)
    ids = np.full((nq, M), -1, np.int64)
    out = np.full((nq, M), np.nan, np.float64)
    for j in range(nq):
        rows = np.flatnonzero(inside[j])
        order = np.lexsort((rows, key[j, rows] if metric == "L2" else -key[j, rows]))[:M]
        ids[j, :len(order)] = rows[order] + id_base
        out[j, :len(order)] = key[j, rows[order]]
    boundary = np.abs(key - np.float64(radius)) <= 1e-9 * max(1.0, abs(float(radius))) if np.isfinite(radius) else np.zeros_like(inside)
    return counts, ids, out, boundary


def brute_range(stored, q, radius, metric, M, id_base=0):
    """the same contract one (query, row) pair at a time, nothing shared with expected_range but the strict compare"""
    nq = len(q)
    counts = np.zeros(nq, np.int32)
    ids = np.full((nq, M), -1, np.int64)
    out = np.full((nq, M), np.nan, np.float64)
    r = float(radius)
    for j in range(nq):
        x = np.asarray(q[j], np.float64)
        if metric == "COSINE":
            x = x / np.sqrt(np.dot(x, x))
        hits = []
        for row in range(len(stored)):
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
    """per query: rows whose key reaches the threshold lowered by EPS_MODEL (everything the scan may emit), rows within the radius"""
    key = keys(stored, q, metric)
    e = EPS_MODEL[metric]
    band = key <= np.float64(radius) + e if metric == "L2" else key >= np.float64(radius) - e
    return band.sum(axis=1), within(key, radius, metric).sum(axis=1)


# ---- the designed stores ----------------------------------------------------------------------------------------------------------------
def graded(metric, nq=300, n=N_ROWS, dim=64, seed=7100, counts=COUNTS, in_levels=IN_LEVELS, out_levels=OUT_LEVELS, common=None,
           crowds=(), crowd_rows=5000, crowd_span=(0.95, 0.99), many=None):
    """-> (db [n, dim] f32, q [nq, dim] f32, info).  Query j has counts[j % len(counts)] rows planted at in_levels (cycled, each
    repeat 1e-4 further in) and as many, at least two, at out_levels (each repeat 1e-4 further out); info["planted_in"][j] their rows.
    metric "IP": the levels are inner products with unit queries, the planted rows carry a random orthogonal part of 0.3 .. 1.0 and the
    random rows norms of 0.5 .. 1.5; otherwise everything has unit norm (the levels are cosines; squared distance 2 - 2 level).
    common: rows and queries are normalise(mu + common z) with one unit mu -- a store with a common component, for a centred plane.
    crowds: queries that get crowd_rows near-copies at levels spread over crowd_span (more than a candidate buffer holds).
    many = (query, count): that query gets `count` rows planted over in_levels[-1] .. in_levels[0] instead."""
    rng = np.random.default_rng(seed)
    if common is None:
        db, qd = unit(rng.standard_normal((n, dim))), unit(rng.standard_normal((nq, dim)))
    else:
        mu = unit(rng.standard_normal(dim))
        db = unit(mu + common * rng.standard_normal((n, dim)) / np.sqrt(dim))
        qd = unit(mu + common * rng.standard_normal((nq, dim)) / np.sqrt(dim))
    if metric == "IP":
        db = db * rng.uniform(0.5, 1.5, (n, 1))
    free = list(rng.permutation(n))
    planted_in = {}

    def put(j, along):
        rows = np.array([free.pop() for _ in range(len(along))], np.int64)
        perp = rng.uniform(0.3, 1.0, len(along)) if metric == "IP" else None
        db[rows] = plant(rng, qd[j], along, perp)
        return rows
    for j in crowds:
        planted_in[j] = put(j, rng.uniform(crowd_span[0], crowd_span[1], crowd_rows))
    for j in range(nq):
        if j in crowds:
            continue
        c = counts[j % len(counts)]
        if many is not None and j == many[0]:
            planted_in[j] = put(j, np.linspace(in_levels[-1], in_levels[0], many[1]))
        else:
            i = np.arange(c)
            planted_in[j] = put(j, np.asarray(in_levels)[i % len(in_levels)] + 1e-4 * (i // len(in_levels)))
        i = np.arange(max(c, 2))
        put(j, np.asarray(out_levels)[i % len(out_levels)] - 1e-4 * (i // len(out_levels)))
    return db.astype(np.float32), qd.astype(np.float32), {"planted_in": planted_in}


def integers(metric, nq=300, n=N_ROWS, dim=64, seed=7500, copies=3):
    """rows and queries with entries in {-2, .., 2}: every key is an integer, exact in fp32 and float64 in any order.  The rows of
    query 0's best key are followed by `copies` duplicates of the first of them at later rows: equal keys, id order.
    -> (db, q, info); info["radius"]: an integer that several rows hit exactly for many queries (IP 40 = 2.5 sigma above the mean 0;
    L2 170 = 2.3 sigma below the mean 256)."""
    rng = np.random.default_rng(seed)
    db = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    k0 = keys(db, q[:1], metric)[0]
    best = int(np.argmin(k0) if metric == "L2" else np.argmax(k0))
    later = np.sort(rng.choice(np.arange(best + 1, n), copies, replace=False))
    db[later] = db[best]
    return db, q, {"radius": 170.0 if metric == "L2" else 40.0, "best": best, "copies": later}


def case(name):
    """the designed cases of tests/test_gpu_knn_range.py -> dict(metric, db, q, radius, M, route, overflow (queries meant to overflow
    their buffer), info, and for the model: model_metric -- "COSINE" where the handle normalises)"""
    c = dict(name=name, M=64, route="tile", overflow=np.zeros(0, np.int64), kind="uncentred")
    if name in ("graded_cosine", "graded_f16", "graded_bf16"):
        db, q, info = graded("COSINE")
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, kind="f16" if name == "graded_f16" else "uncentred")
        if name == "graded_f16":
            c["db"] = db.astype(np.float16).astype(np.float32)
    elif name == "graded_l2":
        db, q, info = graded("L2", seed=7200)
        c.update(metric="L2", db=db, q=q, radius=0.2, info=info)            # squared distance 2 - 2 cos: 0.2 <-> 0.9
    elif name == "graded_ip":
        db, q, info = graded("IP", seed=7300)
        c.update(metric="IP", db=db, q=q, radius=0.9, info=info)
    elif name == "graded_dim128":
        db, q, info = graded("COSINE", dim=128, seed=7350)
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info)
    elif name == "centred":
        db, q, info = graded("COSINE", seed=7400, common=0.3, in_levels=(0.999, 0.995, 0.99, 0.985), out_levels=(0.975, 0.97))
        c.update(metric="COSINE", db=db, q=q, radius=0.98, info=info, kind="centred")
    elif name in ("integer_ip", "integer_l2"):
        metric = "IP" if name == "integer_ip" else "L2"
        db, q, info = integers(metric)
        c.update(metric=metric, db=db, q=q, radius=info["radius"], info=info)
    elif name == "truncation":
        db, q, info = graded("COSINE", nq=17, seed=7600, many=(0, 300))
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, M=16)
    elif name == "overflow":
        db, q, info = graded("COSINE", seed=7700, counts=(0, 1, 5, 12), crowds=(0, 299))
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, overflow=np.array([0, 299]))
    elif name == "nothing":
        db, q, info = graded("COSINE", seed=7800)
        c.update(metric="COSINE", db=db, q=q, radius=1.5, info=info)
    elif name == "everything":
        db, q, info = graded("COSINE", seed=7800)                           # the store of "nothing", its first 17 queries
        c.update(metric="COSINE", db=db, q=q[:17], radius=-np.inf, info=info, overflow=np.arange(17))
    elif name == "exact_nq3":
        db, q, info = graded("COSINE", nq=3, seed=7900, counts=(5, 40, 1))
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, route="exact")
    elif name == "exact_dim36":
        db, q, info = graded("L2", nq=40, n=3000, dim=36, seed=7910)
        c.update(metric="L2", db=db, q=q, radius=0.2, info=info, route="exact")
    elif name == "exact_small_store":
        db, q, info = graded("IP", nq=40, n=1000, seed=7920, counts=(0, 1, 5, 7))
        c.update(metric="IP", db=db, q=q, radius=0.9, info=info, route="exact")
    elif name == "exact_plane_off":
        db, q, info = graded("COSINE", nq=40, seed=7930)
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, route="exact")
    else:
        raise KeyError(name)
    if name == "graded_bf16":
        import torch
        c["q"] = torch.from_numpy(c["q"]).to(torch.bfloat16).float().numpy()          # what a bfloat16 tensor of these queries holds
    return c


CASES = ("graded_cosine", "graded_l2", "graded_ip", "graded_dim128", "centred", "graded_f16", "graded_bf16", "integer_ip", "integer_l2",
         "truncation", "overflow", "nothing", "everything", "exact_nq3", "exact_dim36", "exact_small_store", "exact_plane_off")
