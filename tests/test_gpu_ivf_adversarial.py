"""Adversarial stores through the IVF list scans (csrc/ivf.inc) against the float64 oracle restricted to the probed lists.

DESIGN.md section 1 claims that an IVF search equals the exact search over the rows of its probed lists.  tests/test_gpu_ivf.py checks
that on well-separated gaussian blobs only; here are the stores the flat search's certificate tests are built on (a large
common component that cancels in 2 q.y - |y|^2, hundreds of near-ties, exact duplicates, plateaus of rows no fp32 score
can order, norms spread over 2^20), each through every scan route:

  default   certified f16 list scan ("hi_lists"); the queries its certificate rejects take the exact float64 list scan
  f32       hi_scan=0: fp32 list scan ("f32_lists") behind its own certificate, exact float64 list scan for the rejected
  rejected  hi_scan=2: every query declared rejected, the exact float64 list scan answers all of them
  noplane   dim 96 has no f16 plane: "f32_lists" by itself

ids must equal O.ivf_search exactly, distances to rtol 1e-6 / atol 1e-5, unfilled slots -1 / +inf.

The conditions under which "ids are exactly the oracle's" is a fair demand are ASSERTED on the CPU (assert_gaps): the
oracle's float64 distances of ranks 1 .. k + 1 are exactly equal only for identical rows (decided by id) and differ by
more than 1e-12 relative otherwise, and the nprobe-th and (nprobe + 1)-th centroid are not tied.  So is the hardness of
stores 1, 2 and 5 (fp32_loss > 0: an fp32 ranking that keeps k + 6 rows per list and k + 6 over the lists loses true
neighbours), so that a later change of a generator cannot turn them into blobs again.  The stores with set_centroids are
built and checked without a GPU by test_cpu_conditions_of_the_stores."""
import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth

KS = (1, 5, 15, 26)            # 26 is the last k on the list scans; KSEL 16 and 32 both get used
NQS = (1, 16, 17, 300)         # one query (lists split over workgroups), a full and an overfull task, several tasks per list
ROUTES = ("default", "f32", "rejected")


# ---- CPU side: assignments, conditions on the inputs, the fp32 emulation --------------------------------------------------------
def cpu_assign(db, cent):
    """list of every row: its nearest centroid in float64, the lower id on a tie (as O.knn breaks ties)"""
    out = np.empty(len(db), np.int32)
    c = np.asarray(cent, np.float64)
    for s in range(0, len(db), 2048):
        x = np.asarray(db[s:s + 2048], np.float64)
        d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        out[s:s + 2048] = d.argmin(1)
    return out


def assert_gaps(db, assign, cent, q, k, nprobe, coarse_tie_ok=False, what=""):
    """the oracle's answer for k + 1, after asserting that it is the only defensible one (module docstring)"""
    od, oi = O.ivf_search(db, assign, cent, q, k + 1, nprobe)
    for i in range(len(q)):
        m = int((oi[i] >= 0).sum())
        d = od[i, :m]
        gap = np.diff(d)
        tied = gap <= 1e-12 * np.maximum(d[1:], 1e-300)
        for j in np.flatnonzero(tied):
            assert gap[j] == 0.0 and np.array_equal(db[oi[i, j]], db[oi[i, j + 1]]), \
                f"{what}: query {i} ranks {j + 1},{j + 2} are {gap[j]:.3e} apart at distance {d[j]:.6e} and not duplicates: pick another seed"
    if not coarse_tie_ok and nprobe < len(cent):
        cd, _ = O.knn(cent, q, nprobe + 1, "L2")
        assert np.all(cd[:, nprobe] > cd[:, nprobe - 1]), f"{what}: coarse tie at rank nprobe"
    return od, oi


def fp32_loss(db, assign, cent, q, k, nprobe):
    """share of queries whose float64 top-k (within the probed lists) is not inside what an fp32 ranking by 2 q.y - |y|^2 keeps with
    k + 6 entries per (query, list) and k + 6 over the lists (precision only, not the kernel's summation order)"""
    _, probes = O.knn(cent, q, min(nprobe, len(cent)), "L2")
    _, oi = O.ivf_search(db, assign, cent, q, k, nprobe)
    db32 = np.asarray(db, np.float32)
    yn = (db32 * db32).sum(1, dtype=np.float32)
    lost = 0
    for i in range(len(q)):
        keep_id, keep_s = [], []
        for l in probes[i]:
            rows = np.flatnonzero(assign == l)
            if len(rows) == 0:
                continue
            s = (np.float32(2) * (db32[rows] @ np.asarray(q[i], np.float32)) - yn[rows]).astype(np.float32)
            o = np.lexsort((rows, -s))[:k + 6]
            keep_id.append(rows[o]); keep_s.append(s[o])
        if not keep_id:
            continue
        ids, s = np.concatenate(keep_id), np.concatenate(keep_s)
        kept = set(ids[np.lexsort((ids, -s))[:k + 6]].tolist())
        lost += not set(oi[i][oi[i] >= 0].tolist()) <= kept
    return lost / len(q)


# ---- the stores: (db, q, centroids, nprobe, extra) ------------------------------------------------------------------------------
def _blobs(n, dim, nlist, seed, spread=3.0):
    cent = (synth.rows(0, nlist, dim, seed) * np.float32(spread)).astype(np.float32)
    which = (np.arange(n) * 7919) % nlist
    return cent, (cent[which] + synth.rows(0, n, dim, seed + 1)).astype(np.float32)


def _sphere(rng, centre, m, radius=1.0):
    """m rows at distance radius (1 +- 1e-7) from `centre`: float64 tells them apart, no fp32 score does"""
    u = rng.standard_normal((m, len(centre)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (centre.astype(np.float64) + radius * u * (1 + 1e-7 * rng.standard_normal((m, 1)))).astype(np.float32)


def store_cancellation(dim, long_lists, nq=300):
    """store 1: rows and queries c + 0.05 N(0, 1) (the flat tests' cancellation store); the centroids are rows of the store"""
    from test_gpu_knn_large_k import _cancellation_store
    n, nlist, nprobe = (30000, 8, 3) if long_lists else (16000, 64, 8)
    db, q = _cancellation_store(n, nq, dim, 20.0, 9101 + dim + long_lists)
    cent = db[(np.arange(nlist) * (n // nlist) + 17) % n].copy()
    return db, q, cent, nprobe, {}


def store_near_ties(dim, three_lists, nq=300):
    """store 2: 700 rows at distance 1 +- 1e-7 from each of four queries, all in one list (a centroid AT the query) or spread over
    three probed lists (centroids 0.50, 0.52, 0.54 away from it), among blobs"""
    rng = np.random.default_rng(9201 + three_lists)
    cent, db = _blobs(12000, dim, 24, 9203)
    q = (cent[(np.arange(nq) * 5) % 24] + synth.rows(0, nq, dim, 9205)).astype(np.float32)
    hard = (3, 40, 170, 299)
    extra_c, ties = [], {}
    places = rng.permutation(len(db))
    for h, j in enumerate(hard):
        rows = _sphere(rng, q[j], 700)
        far = (q[j] + np.float32(3.0) * rng.standard_normal((300, dim))).astype(np.float32)
        at = places[1000 * h:1000 * (h + 1)]
        db[at] = np.concatenate([rows, far])
        ties[j] = np.sort(at[:700])
        if three_lists:
            e = np.linalg.qr(rng.standard_normal((dim, 3)))[0].T
            extra_c += [q[j] + np.float32(r) * e[t].astype(np.float32) for t, r in enumerate((0.50, 0.52, 0.54))]
        else:
            extra_c.append(q[j].copy())
    cent = np.concatenate([cent, np.stack(extra_c).astype(np.float32)])
    return db, q, cent, 3, {"ties": ties, "lists_per_query": 3 if three_lists else 1}


def store_duplicates(dim, nq=300):
    """store 3: 100 copies of one row adjacent in insertion order (query 7), 100 copies interleaved with rows of other lists (query 8),
    40 copies of the query itself (query 9, distance 0)"""
    cent, db = _blobs(12000, dim, 32, 9301)
    q = (cent[(np.arange(nq) * 5) % 32] + synth.rows(0, nq, dim, 9305)).astype(np.float32)
    adj = np.arange(2000, 2100)
    inter = 5000 + 3 * np.arange(100)
    zero = 9000 + 7 * np.arange(40)
    db[adj] = q[7] + np.float32(0.05) * synth.rows(0, 1, dim, 9307)[0]
    db[inter] = q[8] + np.float32(0.05) * synth.rows(1, 1, dim, 9307)[0]
    db[zero] = q[9]
    return db, q, cent, 4, {"dups": {7: adj, 8: inter, 9: zero}}


def store_rank_k_ties(dim, nq=300):
    """store 4: 4 clear winners, then 24 rows whose distances differ by ~1e-7 straddling ranks 5, 15 and 26 of query 5"""
    cent, db = _blobs(16000, dim, 32, 9401)
    q = (cent[(np.arange(nq) * 5) % 32] + synth.rows(0, nq, dim, 9405)).astype(np.float32)
    j = 5
    for t in range(4):
        db[1000 + 977 * t] = q[j] + np.float32(0.01 * (t + 1)) * synth.rows(t, 1, dim, 9403)[0]
    base = q[j] + np.float32(0.08) * synth.rows(99, 1, dim, 9403)[0]
    for t in range(24):
        row = base.copy()
        row[t % dim] += np.float32(1e-6 * (t + 1))
        db[2000 + 531 * t] = row
    return db, q, cent, 4, {"winners": {1000 + 977 * t for t in range(4)}}


def store_plateau(dim, nq=300):
    """store 5: every query has 40 rows at distance 1 +- 1e-7 in its home list: more than k + 6 = 32 within fp32 resolution"""
    rng = np.random.default_rng(9511)
    cent, db = _blobs(6000, dim, 32, 9503)
    q = (cent[(np.arange(nq) * 5) % 32] + synth.rows(0, nq, dim, 9505)).astype(np.float32)
    db = np.concatenate([db] + [_sphere(rng, q[j], 40) for j in range(nq)])
    db = db[rng.permutation(len(db))]
    return db, q, cent, 3, {}


def store_magnitudes(dim, nq=300):
    """store 6: list 0 (centroid 0) holds rows with norms spread over 2^-10 .. 2^10; list 1 (centroid of norm 2) holds small rows
    and ONE row of norm 2000: |y|^2 dominates the fp32 score.  The other centroids are 1e5 away."""
    rng = np.random.default_rng(9601)
    u = rng.standard_normal((3000, dim)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    spread = (u * np.exp2(rng.uniform(-10, 10, (3000, 1)))).astype(np.float32)
    m = rng.standard_normal(dim); m = (2 * m / np.linalg.norm(m))
    small = (m + 0.05 * rng.standard_normal((500, dim))).astype(np.float32)
    huge = (1000.0 * m).astype(np.float32)[None]
    farc = rng.standard_normal((6, dim)); farc = 1e5 * farc / np.linalg.norm(farc, axis=1, keepdims=True)
    farr = (farc[np.arange(600) % 6] + rng.standard_normal((600, dim))).astype(np.float32)
    db = np.concatenate([spread, small, huge, farr])
    db = db[rng.permutation(len(db))]
    cent = np.concatenate([np.zeros((1, dim)), m[None], farc]).astype(np.float32)
    scale = np.exp2(rng.uniform(-10, 3, (nq, 1)))
    q = np.where(np.arange(nq)[:, None] % 2 == 0, rng.standard_normal((nq, dim)) * scale / np.sqrt(dim),
                 m + 0.05 * rng.standard_normal((nq, dim))).astype(np.float32)
    return db, q, cent, 2, {"huge": int(np.flatnonzero((db == huge[0]).all(1))[0])}


STORES = {
    "cancellation_short": (lambda dim: store_cancellation(dim, False), True),
    "cancellation_long": (lambda dim: store_cancellation(dim, True), True),
    "near_ties_one_list": (lambda dim: store_near_ties(dim, False), True),
    "near_ties_three_lists": (lambda dim: store_near_ties(dim, True), True),
    "duplicates": (store_duplicates, False),
    "rank_k_ties": (store_rank_k_ties, False),
    "plateau": (store_plateau, True),
    "magnitudes": (store_magnitudes, False),
}
_CACHE = {}


def prepared(name, dim):
    """the store, its CPU-side assignments, the oracle for k = 27 (every smaller k is a prefix) -- all conditions asserted"""
    key = (name, dim)
    if key not in _CACHE:
        build, must_be_hard = STORES[name]
        db, q, cent, nprobe, extra = build(dim)
        assign = cpu_assign(db, cent)
        what = f"{name} dim {dim}"
        od, oi = assert_gaps(db, assign, cent, q, max(KS), nprobe, what=what)
        if "ties" in extra:
            for j, rows in extra["ties"].items():
                lists = np.unique(assign[rows])
                assert len(lists) == extra["lists_per_query"], (what, j, lists)
                assert all((assign[rows] == l).sum() > max(KS) + 6 for l in lists), (what, j)
                assert set(lists) <= set(O.knn(cent, q[j:j + 1], nprobe, "L2")[1][0].tolist()), (what, j)
        if "dups" in extra:
            for j, rows in extra["dups"].items():
                assert len(np.unique(assign[rows])) == 1 and np.array_equal(oi[j, :26], rows[:26]), (what, j)
            between = assign[extra["dups"][8][0] + 1: extra["dups"][8][-1]: 3]
            assert (between != assign[extra["dups"][8][0]]).mean() > 0.5, what        # really interleaved with other lists' rows
        if "huge" in extra:
            assert assign[extra["huge"]] == 1 and (assign == 1).sum() > 400 and (assign == 0).sum() > 2000, what
        if must_be_hard:
            sub = slice(0, 48)         # (the emulation is a Python loop: a sample of the queries -- near_ties' first hard query is inside)
            for k in (5, 15):
                share = fp32_loss(db, assign, cent, q[sub], k, nprobe)
                assert share > 0, f"{what}: an fp32 ranking with k + 6 entries loses nothing at k = {k}: the store is not hard"
        _CACHE[key] = (db, q, cent, nprobe, extra, assign, od, oi)
    return _CACHE[key]


@pytest.mark.parametrize("dim", [128, 96])
@pytest.mark.parametrize("name", list(STORES))
def test_cpu_conditions_of_the_stores(name, dim):
    """no GPU: every store satisfies the gap conditions, and stores 1, 2 and 5 defeat an fp32 ranking with k + 6 entries"""
    if dim == 96 and name not in ("cancellation_short", "cancellation_long", "plateau"):
        dim = 160           # (the other stores' second dimension without a plane)
    prepared(name, dim)


# ---- GPU side ---------------------------------------------------------------------------------------------------------------
def _index(gpu, dim, nlist, route, niter=10):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    hi = {"default": None, "f32": 0, "rejected": 2, "noplane": None}[route]
    return R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, niter=niter, hi_scan=hi)


def _assert_route(info, route, nq, what):
    """the route really taken; on every route the queries the certificate rejected went through the exact list scan"""
    assert info["scan"] == ("hi_lists" if route in ("default", "rejected") else "f32_lists"), (what, info)
    if route == "rejected":
        assert info["rejected"] == nq, (what, info)
    assert info["exact"] == info["rejected"], (what, info)


def _compare(D, I, od, oi, k, what):
    od, oi = od[:, :k], oi[:, :k]
    bad = np.flatnonzero((I != oi).any(1))
    assert len(bad) == 0, f"{what}: ids differ from the oracle for {len(bad)} of {len(I)} queries, first {bad[:5]}: {I[bad[0]]} vs {oi[bad[0]]}"
    fin = oi >= 0
    np.testing.assert_allclose(D[fin], od[fin], rtol=1e-6, atol=1e-5, err_msg=str(what))
    assert np.all(np.isposinf(D[~fin])) and np.all(I[~fin] == -1), what


def _sweep(gpu, name, dim, route):
    db, q, cent, nprobe, extra, assign, od, oi = prepared(name, dim)
    idx = _index(gpu, dim, len(cent), route)
    idx.set_centroids(cent)
    half = len(db) // 2
    idx.add(db[:half]); idx.add(db[half:])
    np.testing.assert_array_equal(idx.assignments(), assign)
    np.testing.assert_array_equal(idx.centroids(), cent)
    idx.nprobe = nprobe
    failures, infos = [], {}
    for nq in NQS:
        for k in KS:
            what = dict(store=name, dim=dim, route=route, nq=nq, k=k)
            sl = slice(3, 3 + nq) if nq < 300 else slice(0, 300)    # (the small batches hold the stores' planted queries 3, 5, 7, 8, 9)
            D, I = idx.search(q[sl], k)
            info = infos[(nq, k)] = idx.last_search_info()
            for check in (lambda: _compare(D, I, od[sl], oi[sl], k, what), lambda: _assert_route(info, route, nq, what)):
                try:
                    check()
                except (AssertionError, KeyError) as e:
                    failures.append(f"{what} {info}: {str(e)[:300]}")
    print(f"{name} dim {dim} {route}: rejected/exact per (nq, k): " + ", ".join(f"{a}:{i['rejected']}/{i.get('exact')}" for a, i in infos.items()))
    assert not failures, f"{len(failures)} of {len(NQS) * len(KS)} searches wrong:\n" + "\n".join(failures)
    return idx, infos


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(STORES))
def test_adversarial_store_dim128(gpu, name, route):
    idx, infos = _sweep(gpu, name, 128, route)
    db, q, cent, nprobe, extra, assign, od, oi = prepared(name, 128)
    if "dups" in extra:                                   # exact ties: the lowest ids first
        D, I = idx.search(q, 15)
        for j, rows in extra["dups"].items():
            assert list(I[j]) == list(rows[:15]), (j, I[j])
        assert np.all(D[9] == 0)
    if name == "rank_k_ties" and route == "default":      # certified by the float64 re-rank of the band: the cheap path is not abandoned
        assert all(i["rejected"] <= max(1, nq // 20) for (nq, k), i in infos.items()), infos
        D, I = idx.search(q, 5)
        assert set(I[5][:4]) == extra["winners"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dim", [("cancellation_short", 96), ("cancellation_long", 96), ("plateau", 96), ("near_ties_one_list", 160),
                                      ("near_ties_three_lists", 160), ("duplicates", 160), ("rank_k_ties", 160), ("magnitudes", 160)])
def test_adversarial_store_without_a_plane(gpu, name, dim):
    _sweep(gpu, name, dim, "noplane")


def _search_check(idx, db, q, k, nprobe, route, coarse_tie_ok=False, what=""):
    idx.nprobe = nprobe
    assign, cent = idx.assignments(), idx.centroids()
    od, oi = assert_gaps(db, assign, cent, q, k, min(nprobe, len(cent)), coarse_tie_ok=coarse_tie_ok, what=what)
    D, I = idx.search(q, k)
    info = idx.last_search_info()
    _assert_route(info, route, len(q), what)
    _compare(D, I, od, oi, k, (what, info))
    return D, I


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", [("default", 128), ("f32", 128), ("rejected", 128), ("noplane", 96)])
def test_structure_edges(gpu, route, dim):
    """what the blob tests do not reach: an empty probed list, fewer than k rows in all probed lists, nprobe 1 with the home list
    empty, a trained index without rows, two equal centroids, a row appended between two searches that enters the top-k, one
    search issued on two streams alternately"""
    import torch
    nlist = 12
    cent, db = _blobs(3000, dim, nlist, 9701)
    cent[4] = cent[3]                                              # coarse tie: every row of blob 4 and blob 3 goes to list 3
    cent[7] = cent[6] + np.float32(0.5)                            # next to centroid 6 ...
    db = db[(np.arange(3000) * 7919) % nlist != 7]                 # ... and none of its blob's rows exist: list 7 stays nearly empty
    cent[11] = np.float32(40.0)                                    # a centroid far from every row: list 11 is empty
    lonely = (cent[11] + synth.rows(0, 3, dim, 9703)).astype(np.float32)
    q = (cent[(np.arange(40) * 5) % nlist] + synth.rows(0, 40, dim, 9705)).astype(np.float32)
    idx = _index(gpu, dim, nlist, route)
    idx.set_centroids(cent)
    # a trained index without rows: every slot unfilled
    idx.nprobe = 3
    D, I = idx.search(q, 5)
    assert np.all(I == -1) and np.all(np.isposinf(D))
    idx.add(db)
    assign = idx.assignments()
    np.testing.assert_array_equal(assign, cpu_assign(db, cent))
    assert (assign == 4).sum() == 0 and (assign == 11).sum() == 0 and (assign == 3).sum() >= 250
    # two equal centroids: the lower id is probed first (nprobe 1 from the queries of blob 3 / 4 must reach list 3, not the empty 4)
    D, I = _search_check(idx, db, q, 5, 1, route, coarse_tie_ok=True, what="coarse tie, nprobe 1")
    j34 = np.flatnonzero(np.isin((np.arange(40) * 5) % nlist, (3, 4)))
    assert len(j34) and np.all(I[j34] >= 0)
    # nprobe 1 with the home list empty: queries at centroid 11
    q11 = (cent[11] + np.float32(0.1) * synth.rows(0, 17, dim, 9707)).astype(np.float32)
    D, I = _search_check(idx, db, q11, 5, 1, route, what="home list empty")
    assert np.all(I == -1)
    # an empty list among the probed ones, and every list probed
    for nprobe in (2, 5, nlist):
        _search_check(idx, db, np.concatenate([q, q11]), 15, nprobe, route, coarse_tie_ok=nprobe >= 3, what=f"empty list probed, nprobe {nprobe}")
    # fewer than k rows in all probed lists together: three rows arrive in list 11
    idx.add(lonely)
    db2 = np.concatenate([db, lonely])
    D, I = _search_check(idx, db2, q11, 26, 1, route, what="fewer than k rows")
    assert np.all((I >= 0).sum(1) == 3) and set(I[0][:3]) == {len(db), len(db) + 1, len(db) + 2}
    # a row appended between two searches enters the top-k
    D0, I0 = _search_check(idx, db2, q, 5, 3, route, coarse_tie_ok=True, what="before the append")
    new = (q[:8] + np.float32(1e-3) * synth.rows(0, 8, dim, 9709)).astype(np.float32)
    idx.add(new)
    db3 = np.concatenate([db2, new])
    D1, I1 = _search_check(idx, db3, q, 5, 3, route, coarse_tie_ok=True, what="after the append")
    assert np.array_equal(I1[:8, 0], len(db2) + np.arange(8))
    old_only = (I1 < len(db2)).all(1)                              # (a new row may be a neighbour of other queries of its blob too)
    assert old_only.any() and np.array_equal(I1[old_only], I0[old_only])
    # the same search on two streams alternately
    s = [torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
    qd = torch.from_numpy(q).to(gpu)
    torch.cuda.synchronize()
    outs = []
    for it in range(6):
        with torch.cuda.stream(s[it % 2]):
            outs.append(idx.search_device(qd, 5))
    torch.cuda.synchronize()
    for Dd, Id in outs:
        assert np.array_equal(Id.cpu().numpy(), I1) and np.array_equal(Dd.cpu().numpy(), D1)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["default", "rejected"])
def test_plateau_full_width_cost(gpu, route):
    """store 5 with all 300 queries rejected at once (hi_scan=2) next to the default route: prints both times (DESIGN.md quotes them)"""
    import time
    import torch
    db, q, cent, nprobe, extra, assign, od, oi = prepared("plateau", 128)
    idx = _index(gpu, 128, len(cent), route)
    idx.set_centroids(cent)
    idx.add(db)
    idx.nprobe = nprobe
    qd = torch.from_numpy(q).to(gpu)
    for _ in range(3):
        D, I = idx.search_device(qd, 15)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20):
        D, I = idx.search_device(qd, 15)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / 20
    info = idx.last_search_info()
    print(f"plateau store, 300 queries, k 15, nprobe {nprobe}, route {route}: {ms:.3f} ms per search, {info}")
    _assert_route(info, route, 300, route)
    _compare(D.cpu().numpy(), I.cpu().numpy(), od, oi, 15, route)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_ivf_adversarial_fuzz(gpu, seed):
    """bounded sweep: store from {blobs, cancellation, shared-mean embeddings}, route from all four, trained centroids (k-means)"""
    from test_gpu_knn_large_k import _cancellation_store
    rng = np.random.default_rng(9800 + seed)
    for case in range(6):
        route = ("default", "f32", "rejected", "noplane")[(case + seed) % 4]
        dim = int(rng.choice([96, 160, 224])) if route == "noplane" else int(rng.choice([64, 128, 256]))
        kind = ("blobs", "cancellation", "embedding_like")[(case + 2 * seed) % 3]
        nlist = int(rng.choice([16, 50, 128]))
        n = int(rng.choice([3000, 12000, 30000]))
        nq = int(rng.choice([1, 2, 16, 17, 100, 400]))
        k = int(rng.choice(KS))
        nprobe = int(rng.choice([1, 3, 8, nlist]))
        s = 9900 + 100 * seed + case
        if kind == "blobs":
            _, db = _blobs(n, dim, 40, s)
            _, q = _blobs(nq, dim, 40, s); q = (q + np.float32(0.3) * synth.rows(0, nq, dim, s + 7)).astype(np.float32)
        elif kind == "cancellation":
            db, q = _cancellation_store(n, nq, dim, 20.0, s)
        else:       # one large positive common component, individual parts an order of magnitude smaller
            base = np.abs(synth.rows(0, 1, dim, s)) + np.float32(0.5)
            db = (base + np.float32(0.3) * synth.rows(0, n, dim, s + 1)).astype(np.float32)
            q = (base + np.float32(0.3) * synth.rows(0, nq, dim, s + 2)).astype(np.float32)
        idx = _index(gpu, dim, nlist, route, niter=int(rng.choice([0, 3])))
        idx.train(db[: min(n, 8000)])
        idx.add(db)
        what = dict(seed=seed, case=case, route=route, kind=kind, dim=dim, nlist=nlist, n=n, nq=nq, k=k, nprobe=nprobe)
        _search_check(idx, db, q, k, nprobe, route, what=str(what))
