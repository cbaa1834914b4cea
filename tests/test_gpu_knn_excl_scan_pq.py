"""Per-query exclusion sets on the certified tile scan (radad_knn_search_excl_scan_pq /
HipFlatIndex.search_excluding_per_query_in_scan): per query the k nearest rows whose tag is not among the query's own tags, with
the plain tile scan in front and k_excl_pq_scrub clearing each query's excluded rows out of the scan's buffers before every floor
and before the re-rank.

Expected results: tests/excl_per_query_ref.expected_pq, the float64 oracle over the rows AS STORED (under cosine: their inner
product with the device's radad_rownorm of the query).  Ids are compared exactly; distances within 1e-4 absolute on unit-norm data,
1e-6 relative and absolute on raw L2 / IP; padding -1 / NaN / NaN; float32(key) == dist bit for bit.  Wherever the tile route is
asserted, so is exact <= nq // 8: a floor raised by excluded rows does not produce wrong ids (the certificate sends the query to the
exact pass), so only that count shows a missing scrub.  It follows a precondition reported separately ("PRECONDITION"): a second
handle holding only the rows NO query of the batch excludes answers the plain certified search of the batch with
rechecked_queries == 0 -- the data itself does not push queries into the exact pass.

The stores are tests/excl_scan_pq_ref.speakers (tests/test_excl_scan_pq_model.py asserts on the CPU what they must be); the
two-phase store has the row count tests/knn_excl_scan_pq_plan_check.cpp prints."""
import numpy as np
import pytest

import excl_per_query_ref as P
import excl_scan_pq_ref as S

pytestmark = pytest.mark.gpu

METRICS = ("L2", "COSINE", "IP")
NQS = (40, 300)          # 300 crosses a 256-query tile
KS = (1, 10)


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _rownorm(gpu, q):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    qt = _dev(np.asarray(q, np.float32), gpu)
    out = torch.empty_like(qt)
    _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), out.data_ptr(), qt.shape[0], qt.shape[1], gpu.index or 0, _lib.stream_ptr(gpu)))
    return out.cpu().numpy()


def _mk(metric, dim, kind="uncentred", id_base=0, **kw):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    if kind == "f16":
        return HipFlatIndex(dim, m, 0, id_base, store_f16=True, **kw)
    return HipFlatIndex(dim, m, 0, id_base, centre=1 if kind == "centred" else 0, **kw)


class _Store:
    def __init__(self, gpu, metric, kind, db, tags, id_base=0, **kw):
        import torch
        self.gpu, self.metric, self.kind, self.id_base = gpu, metric, kind, id_base
        self.idx = _mk(metric, db.shape[1], kind, id_base, **kw)
        self.idx.add_device(_dev(np.asarray(db, np.float32), gpu))
        n = len(db)
        self.stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(id_base + r0, id_base + min(n, r0 + 65536), device=gpu)).cpu().numpy()
                                      for r0 in range(0, n, 65536)])
        self.tags = np.asarray(tags, np.int64)
        self.tags_t = _dev(self.tags, gpu)

    def search(self, q, k, qtags, qcnt=None):
        qt_t = None if qtags is None else _dev(np.asarray(qtags, np.int64), self.gpu)
        qc_t = None if qcnt is None else _dev(np.asarray(qcnt, np.int32), self.gpu)
        D, I, K64 = self.idx.search_excluding_per_query_in_scan(_dev(q, self.gpu), k, self.tags_t, qt_t, qc_t, return_f64=True)
        return D, I, K64, self.idx.last_excl_scan()

    def reference(self, q, k, qtags, qcnt=None):
        qtags = np.zeros((len(q), 0), np.int64) if qtags is None else qtags
        if self.metric == "COSINE":
            return P.expected_pq(self.stored, self.tags, qtags, qcnt, _rownorm(self.gpu, q), k, "IP", self.id_base)
        return P.expected_pq(self.stored, self.tags, qtags, qcnt, q, k, self.metric, self.id_base)


def _check(D, I, K64, ed, ei, metric):
    D, I, K64 = D.cpu().numpy(), I.cpu().numpy(), K64.cpu().numpy()
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    if metric == "COSINE":
        np.testing.assert_allclose(D[f], ed[f], rtol=0, atol=1e-4)
    else:
        np.testing.assert_allclose(D[f], ed[f], rtol=1e-6, atol=1e-6)
    assert np.all(np.isnan(D[~f])) and np.all(np.isnan(K64[~f]))                    # padding: -1 / NaN / NaN
    np.testing.assert_array_equal(K64[f].astype(np.float32), D[f])                  # out_dist is the key, rounded once


def _expect_tile(info, nq):
    assert info["route"] == "tile" and info["queries"] == nq, info
    assert info["exact"] <= nq // 8, info


def _precondition(s, q, k, qtags, qcnt, tile=True):
    """a second handle with only the rows no query of the batch excludes: its plain certified search rechecks nothing (tile=False:
    what is left of the store is too small for the tile scan, the fp32 tile kernels certify it)"""
    qt, cnt = P.clamp_counts(qtags, qcnt)
    excluded = np.unique(np.concatenate([qt[j, :cnt[j]] for j in range(len(qt))] + [np.zeros(0, np.int64)]))
    valid = np.flatnonzero(~np.isin(s.tags, excluded))
    h2 = _mk(s.metric, s.stored.shape[1], s.kind)
    h2.add_device(_dev(s.stored[valid], s.gpu))
    h2.search_device(_dev(q, s.gpu), k)
    launch = h2.last_launch()
    assert (launch["scan_kind"] == "hi_tile") == tile, f"PRECONDITION: the plain search of the rows nobody excludes: {launch}"
    assert launch["rechecked_queries"] == 0, f"PRECONDITION: the plain search of the rows nobody excludes rechecks {launch['rechecked_queries']} queries"


@pytest.fixture(scope="module")
def grid(gpu):
    """the 20 480 x 64 speakers store (4 speakers, c = 200, bystanders), one handle per (kind, metric); the oracle at k = 10, once"""
    cache = {}

    def get(kind, metric):
        if (kind, metric) not in cache:
            db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["grid"])
            if kind == "centred":
                db, q = S.with_common_component(db, q)
            s = _Store(gpu, metric, kind, db, tags)
            s.q, s.qtags, s.qcnt, s.info = q, qtags, qcnt, info
            s.ed, s.ei = s.reference(q, max(KS), qtags, qcnt)                       # a top-k list is a prefix of the top-10 list
            cache[(kind, metric)] = s
        return cache[(kind, metric)]
    yield get
    cache.clear()


# ---- 1: the grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", S.KINDS)
def test_1_grid(gpu, grid, kind, metric):
    s = grid(kind, metric)
    for nq in NQS:
        own = s.info["owner"][:nq]
        assert own.any() and (~own).any()
        _precondition(s, s.q[:nq], max(KS), s.qtags[:nq], s.qcnt[:nq])
        for k in KS:
            D, I, K64, info = s.search(s.q[:nq], k, s.qtags[:nq], s.qcnt[:nq])
            print(f"{kind} {metric} nq {nq} k {k}: {info}")
            _check(D, I, K64, s.ed[:nq, :k], s.ei[:nq, :k], metric)
            _expect_tile(info, nq)
            I = I.cpu().numpy()
            for j in (0, nq - 1, int(np.flatnonzero(~own)[0])):                     # owners never see their crowd, bystanders see nothing else
                assert np.isin(I[j], s.info["crowd"][s.info["speaker"][j]]).all() == (not own[j])
                assert own[j] == (not np.isin(I[j], s.info["crowd"][s.info["speaker"][j]]).any())


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_1_mutual_windows_on_the_tile_route(gpu, metric):
    """excl_per_query_ref.mutual at 20 480 rows: eight identical queries per group, eight different windows of excluded rows"""
    db, q, tags, qtags, qcnt, rows = P.mutual(20480, 64, 5, 9150)
    s = _Store(gpu, metric, "uncentred", db, tags)
    ed, ei = s.reference(q, 10, qtags, qcnt)
    D, I, K64, info = s.search(q, 10, qtags, qcnt)
    print(f"mutual {metric}: {info}")
    _check(D, I, K64, ed, ei, metric)
    _precondition(s, q, 10, qtags, qcnt)
    _expect_tile(info, len(q))
    assert len({tuple(r) for r in I.cpu().numpy()[:8]}) > 1                      # same vector, different admissible sets, different rows


# ---- 2: c = 1500, more than any k_fetch can prove ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_2_a_crowd_of_1500(gpu, metric):
    import torch
    db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["c1500"])
    s = _Store(gpu, metric, "uncentred", db, tags)
    ed, ei = s.reference(q, 10, qtags, qcnt)
    _precondition(s, q, 10, qtags, qcnt, tile=False)                              # (14 480 rows are left: below the tile scan's 16 384)
    D, I, K64, xs = s.search(q, 10, qtags, qcnt)
    counts, _ = s.idx.last_emitted(len(q))
    print(f"c 1500 {metric}: {xs}, emitted min {counts.min()} max {counts.max()} (owners >= 1500: the scrubbed rows are counted)")
    _check(D, I, K64, ed, ei, metric)
    _expect_tile(xs, len(q))
    assert (counts[info["owner"]] >= 1500).all() and counts.max() <= 4096         # emitted INCLUDING what the scrub cleared; it fits
    # the over-fetch call on the same handle cannot prove an owner at any k_fetch: same rows, bit-equal keys, every owner exact
    _, I2, K2 = s.idx.search_excluding_per_query(_dev(q, gpu), 10, s.tags_t, _dev(qtags, gpu), _dev(qcnt, gpu), k_fetch=1024, return_f64=True)
    assert torch.equal(I2, I) and torch.equal(K2.view(torch.int64), K64.view(torch.int64))
    assert s.idx.last_excl()["exact"] == int(info["owner"].sum()), (s.idx.last_excl(), int(info["owner"].sum()))


# ---- 3: c = 5000 overflows the buffer ------------------------------------------------------------------------------------------------------
def test_3_a_crowd_of_5000_overflows_and_is_answered_exactly(gpu):
    import torch
    db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["c5000"])
    assert info["owner"].sum() == 8
    s = _Store(gpu, "L2", "uncentred", db, tags)
    qt = _dev(q, gpu)
    D0, I0 = s.idx.search_device(qt, 10)
    torch.cuda.synchronize()
    s.idx.search_device(qt, 10)                                                   # (consumes the first search's report)
    torch.cuda.synchronize()
    before = s.idx.tuning_info()
    ed, ei = s.reference(q, 10, qtags, qcnt)
    D, I, K64, xs = s.search(q, 10, qtags, qcnt)
    counts, _ = s.idx.last_emitted(len(q))
    print(f"c 5000: {xs}, emitted by the owners {counts[info['owner']]}")
    _check(D, I, K64, ed, ei, "L2")
    assert xs["route"] == "tile" and xs["exact"] >= 8, xs
    assert (counts[info["owner"]] > 4096).all()
    torch.cuda.synchronize()
    assert s.idx.tuning_info() == before
    D1, I1 = s.idx.search_device(qt, 10)
    torch.cuda.synchronize()
    s.idx.search_device(qt, 10)
    after = s.idx.tuning_info()
    assert after["cap_boost"] == before["cap_boost"] and after["fp32_searches_left"] == before["fp32_searches_left"] == 0, (before, after)
    assert s.idx.last_launch()["scan_kind"] == "hi_tile" and torch.equal(I1, I0) and torch.equal(D1, D0)


# ---- 4: two phases -- the scrub in front of k_kth_floor ------------------------------------------------------------------------------------
def test_4_two_phases(gpu):
    db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["two_phase"])
    k, first = 100, 131072
    assert len(db) == S.TWO_PHASE_ROWS and (info["crowd"] < first).any(axis=1).all() and (info["crowd"] >= first).any(axis=1).all()
    s = _Store(gpu, "L2", "uncentred", db, tags)
    ed, ei = s.reference(q, k, qtags, qcnt)
    _precondition(s, q, k, qtags, qcnt)
    D, I, K64, xs = s.search(q, k, qtags, qcnt)
    launch = s.idx.last_launch()
    print(f"two phases: {xs}, scan_phases {launch['scan_phases']}")
    assert launch["scan_phases"] >= 2, launch
    _check(D, I, K64, ed, ei, "L2")
    _expect_tile(xs, len(q))


# ---- 5: the rule's edge cases --------------------------------------------------------------------------------------------------------------
def test_5_sixty_four_tags_counts_duplicates_and_order(gpu, grid):
    s = grid("uncentred", "L2")
    nq = 40
    q = s.q[:nq]
    _, near = P.expected_pq(s.stored, s.tags, s.qtags[:nq], None, q, 63, "L2")
    rng = np.random.default_rng(9501)
    qtags = np.concatenate([s.qtags[:nq], s.tags[near]], axis=1)                  # the speaker's tag and the 63 nearest rows behind its crowd
    for j in range(nq):
        qtags[j] = qtags[j][rng.permutation(64)]                                  # arbitrary order
        qtags[j, 1::7] = qtags[j, 0]                                              # duplicates
    qcnt = np.array([0, 1, 2, 7, 31, 32, 33, 63, 64, 64] * 4, np.int32)
    for cnt in (qcnt, None, np.where(np.arange(nq) % 3 == 0, -5, 1000).astype(np.int32)):      # None = 64 for all; outside [0, m]: clamped
        ed, ei = s.reference(q, 10, qtags, cnt)
        D, I, K64, info = s.search(q, 10, qtags, cnt)
        _check(D, I, K64, ed, ei, "L2")
        assert info["route"] == "tile", info


def test_5_nothing_excluded_is_the_plain_search(gpu, grid):
    import torch
    for kind, metric in (("uncentred", "L2"), ("centred", "COSINE"), ("f16", "IP")):
        s = grid(kind, metric)
        for nq in NQS:
            qt = _dev(s.q[:nq], gpu)
            D0, I0, K0 = s.idx.search_device(qt, 10, return_f64=True)
            zero = _dev(np.zeros(nq, np.int32), gpu)
            for args in ((None, None), (_dev(s.qtags[:nq], gpu), zero)):              # m == 0 (no tags at all), and all-zero counts
                D, I, K64 = s.idx.search_excluding_per_query_in_scan(qt, 10, None if args[0] is None else s.tags_t, *args, return_f64=True)
                info = s.idx.last_excl_scan()
                assert torch.equal(I, I0) and torch.equal(K64.view(torch.int64), K0.view(torch.int64)) and torch.equal(D, D0)
                _expect_tile(info, nq)


def test_5_one_set_for_all_is_the_batch_call(gpu, grid):
    import torch
    s = grid("uncentred", "L2")
    nq = 40
    S_set = np.array([S.SPEAKER_TAG0 + 2, s.tags[5], S.SPEAKER_TAG0, s.tags[77], s.tags[5]], np.int64)      # any order, a duplicate
    qt = _dev(s.q[:nq], gpu)
    D, I, K64 = s.idx.search_excluding_per_query_in_scan(qt, 10, s.tags_t, _dev(np.tile(S_set, (nq, 1)), gpu), None, return_f64=True)
    assert s.idx.last_excl_scan()["route"] == "tile"
    Db, Ib, Kb = s.idx.search_excluding_in_scan(qt, 10, s.tags_t, _dev(np.unique(S_set), gpu), return_f64=True)
    assert s.idx.last_excl_scan()["route"] == "tile"
    assert torch.equal(I, Ib) and torch.equal(K64.view(torch.int64), Kb.view(torch.int64)) and torch.equal(D.view(torch.int32), Db.view(torch.int32))


# ---- 6: a query's result is a function of that query alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_6_batch_independence(gpu, grid, metric):
    import torch
    s = grid("uncentred", metric)
    _, I40, K40, _ = s.search(s.q[:40], 10, s.qtags[:40], s.qcnt[:40])
    _, I300, K300, _ = s.search(s.q, 10, s.qtags, s.qcnt)
    for j in (3, 29):                                                             # an owner and a bystander (queries 28 .. 31)
        assert bool(s.info["owner"][j]) == (j == 3)
        sel = np.concatenate([[j], np.arange(100, 116)])                          # alone among 16 fillers: 17 queries, the tile route
        _, I17, K17, info = s.search(s.q[sel], 10, s.qtags[sel], s.qcnt[sel])
        assert info["route"] == "tile" and info["queries"] == 17
        for Ix, Kx in ((I40, K40), (I300, K300)):
            assert torch.equal(I17[0], Ix[j]) and torch.equal(K17[0].view(torch.int64), Kx[j].view(torch.int64))


# ---- 7: the exact route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["16_queries", "4096_rows", "k_200", "dim_68", "plane_off"])
def test_7_exact_route(gpu, shape):
    n, dim, nq, k, kw = {"16_queries": (20480, 64, 16, 10, {}), "4096_rows": (4096, 64, 40, 10, {}), "k_200": (20480, 64, 40, 200, {}),
                         "dim_68": (20480, 68, 40, 10, {}), "plane_off": (20480, 64, 40, 10, {"hi_plane": 0})}[shape]
    db, q, tags, qtags, qcnt, info = S.speakers(n, dim, 4, 200, nq, 9700, k_max=10)
    for metric in ("L2", "COSINE"):
        s = _Store(gpu, metric, "uncentred", db, tags, **kw)
        ed, ei = s.reference(q, k, qtags, qcnt)
        D, I, K64, xs = s.search(q, k, qtags, qcnt)
        print(f"{shape} {metric}: {xs}")
        _check(D, I, K64, ed, ei, metric)
        assert xs == {"queries": nq, "route": "exact", "exact": nq}, xs
        D, I, K64, xs = s.search(q, k, None)                                      # m == 0 on the exact route: no tags at all
        _check(D, I, K64, *s.reference(q, k, None), metric)
        assert xs == {"queries": nq, "route": "exact", "exact": nq}, xs


# ---- 8: two row shards, merged by radad_topk_merge_f64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_8_two_shards_merge_exactly(gpu, metric):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    db, q, tags, qtags, qcnt, info = S.speakers(**S.SHAPES["shards"])
    n, half, nq, k = len(db), len(db) // 2, len(q), 10
    whole = _Store(gpu, metric, "uncentred", db, tags)
    ed, ei = whole.reference(q, k, qtags, qcnt)
    keys, ids = [], []
    for r in range(2):
        sh = _Store(gpu, metric, "uncentred", db[r * half:(r + 1) * half], tags[r * half:(r + 1) * half], id_base=r * half)
        _, Ir, Kr, info_r = sh.search(q, k, qtags, qcnt)
        print(f"{metric} shard {r}: {info_r}")
        _expect_tile(info_r, nq)
        er_d, er_i = sh.reference(q, k, qtags, qcnt)
        np.testing.assert_array_equal(Ir.cpu().numpy(), er_i)                     # the shard's own exact admissible top k, global ids
        keys.append(Kr)
        ids.append(Ir)
    kd, idd = torch.stack(keys).contiguous(), torch.stack(ids).contiguous()
    od = torch.empty((nq, k), device=gpu)
    oi = torch.empty((nq, k), device=gpu, dtype=torch.int64)
    ok = torch.empty((nq, k), device=gpu, dtype=torch.float64)
    m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
    _lib.check(_lib.load().radad_topk_merge_f64(m, kd.data_ptr(), idd.data_ptr(), 2, nq, k, od.data_ptr(), oi.data_ptr(), ok.data_ptr(),
                                                gpu.index or 0, _lib.stream_ptr(gpu)), "radad_topk_merge_f64")
    _check(od, oi, ok, ed, ei, metric)


# ---- 9: the early abandon changes nothing ------------------------------------------------------------------------------------------------------
def test_9_abandon_on_and_off(gpu):
    """a store built like tests/test_gpu_knn_abandon.py's: queries around one vector, near-duplicates planted in every third tile; the
    rows planted for query j carry tag j and query j excludes them -- its floor then comes from the other queries' planted rows"""
    # (20 000 rows: 78 tiles, the sample takes every 9th -- tiles that hold planted rows, as there; the planted rows of a tile sit in
    # four of the sample's eight 2-entry holders, so that a query's floor survives the loss of its own)
    n, dim, nq, k = 20000, 128, 40, 10
    rng = np.random.default_rng(9901)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    ids = np.array([t * 256 + 16 * i + 3 + 4 * (i % 4) for t in range(0, n // 256, 3) for i in range(8)], np.int64)
    owner_of = np.arange(len(ids)) % nq
    db[ids] = q[owner_of] + (0.03 * amp * rng.standard_normal((len(ids), dim))).astype(np.float32)
    tags = np.arange(n, dtype=np.int64) * 7 + 11
    tags[ids] = S.SPEAKER_TAG0 + owner_of
    qtags = (S.SPEAKER_TAG0 + np.arange(nq)).reshape(nq, 1)
    s = _Store(gpu, "COSINE", "uncentred", db, tags)
    ed, ei = s.reference(q, k, qtags)
    out = {}
    for ab in (0, 1):
        s.idx.set_abandon(ab)
        D, I, K64, xs = s.search(q, k, qtags)
        out[ab] = (D.cpu().numpy(), I.cpu().numpy(), K64.cpu().numpy(), s.idx.last_emitted(nq), s.idx.last_launch()["early_abandon"], xs)
        _check(D, I, K64, ed, ei, "COSINE")
        _expect_tile(xs, nq)
    print(f"abandon off {out[0][4]}, on {out[1][4]}")
    assert out[0][4] == {"checked": 0, "skipped": 0, "tasks": 0} and out[1][4]["skipped"] > 0, (out[0][4], out[1][4])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2].view(np.int64), out[1][2].view(np.int64))
    assert np.array_equal(out[0][3][0], out[1][3][0]) and np.array_equal(out[0][3][1], out[1][3][1])      # emitted counts and floors too


# ---- 10: the handle's state --------------------------------------------------------------------------------------------------------------------
def test_10_state_is_left_alone(gpu, grid):
    import torch
    s = grid("uncentred", "L2")
    qt = _dev(s.q[:256], gpu)
    D0, I0 = s.idx.search_device(qt, 10)
    torch.cuda.synchronize()
    s.idx.search_device(qt, 10)                                                   # (consumes the first search's report)
    cert, tuning, rebuilds = s.idx.last_launch()["certificate"], s.idx.tuning_info(), s.idx.plane_info()["rebuilds"]
    assert cert["queries"] == 256
    D, I, K64, xs = s.search(s.q, 10, s.qtags, s.qcnt)                            # 300 queries: another batch size than the plain search's
    _expect_tile(xs, 300)
    assert s.idx.last_launch()["certificate"] == cert                             # still the plain search's
    assert s.idx.tuning_info() == tuning and s.idx.plane_info()["rebuilds"] == rebuilds
    D1, I1 = s.idx.search_device(qt, 10)
    assert s.idx.last_launch()["scan_kind"] == "hi_tile" and torch.equal(I1, I0) and torch.equal(D1, D0)
    after = s.idx.tuning_info()
    assert after["cap_boost"] == tuning["cap_boost"] and after["fp32_searches_left"] == 0


# ---- 11: arguments and the wrappers that refuse ----------------------------------------------------------------------------------------------
def test_11_arguments(gpu, grid):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipIVFFlatIndex, _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    s = grid("uncentred", "L2")
    nq = 20
    qt = _dev(s.q[:nq], gpu)
    qtags_t = _dev(s.qtags[:nq], gpu)
    D0, I0 = s.idx.search_device(qt, 5)
    D = torch.full((nq, 5), 7.0, device=gpu)
    I = torch.full((nq, 5), 7, device=gpu, dtype=torch.int64)
    lib = _lib.load()

    def call(h, q_ptr, n, k, tags, qtags, m):
        return lib.radad_knn_search_excl_scan_pq(h, q_ptr, _lib.Q_F32, n, k, tags, qtags, m, None, D.data_ptr(), I.data_ptr(), None,
                                                 _lib.stream_ptr(gpu))
    for m in (-1, 65):                                                            # a bad m, before anything is enqueued
        with pytest.raises(ValueError, match="RADAD_EXCL_PQ_MAX_TAGS"):
            _lib.check(call(s.idx._h, qt.data_ptr(), nq, 5, s.tags_t.data_ptr(), qtags_t.data_ptr(), m))
    with pytest.raises(ValueError):                                               # tags per query without the query tags ...
        _lib.check(call(s.idx._h, qt.data_ptr(), nq, 5, s.tags_t.data_ptr(), None, 1))
    with pytest.raises(ValueError):                                               # ... or without the row tags
        _lib.check(call(s.idx._h, qt.data_ptr(), nq, 5, None, qtags_t.data_ptr(), 1))
    for k in (0, 1025):
        with pytest.raises(ValueError):
            s.idx.search_excluding_per_query_in_scan(qt, k, s.tags_t, qtags_t)
    torch.cuda.synchronize()
    assert bool((D == 7.0).all()) and bool((I == 7).all())                        # nothing was written
    _lib.check(call(s.idx._h, qt.data_ptr(), 0, 5, None, None, 0))                # nq == 0: OK
    s.idx.search_begin(qt, 5)
    with pytest.raises(ValueError, match="begin"):                                # a begun search owns the handle
        s.idx.search_excluding_per_query_in_scan(qt, 5, s.tags_t, qtags_t)
    s.idx.search_abort()
    with pytest.raises(ValueError, match="empty"):                                # an empty store: RADAD_ESTATE
        _mk("L2", 64).search_excluding_per_query_in_scan(qt, 5, None, None)
    wide = _mk("L2", 16384)                                                       # the width x k limit, before anything is enqueued
    wide.add(np.zeros((4, 16384), np.float32))
    with pytest.raises(ValueError, match="too large"):
        wide.search_excluding_per_query_in_scan(torch.zeros((2, 16384), device=gpu), 1024, None, None)
    with pytest.raises(ValueError, match="search_probed_excluding_per_query"):
        HipIVFFlatIndex(64, 64).search_excluding_per_query_in_scan(qt, 5, None, None)
    with pytest.raises(ValueError, match="search_excluding_per_query_in_scan"):
        ShardedSearch(None, _lib.METRIC_L2).search_excluding_per_query_in_scan(qt, 5)
    qb = qt.bfloat16()                                                            # bf16 queries, as every search takes them
    Db, Ib = s.idx.search_excluding_per_query_in_scan(qb, 5, s.tags_t, qtags_t, _dev(s.qcnt[:nq], gpu))
    _, ei = s.reference(qb.float().cpu().numpy(), 5, s.qtags[:nq], s.qcnt[:nq])
    np.testing.assert_array_equal(Ib.cpu().numpy(), ei)
    assert s.idx.last_excl_scan()["route"] == "tile"
    D1, I1 = s.idx.search_device(qt, 5)                                           # after the refused calls a plain search still works
    assert torch.equal(I1, I0) and torch.equal(D1, D0)


# ---- 12: retrieve_similar_vectors, every clip excluding its own basename -------------------------------------------------------------------------
def test_12_pipeline_scope_query_in_scan(gpu, tmp_path):
    import os
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    from oracle import synth

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")

    def pipeline(**knobs):
        cfg = R.Config()
        cfg.update(device=gpu, feature_dim=64, tpp_levels=[1], top_k=5, vector_db_index_type="L2",
                   vector_db_path=str(tmp_path / ("vdb_" + "_".join(knobs))), **knobs)
        return R.HotPathPipeline(cfg, feature_extractor=NoExtractor()), cfg

    n, nq, per = 20480, 24, 60
    pipe, cfg = pipeline(exact_exclusion=True, exclusion_scope="query", exclusion_per_query_in_scan=True)
    dim = pipe.tpp.get_output_dim()
    rng = np.random.default_rng(9991)
    db, q = synth.rows(0, n, dim, 9992), synth.rows(0, nq, dim, 9993)
    paths = [f"/data/d{i}/f{i}.wav" for i in range(n)]
    mine = rng.choice(n, nq * per, replace=False).reshape(nq, per)               # 60 rows share each query's basename, and crowd it
    for j in range(nq):
        db[mine[j]] = q[j] + 0.05 * rng.standard_normal((per, dim)).astype(np.float32)
        for i in mine[j]:
            paths[i] = f"/data/d{i}/clip{j}.wav"
    labels = [float(i % 2) for i in range(n)]
    pipe.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * n})
    qpaths = [f"/eval/clip{j}.wav" for j in range(nq)]
    qd = torch.from_numpy(q).to(gpu)
    vec, lbl, rp, dist = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, exclude_self=True, return_info=True, return_distances=True)
    tags = np.array([path_tag(p) for p in paths], np.int64)
    own = np.array([[path_tag(os.path.basename(p))] for p in qpaths], np.int64)
    ed, ei = P.expected_pq(db, tags, own, None, q, cfg.top_k, "L2")
    assert (ei >= 0).all()
    assert rp == [[paths[i] for i in row] for row in ei]                          # K admissible neighbours per clip
    assert all(os.path.basename(x) != os.path.basename(qpaths[j]) for j, row in enumerate(rp) for x in row)
    np.testing.assert_array_equal(vec.cpu().numpy(), db[ei])
    np.testing.assert_allclose(dist.cpu().numpy(), ed, rtol=1e-6, atol=1e-6)
    info = pipe.vector_db.index.last_excl_scan()
    assert info["route"] == "tile" and info["queries"] == nq and info["exact"] <= nq // 8, info
    # exclusion_in_scan with scope "query" still raises; the new knob needs scope "query" and exact_exclusion; it is off by default
    cfg.exclusion_in_scan = True
    with pytest.raises(ValueError, match="exclusion_in_scan"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths, exclude_self=True)
    cfg.exclusion_in_scan = False
    cfg.exclusion_scope = "batch"
    with pytest.raises(ValueError, match="exclusion_per_query_in_scan"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths, exclude_self=True)
    assert R.Config().exclusion_per_query_in_scan is False
