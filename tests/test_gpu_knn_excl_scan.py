"""Exclusion inside the certified tile scan (radad_knn_search_excl_scan / HipFlatIndex.search_excluding_in_scan): the k nearest rows
whose tag is not excluded, with the admission test in the scan itself -- a per-call bias array that is NaN for the excluded rows -- so
that the cost does not depend on how much of the store is excluded (the reference's training_file_ids mode, pipeline.py:500-502).

Expected results: tests/exclusion_ref.expected_excluding, the float64 oracle over the admissible rows AS STORED (under cosine: their
inner product with the device's normalised query), ids remapped; ids are compared exactly, distances with the tolerances of tests/test_gpu_knn_exclusion.py (1e-4 absolute on unit-norm data, 1e-6 on raw
L2 / IP).  Where a case says so the result is also compared with radad_knn_search_excl at k_fetch = min(1024, ntotal) on the same
handle: ids equal, float64 keys bit-equal.

Route.  The tile route is taken exactly when the plain search of the batch takes RADAD_SCAN_HI_TILE.  On the 20 480 x 64 stores of
case 1 that is k = 1 and k = 10; k = 128 is NOT a tile-scan shape there (the sample pre-pass of a 20 480-row store holds 8 tiles x 16
entries, the floor's rank 2 (k + 6) must exist in it: k <= 58 -- knn_tile_eligibility), the plain search reports the fp32 tile kernel,
so the new call reports the exact route and the test asserts THAT; k = 128 on the tile route is asserted on a 49 152-row store
(test_k128_on_the_tile_route).  Wherever the tile route is asserted, so is n_exact <= nq / 8, after a precondition reported
separately ("PRECONDITION"): a second handle holding only the admissible rows, in order, answers the plain certified search with
radad_knn_last_recheck == 0 and the same rows after mapping its ids back."""
import numpy as np
import pytest

from exclusion_ref import crowded, expected_excluding
from oracle import synth

pytestmark = pytest.mark.gpu

N1, DIM1 = 20480, 64
KS = (1, 10, 128)
NQS = (40, 300)          # 300 crosses a 256-query tile
METRICS = ("L2", "COSINE", "IP")
STORES = ("centred", "uncentred", "f16")
TILE_K_MAX_N1 = 58       # largest k the tile scan takes on a 20 480-row store (see above)


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


def _mk(metric, dim, kind="uncentred", id_base=0):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    if kind == "f16":
        return HipFlatIndex(dim, m, 0, id_base, store_f16=True)
    return HipFlatIndex(dim, m, 0, id_base, centre=1 if kind == "centred" else 0)


def _data(kind, n, dim, nq, seed):
    """rows and queries; the centred stores share a common component (what centring is for)"""
    db, q = synth.rows(0, n, dim, seed), synth.rows(0, nq, dim, seed + 1)
    if kind == "centred":
        db, q = db + np.float32(0.25), q + np.float32(0.25)
    return db, q


class _Store:
    def __init__(self, gpu, metric, kind, db, tags=None, id_base=0):
        import torch
        self.gpu, self.metric, self.kind, self.id_base = gpu, metric, kind, id_base
        self.idx = _mk(metric, db.shape[1], kind, id_base)
        self.idx.add(db)
        n = len(db)
        self.stored = self.idx.reconstruct_batch(torch.arange(id_base, id_base + n, device=gpu)).cpu().numpy()
        self.tags = (np.arange(n, dtype=np.int64) * 7 + 11) if tags is None else np.asarray(tags, np.int64)
        self.tags_t = _dev(self.tags, gpu)

    def search(self, q, k, excl):
        excl_t = None if excl is None else _dev(np.asarray(excl, np.int64), self.gpu)
        D, I, K64 = self.idx.search_excluding_in_scan(_dev(q, self.gpu), k, self.tags_t, excl_t, return_f64=True)
        return D, I, K64, self.idx.last_excl_scan()

    def reference(self, q, k, excl):
        """the float64 oracle over the admissible rows as the store holds them; under cosine the stored rows are the normalised ones
        and the query is the device's radad_rownorm of it (as tests/test_gpu_knn_widths.py does), so the key is their inner product"""
        if self.metric == "COSINE":
            return expected_excluding(self.stored, self.tags, excl, _rownorm(self.gpu, q), k, "IP", self.id_base)
        return expected_excluding(self.stored, self.tags, excl, q, k, self.metric, self.id_base)

    def plane(self):
        return self.idx.plane_info()


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


def _same_as_search_excl(s, q, k, excl, I, K64):
    """radad_knn_search_excl at k_fetch = min(1024, ntotal) on the same handle: ids equal, float64 keys bit-equal"""
    import torch
    excl_t = None if excl is None else _dev(np.asarray(excl, np.int64), s.gpu)
    _, I2, K2 = s.idx.search_excluding(_dev(q, s.gpu), k, s.tags_t, excl_t, k_fetch=min(1024, len(s.stored)), return_f64=True)
    assert torch.equal(I2, I)
    f = I >= 0
    assert torch.equal(K2[f].view(torch.int64), K64[f].view(torch.int64))


def _precondition(s, q, k, excl, ei):
    """a second handle with the admissible rows only, in order: its plain certified search rechecks nothing and returns the same rows"""
    valid = np.flatnonzero(~np.isin(s.tags, np.asarray([] if excl is None else excl, np.int64)))
    h2 = _mk(s.metric, s.stored.shape[1], s.kind)
    h2.add(s.stored[valid])
    _, I2 = h2.search_device(_dev(q, s.gpu), k)
    rechecked = h2.last_launch()["rechecked_queries"]
    assert rechecked == 0, f"PRECONDITION: the plain search of the admissible rows alone rechecks {rechecked} queries on these inputs"
    I2 = I2.cpu().numpy()
    back = np.where(I2 >= 0, valid[np.clip(I2, 0, None)] + s.id_base, -1)
    assert np.array_equal(back, ei), "PRECONDITION: the plain search of the admissible rows alone returns other rows"


def _expect_tile(info, nq):
    assert info["route"] == "tile" and info["queries"] == nq, info
    assert info["exact"] <= nq // 8, info


def _plain_kind(s, q, k):
    s.idx.search_device(_dev(q, s.gpu), k)
    return s.idx.last_launch()["scan_kind"]


def _random_excl(tags, fraction, seed):
    n = len(tags)
    return np.unique(tags[np.random.default_rng(seed).choice(n, int(n * fraction), replace=False)])


@pytest.fixture(scope="module")
def stores(gpu):
    """the 20 480 x 64 stores of case 1, one per (kind, metric), with 300 queries"""
    cache = {}

    def get(kind, metric):
        if (kind, metric) not in cache:
            db, q = _data(kind, N1, DIM1, 300, 7100 + 10 * STORES.index(kind))
            s = _Store(gpu, metric, kind, db)
            s.q = q
            cache[(kind, metric)] = s
        return cache[(kind, metric)]
    yield get
    cache.clear()


# ---- case 1: 20 480 x 64, 40 and 300 queries, k in {1, 10, 128}; centred, un-centred and fp16 stores; L2, cosine, IP -------------------
@pytest.mark.parametrize("excl_kind", ["none", "half", "most"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", STORES)
def test_case1_exclusion_sets(gpu, stores, kind, metric, excl_kind):
    import torch
    s = stores(kind, metric)
    excl = {"none": None, "half": _random_excl(s.tags, 0.5, 7201), "most": _random_excl(s.tags, 0.9, 7202)}[excl_kind]
    ed, ei = s.reference(s.q, max(KS), excl)                                 # once: a top-k list is a prefix of the top-128 list
    for nq in NQS:
        for k in KS:
            q = s.q[:nq]
            D, I, K64, info = s.search(q, k, excl)
            print(f"{kind} {metric} {excl_kind} nq {nq} k {k}: {info}, plane {s.plane()}")
            _check(D, I, K64, ed[:nq, :k], ei[:nq, :k], metric)
            if k <= TILE_K_MAX_N1:
                if excl is not None:
                    _precondition(s, q, k, excl, ei[:nq, :k])
                _expect_tile(info, nq)
            else:                                                            # not a tile-scan shape on this store (module docstring)
                assert _plain_kind(s, q, k) != "hi_tile"
                assert info == {"queries": nq, "route": "exact", "exact": nq}, info
            if excl is None:
                # n_excl = 0: ids and the keys of filled slots equal radad_knn_search_f64's
                D0, I0, K0 = s.idx.search_device(_dev(q, gpu), k, return_f64=True)
                assert torch.equal(I, I0) and torch.equal(K64.view(torch.int64), K0.view(torch.int64))
            elif nq == 40:
                _same_as_search_excl(s, q, k, excl, I, K64)
    if kind != "f16":
        p = s.plane()
        assert p["built"] and p["centred"] == (kind == "centred"), p         # un-centred IP / cosine: RSC 0 / 1 ran as 3 / 2


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", STORES)
def test_case1_crowded(gpu, kind, metric):
    """the crowded() stores of tests/exclusion_ref.py: 300 excluded near-duplicates in front of EVERY query (40 queries: 300 queries x
    300 duplicates do not fit 20 480 rows)"""
    db, q, tags, excl, which = crowded(N1, DIM1, 40, 40, 300, 7301)
    if kind == "centred":
        db, q = db + np.float32(0.25), q + np.float32(0.25)
    s = _Store(gpu, metric, kind, db, tags)
    assert len(which) == 40 and np.isin(tags, excl).sum() >= 40 * 300
    ed, ei = s.reference(q, max(KS), excl)
    for k in KS:
        D, I, K64, info = s.search(q, k, excl)
        print(f"{kind} {metric} crowded k {k}: {info}")
        _check(D, I, K64, ed[:, :k], ei[:, :k], metric)
        assert info["route"] == ("tile" if k <= TILE_K_MAX_N1 else "exact"), info
        _same_as_search_excl(s, q, k, excl, I, K64)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", STORES)
def test_case1_padding(gpu, stores, kind, metric):
    """all but k - 3 rows excluded (k = 1: none left), and every row excluded: -1 / NaN / NaN"""
    s = stores(kind, metric)
    rng = np.random.default_rng(7401)
    for nq in NQS:
        for k in KS:
            keep = np.sort(rng.choice(N1, max(k - 3, 0), replace=False))
            excl = np.unique(np.delete(s.tags, keep))
            ed, ei = s.reference(s.q[:nq], k, excl)
            assert (ei >= 0).sum(axis=1).max() == max(k - 3, 0)
            D, I, K64, info = s.search(s.q[:nq], k, excl)
            print(f"{kind} {metric} all but {max(k - 3, 0)} nq {nq} k {k}: {info}")
            _check(D, I, K64, ed, ei, metric)
            assert info["route"] == ("tile" if k <= TILE_K_MAX_N1 else "exact"), info
        D, I, K64, info = s.search(s.q[:nq], 10, np.unique(s.tags))
        assert info["route"] == "tile", info
        assert np.all(I.cpu().numpy() == -1) and np.all(np.isnan(D.cpu().numpy())) and np.all(np.isnan(K64.cpu().numpy()))


@pytest.mark.parametrize("metric", METRICS)
def test_case1_excluded_bit_copies_tie_to_the_lower_admissible_id(gpu, metric):
    """every excluded row (3 i + 1) is a bit-copy of an admissible row with a lower (3 i) and a higher (3 i + 2) id"""
    db, q = _data("uncentred", N1, DIM1, 40, 7501)
    n3 = N1 // 3
    db[1:3 * n3:3] = db[0:3 * n3:3]
    db[2:3 * n3:3] = db[0:3 * n3:3]
    s = _Store(gpu, metric, "uncentred", db)
    excl = np.unique(s.tags[1:3 * n3:3])
    ed, ei = s.reference(q, 10, excl)
    D, I, K64, info = s.search(q, 10, excl)
    print(f"{metric} bit copies: {info}")
    _check(D, I, K64, ed, ei, metric)
    I = I.cpu().numpy()
    assert np.all(I[:, 0::2] % 3 == 0) and np.all(I[:, 1::2] == I[:, 0::2] + 2)      # (3 i, 3 i + 2) pairs, the lower id first
    assert info["route"] == "tile", info
    _same_as_search_excl(s, q, 10, excl, _dev(I, gpu), K64)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", STORES)
def test_case1_excluded_rows_of_100x_the_norm(gpu, kind, metric):
    """the excluded rows have 100x the norm of the rest: they move eps (the maxima over ALL rows bound the admitted ones) and must
    never appear"""
    db, q = _data(kind, N1, DIM1, 300, 7601)
    big = np.random.default_rng(7602).choice(N1, N1 // 2, replace=False)
    db[big] *= np.float32(100.0)
    s = _Store(gpu, metric, kind, db)
    excl = np.unique(s.tags[big])
    ed, ei = s.reference(q, 10, excl)
    for nq in NQS:
        D, I, K64, info = s.search(q[:nq], 10, excl)
        print(f"{kind} {metric} 100x nq {nq}: {info}")
        _check(D, I, K64, ed[:nq], ei[:nq], metric)
        assert not np.isin(I.cpu().numpy(), big).any()
        assert info["route"] == "tile", info


@pytest.mark.parametrize("kind,metric", [("uncentred", "L2"), ("centred", "COSINE"), ("f16", "IP")])
def test_k128_on_the_tile_route(gpu, kind, metric):
    """k = 128 where the plain search gives it to the tile scan: 49 152 rows (24 sample tiles x 16 entries >= 2 (128 + 6)), 90 % excluded"""
    n = 49152
    db, q = _data(kind, n, DIM1, 300, 7701)
    s = _Store(gpu, metric, kind, db)
    excl = _random_excl(s.tags, 0.9, 7702)
    ed, ei = s.reference(q, 128, excl)
    for nq in NQS:
        assert _plain_kind(s, q[:nq], 128) == "hi_tile"
        D, I, K64, info = s.search(q[:nq], 128, excl)
        print(f"{kind} {metric} k 128 nq {nq}: {info}")
        _check(D, I, K64, ed[:nq], ei[:nq], metric)
        _precondition(s, q[:nq], 128, excl, ei[:nq])
        _expect_tile(info, nq)


# ---- case 2: the sample pre-pass on the two-workgroup K split ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_case2_k_split(gpu, metric):
    """16 384 x 1024, 24 queries: dim >= 1024 and <= 128 workgroups (knn_tile_ksplit), 90 % excluded -- the half of a tile that does
    not carry the bias adds a finite partial sum to the other half's NaN"""
    db, q = _data("uncentred", 16384, 1024, 24, 7801)
    s = _Store(gpu, metric, "uncentred", db)
    excl = _random_excl(s.tags, 0.9, 7802)
    ed, ei = s.reference(q, 10, excl)
    assert _plain_kind(s, q, 10) == "hi_tile"
    D, I, K64, info = s.search(q, 10, excl)
    print(f"{metric} K split: {info}")
    _check(D, I, K64, ed, ei, metric)
    _precondition(s, q, 10, excl, ei)
    _expect_tile(info, 24)
    _same_as_search_excl(s, q, 10, excl, I, K64)


# ---- case 3: two phases; the first phase's k best of every query excluded ------------------------------------------------------------------
def test_case3_second_floor_from_admitted_rows_only(gpu):
    """22 016 x 64 at k = 58 is the smallest store whose tile scan runs two phases (knn_hi_phases on the host: 8 sample tiles, the
    first phase covers rows [0, 16 384), the sample's floor alone no longer filters the store into a third of the buffer).  Every
    query's 58 best rows of the first phase are excluded: k_kth_floor raises the second phase's floor from admitted rows only."""
    n, k, nq, r1 = 22016, 58, 40, 16384
    db, q = _data("uncentred", n, DIM1, nq, 7901)
    s = _Store(gpu, "L2", "uncentred", db)
    s.idx.search_device(_dev(q, gpu), k)
    assert s.idx.last_launch()["scan_kind"] == "hi_tile" and s.idx.last_launch()["scan_phases"] >= 2, s.idx.last_launch()
    _, first = expected_excluding(s.stored[:r1], s.tags[:r1], None, q, k, "L2")
    excl = np.unique(s.tags[first.reshape(-1)])
    ed, ei = s.reference(q, k, excl)
    D, I, K64, info = s.search(q, k, excl)
    print(f"two phases: {info}, {len(excl)} rows excluded")
    assert s.idx.last_launch()["scan_phases"] >= 2
    _check(D, I, K64, ed, ei, "L2")
    assert not np.isin(I.cpu().numpy(), first).any()
    assert info["route"] == "tile", info
    _same_as_search_excl(s, q, k, excl, I, K64)


# ---- case 4: the exact route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["8_queries", "k_200", "dim_96", "3000_rows"])
def test_case4_exact_route(gpu, shape):
    n, dim, nq, k = {"8_queries": (N1, 64, 8, 10), "k_200": (N1, 64, 40, 200), "dim_96": (N1, 96, 40, 10),
                     "3000_rows": (3000, 64, 40, 10)}[shape]
    for metric in ("L2", "COSINE"):
        db, q = _data("uncentred", n, dim, nq, 8001)
        s = _Store(gpu, metric, "uncentred", db)
        for fraction in (0.5, 0.9):
            excl = _random_excl(s.tags, fraction, 8002)
            ed, ei = s.reference(q, k, excl)
            D, I, K64, info = s.search(q, k, excl)
            print(f"{shape} {metric} {fraction}: {info}")
            _check(D, I, K64, ed, ei, metric)
            assert info == {"queries": nq, "route": "exact", "exact": nq}, info
        D, I, K64, info = s.search(q, k, None)                                # nothing excluded, no tags: the exact pass over all rows
        _check(D, I, K64, *s.reference(q, k, None), metric)
        assert info["route"] == "exact"


# ---- case 5: two row shards, merged by radad_topk_merge_f64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_case5_two_shards_merge_exactly(gpu, metric):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    n, half, nq, k = 32768, 16384, 40, 10
    db, q = _data("uncentred", n, DIM1, nq, 8101)
    tags = np.arange(n, dtype=np.int64) * 7 + 11
    excl = _random_excl(tags, 0.9, 8102)
    whole = _Store(gpu, metric, "uncentred", db, tags)
    ed, ei = whole.reference(q, k, excl)
    D, I, K64, info = whole.search(q, k, excl)
    _check(D, I, K64, ed, ei, metric)
    _precondition(whole, q, k, excl, ei)
    _expect_tile(info, nq)
    keys, ids = [], []
    for r in range(2):
        sh = _Store(gpu, metric, "uncentred", db[r * half:(r + 1) * half], tags[r * half:(r + 1) * half], id_base=r * half)
        _, Ir, Kr, info_r = sh.search(q, k, excl)
        print(f"{metric} shard {r}: {info_r}")
        _expect_tile(info_r, nq)
        keys.append(Kr)
        ids.append(Ir)
    kd, idd = torch.stack(keys).contiguous(), torch.stack(ids).contiguous()
    od = torch.empty((nq, k), device=gpu)
    oi = torch.empty((nq, k), device=gpu, dtype=torch.int64)
    ok = torch.empty((nq, k), device=gpu, dtype=torch.float64)
    m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
    _lib.check(_lib.load().radad_topk_merge_f64(m, kd.data_ptr(), idd.data_ptr(), 2, nq, k, od.data_ptr(), oi.data_ptr(), ok.data_ptr(),
                                                gpu.index or 0, _lib.stream_ptr(gpu)), "radad_topk_merge_f64")
    assert torch.equal(oi, I) and torch.equal(ok.view(torch.int64), K64.view(torch.int64)) and torch.equal(od, D)


# ---- case 6: the tuning state is left alone ---------------------------------------------------------------------------------------------------
def test_case6_tuning_state_untouched(gpu, stores):
    import torch
    s = stores("uncentred", "L2")
    q = s.q[:256]
    qt = _dev(q, gpu)
    s.idx.search_device(qt, 10)
    torch.cuda.synchronize()
    s.idx.search_device(qt, 10)                                               # (consumes the first search's report)
    torch.cuda.synchronize()
    before = s.idx.tuning_info()
    rebuilds = s.plane()["rebuilds"]
    keep = np.array([5, 9000, 20479])
    excl = np.unique(np.delete(s.tags, keep))
    D, I, K64, info = s.search(q, 10, excl)                                   # 3 admissible rows: every candidate buffer is short
    _check(D, I, K64, *s.reference(q, 10, excl), "L2")
    assert info["route"] == "tile" and info["queries"] == 256, info
    torch.cuda.synchronize()
    assert s.idx.tuning_info() == before and s.plane()["rebuilds"] == rebuilds
    D1, I1 = s.idx.search_device(qt, 10)
    assert s.idx.last_launch()["scan_kind"] == "hi_tile"
    torch.cuda.synchronize()
    s.idx.search_device(qt, 10)                                               # ... and whatever report arrived since retunes nothing
    after = s.idx.tuning_info()
    assert after["cap_boost"] == before["cap_boost"] and after["fp32_searches_left"] == before["fp32_searches_left"] == 0, (before, after)
    assert s.idx.last_launch()["scan_kind"] == "hi_tile"
    od, oi = s.reference(q, 10, None)
    np.testing.assert_array_equal(I1.cpu().numpy(), oi)


# ---- case 7: retrieve_similar_vectors in the training_file_ids mode ----------------------------------------------------------------------------
def test_case7_pipeline_training_file_ids(gpu, tmp_path):
    import os
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")

    def pipeline(**knobs):
        cfg = R.Config()
        cfg.update(device=gpu, feature_dim=64, tpp_levels=[1], top_k=5, vector_db_index_type="L2",       # (dim 64: a tile-scan shape)
                   vector_db_path=str(tmp_path / ("vdb_" + "_".join(knobs))), **knobs)
        return R.HotPathPipeline(cfg, feature_extractor=NoExtractor()), cfg

    n, nq = 20480, 24
    pipe, cfg = pipeline(exact_exclusion=True, exclusion_in_scan=True)
    dim = pipe.tpp.get_output_dim()
    db, q = synth.rows(0, n, dim, 8201), synth.rows(0, nq, dim, 8202)
    paths = [f"/data/f{i}.wav" for i in range(n)]
    labels = [float(i % 2) for i in range(n)]
    train = np.random.default_rng(8203).choice(n, int(0.9 * n), replace=False)
    names = {os.path.basename(paths[i]) for i in train}
    pipe.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * n})
    pipe.training_file_ids = set(names)
    qd = torch.from_numpy(q).to(gpu)
    vec, lbl, rp, dist = pipe.retrieve_similar_vectors(qd, query_paths=None, exclude_self=True, return_info=True, return_distances=True)
    tags = np.array([path_tag(p) for p in paths], np.int64)
    excl = np.unique(tags[train])
    ed, ei = expected_excluding(db, tags, excl, q, cfg.top_k, "L2")
    assert (ei >= 0).all()
    assert rp == [[paths[i] for i in row] for row in ei]                       # K admissible neighbours per clip
    assert all(os.path.basename(x) not in names for row in rp for x in row)
    np.testing.assert_array_equal(vec.cpu().numpy(), db[ei])
    np.testing.assert_allclose(dist.cpu().numpy(), ed, rtol=1e-6, atol=1e-6)
    info = pipe.vector_db.index.last_excl_scan()
    assert info["route"] == "tile" and info["queries"] == nq and info["exact"] <= nq // 8, info
    # scope "query" with it raises; the default path pads
    cfg.exclusion_scope = "query"
    with pytest.raises(ValueError, match="exclusion_in_scan"):
        pipe.retrieve_similar_vectors(qd, query_paths=[f"/eval/c{j}.wav" for j in range(nq)], exclude_self=True)
    pipe0, cfg0 = pipeline()
    assert cfg0.exclusion_in_scan is False
    pipe0.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * n})
    pipe0.training_file_ids = set(names)
    _, _, rp0 = pipe0.retrieve_similar_vectors(qd, query_paths=None, exclude_self=True, return_info=True)
    assert sum(x == "" for row in rp0 for x in row) > nq                       # K + 10 hits, 90 % of them excluded: padding


# ---- arguments and the wrappers that refuse ---------------------------------------------------------------------------------------------------
def test_arguments(gpu, stores):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipIVFFlatIndex, _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    s = stores("uncentred", "L2")
    qt = _dev(s.q[:20], gpu)
    excl_t = _dev(_random_excl(s.tags, 0.5, 8301), gpu)
    D0, I0 = s.idx.search_device(qt, 5)
    for k in (0, 1025):
        with pytest.raises(ValueError):
            s.idx.search_excluding_in_scan(qt, k, s.tags_t, excl_t)
    D = torch.empty((20, 5), device=gpu)
    I = torch.empty((20, 5), device=gpu, dtype=torch.int64)
    lib = _lib.load()
    with pytest.raises(ValueError):                                           # an exclusion set of 3 tags that is not there
        _lib.check(lib.radad_knn_search_excl_scan(s.idx._h, qt.data_ptr(), _lib.Q_F32, 20, 5, s.tags_t.data_ptr(), None, 3, D.data_ptr(),
                                                  I.data_ptr(), None, _lib.stream_ptr(gpu)))
    with pytest.raises(ValueError):                                           # ... or without the row tags
        _lib.check(lib.radad_knn_search_excl_scan(s.idx._h, qt.data_ptr(), _lib.Q_F32, 20, 5, None, excl_t.data_ptr(), 3, D.data_ptr(),
                                                  I.data_ptr(), None, _lib.stream_ptr(gpu)))
    s.idx.search_begin(qt, 5)
    with pytest.raises(ValueError):                                           # a begun search owns the handle
        s.idx.search_excluding_in_scan(qt, 5, s.tags_t, excl_t)
    s.idx.search_abort()
    with pytest.raises(ValueError):                                           # an empty store
        _mk("L2", 64).search_excluding_in_scan(qt, 5, None, None)
    wide = _mk("L2", 16384)                                                   # the width x k limit, before anything is enqueued
    wide.add(np.zeros((4, 16384), np.float32))
    with pytest.raises(ValueError):
        wide.search_excluding_in_scan(torch.zeros((2, 16384), device=gpu), 1024, None, None)
    with pytest.raises(ValueError, match="search_probed_excluding"):
        HipIVFFlatIndex(64, 64).search_excluding_in_scan(qt, 5, None, None)
    with pytest.raises(ValueError, match="search_excluding"):
        ShardedSearch(None, _lib.METRIC_L2).search_excluding_in_scan(qt, 5)
    qb = qt.bfloat16()                                                        # bf16 queries, as every search takes them
    Db, Ib = s.idx.search_excluding_in_scan(qb, 5, s.tags_t, excl_t)
    _, ei = s.reference(qb.float().cpu().numpy(), 5, excl_t.cpu().numpy())
    np.testing.assert_array_equal(Ib.cpu().numpy(), ei)
    D1, I1 = s.idx.search_device(qt, 5)                                       # after the refused calls a plain search still works
    assert torch.equal(I1, I0) and torch.equal(D1, D0)
