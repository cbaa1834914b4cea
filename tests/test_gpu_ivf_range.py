"""GPU: certified range search over the probed lists of an IVF index (radad_ivf_range_search) against the float64 reference of
tests/ivf_range_ref.py, given the centroids and list assignments the index holds.

Every comparison: counts and ids equal, float64 keys within rtol 1e-12 (a float64 sum of at most 5376 non-negative terms is good to
about 6e-13), D within rtol 1.2e-7 of the float32-rounded reference key, padding -1 / NaN.  Every case first asserts ON THE REFERENCE
that no probed row of any query lies within 1e-9 (relative) of the radius, so membership does not depend on the order of a float64
sum; radii are planted midway between two consecutive reference keys (ivf_range_ref.radius_between).

The stores are built once per module and shared; so are the reference's probed keys."""
import ctypes as C
import os

import numpy as np
import pytest

import ivf_range_ref as RR
from oracle import radad_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

M = 128
CAP = 4096          # positions of a query's candidate buffer (IVF_RANGE_CAP)


def _clustered(n, dim, n_clusters, seed):
    centers = synth.rows(0, n_clusters, dim, seed) * np.float32(3.0)
    which = (np.arange(n) * 7919) % n_clusters
    return (centers[which] + synth.rows(0, n, dim, seed + 1)).astype(np.float32)


def _queries(nq, dim, n_clusters, seed):
    """queries around the centres of the store built from `seed`, with noise of their own"""
    centers = synth.rows(0, n_clusters, dim, seed) * np.float32(3.0)
    which = (np.arange(nq) * 7919 + 5) % n_clusters
    return (centers[which] + synth.rows(0, nq, dim, seed + 7)).astype(np.float32)


class Store:
    """an index over `db`, added in two halves, with what the reference needs read back from it"""

    def __init__(self, gpu, db, q, nlist, nprobe, hi_scan=None):
        import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
        n, dim = db.shape
        self.db, self.q, self.nlist = db, q, nlist
        self.idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, hi_scan=hi_scan)
        self.idx.train(db[: min(n, 10000)])
        self.idx.add(db[: n // 2])
        self.idx.add(db[n // 2:])
        self.cent, self.assign = self.idx.centroids(), self.idx.assignments()
        self.idx.nprobe = nprobe
        self._pk = {}

    def pk(self, nprobe):
        if nprobe not in self._pk:
            self._pk[nprobe] = RR.probed_keys(self.db, self.assign, self.cent, self.q, nprobe)
        return self._pk[nprobe]

    def set_hi_scan(self, value):
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
        _lib.check(self.idx._lib.radad_ivf_set_option(self.idx._h, _lib.IVF_OPT_HI_SCAN, int(value)), "radad_ivf_set_option")


@pytest.fixture(scope="module")
def store1(gpu):
    return Store(gpu, _clustered(20000, 64, 50, 8101), _queries(100, 64, 50, 8101), 64, 8)


@pytest.fixture(scope="module")
def store2(gpu):
    return Store(gpu, _clustered(30000, 512, 50, 8201), _queries(300, 512, 50, 8201), 128, 32)


def _run(idx, q, radius, m=M):
    counts, D, I, K = idx.range_search_probed_device(q, radius, max_per_query=m, return_f64=True)
    return counts.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy(), K.cpu().numpy()


def _compare(got, ref, m=M):
    counts, D, I, K = got
    rc, ri, rk, _ = ref
    np.testing.assert_array_equal(counts, rc)
    np.testing.assert_array_equal(I, ri)
    have = ri >= 0
    np.testing.assert_allclose(K[have], rk[have], rtol=1e-12, atol=0)
    np.testing.assert_allclose(D[have], rk[have].astype(np.float32), rtol=1.2e-7, atol=0)
    assert np.isnan(D[~have]).all() and np.isnan(K[~have]).all()
    assert (have.sum(1) == np.minimum(rc, m)).all()


def _check(idx, q, pk, radius, m=M):
    ref = RR.members(pk, radius, m)
    assert (ref[3] >= 1e-9).all(), ("a probed row within 1e-9 of the radius: membership is not decidable", float(ref[3].min()))
    got = _run(idx, q, radius, m)
    _compare(got, ref, m)
    return got, ref


def _three_radii(pk, cluster):
    """below every distance; around the median distance of query 0's own cluster (`cluster` rows); one with more than M members for
    query 0 and, the clusters being alike, for most queries"""
    lo = 0.5 * min(float(k.min()) for _, k in pk if len(k))
    rows = len(pk[0][1])
    mid = RR.radius_between(pk, 0, min(rows - 1, max(2, cluster // 2)))
    big = RR.radius_between(pk, 0, min(rows - 1, max(cluster, M + 100)))
    return float(np.float32(lo)), mid, big


def _hi_route_case(s, nprobe):
    pk = s.pk(nprobe)
    s.idx.nprobe = nprobe
    lo, mid, big = _three_radii(pk, len(s.db) // 50)
    out = []
    for radius in (lo, mid, big):
        got, ref = _check(s.idx, s.q, pk, radius)
        info = s.idx.last_range()
        assert info["route"] == "hi_lists" and info["queries"] == len(s.q), info
        out.append((radius, got, ref, info))
    assert (out[0][2][0] == 0).all()                                  # below every distance: nobody has a member
    assert (out[1][2][0] > 0).any() and out[1][2][0][0] == max(2, len(s.db) // 100)
    assert (out[2][2][0] > M).any()                                   # some counts exceed M: the slots are the best M (compared above)
    return out


def test_01_hi_route_three_radii(store1):
    """A query's 8 probed lists hold 2 500 rows on average and up to 5 600 on this clustered store, so a buffer of 4 096 positions
    COULD overflow if eps were as large as the radius; at these radii the scan emits the members and the rows within eps of the
    boundary, far fewer: no query goes to the exact pass."""
    s = store1
    probed_rows = max(len(c) for c, _ in s.pk(8))
    for radius, got, ref, info in _hi_route_case(s, 8):
        assert info["exact"] == 0 and int(ref[0].max()) <= info["max_emitted"] <= min(CAP, probed_rows), (radius, info)


def test_02_hi_route_dim_512(store2):
    """the same at dim 512, with the same assertions: no query overflows its buffer at these radii"""
    for radius, got, ref, info in _hi_route_case(store2, 32):
        assert info["exact"] == 0 and int(ref[0].max()) <= info["max_emitted"] <= CAP, (radius, info)


@pytest.mark.parametrize("nq", [1, 3, 16])
def test_03_small_batches_split_lists(store1, nq):
    """<= 64 tasks: every list is split over 8 workgroups"""
    s = store1
    s.idx.nprobe = 8
    pk = s.pk(8)[:nq]
    for radius in _three_radii(s.pk(8), 400):
        _check(s.idx, s.q[:nq], pk, radius)
        info = s.idx.last_range()
        assert info == {"queries": nq, "route": "hi_lists", "exact": 0, "max_emitted": info["max_emitted"]}


@pytest.mark.parametrize("dim", [96, 32])
def test_04_exact_route_by_shape(gpu, dim):
    """dim % 64 != 0: no f16 plane"""
    s = Store(gpu, _clustered(5000, dim, 30, 8301 + dim), _queries(20, dim, 30, 8301 + dim), 64, 8)
    pk = s.pk(8)
    radii = _three_radii(pk, 5000 // 30)
    for radius in radii:
        _check(s.idx, s.q, pk, radius)
        assert s.idx.last_range() == {"queries": 20, "route": "exact_lists", "exact": 20, "max_emitted": 0}
    _check(s.idx, s.q, pk, radii[2], m=1)
    _check(s.idx, s.q, pk, radii[2], m=65)                 # a wave's list in both halves of its lanes, not a multiple of 64


def test_05_exact_route_forced_and_behind_the_hi_route(store1):
    s = store1
    s.idx.nprobe = 8
    pk = s.pk(8)
    radii = _three_radii(pk, 400)
    base = [_run(s.idx, s.q, r) for r in radii]
    try:
        for opt, route in ((0, "exact_lists"), (2, "hi_lists")):
            s.set_hi_scan(opt)
            for r, b in zip(radii, base):
                got, _ = _check(s.idx, s.q, pk, r)
                assert s.idx.last_range()["route"] == route and s.idx.last_range()["exact"] == len(s.q)
                np.testing.assert_array_equal(got[0], b[0])
                np.testing.assert_array_equal(got[2], b[2])
    finally:
        s.set_hi_scan(1)
    _check(s.idx, s.q, pk, radii[1])
    assert s.idx.last_range()["route"] == "hi_lists" and s.idx.last_range()["exact"] == 0


def test_06_overflow_goes_to_the_exact_pass(store1):
    s = store1
    n, nlist = len(s.db), s.nlist
    s.idx.nprobe = nlist
    try:
        counts, D, I, K = _run(s.idx, s.q, float("inf"))
        info = s.idx.last_range()
        assert info == {"queries": len(s.q), "route": "hi_lists", "exact": len(s.q), "max_emitted": n}, info
        assert (counts == n).all()
        od, oi = O.knn(s.db, s.q, M, "L2")
        np.testing.assert_array_equal(I, oi)
        np.testing.assert_allclose(K, od, rtol=1e-12, atol=0)
        np.testing.assert_allclose(D, od.astype(np.float32), rtol=1.2e-7, atol=0)
        pk = s.pk(nlist)
        radius = RR.radius_between(pk, 0, 5000)
        got, ref = _check(s.idx, s.q, pk, radius)
        info = s.idx.last_range()
        assert ref[0][0] == 5000 and info["max_emitted"] > CAP and 1 <= info["exact"] <= len(s.q), info
    finally:
        s.idx.nprobe = 8


def test_07_ties_come_in_ascending_insertion_id(gpu, store1):
    """40 exact duplicates of one row at scattered insertion ids, some in each half of the store: equal keys, ordered by insertion id
    (their list positions are in another order only by accident; the ids decide)"""
    db = store1.db.copy()
    n = len(db)
    base = 4321
    dup = np.arange(40) * 487 + 13
    assert dup.max() < n and (dup < n // 2).any() and (dup >= n // 2).any() and base not in dup
    db[dup] = db[base]
    q = np.stack([db[base] + synth.rows(0, 1, 64, 8401 + j)[0] * np.float32(0.01 * j) for j in range(4)]).astype(np.float32)
    s = Store(gpu, db, q, 64, 8)
    pk = s.pk(8)
    same = np.sort(np.concatenate([dup, [base]]))
    for j in range(4):
        keys = pk[j][1][np.isin(pk[j][0], same)]
        assert len(keys) == 41 and (keys == keys[0]).all()             # the probed lists hold all 41, their float64 keys are equal
    k0 = np.sort(pk[1][1])
    radius = RR.radius_between(pk, 1, int((k0 <= pk[1][1][np.isin(pk[1][0], same)][0]).sum()) + 3)
    try:
        for opt in (1, 0):
            s.set_hi_scan(opt)
            got, ref = _check(s.idx, s.q, pk, radius)
            assert s.idx.last_range()["route"] == ("hi_lists" if opt else "exact_lists")
            for j in range(4):
                ids = got[2][j]
                at = np.flatnonzero(np.isin(ids, same))
                assert len(at) == 41 and (np.diff(at) == 1).all()          # one run of equal keys ...
                np.testing.assert_array_equal(ids[at], same)               # ... in ascending insertion id
    finally:
        s.set_hi_scan(1)


def test_08_every_list_probed_equals_the_flat_store(gpu, store1):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = store1
    flat = R.HipFlatIndex(64, _lib.METRIC_L2, device=gpu.index or 0)
    flat.add(s.db)
    pk = s.pk(s.nlist)
    radius = RR.radius_between(pk, 0, 100)
    s.idx.nprobe = s.nlist
    try:
        got, ref = _check(s.idx, s.q, pk, radius)
    finally:
        s.idx.nprobe = 8
    import torch
    fc, fd, fi = flat.range_search_device(torch.from_numpy(s.q).to(gpu), radius, max_per_query=M)
    np.testing.assert_array_equal(got[0], fc.cpu().numpy())
    np.testing.assert_array_equal(got[2], fi.cpu().numpy())
    b = RR.brute_range(s.db, s.q, radius, M)
    np.testing.assert_array_equal(got[0], b[0])
    np.testing.assert_array_equal(got[2], b[1])


def test_09_edges(gpu, store1):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    s = store1
    s.idx.nprobe = 8
    pk = s.pk(8)
    lo, mid, big = _three_radii(pk, 400)
    # an empty trained index: counts 0 and padding; nq == 0
    e = R.HipIVFFlatIndex(64, 64, gpu.index or 0)
    e.train(s.db[:5000])
    e.nprobe = 8
    counts, D, I, K = _run(e, s.q[:7], mid)
    assert (counts == 0).all() and (I == -1).all() and np.isnan(D).all() and np.isnan(K).all()
    assert e.last_range() == {"queries": 7, "route": "exact_lists", "exact": 0, "max_emitted": 0}
    counts, D, I, K = _run(s.idx, s.q[:0], mid)
    assert counts.shape == (0,) and D.shape == (0, M) and I.shape == (0, M)
    # a radius with no member (and a negative one); M = 1
    got, _ = _check(s.idx, s.q, pk, lo)
    assert (got[0] == 0).all() and (got[2] == -1).all()
    counts, D, I, K = _run(s.idx, s.q, -1.0)
    assert (counts == 0).all() and (I == -1).all() and np.isnan(D).all()
    _check(s.idx, s.q, pk, big, m=1)
    # two runs give identical bytes
    a, b = _run(s.idx, s.q, big), _run(s.idx, s.q, big)
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert x.tobytes() == y.tobytes()
    # a range search, a top-k search, the range search again: the top-k result is what it was, the shared workspaces hold
    D0, I0 = s.idx.search(s.q, 10)
    r1 = _run(s.idx, s.q, mid)
    D1, I1 = s.idx.search(s.q, 10)
    with pytest.raises(ValueError, match="not a range search"):
        s.idx.last_range()
    r2 = _run(s.idx, s.q, mid)
    with pytest.raises(ValueError, match="was a range search"):      # and the top-k read-backs do not describe a range search
        s.idx.last_search_info()
    assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes()
    for x, y in zip((r1[0], r1[2], r1[3]), (r2[0], r2[2], r2[3])):
        assert x.tobytes() == y.tobytes()
    od, oi = O.ivf_search(s.db, s.assign, s.cent, s.q, 10, 8)
    np.testing.assert_array_equal(I1, oi)
    # add after a range search, then another range search: the list-major layout is rebuilt
    db = _clustered(6000, 64, 30, 8501)
    g = Store(gpu, db[:4000], _queries(20, 64, 30, 8501), 64, 8)
    _check(g.idx, g.q, g.pk(8), _three_radii(g.pk(8), 4000 // 30)[2])
    g.idx.add(db[4000:])
    g.db, g.assign, g._pk = db, g.idx.assignments(), {}
    assert g.idx.ntotal == 6000 and (g.assign[:4000] == g.idx.assignments()[:4000]).all()
    _check(g.idx, g.q, g.pk(8), _three_radii(g.pk(8), 6000 // 30)[2])


def _config(gpu, tmp_path, index_type, nprobe=16):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as Rad
    cfg = Rad.Config()
    cfg.update(device=gpu, feature_dim=64, tpp_levels=[1], top_k=5, vector_db_index_type=index_type, vector_db_nprobe=nprobe,
               vector_db_path=str(tmp_path / ("vdb_" + index_type)))
    cfg.ivf_nlist = 32                                                # max(64, 32) -> 64 lists
    return Rad, cfg


def test_10_vector_database_and_near_duplicates(gpu, tmp_path):
    import torch
    Rad, cfg = _config(gpu, tmp_path, "IVF")

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")
    pipe = Rad.HotPathPipeline(cfg, feature_extractor=NoExtractor())
    vdb = pipe.vector_db
    db = _clustered(12000, 64, 40, 8601)
    q = _queries(20, 64, 40, 8601)
    # query 2 has two planted near-copies: the file itself under its own basename, and a renamed copy
    own, renamed = 777, 9031
    db[own] = q[2] + synth.rows(0, 1, 64, 8605)[0] * np.float32(1e-3)
    db[renamed] = q[2] + synth.rows(0, 1, 64, 8606)[0] * np.float32(2e-3)
    n = len(db)
    paths = [f"/train/f{i}.wav" for i in range(n)]
    paths[own] = "/train/vocoder3/clip2.wav"
    paths[renamed] = "/train/renamed_copy.wav"
    labels = [i % 2 for i in range(n)]
    # an empty store: empty results
    vdb0 = Rad.VectorDatabase(cfg)
    vdb0.index = Rad.HipIVFFlatIndex(64, 64, gpu.index or 0)
    lims, D, I, counts = vdb0.range_search_probed_batch(q, 1.0, return_counts=True)
    assert lims.shape == (21,) and (lims == 0).all() and len(D) == 0 and len(I) == 0 and (counts == 0).all()
    vdb.add_vectors(db, paths, labels, {})
    assert isinstance(vdb.index, Rad.HipIVFFlatIndex) and vdb.index.ntotal == n
    cent, assign = vdb.index.centroids(), vdb.index.assignments()
    pk = RR.probed_keys(db, assign, cent, q, 16)
    radius = RR.radius_between(pk, 0, 40)
    ref = RR.members(pk, radius, M)
    assert (ref[3] >= 1e-9).all() and ref[0][2] >= 2
    # CSR form and counts, numpy in -> numpy out, a CUDA tensor in -> CUDA tensors out; max_per_query cuts the lists, not the counts
    for m in (M, 5):
        lims, D, I, counts = vdb.range_search_probed_batch(q, radius, max_per_query=m, return_counts=True)
        assert isinstance(lims, np.ndarray) and vdb.index.nprobe == 16
        np.testing.assert_array_equal(counts, ref[0])
        kept = np.minimum(ref[0], m)
        np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(kept)]))
        for j in range(len(q)):
            np.testing.assert_array_equal(I[lims[j]:lims[j + 1]], ref[1][j, :kept[j]])
            np.testing.assert_allclose(D[lims[j]:lims[j + 1]], ref[2][j, :kept[j]].astype(np.float32), rtol=1.2e-7)
    out = vdb.range_search_probed_batch(torch.from_numpy(q).to(gpu), radius)
    assert len(out) == 3 and all(t.is_cuda for t in out)
    np.testing.assert_array_equal(out[2].cpu().numpy(), np.concatenate([ref[1][j, :min(ref[0][j], M)] for j in range(len(q))]))
    # the audit: probed=True returns the same (path, label, score) lists; the file itself is dropped by basename, the renamed copy stays
    plain = pipe.near_duplicates(q, radius, probed=True)
    for j in range(len(q)):
        k = min(ref[0][j], M)
        assert [h[0] for h in plain[j]] == [paths[int(i)] for i in ref[1][j, :k]]
        assert all(h[1] == labels[paths.index(h[0])] and h[2] < radius for h in plain[j])
    assert {paths[own], paths[renamed]} <= {h[0] for h in plain[2]}
    query_paths = [f"/eval/clip{j}.wav" for j in range(len(q))]
    audit = pipe.near_duplicates(torch.from_numpy(q).to(gpu), radius, query_paths=query_paths, probed=True)
    got = {h[0] for h in audit[2]}
    assert "/train/vocoder3/clip2.wav" not in got and "/train/renamed_copy.wav" in got and len(audit[2]) == len(plain[2]) - 1
    assert os.path.basename(paths[own]) == os.path.basename(query_paths[2])
    # what is not offered says so
    with pytest.raises(ValueError, match="exact_exclusion is not offered with probed=True"):
        pipe.near_duplicates(q, radius, query_paths=query_paths, probed=True, exact_exclusion=True)
    with pytest.raises(ValueError, match="flat and single-handle only"):
        pipe.near_duplicates(q, radius)                               # the default on an IVF store refuses as it always did
    with pytest.raises(ValueError, match="flat and single-handle only"):
        vdb.range_search_batch(q, radius)
    with pytest.raises(ValueError, match="flat store's search"):
        vdb.index.range_search(q, radius)
    Rad2, cfg2 = _config(gpu, tmp_path, "L2")
    flat_pipe = Rad2.HotPathPipeline(cfg2, feature_extractor=NoExtractor())
    flat_pipe.vector_db.add_vectors(db[:2000], paths[:2000], labels[:2000], {})
    with pytest.raises(ValueError, match="range_search_batch"):
        flat_pipe.vector_db.range_search_probed_batch(q, radius)
    with pytest.raises(ValueError, match="range_search_batch"):
        flat_pipe.near_duplicates(q, radius, probed=True)


def test_10_c_argument_errors_leave_the_outputs_untouched(gpu, store1):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = store1
    lib, h = s.idx._lib, s.idx._h
    q = torch.from_numpy(s.q[:4]).to(gpu)
    counts = torch.full((4,), 77, device=gpu, dtype=torch.int32)
    D = torch.full((4, M), 5.0, device=gpu)
    I = torch.full((4, M), 9, device=gpu, dtype=torch.int64)
    K = torch.full((4, M), 6.0, device=gpu, dtype=torch.float64)
    st = _lib.stream_ptr(gpu)

    def call(handle=h, nq=4, nprobe=8, radius=1.0, m=M, c=counts.data_ptr(), d=D.data_ptr(), i=I.data_ptr()):
        return lib.radad_ivf_range_search(handle, q.data_ptr(), nq, nprobe, radius, m, c, d, i, K.data_ptr(), st)
    for kw in (dict(m=0), dict(m=-3), dict(m=129), dict(radius=float("nan")), dict(c=None), dict(d=None), dict(i=None), dict(nprobe=0),
               dict(nq=-1)):
        assert call(**kw) == _lib.RADAD_EINVAL, kw
    untrained = R.HipIVFFlatIndex(64, 64, gpu.index or 0)
    assert call(handle=untrained._h) == _lib.RADAD_ESTATE
    with pytest.raises(ValueError, match="not trained"):
        untrained.range_search_probed_device(s.q[:4], 1.0)
    torch.cuda.synchronize()
    assert (counts == 77).all() and (D == 5.0).all() and (I == 9).all() and (K == 6.0).all()
    assert call(nq=0) == _lib.RADAD_OK                                # nothing to do, nothing written
    torch.cuda.synchronize()
    assert (counts == 77).all() and (I == 9).all()
    # the handle is usable: the same call with good arguments, and without the float64 keys
    s.idx.nprobe = 8
    radius = _three_radii(s.pk(8), 400)[1]
    assert lib.radad_ivf_range_search(h, q.data_ptr(), 4, 8, radius, M, counts.data_ptr(), D.data_ptr(), I.data_ptr(), None, st) == _lib.RADAD_OK
    ref = RR.members(s.pk(8)[:4], radius, M)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])
    nq, route, ex, me = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    assert lib.radad_ivf_last_range(h, C.byref(nq), C.byref(route), None, None) == _lib.RADAD_OK and nq.value == 4 and route.value == 0
    assert lib.radad_ivf_last_range(h, None, None, C.byref(ex), C.byref(me)) == _lib.RADAD_OK and ex.value == 0 and me.value >= int(ref[0].max())
