"""GPU: certified range search among the rows of the probed lists that a query does not exclude (radad_ivf_range_search_excl: one set
for the batch; radad_ivf_range_search_excl_pq: one set per query) against the float64 reference of tests/ivf_range_excl_ref.py, given
the centroids and list assignments the index holds.

Every comparison is tests/test_gpu_ivf_range.py's, with its tolerances (derived there): counts and ids equal, float64 keys within rtol
1e-12, D within rtol 1.2e-7 of the float32-rounded reference key, padding -1 / NaN / NaN.  Every case first asserts ON THE REFERENCE
that no ADMISSIBLE probed row of any query lies within 1e-9 (relative) of the radius; radii are planted midway between two consecutive
keys (ivf_range_ref.radius_between) of the filtered rows unless a case says otherwise.

The stores are built once per module and shared; so are the reference's probed keys."""
import ctypes as C
import os

import numpy as np
import pytest

import ivf_range_excl_ref as XR
import ivf_range_ref as RR
from ivf_excl_pq_ref import list_major
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
    """an index over `db`, added in two halves, with what the reference needs read back from it (tests/test_gpu_ivf_range.py's)"""

    def __init__(self, gpu, db, q, nlist, nprobe, hi_scan=None):
        import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
        n, dim = db.shape
        self.gpu, self.db, self.q, self.nlist = gpu, db, q, nlist
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

    def dev(self, a, dtype=None):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).to(self.gpu)


@pytest.fixture(scope="module")
def store_a(gpu):
    return Store(gpu, _clustered(20000, 64, 50, 8101), _queries(100, 64, 50, 8101), 64, 8)


@pytest.fixture(scope="module")
def store_b(gpu):
    return Store(gpu, _clustered(12000, 512, 50, 8701), _queries(60, 512, 50, 8701), 64, 16)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _run_plain(s, q, radius, m=M):
    return _host(s.idx.range_search_probed_device(s.dev(q), radius, max_per_query=m, return_f64=True))


def _run_batch(s, q, radius, tags, excl, m=M):
    excl_t = None if excl is None else s.dev(np.sort(np.asarray(excl, np.int64)))
    return _host(s.idx.range_search_probed_excluding_device(s.dev(q), radius, s.dev(np.asarray(tags, np.int64)), excl_t, max_per_query=m,
                                                            return_f64=True))


def _run_pq(s, q, radius, tags, qtags, counts=None, m=M):
    import torch
    qt = None if qtags is None else s.dev(np.asarray(qtags, np.int64))
    ct = None if counts is None else s.dev(np.asarray(counts, np.int32), torch.int32)
    return _host(s.idx.range_search_probed_excluding_per_query_device(s.dev(q), radius, s.dev(np.asarray(tags, np.int64)), qt, ct, max_per_query=m,
                                                                      return_f64=True))


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


def _guard(ref):
    assert (ref[3] >= 1e-9).all(), ("an admissible probed row within 1e-9 of the radius: membership is not decidable", float(ref[3].min()))
    return ref


def _check_batch(s, q, pk, radius, tags, excl, m=M):
    ref = _guard(XR.members_batch(pk, tags, excl, radius, m))
    got = _run_batch(s, q, radius, tags, excl, m)
    _compare(got, ref, m)
    listed = got[2][got[2] >= 0]
    assert excl is None or not np.isin(np.asarray(tags)[listed], excl).any()
    return got, ref


def _check_pq(s, q, pk, radius, tags, qtags, counts=None, m=M):
    ref = _guard(XR.members_pq(pk, tags, qtags, counts, radius, m))
    got = _run_pq(s, q, radius, tags, qtags, counts, m)
    _compare(got, ref, m)
    return got, ref


def _three_radii(fpk, cluster):
    """on FILTERED keys: below every distance; around the median distance of query 0's admissible rows of its own cluster (`cluster` of
    them); one with more than M admissible members for query 0 and, the clusters being alike, for most queries"""
    lo = 0.5 * min(float(k.min()) for _, k in fpk if len(k))
    rows = len(fpk[0][1])
    mid = RR.radius_between(fpk, 0, min(rows - 1, max(2, cluster // 2)))
    big = RR.radius_between(fpk, 0, min(rows - 1, max(cluster, M + 100)))
    return float(np.float32(lo)), mid, big


def _pair_tags(nq, m=4, counts_value=2):
    """query j excludes the tags {j % 8, (j + 3) % 8}: m columns, `counts_value` of them live, the others hold tags that rows DO carry"""
    qtags = np.empty((nq, m), np.int64)
    for j in range(nq):
        qtags[j] = [j % 8, (j + 3) % 8] + [(j + 1 + c) % 8 for c in range(m - 2)]
    return qtags, np.full(nq, counts_value, np.int32)


# ---- 1. hi route, one set for the batch ---------------------------------------------------------------------------------------------
def test_01_hi_route_batch_set(store_a):
    s = store_a
    s.idx.nprobe = 8
    tags = np.arange(len(s.db)) % 8
    excl = np.array([1, 3, 4])
    pk = s.pk(8)
    fpk = XR.filter_batch(pk, tags, excl)
    lo, mid, big = _three_radii(fpk, 400 * 5 // 8)
    seen = []
    for radius in (lo, mid, big):
        got, ref = _check_batch(s, s.q, pk, radius, tags, excl)
        info = s.idx.last_range()
        assert info["route"] == "hi_lists" and info["exact"] == 0 and info["queries"] == len(s.q), info
        assert int(ref[0].max()) <= info["max_emitted"] <= CAP, info
        seen.append(ref[0])
    assert (seen[0] == 0).all() and (seen[1] > 0).any() and (seen[2] > M).any()
    plain = RR.members(pk, big, M)
    assert (plain[0] > seen[2]).any()                                 # the set does exclude members of the plain search


# ---- 2. hi route, one set per query -------------------------------------------------------------------------------------------------
def test_02_hi_route_per_query(store_a):
    s = store_a
    s.idx.nprobe = 8
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    pk = s.pk(8)
    qtags, counts = _pair_tags(nq)
    fpk = XR.filter_pq(pk, tags, qtags, counts)
    for radius in _three_radii(fpk, 400 * 6 // 8):
        got, ref = _check_pq(s, s.q, pk, radius, tags, qtags, counts)
        info = s.idx.last_range()
        assert info["route"] == "hi_lists" and info["exact"] == 0, info
        for j in range(nq):
            ids = got[2][j][got[2][j] >= 0]
            assert not np.isin(tags[ids], qtags[j, :2]).any()
    big = _three_radii(fpk, 400 * 6 // 8)[2]
    assert (ref[0] > M).any()
    # counts 0, above m and negative: 0 and negative = nothing excluded, above m = all four columns live
    counts2 = np.array([(2, 0, 9, -1)[j % 4] for j in range(nq)], np.int32)
    got2, ref2 = _check_pq(s, s.q, pk, big, tags, qtags, counts2)
    plain = RR.members(pk, big, M)
    for j in range(nq):
        if j % 4 in (1, 3):
            assert ref2[0][j] == plain[0][j]
        if j % 4 == 2:
            assert ref2[0][j] <= ref[0][j]
    assert (ref2[0][2::4] < ref[0][2::4]).any() and (ref2[0][1::4] > ref[0][1::4]).any()
    # NULL counts = m for every query
    _check_pq(s, s.q, pk, big, tags, qtags, None)
    # duplicates within a query's tags, in any order
    dup = np.stack([[j % 8, j % 8, (j + 3) % 8, j % 8] for j in range(nq)]).astype(np.int64)
    got3, ref3 = _check_pq(s, s.q, pk, big, tags, dup, None)
    np.testing.assert_array_equal(ref3[0], ref[0])
    np.testing.assert_array_equal(got3[2], got[2])


# ---- 3. positions -------------------------------------------------------------------------------------------------------------------
def _special_positions(s, pk8):
    """rows (insertion ids) at the list-major positions where an index could go wrong, inside the list of query 0's probed lists that
    holds most of its 400 nearest rows: the first and the last row of the list, the positions = 63 and 0 (mod 64), both sides of the
    first 16-row step edge, both sides of the first share edge of a list split over 8 and over 4 workgroups"""
    off, pos = list_major(s.assign, s.nlist)
    ids0, keys0 = pk8[0]
    near = ids0[np.argsort(keys0)[:400]]
    home = int(np.bincount(s.assign[near], minlength=s.nlist).argmax())
    b, e = int(off[home]), int(off[home + 1])
    want = {b, e - 1, b + 15, b + 16}
    p63 = b + ((63 - b) % 64)
    want |= {p63, p63 + 1}
    for split in (8, 4):
        share = ((e - b + split - 1) // split + 15) // 16 * 16
        want |= {b + share - 1, b + share}
    want = np.array(sorted(p for p in want if b <= p < e), np.int64)
    assert len(want) >= 10 and e - b > 128, (b, e)
    by_pos = np.empty(len(pos), np.int64)
    by_pos[pos] = np.arange(len(pos))
    return by_pos[want], home


def test_03_positions(store_a):
    s = store_a
    s.idx.nprobe = 8
    n, nq_all = len(s.db), len(s.q)
    tags = np.arange(n, dtype=np.int64)                               # a row's tag is its insertion id
    pk = s.pk(8)
    special, home = _special_positions(s, pk)
    # every query's own cluster lies within the radius (400 rows against ~40 times the distance to the next cluster)
    radius = RR.radius_between(pk, 0, 400)
    plain = RR.members(pk, radius, M)
    assert plain[0][0] == 400
    in_radius = np.isin(special, pk[0][0][pk[0][1] < radius])
    assert in_radius.sum() >= 6, (special, in_radius)                 # the special rows are members of query 0: excluding them shows
    near5 = np.stack([c[np.argsort(k, kind="stable")[:5]] for c, k in pk])
    for nq in (1, 3, 16, nq_all):
        excl = np.unique(np.concatenate([special, near5[:nq].reshape(-1)]))
        got, ref = _check_batch(s, s.q[:nq], pk[:nq], radius, tags, excl)
        assert s.idx.last_range()["route"] == "hi_lists" and s.idx.last_range()["exact"] == 0
        if nq <= 16:                                                  # (no other query of these shares query 0's cluster)
            assert ref[0][0] == 400 - in_radius.sum() - (~np.isin(near5[0], special)).sum()
        assert not np.isin(got[2], excl).any()
        # per query: the special rows and the query's OWN five nearest (m <= 64), the columns shuffled
        rng = np.random.default_rng(8800 + nq)
        qtags = np.stack([rng.permutation(np.concatenate([special, near5[j]])) for j in range(nq)])
        assert qtags.shape[1] <= 64
        gotq, refq = _check_pq(s, s.q[:nq], pk[:nq], radius, tags, qtags)
        for j in range(nq):
            assert not np.isin(gotq[2][j], qtags[j]).any()
        assert refq[0][0] == 400 - in_radius.sum() - (~np.isin(near5[0], special)).sum()


# ---- 4. dim 512 ---------------------------------------------------------------------------------------------------------------------
def test_04_dim_512_both_calls(store_b):
    s = store_b
    s.idx.nprobe = 16
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    pk = s.pk(16)
    excl = np.array([1, 3, 4])
    mid = _three_radii(XR.filter_batch(pk, tags, excl), 240 * 5 // 8)[1]
    got, ref = _check_batch(s, s.q, pk, mid, tags, excl)
    info = s.idx.last_range()
    assert info["route"] == "hi_lists" and info["exact"] == 0 and (ref[0] > 0).any(), info
    qtags, counts = _pair_tags(nq)
    mid = _three_radii(XR.filter_pq(pk, tags, qtags, counts), 240 * 6 // 8)[1]
    got, ref = _check_pq(s, s.q, pk, mid, tags, qtags, counts)
    info = s.idx.last_range()
    assert info["route"] == "hi_lists" and info["exact"] == 0 and (ref[0] > 0).any(), info


# ---- 5. the exact route by shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [96, 32])
def test_05_exact_route_by_shape(gpu, dim):
    """dim % 64 != 0: no f16 plane"""
    s = Store(gpu, _clustered(5000, dim, 30, 8901 + dim), _queries(20, dim, 30, 8901 + dim), 64, 8)
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    pk = s.pk(8)
    excl = np.array([1, 3, 4])
    qtags, counts = _pair_tags(nq)
    want = {"queries": nq, "route": "exact_lists", "exact": nq, "max_emitted": 0}
    big_b = _three_radii(XR.filter_batch(pk, tags, excl), 5000 // 30 * 5 // 8)[2]
    big_q = _three_radii(XR.filter_pq(pk, tags, qtags, counts), 5000 // 30 * 6 // 8)[2]
    for m in (1, 65, 128):
        got, ref = _check_batch(s, s.q, pk, big_b, tags, excl, m=m)
        assert s.idx.last_range() == want
        got, ref = _check_pq(s, s.q, pk, big_q, tags, qtags, counts, m=m)
        assert s.idx.last_range() == want
    assert (ref[0] > 65).any()
    lo = _three_radii(XR.filter_batch(pk, tags, excl), 100)[0]
    got, _ = _check_batch(s, s.q, pk, lo, tags, excl)
    assert (got[0] == 0).all()


# ---- 6. RADAD_IVF_OPT_HI_SCAN 0 and 2 -----------------------------------------------------------------------------------------------
def test_06_exact_route_forced_and_behind_the_hi_route(store_a):
    s = store_a
    s.idx.nprobe = 8
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    pk = s.pk(8)
    excl = np.array([1, 3, 4])
    qtags, counts = _pair_tags(nq)
    rb = _three_radii(XR.filter_batch(pk, tags, excl), 250)[1:]
    rq = _three_radii(XR.filter_pq(pk, tags, qtags, counts), 300)[1:]
    base_b = [_run_batch(s, s.q, r, tags, excl) for r in rb]
    base_q = [_run_pq(s, s.q, r, tags, qtags, counts) for r in rq]
    assert s.idx.last_range()["route"] == "hi_lists" and s.idx.last_range()["exact"] == 0
    try:
        for opt, route in ((0, "exact_lists"), (2, "hi_lists")):
            s.set_hi_scan(opt)
            for r, b in zip(rb, base_b):
                got, _ = _check_batch(s, s.q, pk, r, tags, excl)
                info = s.idx.last_range()
                assert info["route"] == route and info["exact"] == nq, info
                np.testing.assert_array_equal(got[0], b[0])
                np.testing.assert_array_equal(got[2], b[2])
            for r, b in zip(rq, base_q):
                got, _ = _check_pq(s, s.q, pk, r, tags, qtags, counts)
                info = s.idx.last_range()
                assert info["route"] == route and info["exact"] == nq, info
                np.testing.assert_array_equal(got[0], b[0])
                np.testing.assert_array_equal(got[2], b[2])
    finally:
        s.set_hi_scan(1)


# ---- 7. the excluded crowd does not overflow ----------------------------------------------------------------------------------------
def test_07_the_excluded_crowd_takes_no_slot(store_a):
    """the in-scan property: 5000 rows lie within the radius of query 0 and the plain search overflows its 4096-position buffers; with
    63 of 64 tags excluded the store holds at most ceil(20000 / 64) = 313 admissible rows per query, so no buffer can overflow whatever
    the scan's error bound is -- unless excluded rows took slots"""
    s = store_a
    n, nlist, nq = len(s.db), s.nlist, len(s.q)
    s.idx.nprobe = nlist
    try:
        pk = s.pk(nlist)
        radius = RR.radius_between(pk, 0, 5000)                        # (on the unfiltered keys)
        _run_plain(s, s.q, radius)
        assert s.idx.last_range()["max_emitted"] > CAP
        tags = np.arange(n) % 64
        assert np.bincount(tags).max() == 313
        for keep in (0, 37):
            excl = np.setdiff1d(np.arange(64), [keep])
            got, ref = _check_batch(s, s.q, pk, radius, tags, excl)
            info = s.idx.last_range()
            assert info["route"] == "hi_lists" and info["exact"] == 0 and int(ref[0].max()) <= info["max_emitted"] <= 313, info
            assert ref[0].max() > 0 and (tags[got[2][got[2] >= 0]] == keep).all()
        qtags = np.stack([np.setdiff1d(np.arange(64), [j % 64]) for j in range(nq)])          # m = 63
        got, ref = _check_pq(s, s.q, pk, radius, tags, qtags)
        info = s.idx.last_range()
        assert info["route"] == "hi_lists" and info["exact"] == 0 and int(ref[0].max()) <= info["max_emitted"] <= 313, info
        for j in range(nq):
            assert (tags[got[2][j][got[2][j] >= 0]] == j % 64).all()
    finally:
        s.idx.nprobe = 8


# ---- 8. overflow by admissible rows -------------------------------------------------------------------------------------------------
def test_08_overflow_by_admissible_rows_goes_to_the_exact_pass(store_a):
    s = store_a
    n, nlist, nq = len(s.db), s.nlist, len(s.q)
    tags = np.arange(n) % 8
    s.idx.nprobe = nlist
    try:
        pk = s.pk(nlist)
        excl = np.array([5])
        got, ref = _check_batch(s, s.q, pk, float("inf"), tags, excl)
        info = s.idx.last_range()
        assert info == {"queries": nq, "route": "hi_lists", "exact": nq, "max_emitted": n - n // 8}, info
        assert (got[0] == n - n // 8).all()
        _, I10 = s.idx.search_probed_excluding(s.dev(s.q), 10, s.dev(tags.astype(np.int64)), s.dev(excl.astype(np.int64)))
        np.testing.assert_array_equal(got[2][:, :10], I10.cpu().numpy())
        got1, _ = _check_batch(s, s.q, pk, float("inf"), tags, excl, m=10)
        np.testing.assert_array_equal(got1[2], I10.cpu().numpy())
        # one set per query: query j excludes tag j % 8
        qtags = (np.arange(nq) % 8).reshape(-1, 1)
        gotq, refq = _check_pq(s, s.q, pk, float("inf"), tags, qtags)
        info = s.idx.last_range()
        assert info == {"queries": nq, "route": "hi_lists", "exact": nq, "max_emitted": n - n // 8}, info
        assert (gotq[0] == n - n // 8).all()
        _, Iq = s.idx.search_probed_excluding_per_query(s.dev(s.q), 10, s.dev(tags.astype(np.int64)), s.dev(qtags.astype(np.int64)))
        np.testing.assert_array_equal(gotq[2][:, :10], Iq.cpu().numpy())
        gotq1, _ = _check_pq(s, s.q, pk, float("inf"), tags, qtags, m=10)
        np.testing.assert_array_equal(gotq1[2], Iq.cpu().numpy())
    finally:
        s.idx.nprobe = 8


# ---- 9. identities, bit for bit -----------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))
    np.testing.assert_array_equal(a[3].view(np.int64), b[3].view(np.int64))


def test_09_identities_bit_for_bit(store_a):
    s = store_a
    s.idx.nprobe = 8
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    pk = s.pk(8)
    mid, big = _three_radii(pk, 400)[1:]
    try:
        for opt in (1, 0):
            s.set_hi_scan(opt)
            for radius in (mid, big):
                plain = _run_plain(s, s.q, radius)
                route = s.idx.last_range()["route"]
                for other in (_run_batch(s, s.q, radius, tags, None), _run_batch(s, s.q, radius, tags, np.zeros(0, np.int64)),
                              _run_batch(s, s.q, radius, tags, np.array([8, 99, -1])),               # a set that names no stored tag
                              _run_pq(s, s.q, radius, tags, None), _run_pq(s, s.q, radius, tags, np.zeros((nq, 0), np.int64)),
                              _run_pq(s, s.q, radius, tags, np.full((nq, 3), 77)),                   # tags no row carries
                              _run_pq(s, s.q, radius, tags, np.full((nq, 3), 2), np.zeros(nq, np.int32))):      # every count 0
                    assert s.idx.last_range()["route"] == route
                    _same_bits(other, plain)
                S = np.array([6, 1, 1, 4])
                a = _run_pq(s, s.q, radius, tags, np.tile(S, (nq, 1)))
                b = _run_batch(s, s.q, radius, tags, np.unique(S))
                _same_bits(a, b)
                assert (b[0] < plain[0]).any()
    finally:
        s.set_hi_scan(1)


# ---- 10. ties -----------------------------------------------------------------------------------------------------------------------
def test_10_ties_come_in_ascending_insertion_id(gpu, store_a):
    """41 rows with equal keys at scattered insertion ids (tests/test_gpu_ivf_range.py's test_07); 10 of them excluded: the 31 left come
    out as one run in ascending insertion id"""
    db = store_a.db.copy()
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
        assert len(keys) == 41 and (keys == keys[0]).all()
    tags = np.arange(n, dtype=np.int64)
    excl = same[[0, 3, 4, 9, 17, 18, 19, 30, 39, 40]]
    left = np.setdiff1d(same, excl)
    assert len(left) == 31
    fpk = XR.filter_batch(pk, tags, excl)
    k1 = np.sort(fpk[1][1])
    radius = RR.radius_between(fpk, 1, int((k1 <= fpk[1][1][np.isin(fpk[1][0], same)][0]).sum()) + 3)
    qtags = np.tile(excl[::-1], (4, 1))
    try:
        for opt in (1, 0):
            s.set_hi_scan(opt)
            for got, ref in (_check_batch(s, s.q, pk, radius, tags, excl), _check_pq(s, s.q, pk, radius, tags, qtags)):
                assert s.idx.last_range()["route"] == ("hi_lists" if opt else "exact_lists")
                for j in range(4):
                    ids = got[2][j]
                    at = np.flatnonzero(np.isin(ids, same))
                    assert len(at) == 31 and (np.diff(at) == 1).all()          # one run of equal keys ...
                    np.testing.assert_array_equal(ids[at], left)               # ... in ascending insertion id, the excluded ones gone
    finally:
        s.set_hi_scan(1)


# ---- 11. every list probed equals the flat store ------------------------------------------------------------------------------------
def test_11_every_list_probed_equals_the_flat_store(gpu, store_a):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = store_a
    nq = len(s.q)
    flat = R.HipFlatIndex(64, _lib.METRIC_L2, device=gpu.index or 0)
    flat.add(s.db)
    tags = np.arange(len(s.db)) % 8
    excl = np.array([1, 3, 4])
    qtags, counts = _pair_tags(nq)
    pk = s.pk(s.nlist)
    s.idx.nprobe = s.nlist
    try:
        rb = RR.radius_between(XR.filter_batch(pk, tags, excl), 0, 100)
        got, ref = _check_batch(s, s.q, pk, rb, tags, excl)
        rq = RR.radius_between(XR.filter_pq(pk, tags, qtags, counts), 0, 100)
        gotq, refq = _check_pq(s, s.q, pk, rq, tags, qtags, counts)
    finally:
        s.idx.nprobe = 8
    t_tags = s.dev(tags.astype(np.int64))
    fc, fd, fi, fk = _host(flat.range_search_excluding_device(s.dev(s.q), rb, t_tags, s.dev(np.sort(excl).astype(np.int64)), max_per_query=M,
                                                              return_f64=True))
    np.testing.assert_array_equal(got[0], fc)
    np.testing.assert_array_equal(got[2], fi)
    np.testing.assert_allclose(got[3][fi >= 0], fk[fi >= 0], rtol=1e-12, atol=0)
    import torch
    fc, fd, fi, fk = _host(flat.range_search_excluding_per_query_device(s.dev(s.q), rq, t_tags, s.dev(qtags), s.dev(counts, torch.int32),
                                                                        max_per_query=M, return_f64=True))
    np.testing.assert_array_equal(gotq[0], fc)
    np.testing.assert_array_equal(gotq[2], fi)
    np.testing.assert_allclose(gotq[3][fi >= 0], fk[fi >= 0], rtol=1e-12, atol=0)
    b = XR.brute_batch(s.db, s.q, tags, excl, rb, M)
    np.testing.assert_array_equal(got[0], b[0])
    np.testing.assert_array_equal(got[2], b[1])


# ---- 12. edges and errors -----------------------------------------------------------------------------------------------------------
def test_12_edges(gpu, store_a):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    s = store_a
    s.idx.nprobe = 8
    nq = len(s.q)
    tags = np.arange(len(s.db)) % 8
    excl = np.array([1, 3, 4])
    qtags, counts = _pair_tags(nq)
    pk = s.pk(8)
    mid = _three_radii(XR.filter_batch(pk, tags, excl), 250)[1]
    # a trained index without rows: count 0 and the padding, from both calls; nq == 0
    e = Store.__new__(Store)
    e.gpu, e.idx = gpu, R.HipIVFFlatIndex(64, 64, gpu.index or 0)
    e.idx.train(s.db[:5000])
    e.idx.nprobe = 8
    for out in (_host(e.idx.range_search_probed_excluding_device(e.dev(s.q[:7]), mid, None, None, return_f64=True)),
                _host(e.idx.range_search_probed_excluding_per_query_device(e.dev(s.q[:7]), mid, None, None, return_f64=True))):
        c, D, I, K = out
        assert (c == 0).all() and (I == -1).all() and np.isnan(D).all() and np.isnan(K).all()
        assert e.idx.last_range() == {"queries": 7, "route": "exact_lists", "exact": 0, "max_emitted": 0}
    lib, h = e.idx._lib, e.idx._h
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    q7 = e.dev(s.q[:7])
    c7 = torch.full((7,), 77, device=gpu, dtype=torch.int32)
    D7 = torch.full((7, M), 5.0, device=gpu)
    I7 = torch.full((7, M), 9, device=gpu, dtype=torch.int64)
    t1, x1 = e.dev(np.zeros(1, np.int64)), e.dev(np.zeros(1, np.int64))
    st = _lib.stream_ptr(gpu)
    # (an empty index has no row to tag: any non-NULL pointers with n_excl > 0 / m > 0 are never read)
    assert lib.radad_ivf_range_search_excl(h, q7.data_ptr(), 7, 8, mid, M, t1.data_ptr(), x1.data_ptr(), 1, c7.data_ptr(), D7.data_ptr(),
                                           I7.data_ptr(), None, st) == _lib.RADAD_OK
    torch.cuda.synchronize()
    assert (c7 == 0).all() and (I7 == -1).all() and torch.isnan(D7).all()
    c, D, I, K = _run_batch(s, s.q[:0], mid, tags, excl)
    assert c.shape == (0,) and D.shape == (0, M) and I.shape == (0, M)
    c, D, I, K = _run_pq(s, s.q[:0], mid, tags, qtags[:0], counts[:0])
    assert c.shape == (0,) and D.shape == (0, M) and I.shape == (0, M)
    # two runs give identical bytes; the top-k read-backs do not describe either call
    for run in (lambda: _run_batch(s, s.q, mid, tags, excl), lambda: _run_pq(s, s.q, mid, tags, qtags, counts)):
        a, b = run(), run()
        for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
            assert x.tobytes() == y.tobytes()
        with pytest.raises(ValueError, match="was a range search"):
            s.idx.last_search_info()
    # a call on a second stream right after one on the first gives the same result
    first = _run_batch(s, s.q, mid, tags, excl)
    firstq = _run_pq(s, s.q, mid, tags, qtags, counts)
    side = torch.cuda.Stream(device=gpu)
    q_t, t_t, x_t = s.dev(s.q), s.dev(tags.astype(np.int64)), s.dev(np.sort(excl).astype(np.int64))
    qt_t, ct_t = s.dev(qtags), s.dev(counts, torch.int32)
    torch.cuda.synchronize()
    main_out = s.idx.range_search_probed_excluding_device(q_t, mid, t_t, x_t, return_f64=True)
    with torch.cuda.stream(side):
        side_out = s.idx.range_search_probed_excluding_per_query_device(q_t, mid, t_t, qt_t, ct_t, return_f64=True)
    main_again = s.idx.range_search_probed_excluding_device(q_t, mid, t_t, x_t, return_f64=True)
    torch.cuda.synchronize()
    _same_bits(_host(main_out), first)
    _same_bits(_host(side_out), firstq)
    _same_bits(_host(main_again), first)


def test_12_c_argument_errors_leave_the_outputs_untouched(gpu, store_a):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = store_a
    s.idx.nprobe = 8
    lib, h = s.idx._lib, s.idx._h
    tags = np.arange(len(s.db)) % 8
    excl = np.array([1, 3, 4])
    q = s.dev(s.q[:4])
    t_tags, t_excl = s.dev(tags.astype(np.int64)), s.dev(excl.astype(np.int64))
    qtags, qcounts = _pair_tags(4)
    t_qtags, t_qcounts = s.dev(qtags), s.dev(qcounts, torch.int32)
    counts = torch.full((4,), 77, device=gpu, dtype=torch.int32)
    D = torch.full((4, M), 5.0, device=gpu)
    I = torch.full((4, M), 9, device=gpu, dtype=torch.int64)
    K = torch.full((4, M), 6.0, device=gpu, dtype=torch.float64)
    st = _lib.stream_ptr(gpu)

    def call_b(handle=h, nq=4, nprobe=8, radius=1.0, m=M, rt=t_tags.data_ptr(), ex=t_excl.data_ptr(), n_excl=3, c=counts.data_ptr(),
               d=D.data_ptr(), i=I.data_ptr()):
        return lib.radad_ivf_range_search_excl(handle, q.data_ptr(), nq, nprobe, radius, m, rt, ex, n_excl, c, d, i, K.data_ptr(), st)

    def call_q(handle=h, nq=4, nprobe=8, radius=1.0, m=M, rt=t_tags.data_ptr(), qt=t_qtags.data_ptr(), tm=4, qc=t_qcounts.data_ptr(),
               c=counts.data_ptr(), d=D.data_ptr(), i=I.data_ptr()):
        return lib.radad_ivf_range_search_excl_pq(handle, q.data_ptr(), nq, nprobe, radius, m, rt, qt, tm, qc, c, d, i, K.data_ptr(), st)
    shared = (dict(m=0), dict(m=-3), dict(m=129), dict(radius=float("nan")), dict(c=None), dict(d=None), dict(i=None), dict(nprobe=0), dict(nq=-1))
    for kw in shared + (dict(n_excl=-1), dict(rt=None), dict(ex=None)):
        assert call_b(**kw) == _lib.RADAD_EINVAL, kw
    for kw in shared + (dict(tm=-1), dict(tm=65), dict(rt=None), dict(qt=None)):
        assert call_q(**kw) == _lib.RADAD_EINVAL, kw
    untrained = R.HipIVFFlatIndex(64, 64, gpu.index or 0)
    assert call_b(handle=untrained._h) == _lib.RADAD_ESTATE and call_q(handle=untrained._h) == _lib.RADAD_ESTATE
    with pytest.raises(ValueError, match="not trained"):
        untrained.range_search_probed_excluding_device(s.q[:4], 1.0, None, None)
    torch.cuda.synchronize()
    assert (counts == 77).all() and (D == 5.0).all() and (I == 9).all() and (K == 6.0).all()
    assert call_b(nq=0) == _lib.RADAD_OK and call_q(nq=0) == _lib.RADAD_OK      # nothing to do, nothing written
    torch.cuda.synchronize()
    assert (counts == 77).all() and (I == 9).all()
    # NULL tag arrays are fine when nothing is excluded
    pk = s.pk(8)[:4]
    radius = _three_radii(s.pk(8), 400)[1]
    plain = RR.members(pk, radius, M)
    assert call_b(radius=radius, rt=None, ex=None, n_excl=0) == _lib.RADAD_OK
    np.testing.assert_array_equal(counts.cpu().numpy(), plain[0])
    assert call_q(radius=radius, rt=None, qt=None, tm=0, qc=None) == _lib.RADAD_OK
    np.testing.assert_array_equal(I.cpu().numpy(), plain[1])
    # the handle is usable: a plain range search afterwards is correct, and last_range describes the calls with its four fields
    assert lib.radad_ivf_range_search(h, q.data_ptr(), 4, 8, radius, M, counts.data_ptr(), D.data_ptr(), I.data_ptr(), None, st) == _lib.RADAD_OK
    np.testing.assert_array_equal(counts.cpu().numpy(), plain[0])
    np.testing.assert_array_equal(I.cpu().numpy(), plain[1])
    ref = XR.members_batch(pk, tags, excl, radius, M)
    assert call_b(radius=radius) == _lib.RADAD_OK
    np.testing.assert_array_equal(counts.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])
    nq, route, ex, me = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    assert lib.radad_ivf_last_range(h, C.byref(nq), C.byref(route), C.byref(ex), C.byref(me)) == _lib.RADAD_OK
    assert (nq.value, route.value, ex.value) == (4, 0, 0) and int(ref[0].max()) <= me.value <= CAP
    kind, rej = C.c_int(), C.c_int()
    assert lib.radad_ivf_last_search_info(h, C.byref(kind), C.byref(rej)) == _lib.RADAD_ESTATE
    assert lib.radad_ivf_last_search_counts(h, C.byref(kind), C.byref(rej)) == _lib.RADAD_ESTATE
    refq = XR.members_pq(pk, tags, qtags, qcounts, radius, M)
    assert call_q(radius=radius) == _lib.RADAD_OK
    np.testing.assert_array_equal(counts.cpu().numpy(), refq[0])
    np.testing.assert_array_equal(I.cpu().numpy(), refq[1])
    assert lib.radad_ivf_last_search_info(h, C.byref(kind), C.byref(rej)) == _lib.RADAD_ESTATE


# ---- 13. the shell ------------------------------------------------------------------------------------------------------------------
def _config(gpu, tmp_path, index_type, nprobe=16):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as Rad
    cfg = Rad.Config()
    cfg.update(device=gpu, feature_dim=64, tpp_levels=[1], top_k=5, vector_db_index_type=index_type, vector_db_nprobe=nprobe,
               vector_db_path=str(tmp_path / ("vdb_" + index_type)))
    cfg.ivf_nlist = 32                                                # max(64, 32) -> 64 lists
    return Rad, cfg


def test_13_vector_database_and_near_duplicates(gpu, tmp_path):
    """a clip with 200 stored segments of its own within the radius: the post-filter audit gives them all 128 slots, the exclusion inside
    the list scans gives every slot to another file's (another speaker's) rows and counts those exactly"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    Rad, cfg = _config(gpu, tmp_path, "IVF")

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")
    pipe = Rad.HotPathPipeline(cfg, feature_extractor=NoExtractor())
    vdb = pipe.vector_db
    db = _clustered(12000, 64, 40, 8601)
    q = _queries(20, 64, 40, 8601)
    n = len(db)
    paths = [f"/train/spk{i % 97}/f{i}.wav" for i in range(n)]
    speakers = [f"spk{i % 97}" for i in range(n)]
    # query 2: 200 stored segments of the clip itself (one basename, one speaker), nearer than anything else
    own = np.arange(200) * 53 + 11
    db[own] = q[2] + synth.rows(0, 200, 64, 8611) * np.float32(1e-2)
    for i in own:
        paths[i], speakers[i] = "/train/spk_own/clip2.wav", "spk_own"
    labels = [i % 2 for i in range(n)]
    query_paths = [f"/eval/clip{j}.wav" for j in range(len(q))]
    query_speakers = [f"evalspk{j}" for j in range(len(q))]
    query_speakers[2] = "spk_own"
    query_speakers[5] = "spk3"                                        # an ordinary speaker: 124 rows scattered over the store
    vdb.add_vectors(db, paths, labels, {"speaker_id": speakers})
    assert isinstance(vdb.index, Rad.HipIVFFlatIndex) and vdb.index.ntotal == n
    cent, assign = vdb.index.centroids(), vdb.index.assignments()
    pk = RR.probed_keys(db, assign, cent, q, 16)
    file_tags = np.array([path_tag(p) for p in paths], np.int64)
    spk_tags = np.array([pipe._speaker_tag(s_) for s_ in speakers], np.int64)
    q_file = np.array([path_tag(p) for p in query_paths], np.int64).reshape(-1, 1)
    q_spk = np.array([pipe._speaker_tag(s_) for s_ in query_speakers], np.int64).reshape(-1, 1)
    radius = RR.radius_between(XR.filter_pq(pk, file_tags, q_file), 2, 150)      # 150 OTHER rows within the radius of query 2
    ref_file = _guard(XR.members_pq(pk, file_tags, q_file, None, radius, M))
    ref_spk = _guard(XR.members_pq(pk, spk_tags, q_spk, None, radius, M))
    plain = RR.members(pk, radius, M)
    assert plain[0][2] == 350 and ref_file[0][2] == 150 and np.isin(plain[1][2], own).all()      # the own segments fill all 128 slots
    # VectorDatabase: CSR form and counts, one set per query (the store's basename tags by default) and one set for the batch
    lims, D, I, counts = vdb.range_search_probed_excluding_per_query_batch(q, radius, query_tags=q_file, return_counts=True)
    assert isinstance(lims, np.ndarray) and vdb.index.nprobe == 16
    np.testing.assert_array_equal(counts, ref_file[0])
    kept = np.minimum(ref_file[0], M)
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(kept)]))
    for j in range(len(q)):
        np.testing.assert_array_equal(I[lims[j]:lims[j + 1]], ref_file[1][j, :kept[j]])
        np.testing.assert_allclose(D[lims[j]:lims[j + 1]], ref_file[2][j, :kept[j]].astype(np.float32), rtol=1.2e-7)
    out = vdb.range_search_probed_excluding_per_query_batch(torch.from_numpy(q).to(gpu), radius, query_tags=q_spk, row_tags=spk_tags, max_per_query=5,
                                                            return_counts=True)
    assert all(t.is_cuda for t in out)
    np.testing.assert_array_equal(out[3].cpu().numpy(), ref_spk[0])
    np.testing.assert_array_equal(out[0].cpu().numpy(), np.concatenate([[0], np.cumsum(np.minimum(ref_spk[0], 5))]))
    excl = [path_tag("/x/clip2.wav"), path_tag("/train/f3.wav")]
    ref_b = _guard(XR.members_batch(pk, file_tags, np.array(excl), radius, M))
    lims, D, I, counts = vdb.range_search_probed_excluding_batch(q, radius, exclude_tags=excl, return_counts=True)
    np.testing.assert_array_equal(counts, ref_b[0])
    np.testing.assert_array_equal(I, np.concatenate([ref_b[1][j, :min(ref_b[0][j], M)] for j in range(len(q))]))
    lims0, _, I0 = vdb.range_search_probed_excluding_batch(q, radius)[:3]       # nothing excluded: the plain search
    np.testing.assert_array_equal(I0, np.concatenate([plain[1][j, :min(plain[0][j], M)] for j in range(len(q))]))
    # the audit
    for exclude, ref, kw in (("file", ref_file, dict(query_paths=query_paths)), ("speaker", ref_spk, dict(query_speakers=query_speakers))):
        hits, counts = pipe.near_duplicates(q, radius, probed=True, probed_exclusion=True, exclude=exclude, **kw)
        np.testing.assert_array_equal(counts, ref[0])
        for j in range(len(q)):
            k = min(ref[0][j], M)
            assert [h[0] for h in hits[j]] == [paths[int(i)] for i in ref[1][j, :k]]
            assert all(h[2] < radius for h in hits[j])
        assert counts[2] == 150 and len(hits[2]) == M                  # all slots go to other rows ...
        assert not any(os.path.basename(h[0]) == "clip2.wav" for h in hits[2])
        if exclude == "speaker":
            assert not any("/spk_own/" in h[0] for h in hits[2]) and not any("/spk3/" in h[0] for h in hits[5])
    post = pipe.near_duplicates(q, radius, query_paths=query_paths, probed=True)
    assert len(post[2]) == 0 < M                                      # ... where the default post-filter path returns fewer: none at all
    # what is not offered says so
    with pytest.raises(ValueError, match="exact_exclusion is not offered with probed=True"):
        pipe.near_duplicates(q, radius, query_paths=query_paths, probed=True, exact_exclusion=True)
    with pytest.raises(ValueError, match="probed_exclusion needs probed=True"):
        pipe.near_duplicates(q, radius, query_paths=query_paths, probed_exclusion=True)
    Rad2, cfg2 = _config(gpu, tmp_path, "L2")
    flat_pipe = Rad2.HotPathPipeline(cfg2, feature_extractor=NoExtractor())
    flat_pipe.vector_db.add_vectors(db[:2000], paths[:2000], labels[:2000], {})
    with pytest.raises(ValueError, match="a flat store has range_search_excluding_batch"):
        flat_pipe.vector_db.range_search_probed_excluding_batch(q, radius, exclude_tags=excl)
    with pytest.raises(ValueError, match="a flat store has range_search_excluding_per_query_batch"):
        flat_pipe.near_duplicates(q, radius, query_paths=query_paths, probed=True, probed_exclusion=True)
