"""Certified range search of a batch of 16 or fewer queries (RADAD_KNN_OPT_RANGE_SMALLQ, route RADAD_RANGE_STREAM): the f16 plane
streamed once by k_range_hi_smallq in front of the range search's own re-rank.

Every case is compared two ways: against range_ref.expected_range (one set / a set per query: range_excl_ref.expected_range_excl),
float64 numpy over the rows AS STORED, with tests/test_gpu_knn_range.py's tolerances and its _check contract; and against the same call
on a second handle with the option off (the float64 exact route): counts, ids and float64 keys equal bit for bit.  Every stream-route
case asserts the route, the number of queries the exact kernel answered, one scan launch, and that the measured eps (the threshold
minus the floor the scan ran with, radad_knn_last_emitted) is positive and within range_ref.EPS_MODEL.

The stores are tests/range_smallq_ref.case's, 16 677 rows each; tests/test_range_smallq_model.py asserts on the CPU that none has a row
within 1e-9 of its radius and that only the crowd query can overflow a buffer.

Measured on an MI355X (largest threshold - floor over the batch): see profiles/README.md, "Range search", small batches.

The keys of the two routes: the stream route's re-rank is k_range_refine<.., true>, whose re-score adds a row's float64 products in
the order and with the roundings of k_exact_scan_any (refine_rescore_f64<true>); the plain re-score's 16-lane sums differ from that
kernel's 64-lane sums by 1 unit of the last place at dim 128 (ip1) and 2 at dim 576 (knife_l2).  Every case prints the largest
difference before it asserts that there is none."""
import numpy as np
import pytest

import range_excl_ref as X
import range_ref as R
import range_smallq_ref as S

pytestmark = pytest.mark.gpu


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


def _mk(metric, dim, kind="uncentred", **kw):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    if kind == "f16":
        return HipFlatIndex(dim, m, 0, 0, store_f16=True, **kw)
    return HipFlatIndex(dim, m, 0, 0, centre=1 if kind == "centred" else 0, **kw)


class _Pair:
    """two handles holding a designed case's rows -- `on` with the option set, `off` without (the exact route) -- and the rows as stored"""

    def __init__(self, gpu, c, **kw):
        import torch
        self.gpu, self.metric, self.kind, self.c = gpu, c["metric"], c["kind"], c
        rows = _dev(np.asarray(c["db"], np.float32), gpu)
        self.on = _mk(self.metric, c["db"].shape[1], self.kind, range_smallq=1, **kw)
        self.off = _mk(self.metric, c["db"].shape[1], self.kind)
        self.on.add_device(rows)
        self.off.add_device(rows)
        n = self.on.ntotal
        self.stored = self.on.reconstruct_batch(torch.arange(n, device=gpu)).cpu().numpy()
        self._keys_of = None
        self.key_pairs = []

    def call(self, idx, q, radius, M, bf16=False, excl=None, pq=None):
        """excl = (row_tags, set or None): one set for the batch; pq = (row_tags, q_tags, q_cnt or None): a set per query"""
        import torch
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        if bf16:
            qt = qt.to(torch.bfloat16)
        if excl is not None:
            out = idx.range_search_excluding_device(qt, radius, _dev(excl[0], self.gpu), None if excl[1] is None else _dev(excl[1], self.gpu),
                                                    M, return_f64=True)
        elif pq is not None:
            out = idx.range_search_excluding_per_query_device(qt, radius, _dev(pq[0], self.gpu), _dev(pq[1], self.gpu),
                                                              None if pq[2] is None else _dev(pq[2], self.gpu), M, return_f64=True)
        else:
            out = idx.range_search_device(qt, radius, M, return_f64=True)
        return out + (idx.last_range(),)

    def both(self, q, radius, M, **kw):
        """the call on both handles; the option-off handle took the exact route and the two agree: counts and ids here, the bits of
        the float64 keys when the test ends (keys_bit_equal), so that a test's other checks run first"""
        a = self.call(self.on, q, radius, M, **kw)
        b = self.call(self.off, q, radius, M, **kw)
        assert b[4] == {"queries": len(q), "route": "exact", "exact": len(q)}, b[4]
        _same_rows(a, b)
        self.key_pairs.append((a, b))
        return a

    def keys_bit_equal(self):
        """every pair of results both() has seen since the last call: the float64 keys (and the float32 distances rounded from them)
        of the stream route and of the exact route, bit for bit; prints the largest distance in units of the last place first"""
        import torch
        pairs, self.key_pairs = self.key_pairs, []
        worst = 0
        for a, b in pairs:
            f = a[2] >= 0
            if bool(f.any()):
                worst = max(worst, int((a[3][f].view(torch.int64) - b[3][f].view(torch.int64)).abs().max()))
        print(f"{self.c['name']}: float64 keys of the stream route against the exact route over {len(pairs)} calls: largest difference {worst} ulp")
        for a, b in pairs:
            _same_bits(a, b)

    def keys(self, q):
        metric = "IP" if self.metric == "COSINE" else self.metric
        tag = np.asarray(q, np.float32).tobytes()
        if self._keys_of != tag:
            self._keys = R.keys(self.stored, _rownorm(self.gpu, q) if self.metric == "COSINE" else q, metric)
            self._keys_of = tag
        return self._keys

    def reference(self, q, radius, M, adm=None):
        metric = "IP" if self.metric == "COSINE" else self.metric
        if adm is None:
            return R.expected_range(self.stored, q, radius, metric, M, 0, key=self.keys(q))
        return X.expected_range_excl(self.stored, q, radius, metric, M, adm, 0, key=self.keys(q))


def _same_rows(a, b):
    import torch
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.equal(a[2], b[2])


def _same_bits(a, b):
    import torch
    _same_rows(a, b)
    assert torch.equal(a[3].view(torch.int64), b[3].view(torch.int64))                # NaN padding included: the same bits
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _check(out, ref, metric, M):
    """tests/test_gpu_knn_range.py's contract and tolerances"""
    counts, D, I, K64 = (t.cpu().numpy() for t in out[:4])
    ec, ei, ek, boundary = ref
    assert not boundary.any(), "boundary rows in a store that should have none"
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    np.testing.assert_array_equal(f.sum(axis=1), np.minimum(ec, M))
    if metric == "COSINE":
        np.testing.assert_allclose(K64[f], ek[f], rtol=0, atol=1e-4)
    else:
        np.testing.assert_allclose(K64[f], ek[f], rtol=1e-6, atol=1e-6)
    assert np.all(I[~f] == -1) and np.all(np.isnan(D[~f])) and np.all(np.isnan(K64[~f]))      # padding: -1 / NaN / NaN
    np.testing.assert_array_equal(K64[f].astype(np.float32), D[f])                  # out_dist is the key, rounded once


def _expect_stream(p, info, nq, radius, n_exact, what=""):
    """the stream route ran in one launch, exactly `n_exact` queries went to the exact pass, and the scan's eps is within the model's"""
    assert info == {"queries": nq, "route": "stream", "exact": n_exact}, info
    emitted, floors = p.on.last_emitted(nq)
    launch = p.on.last_launch()
    assert launch["scan_launches"] == 1 and launch["scan_phases"] == 1, launch
    slices = (p.on.ntotal + S.ROWS_PER_WAVE - 1) // S.ROWS_PER_WAVE
    assert launch["db_splits"] == (slices + 3) // 4, launch                          # workgroups of four 128-row slices
    assert launch["early_abandon"]["tasks"] == 0
    if np.isfinite(radius):
        T = -radius if p.metric == "L2" else radius
        eps = np.float64(T) - floors.astype(np.float64)
        print(f"{p.c['name']}{what} {p.metric} nq {nq}: measured eps (threshold - floor) max {eps.max():.3e} min {eps.min():.3e}; "
              f"emitted {emitted.tolist()}; {info}")
        assert (eps > 0).all()
        assert eps.max() <= R.EPS_MODEL[p.metric], \
            f"the scan's eps {eps.max():.3e} exceeds range_ref.EPS_MODEL[{p.metric!r}] = {R.EPS_MODEL[p.metric]}"
    else:
        assert (floors == -np.inf).all()
    return emitted


@pytest.fixture(scope="module")
def pairs(gpu):
    """one pair of handles per designed case, built once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Pair(gpu, S.case(name))
        cache[name].key_pairs = []
        return cache[name]
    yield get
    cache.clear()


# ---- must fail without the feature ---------------------------------------------------------------------------------------------------------
def test_0_the_option_is_taken_and_selects_the_stream(gpu, pairs):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    c = S.case("knife_cos16")
    idx = _mk("COSINE", 64)
    lib = idx._lib
    assert lib.radad_knn_set_option(idx._h, 6, 1) == _lib.RADAD_OK                   # (RADAD_EINVAL before the option existed)
    assert lib.radad_knn_set_option(idx._h, 6, 2) == _lib.RADAD_EINVAL and lib.radad_knn_set_option(idx._h, 6, -1) == _lib.RADAD_EINVAL
    idx.add_device(_dev(c["db"], gpu))
    idx.range_search_device(_dev(c["q"][:1], gpu), 0.9, 8)
    assert idx.last_range() == {"queries": 1, "route": "stream", "exact": 0}
    assert lib.radad_knn_set_option(idx._h, 6, 0) == _lib.RADAD_OK                   # ... and off again: the exact route, as before
    idx.range_search_device(_dev(c["q"][:1], gpu), 0.9, 8)
    assert idx.last_range() == {"queries": 1, "route": "exact", "exact": 1}


# ---- the store cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["knife_cos16", "knife_l2", "ip1", "centred16", "knife_f16", "knife_bf16"])
def test_1_store_cases(gpu, pairs, name):
    p = pairs(name)
    c = p.c
    for nq in sorted({len(c["q"]), min(len(c["q"]), 7)}):                            # all the case's queries; fewer than 16 columns
        q = c["q"][:nq]
        ref = p.reference(q, c["radius"], c["M"])
        out = p.both(q, c["radius"], c["M"], bf16=name == "knife_bf16")
        _check(out, ref, p.metric, c["M"])
        _expect_stream(p, out[4], nq, c["radius"], 0)
        if name in ("knife_f16", "knife_bf16"):
            # rows rounded to fp16 / queries rounded to bfloat16 move the knife rows (1e-5 from the threshold) across it either way:
            # the reference over the rows and queries as used decides; the rows planted well inside are all there
            assert ref[0].sum() > 0 and (ref[0] <= np.array(c["counts"][:nq]) + 40).all()
            continue
        np.testing.assert_array_equal(ref[0], c["counts"][:nq])                      # the planted rows: every one inside, none outside
        for j in range(nq):
            np.testing.assert_array_equal(np.sort(out[2][j, :ref[0][j]].cpu().numpy()), np.sort(c["info"]["planted_in"][j]))
    if name == "centred16":
        assert p.on.plane_info()["centred"], p.on.plane_info()
    if name == "knife_f16":
        assert not p.on.plane_info()["built"]                                        # an fp16 store is its own plane
    p.keys_bit_equal()


def test_2_a_list_cut_to_max_per_query_keeps_the_exact_count(gpu, pairs):
    p = pairs("many9")
    c = p.c
    for M in (16, 1024):
        ref = p.reference(c["q"], c["radius"], M)
        out = p.both(c["q"], c["radius"], M)
        _check(out, ref, p.metric, M)
        _expect_stream(p, out[4], 9, c["radius"], 0, f" M {M}")
        assert int(out[0][0]) == 300 and int((out[2][0] >= 0).sum()) == min(M, 300)
    p.keys_bit_equal()


def test_3_an_overflowing_query_goes_to_the_exact_pass_alone(gpu, pairs):
    p = pairs("crowd5")
    c = p.c
    ref = p.reference(c["q"], c["radius"], c["M"])
    out = p.both(c["q"], c["radius"], c["M"])
    _check(out, ref, p.metric, c["M"])
    emitted = _expect_stream(p, out[4], 5, c["radius"], 1)
    assert emitted[0] >= 5000 > R.BUFFER and (emitted[1:] <= R.BAND_CAP).all()       # the counter counts past the buffer
    assert out[0].cpu().tolist() == [5000, 1, 5, 12, 0]
    # emitted once each: a query's count of emitted rows is at least its rows within the radius and at most its rows in the band
    band, inside = R.band_counts(p.stored, _rownorm(gpu, c["q"]), c["radius"], "IP")
    assert (emitted >= inside).all() and (emitted <= band).all(), (emitted, inside, band)
    p.keys_bit_equal()


def test_4_rows_at_step_wave_and_workgroup_boundaries(gpu):
    d, src = S.with_boundary_copies(S.case("knife_cos16"))
    p = _Pair(gpu, d)
    ref = p.reference(d["q"], d["radius"], d["M"])
    out = p.both(d["q"], d["radius"], d["M"])
    _check(out, ref, p.metric, d["M"])
    _expect_stream(p, out[4], 16, d["radius"], 0, " boundary copies")
    got = out[2][3].cpu().numpy()
    K = out[3][3].cpu().numpy()
    copies = np.sort(np.array(S.BOUNDARY_ROWS + (src,)))
    at = np.flatnonzero(np.isin(got, copies))
    assert len(at) == len(copies) and (np.diff(at) == 1).all()                       # all nine and the original, next to each other ...
    np.testing.assert_array_equal(got[at], copies)                                   # ... in id order ...
    assert len(set(K[at].tolist())) == 1                                             # ... among their equal keys
    p.keys_bit_equal()


def test_5_everything_and_nothing(gpu, pairs):
    p = pairs("knife_cos16")
    c = p.c
    q = c["q"][:2]
    out = p.both(q, -np.inf, 64)
    _check(out, p.reference(q, -np.inf, 64), p.metric, 64)
    emitted = _expect_stream(p, out[4], 2, -np.inf, 2)
    assert (emitted == p.on.ntotal).all() and (out[0].cpu().numpy() == p.on.ntotal).all()
    out = p.both(c["q"], 1.5, 64)
    _check(out, p.reference(c["q"], 1.5, 64), p.metric, 64)
    emitted = _expect_stream(p, out[4], 16, 1.5, 0)
    assert (emitted == 0).all()
    assert int(out[0].abs().sum()) == 0 and int((out[2] != -1).sum()) == 0 and bool(out[1].isnan().all()) and bool(out[3].isnan().all())
    p.keys_bit_equal()


def test_6_a_nan_radius_is_refused_with_the_outputs_untouched(gpu, pairs):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    p = pairs("knife_cos16")
    q = _dev(p.c["q"], gpu)
    M = 8
    cnt = torch.full((16,), -7, dtype=torch.int32, device=gpu)
    D = torch.full((16, M), 123.0, dtype=torch.float32, device=gpu)
    I = torch.full((16, M), -7, dtype=torch.int64, device=gpu)
    rc = p.on._lib.radad_knn_range_search(p.on._h, q.data_ptr(), _lib.Q_F32, 16, float("nan"), M, cnt.data_ptr(), D.data_ptr(), I.data_ptr(),
                                          None, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == _lib.RADAD_EINVAL
    assert (cnt == -7).all() and (D == 123.0).all() and (I == -7).all()
    out = p.call(p.on, p.c["q"], 0.9, M)                                             # the handle is usable
    assert out[4]["route"] == "stream"
    np.testing.assert_array_equal(out[0].cpu().numpy(), p.c["counts"])


def test_7_seventeen_queries_on_the_same_handle_take_the_tile_route(gpu, pairs):
    p = pairs("knife_cos16")
    c = p.c
    q = np.concatenate([c["q"], c["q"][3:4]])
    out = p.call(p.on, q, c["radius"], c["M"])
    assert out[4] == {"queries": 17, "route": "tile", "exact": 0}, out[4]
    _check(out, p.reference(q, c["radius"], c["M"]), p.metric, c["M"])
    again = p.call(p.on, c["q"], c["radius"], c["M"])
    assert again[4]["route"] == "stream"


@pytest.mark.parametrize("kw", [dict(hi_plane=0), dict(smallq_hi=0)], ids=["plane_off", "smallq_hi_0"])
def test_8_without_the_plane_or_the_small_batch_stream_the_route_is_exact(gpu, kw):
    c = S.case("knife_cos16")
    p = _Pair(gpu, c, **kw)
    out = p.call(p.on, c["q"], c["radius"], c["M"])
    assert out[4] == {"queries": 16, "route": "exact", "exact": 16}, out[4]
    _check(out, p.reference(c["q"], c["radius"], c["M"]), p.metric, c["M"])


# ---- exclusion -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes", [None, 5, 9], ids=["none", "half", "nine_tenths"])
def test_9_one_set_for_the_batch(gpu, pairs, n_classes):
    p = pairs("knife_cos16")
    c = p.c
    row_tags = S.tags_by_class(c)
    excl = None if n_classes is None else S.class_set(n_classes)
    adm = X.admissible_batch(row_tags, excl, 16)
    if excl is not None:
        assert abs((~adm[0]).mean() - n_classes / 10) < 0.01 and not adm[3, c["info"]["planted_in"][3]].any()
    ref = p.reference(c["q"], c["radius"], c["M"], adm)
    out = p.both(c["q"], c["radius"], c["M"], excl=(row_tags, excl))
    _check(out, ref, p.metric, c["M"])
    emitted = _expect_stream(p, out[4], 16, c["radius"], 0, f" one set, {n_classes} classes")
    I = out[2].cpu().numpy()
    assert adm[0][I[I >= 0]].all()                                                   # no excluded id is ever returned
    if excl is None:
        _same_bits(out, p.call(p.on, c["q"], c["radius"], c["M"]))                   # nothing excluded: the plain stream call
    else:
        assert int(out[0][3]) == 0                                                   # every planted row of query 3 is excluded
        band = R.band_counts(p.stored, _rownorm(gpu, c["q"]), c["radius"], "IP")[0]
        assert emitted[3] <= band[3] - 40, (emitted, band)                           # ... and none of the 40 was emitted
        assert ref[0].sum() < sum(c["counts"])
    # against a floor of -inf an excluded row is still never emitted: its NaN score passes no compare
    if n_classes == 9:
        q2 = c["q"][:2]
        out2 = p.both(q2, -np.inf, c["M"], excl=(row_tags, excl))
        _check(out2, p.reference(q2, -np.inf, c["M"], adm[:2]), p.metric, c["M"])
        emitted2 = _expect_stream(p, out2[4], 2, -np.inf, 0, " one set, radius -inf")
        assert (emitted2 == adm[0].sum()).all() and adm[0].sum() <= R.BUFFER
    p.keys_bit_equal()


@pytest.mark.parametrize("m", [1, 64])
def test_10_one_set_per_query(gpu, pairs, m):
    p = pairs("knife_cos16")
    c = p.c
    row_tags = S.tags_by_query(c)
    q_tags = S.query_tags(16, m)
    adm = X.admissible_pq(row_tags, q_tags, None)
    ref = p.reference(c["q"], c["radius"], c["M"], adm)
    out = p.both(c["q"], c["radius"], c["M"], pq=(row_tags, q_tags, None))
    _check(out, ref, p.metric, c["M"])
    _expect_stream(p, out[4], 16, c["radius"], 0, f" per query, m {m}")
    np.testing.assert_array_equal(ref[0], [n // 2 for n in c["counts"]])             # each query lost every second planted row
    I = out[2].cpu().numpy()
    for j in range(16):
        assert adm[j][I[j][I[j] >= 0]].all()
    zero = np.zeros(16, np.int32)                                                    # all counts 0: the plain call
    _same_bits(p.call(p.on, c["q"], c["radius"], c["M"], pq=(row_tags, q_tags, zero)), p.call(p.on, c["q"], c["radius"], c["M"]))
    p.keys_bit_equal()


# ---- state and determinism -----------------------------------------------------------------------------------------------------------------
def test_11_a_stream_call_leaves_the_handle_state_alone(gpu):
    import torch
    c = S.case("crowd5")
    p = _Pair(gpu, c)
    qt = _dev(c["q"], gpu)
    p.on.search_device(qt, 10, return_f64=True)
    torch.cuda.synchronize()
    D0, I0, K0 = p.on.search_device(qt, 10, return_f64=True)                         # (consumes the first search's report)
    torch.cuda.synchronize()
    before, cert = p.on.tuning_info(), p.on.last_launch()
    assert cert["scan_kind"] == "hi_smallq" and cert["certificate"]["queries"] == 5
    o = p.call(p.on, c["q"], c["radius"], c["M"])                                    # one query overflows
    o2 = p.call(p.on, c["q"][:2], -np.inf, c["M"])
    torch.cuda.synchronize()
    assert o[4] == {"queries": 5, "route": "stream", "exact": 1} and o2[4] == {"queries": 2, "route": "stream", "exact": 2}
    assert p.on.tuning_info() == before
    after = p.on.last_launch()
    assert after["certificate"] == cert["certificate"] and after["rechecked_queries"] == cert["rechecked_queries"]
    assert after["scan_kind"] == cert["scan_kind"]
    D1, I1, K1 = p.on.search_device(qt, 10, return_f64=True)
    assert torch.equal(I0, I1) and torch.equal(D0.view(torch.int32), D1.view(torch.int32)) and torch.equal(K0.view(torch.int64), K1.view(torch.int64))
    assert p.on.tuning_info()["fp32_searches_left"] == before["fp32_searches_left"]
    # the keys of the range search are the keys the plain search reports
    assert int(o[0][3]) == 12 and torch.equal(o[2][3, :10], I1[3])
    np.testing.assert_allclose(o[3][3, :10].cpu().numpy(), K1[3].cpu().numpy(), rtol=1e-13, atol=0)


def test_12_the_same_call_twice(gpu, pairs):
    p = pairs("crowd5")
    c = p.c
    a = p.call(p.on, c["q"], c["radius"], c["M"])
    ea = p.on.last_emitted(5)
    b = p.call(p.on, c["q"], c["radius"], c["M"])
    eb = p.on.last_emitted(5)
    _same_bits(a, b)
    assert a[4] == b[4]
    np.testing.assert_array_equal(ea[0], eb[0])
    np.testing.assert_array_equal(ea[1].view(np.int32), eb[1].view(np.int32))
