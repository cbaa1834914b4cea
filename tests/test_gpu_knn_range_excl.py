"""Certified range search among the rows a query does not exclude (radad_knn_range_search_excl / _excl_pq,
HipFlatIndex.range_search_excluding / _per_query): every ADMISSIBLE row within a radius of each query, exactly -- the exact count, the
best max_per_query admissible rows in (float64 key, lower id) order, -1 / NaN / NaN in the other slots.

Expected results: tests/range_excl_ref.expected_range_excl, float64 numpy over the rows AS STORED (under cosine: their inner product
with the device's radad_rownorm of the query), restricted to the admissible rows.  Counts, ids and padding are compared exactly; the
float64 keys to 1e-12 relative (both sides sum the same float64 products of the same stored values, in another order).  The stores are range_excl_ref.case's: tests/test_range_excl_model.py asserts on the CPU that none has a boundary row
(the integer stores apart), that no tile-route query can overflow its 4096-entry buffer while the scan's eps stays below
range_ref.EPS_MODEL, and that the designed overflow queries must overflow.  On the tile route the number of queries the exact kernel
answered must EQUAL the number of designed overflow queries: a floor or filter mistake shows there and nowhere else.

Measured on an MI355X (largest threshold - floor over the batch; the batch twins' biased instantiation measures the same eps as the
per-query cases on the same store): see profiles/README.md, "Range search with exclusion"."""
import numpy as np
import pytest

import range_excl_ref as X
import range_ref as R

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


def _mk(metric, dim, kind="uncentred", id_base=0, **kw):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    if kind == "f16":
        return HipFlatIndex(dim, m, 0, id_base, store_f16=True, **kw)
    return HipFlatIndex(dim, m, 0, id_base, centre=1 if kind == "centred" else 0, **kw)


class _Store:
    """a handle holding a designed case's rows, the rows as it stores them, and the case's tags on the device"""

    def __init__(self, gpu, c, id_base=0, **kw):
        self.gpu, self.metric, self.kind, self.id_base, self.c = gpu, c["metric"], c["kind"], id_base, c
        self.idx = _mk(self.metric, c["db"].shape[1], self.kind, id_base, **kw)
        self.idx.add_device(_dev(np.asarray(c["db"], np.float32), gpu))
        self.row_tags = _dev(c["row_tags"], gpu)
        self.refresh()

    def refresh(self):
        import torch
        n, b = self.idx.ntotal, self.id_base
        self.stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(b + r0, b + min(n, r0 + 65536), device=self.gpu)).cpu().numpy()
                                      for r0 in range(0, n, 65536)])
        self._keys_of = None

    def run(self, q, radius, M, mode=None, sel=None, bf16=False, **tags):
        """the case's own tags for the queries sel (None: the first len(q)), or the ones handed in"""
        import torch
        c = self.c
        mode = mode or c["mode"]
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        if bf16:
            qt = qt.to(torch.bfloat16)
        sel = np.arange(len(q)) if sel is None else sel
        if mode == "batch":
            excl = tags.get("excl", c.get("excl"))
            out = self.idx.range_search_excluding_device(qt, radius, self.row_tags, None if excl is None else _dev(excl, self.gpu), M,
                                                         return_f64=True)
        else:
            q_tags = tags.get("q_tags", c["q_tags"][sel] if c.get("q_tags") is not None else None)
            q_cnt = tags.get("q_cnt", c["q_cnt"][sel] if c.get("q_cnt") is not None else None)
            out = self.idx.range_search_excluding_per_query_device(qt, radius, self.row_tags, None if q_tags is None else _dev(q_tags, self.gpu),
                                                                   None if q_cnt is None else _dev(q_cnt, self.gpu), M, return_f64=True)
        return out + (self.idx.last_range(),)

    def plain(self, q, radius, M):
        return self.idx.range_search_device(_dev(np.asarray(q, np.float32), self.gpu), radius, M, return_f64=True) + (self.idx.last_range(),)

    def keys(self, q):
        metric = "IP" if self.metric == "COSINE" else self.metric
        tag = (len(self.stored), np.asarray(q, np.float32).tobytes())
        if self._keys_of != tag:
            self._keys = R.keys(self.stored, _rownorm(self.gpu, q) if self.metric == "COSINE" else q, metric)
            self._keys_of = tag
        return self._keys

    def reference(self, q, radius, M, adm):
        """range_excl_ref.expected_range_excl over the rows as stored; the float64 keys of a batch are computed once per store"""
        metric = "IP" if self.metric == "COSINE" else self.metric
        return X.expected_range_excl(self.stored, q, radius, metric, M, adm, self.id_base, key=self.keys(q))


def _check(out, ref, metric, M):
    counts, D, I, K64 = (t.cpu().numpy() for t in out[:4])
    ec, ei, ek, boundary = ref
    assert not boundary.any() or metric in ("IP", "L2"), "boundary rows in a store that should have none"
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    np.testing.assert_array_equal(f.sum(axis=1), np.minimum(ec, M))
    np.testing.assert_allclose(K64[f], ek[f], rtol=1e-12, atol=0)
    assert np.all(I[~f] == -1) and np.all(np.isnan(D[~f])) and np.all(np.isnan(K64[~f]))      # padding: -1 / NaN / NaN
    np.testing.assert_array_equal(K64[f].astype(np.float32), D[f])                  # out_dist is the key, rounded once


def _expect_tile(s, info, nq, radius, n_exact):
    """the tile route ran, EXACTLY `n_exact` queries went to the exact pass, and the scan's eps is within the model's"""
    assert info["route"] == "tile" and info["queries"] == nq, info
    emitted, floors = s.idx.last_emitted(nq)
    launch = s.idx.last_launch()
    assert launch["scan_launches"] == 1 and launch["scan_phases"] == 1, launch
    if np.isfinite(radius):
        T = -radius if s.metric == "L2" else radius
        eps = np.float64(T) - floors.astype(np.float64)
        print(f"{s.c['name']} {s.metric} nq {nq}: measured eps (threshold - floor) max {eps.max():.3e} min {eps.min():.3e}; "
              f"emitted max {emitted.max()}; {info}")
        assert (eps > 0).all()
        assert eps.max() <= R.EPS_MODEL[s.metric], \
            f"the scan's eps {eps.max():.3e} exceeds range_ref.EPS_MODEL[{s.metric!r}] = {R.EPS_MODEL[s.metric]}: widen the constant, re-check the CPU caps"
    assert info["exact"] == n_exact, f"{info}: the design sends exactly {n_exact} queries to the exact pass"
    return emitted


@pytest.fixture(scope="module")
def stores(gpu):
    """one handle per designed store, built once (a case and its batch twin share the rows: the handle is the per-query case's)"""
    cache = {}

    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = _Store(gpu, X.case(name), **kw)
        return cache[key]
    yield get
    cache.clear()


def _case_run(gpu, stores, name, nqs=None, **kw):
    s = stores(name, **kw)
    c = s.c
    adm = X.admissible(c)
    outs = []
    for nq in nqs or (len(c["q"]),):
        q = c["q"][:nq]
        ref = s.reference(q, c["radius"], c["M"], adm[:nq])
        out = s.run(q, c["radius"], c["M"], bf16=name.startswith("graded_bf16"))
        _check(out, ref, s.metric, c["M"])
        n_over = int((c["overflow"] < nq).sum())
        if c["route"] == "tile":
            emitted = _expect_tile(s, out[4], nq, c["radius"], n_over)
            if n_over:
                assert (emitted[c["overflow"][c["overflow"] < nq]] > R.BUFFER).all()
        else:
            assert out[4] == {"queries": nq, "route": "exact", "exact": nq}, out[4]
        outs.append((out, ref))
    return s, outs


# ---- 1: graded neighbours, one set per query ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["graded_cosine", "graded_l2", "graded_ip", "centred", "graded_f16", "graded_bf16", "graded_dim128"])
def test_1_graded_neighbours_per_query_sets(gpu, stores, name):
    if name == "centred":
        s = stores(name)
        s.idx.search_device(_dev(s.c["q"], gpu), 1)                                  # (builds the plane)
        assert s.idx.plane_info()["centred"], s.idx.plane_info()
    s, outs = _case_run(gpu, stores, name, nqs=(17, 300))
    c = s.c
    (out, ref) = outs[1]
    live = X.live_counts(c["q_cnt"], 300, X.M_TAGS)
    want = [R.COUNTS[j % 4] - (len(c["info"]["planted_in"][j][0::2]) if live[j] else 0) for j in range(300)]
    np.testing.assert_array_equal(ref[0], want)                                      # the planted rows that do not carry the query's own tag
    plain = s.plain(c["q"], c["radius"], c["M"])
    assert int((plain[0] != out[0]).sum()) >= 150                                    # a call that ignored the tags would fail
    for j in (1, 2, 3):                                                              # the rows left are the planted rows at odd positions
        np.testing.assert_array_equal(np.sort(out[2][j, :ref[0][j]].cpu().numpy()), np.sort(c["info"]["planted_in"][j][1::2]))


# ---- 2: strictness and ties on exact keys ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["integer_ip", "integer_l2"])
def test_2_rows_that_hit_the_radius_are_out_and_ties_are_among_admissible_rows(gpu, stores, name):
    s, outs = _case_run(gpu, stores, name, nqs=(17, 300))
    c = s.c
    np.testing.assert_array_equal(s.stored, c["db"])
    out, ref = outs[1]
    K64 = out[3].cpu().numpy()
    filled = ref[1] >= 0
    assert (K64[filled] < c["radius"]).all() if s.metric == "L2" else (K64[filled] > c["radius"]).all()       # strictly
    np.testing.assert_array_equal(K64[filled], np.round(K64[filled]))                # integers: the keys compare equal bit for bit
    assert (ref[3] & X.admissible(c)).any(axis=1).sum() >= 150                       # admissible rows that hit it exactly exist, and are out
    rows = np.concatenate([[c["info"]["best"]], c["info"]["copies"][1:]])            # duplicates of one row, the excluded copy left out: id order
    np.testing.assert_array_equal(out[2][0, :len(rows)].cpu().numpy(), rows)


# ---- 3: crowds -----------------------------------------------------------------------------------------------------------------------------
def test_3_a_crowd_that_fits_is_dropped_in_the_re_rank(gpu, stores):
    s, outs = _case_run(gpu, stores, "crowd_fits")
    out, ref = outs[0]
    emitted, _ = s.idx.last_emitted(299)
    assert int(out[0][0]) == 40 and emitted[0] >= 1540                               # emitted, excluded ones included; count 40
    assert out[4]["exact"] == 0


def test_3_a_crowd_that_overflows_goes_to_the_exact_pass_with_the_query_tags(gpu, stores):
    s, outs = _case_run(gpu, stores, "crowd_overflows")
    out, ref = outs[0]
    assert int(out[0][299]) == 5 and int((out[2][299] >= 0).sum()) == 5 and out[4]["exact"] == 1


# ---- 4: truncation -------------------------------------------------------------------------------------------------------------------------
def test_4_the_slots_hold_admissible_rows_only(gpu, stores):
    s, outs = _case_run(gpu, stores, "truncation")
    out, ref = outs[0]
    c = s.c
    assert c["M"] == 16 and int(out[0][0]) == 300 and (out[2][0] >= 0).all()
    excluded = c["info"]["planted_in"][0][300:]
    assert len(excluded) == 200 and not np.isin(out[2][0].cpu().numpy(), excluded).any()
    plain = s.plain(c["q"], c["radius"], 16)
    assert int(plain[0][0]) == 500 and np.isin(plain[2][0].cpu().numpy(), excluded).all()   # unfiltered: the excluded rows fill every slot


# ---- 5: everything, all excluded -----------------------------------------------------------------------------------------------------------
def test_5_everything_counts_the_admissible_rows(gpu, stores):
    s, outs = _case_run(gpu, stores, "everything")
    out, ref = outs[0]
    adm = X.admissible(s.c)
    np.testing.assert_array_equal(out[0].cpu().numpy(), adm.sum(axis=1))
    assert out[4]["exact"] == 17 and (adm.sum(axis=1) < s.idx.ntotal).any()


def test_5_a_batch_set_that_names_every_tag(gpu, stores):
    s, outs = _case_run(gpu, stores, "all_excluded")
    out, ref = outs[0]
    assert int(out[0].abs().sum()) == 0 and int((out[2] != -1).sum()) == 0
    emitted, _ = s.idx.last_emitted(300)
    assert emitted.max() == 0                                                        # a NaN score passes no compare: nothing is emitted


# ---- 6: one set for the batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["graded_cosine_batch", "graded_l2_batch", "centred_batch", "graded_f16_batch", "crowd_overflows_batch"])
def test_6_one_set_for_the_batch(gpu, stores, name):
    if name == "centred_batch":
        s = stores(name)
        s.idx.search_device(_dev(s.c["q"], gpu), 1)
        assert s.idx.plane_info()["centred"], s.idx.plane_info()
    s, outs = _case_run(gpu, stores, name, nqs=(17, 300) if name != "crowd_overflows_batch" else None)
    out, ref = outs[-1]
    c = s.c
    emitted, _ = s.idx.last_emitted(300)
    plain = s.plain(c["q"], c["radius"], c["M"])
    assert int((plain[0] != out[0]).sum()) >= 75
    if name == "crowd_overflows_batch":
        assert emitted[0] < 100 and int(out[0][0]) < 40                              # query 0's crowd is in the set: never emitted
        assert int(out[0][299]) > R.BUFFER and out[4]["exact"] == 1


# ---- 7: the exact route's shapes, both modes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pq", "batch"])
@pytest.mark.parametrize("name", ["exact_nq3", "exact_dim36", "exact_small_store", "exact_plane_off"])
def test_7_exact_route(gpu, stores, name, mode):
    s, outs = _case_run(gpu, stores, name + ("_batch" if mode == "batch" else ""), **({"hi_plane": 0} if name == "exact_plane_off" else {}))
    c = s.c
    adm = X.admissible(c)
    ref2 = s.reference(c["q"], c["radius"], 2, adm)                                  # M = 2 cuts lists: the count stays exact
    out2 = s.run(c["q"], c["radius"], 2)
    _check(out2, ref2, s.metric, 2)
    assert ref2[0].max() > 2 and out2[4]["route"] == "exact"
    plain = s.plain(c["q"], c["radius"], c["M"])
    assert (plain[0].cpu().numpy() >= outs[0][1][0]).all() and int((plain[0] != outs[0][0][0]).sum()) > 0


# ---- 8: nothing excluded is the plain range search, bit for bit ----------------------------------------------------------------------------
def _same_bits(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3].view(torch.int64), b[3].view(torch.int64)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("name", ["graded_cosine", "graded_l2", "crowd_overflows", "exact_small_store"])
def test_8_nothing_excluded_equals_the_plain_range_search(gpu, stores, name):
    s = stores(name)
    c = s.c
    q, nq = c["q"], len(c["q"])
    plain = s.plain(q, c["radius"], c["M"])
    assert plain[0].sum() > 0
    m0 = s.run(q, c["radius"], c["M"], mode="pq", q_tags=None, q_cnt=None)            # m == 0: no tags at all
    assert _same_bits(m0, plain) and m0[4] == plain[4]
    zero = s.run(q, c["radius"], c["M"], mode="pq", q_tags=c["q_tags"], q_cnt=np.zeros(nq, np.int32))     # every count 0
    assert _same_bits(zero, plain) and zero[4] == plain[4]
    none = s.run(q, c["radius"], c["M"], mode="batch", excl=None)                    # n_excl == 0: NULL tag arrays
    assert _same_bits(none, plain) and none[4] == plain[4]
    absent = s.run(q, c["radius"], c["M"], mode="batch", excl=np.array([X.ABSENT - 1, X.ABSENT - 2][::-1], np.int64))   # tags no row carries
    assert _same_bits(absent, plain)


# ---- 9: early abandon on / off -------------------------------------------------------------------------------------------------------------
def test_9_abandon_on_and_off_agree_bit_for_bit(gpu, stores):
    on, off = stores("graded_dim128", abandon=1), stores("graded_dim128", abandon=0)
    c = on.c
    adm = X.admissible(c)
    ref = on.reference(c["q"], c["radius"], c["M"], adm)
    a = on.run(c["q"], c["radius"], c["M"])
    ab = on.idx.last_abandon()
    b = off.run(c["q"], c["radius"], c["M"])
    print(f"abandon on: {ab}; off: {off.idx.last_abandon()}")
    _check(a, ref, on.metric, c["M"])
    _expect_tile(on, a[4], len(c["q"]), c["radius"], 0)
    assert b[4]["route"] == "tile" and b[4]["exact"] == 0
    assert ab["tasks"] > 0 and off.idx.last_abandon()["tasks"] == 0                  # per-query sets: the plain range search's launch
    assert _same_bits(a, b)
    # one set for the batch: a per-call bias, so neither handle takes the ABANDON form (knn_abandon_launch) -- and they agree
    excl = X.batch_set(c["row_tags"])
    a2 = on.run(c["q"], c["radius"], c["M"], mode="batch", excl=excl)
    assert on.idx.last_abandon()["tasks"] == 0
    b2 = off.run(c["q"], c["radius"], c["M"], mode="batch", excl=excl)
    _check(a2, on.reference(c["q"], c["radius"], c["M"], X.admissible_batch(c["row_tags"], excl, len(c["q"]))), on.metric, c["M"])
    assert _same_bits(a2, b2) and a2[4] == b2[4] == {"queries": 300, "route": "tile", "exact": 0}


# ---- 10: ids and growth --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pq", "batch"])
def test_10_id_base_and_growth(gpu, mode):
    c = X.case("graded_cosine" + ("_batch" if mode == "batch" else ""))
    s = _Store(gpu, c, id_base=1000)
    q = c["q"][:17]
    adm = X.admissible(c)[:17]
    ref = s.reference(q, c["radius"], c["M"], adm)
    out = s.run(q, c["radius"], c["M"])
    _check(out, ref, s.metric, c["M"])
    _expect_tile(s, out[4], 17, c["radius"], 0)
    I = out[2].cpu().numpy()
    assert I[I >= 0].min() >= 1000                                                   # ids carry the base, tags are indexed without it
    # growth between calls: 300 copies of an admissible row of query 3 and 300 of an excluded one, with their tags
    rows = c["info"]["planted_in"][3]
    a_row = int(rows[adm[3, rows]][0])
    x_row = int(rows[~adm[3, rows]][0])
    s.idx.add_device(_dev(np.concatenate([np.repeat(s.stored[a_row:a_row + 1], 300, axis=0), np.repeat(s.stored[x_row:x_row + 1], 300, axis=0)]), gpu))
    grown_tags = np.concatenate([c["row_tags"], np.full(300, c["row_tags"][a_row]), np.full(300, c["row_tags"][x_row])])
    s.row_tags = _dev(grown_tags, gpu)
    s.refresh()
    adm2 = (X.admissible_batch(grown_tags, c["excl"], 17) if mode == "batch" else X.admissible_pq(grown_tags, c["q_tags"][:17], c["q_cnt"][:17]))
    out2 = s.run(q, c["radius"], c["M"])
    _check(out2, s.reference(q, c["radius"], c["M"], adm2), s.metric, c["M"])
    _expect_tile(s, out2[4], 17, c["radius"], 0)
    grown = (out2[0] - out[0]).cpu().numpy()
    assert grown[3] == 300 and grown.sum() == 300                                    # the admissible copies count, the excluded ones do not


# ---- 11: errors ----------------------------------------------------------------------------------------------------------------------------
def test_11_errors_leave_the_outputs_untouched_and_the_handle_usable(gpu, stores):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = stores("graded_cosine")
    c = s.c
    lib = s.idx._lib
    q = _dev(c["q"][:17], gpu)
    M = 8
    cnt = torch.full((17,), -7, dtype=torch.int32, device=gpu)
    D = torch.full((17, M), 123.0, dtype=torch.float32, device=gpu)
    I = torch.full((17, M), -7, dtype=torch.int64, device=gpu)
    st = _lib.stream_ptr(gpu)
    qt, qc = _dev(c["q_tags"][:17], gpu), _dev(c["q_cnt"][:17], gpu)
    excl = _dev(X.batch_set(c["row_tags"]), gpu)
    tags = s.row_tags.data_ptr()

    def pq(h=None, nq=17, radius=0.9, m=M, rt=tags, pt=qt.data_ptr(), n_tags=X.M_TAGS, pcnt=qc.data_ptr(), pc=cnt.data_ptr(), pd=D.data_ptr(),
           pi=I.data_ptr()):
        return lib.radad_knn_range_search_excl_pq(h if h is not None else s.idx._h, q.data_ptr(), _lib.Q_F32, nq, radius, m, rt, pt, n_tags, pcnt,
                                                  pc, pd, pi, None, st)

    def batch(h=None, nq=17, radius=0.9, m=M, rt=tags, pe=excl.data_ptr(), n_excl=excl.numel(), pc=cnt.data_ptr(), pd=D.data_ptr(),
              pi=I.data_ptr()):
        return lib.radad_knn_range_search_excl(h if h is not None else s.idx._h, q.data_ptr(), _lib.Q_F32, nq, radius, m, rt, pe, n_excl,
                                               pc, pd, pi, None, st)
    wide = _mk("L2", 16384)                                                          # 16384 * 4 + 96 * 1024 + 16 > 160 KB
    for call in (pq, batch):
        assert call(m=0) == _lib.RADAD_EINVAL and call(m=_lib.KNN_MAX_K + 1) == _lib.RADAD_EINVAL
        assert call(radius=float("nan")) == _lib.RADAD_EINVAL
        assert call(pc=None) == _lib.RADAD_EINVAL and call(pd=None) == _lib.RADAD_EINVAL and call(pi=None) == _lib.RADAD_EINVAL
        assert call(h=wide._h, m=1024) == _lib.RADAD_EINVAL
        assert call(h=wide._h, m=8, rt=None) == _lib.RADAD_EINVAL                    # (the tags are checked before the store)
        assert call(rt=None) == _lib.RADAD_EINVAL                                    # tags listed, no row tags
    assert pq(n_tags=-1) == _lib.RADAD_EINVAL and pq(n_tags=_lib.EXCL_PQ_MAX_TAGS + 1) == _lib.RADAD_EINVAL
    assert pq(pt=None) == _lib.RADAD_EINVAL
    assert batch(pe=None) == _lib.RADAD_EINVAL and batch(n_excl=-1) == _lib.RADAD_EINVAL
    assert pq(h=wide._h, m=8, rt=None, pt=None, n_tags=0) == _lib.RADAD_ESTATE        # an empty store
    assert batch(h=wide._h, m=8, rt=None, pe=None, n_excl=0) == _lib.RADAD_ESTATE
    s.idx.search_begin(q, 5)
    assert pq() == _lib.RADAD_EINVAL and batch() == _lib.RADAD_EINVAL                # a begun search
    s.idx.search_abort()
    assert pq(nq=0) == _lib.RADAD_OK and batch(nq=0) == _lib.RADAD_OK
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (D == 123.0).all() and (I == -7).all()
    adm = X.admissible(c)[:17]
    assert pq() == _lib.RADAD_OK                                                     # the handle is usable
    ref = s.reference(c["q"][:17], 0.9, M, adm)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])
    assert pq(pcnt=None) == _lib.RADAD_OK                                            # NULL counts: all four slots live
    ref = s.reference(c["q"][:17], 0.9, M, X.admissible_pq(c["row_tags"], c["q_tags"][:17], None))
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])
    assert batch() == _lib.RADAD_OK
    ref = s.reference(c["q"][:17], 0.9, M, X.admissible_batch(c["row_tags"], excl.cpu().numpy(), 17))
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])


# ---- 12: state -----------------------------------------------------------------------------------------------------------------------------
def test_12_the_calls_leave_the_handle_state_alone(gpu):
    import torch
    s = _Store(gpu, X.case("crowd_overflows"))
    c = s.c
    qt = _dev(c["q"], gpu)
    s.idx.search_device(qt, 10, return_f64=True)
    torch.cuda.synchronize()
    D0, I0, K0 = s.idx.search_device(qt, 10, return_f64=True)                        # (consumes the first search's report)
    torch.cuda.synchronize()
    before, cert = s.idx.tuning_info(), s.idx.last_launch()
    assert cert["scan_kind"] == "hi_tile" and cert["certificate"]["queries"] == len(c["q"])
    a = s.run(c["q"], c["radius"], c["M"])                                           # one query overflows
    b = s.run(c["q"], c["radius"], c["M"], mode="batch", excl=X.case("crowd_overflows_batch")["excl"])
    e = s.run(c["q"][:17], -np.inf, c["M"], sel=np.arange(17))                       # everything: all 17 in the exact pass
    torch.cuda.synchronize()
    assert a[4]["exact"] == 1 and b[4]["exact"] == 1 and e[4]["exact"] == 17
    assert s.idx.tuning_info() == before
    after = s.idx.last_launch()
    assert after["certificate"] == cert["certificate"] and after["rechecked_queries"] == cert["rechecked_queries"]
    assert s.idx.last_excl_scan()["queries"] == 0
    D1, I1, K1 = s.idx.search_device(qt, 10, return_f64=True)
    assert torch.equal(I0, I1) and torch.equal(D0.view(torch.int32), D1.view(torch.int32)) and torch.equal(K0.view(torch.int64), K1.view(torch.int64))
    # last_range describes whichever range call ran last
    p = s.plain(c["q"][:17], c["radius"], c["M"])
    assert p[4] == {"queries": 17, "route": "tile", "exact": 0}
    assert s.run(c["q"][:3], c["radius"], c["M"], sel=np.arange(3))[4] == {"queries": 3, "route": "exact", "exact": 3}


# ---- 13: the Python surface ----------------------------------------------------------------------------------------------------------------
def _config(gpu, tmp_path, index_type, dim=64):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as Rad
    cfg = Rad.Config()
    cfg.update(device=gpu, feature_dim=dim, tpp_levels=[1], top_k=5, vector_db_index_type=index_type,
               vector_db_path=str(tmp_path / ("vdb_" + index_type)))
    return Rad, cfg


def test_13_vector_database_wrappers(gpu, tmp_path):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    Rad, cfg = _config(gpu, tmp_path, "IP")                                          # normalize_for_ip: cosine
    c = R.case("graded_cosine")
    n = len(c["db"])
    paths = [f"/train/f{i}.wav" for i in range(n)]
    for j in range(40):                                                              # every second near-copy of query j is a file named clip<j>.wav
        for r in c["info"]["planted_in"][j][0::2]:
            paths[int(r)] = f"/train/v{int(r)}/clip{j}.wav"
    vdb = Rad.VectorDatabase(cfg)
    vdb.add_vectors(c["db"], paths, [i % 2 for i in range(n)], {})
    q = c["q"][:40]
    want = np.array([R.COUNTS[j % 4] - len(c["info"]["planted_in"][j][0::2]) for j in range(40)], np.int32)
    q_tags = [[path_tag(f"/eval/clip{j}.wav")] for j in range(40)]
    lims, D, I, counts = vdb.range_search_excluding_per_query_batch(q, 0.9, query_tags=q_tags, max_per_query=64, return_counts=True)
    assert isinstance(lims, np.ndarray) and lims.dtype == np.int64 and lims.shape == (41,) and counts.dtype == np.int32
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(np.diff(lims), want)
    assert len(D) == len(I) == lims[-1] and D.dtype == np.float32 and I.dtype == np.int64
    for j in (1, 2, 3):
        np.testing.assert_array_equal(np.sort(I[lims[j]:lims[j + 1]]), np.sort(c["info"]["planted_in"][j][1::2]))
        assert (np.diff(D[lims[j]:lims[j + 1]]) <= 0).all() and (D[lims[j]:lims[j + 1]] > 0.9).all()      # best first
    assert vdb.index.last_range() == {"queries": 40, "route": "tile", "exact": 0}
    assert len(vdb.range_search_excluding_per_query_batch(q, 0.9, query_tags=q_tags)) == 3
    # one set for the batch: the files of queries 1, 2, 3
    excl = [path_tag(f"clip{j}.wav") for j in (1, 2, 3)]
    lims_b, D_b, I_b, counts_b = vdb.range_search_excluding_batch(_dev(q, gpu), 0.9, exclude_tags=excl, return_counts=True)
    assert all(t.is_cuda for t in (lims_b, D_b, I_b, counts_b))
    plain = vdb.range_search_batch(q, 0.9, return_counts=True)
    want_b = plain[3].copy()
    want_b[1:4] = want[1:4]
    np.testing.assert_array_equal(counts_b.cpu().numpy(), want_b)
    # nothing excluded: the plain result
    same = vdb.range_search_excluding_batch(q, 0.9, return_counts=True)
    for a, b in zip(same, plain):
        np.testing.assert_array_equal(a, b)
    same = vdb.range_search_excluding_per_query_batch(q, 0.9, return_counts=True)
    for a, b in zip(same, plain):
        np.testing.assert_array_equal(a, b)
    # a column of the caller's own instead of the basename tags
    col = torch.arange(n, dtype=torch.int64, device=gpu)
    l3, d3, i3, c3 = vdb.range_search_excluding_per_query_batch(q[3], 0.9, query_tags=[[int(c["info"]["planted_in"][3][0])]], return_counts=True,
                                                                row_tags=col)
    assert c3.tolist() == [39] and int(c["info"]["planted_in"][3][0]) not in i3.tolist()
    # an empty store
    empty = Rad.VectorDatabase(cfg)
    empty.create_index(64)
    le, de, ie, ce = empty.range_search_excluding_per_query_batch(q, 0.9, query_tags=q_tags, return_counts=True)
    assert le.tolist() == [0] * 41 and len(de) == len(ie) == 0 and ce.tolist() == [0] * 40
    assert len(empty.range_search_excluding_batch(q, 0.9, exclude_tags=excl)) == 3


def test_13_ivf_and_sharded_refuse(gpu, tmp_path):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipIVFFlatIndex
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ReplicatedSearch, ShardedSearch
    Rad, cfg = _config(gpu, tmp_path, "IVF")
    ivf = HipIVFFlatIndex(64, 64)
    for call in (ivf.range_search_excluding, ivf.range_search_excluding_per_query):
        with pytest.raises(ValueError, match="flat store"):
            call(np.zeros((1, 64), np.float32), 0.5, None, None)
    vdb = Rad.VectorDatabase(cfg)
    vdb.create_index(64)
    for call in (vdb.range_search_excluding_batch, vdb.range_search_excluding_per_query_batch):
        with pytest.raises(ValueError, match="flat"):
            call(np.zeros((1, 64), np.float32), 0.5)
    for call in (ShardedSearch(None, 0).range_search_excluding, ShardedSearch(None, 0).range_search_excluding_per_query):
        with pytest.raises(ValueError, match="no sharded form.*concatenating"):
            call(None, 0.5)
    for call in (ReplicatedSearch(None).range_search_excluding, ReplicatedSearch(None).range_search_excluding_per_query):
        with pytest.raises(ValueError, match="no replicated form"):
            call(None, 0.5)


def test_13_near_duplicates_with_more_stored_copies_than_slots(gpu, tmp_path):
    """One file has more stored copies (segments) than max_per_query: filtering after the search loses a renamed copy of ANOTHER
    file, the exclusion inside the search returns it, with the exact count."""
    Rad, cfg = _config(gpu, tmp_path, "IP")

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")
    pipe = Rad.HotPathPipeline(cfg, feature_extractor=NoExtractor())
    c = R.case("graded_cosine")
    n = len(c["db"])
    paths = [f"/train/f{i}.wav" for i in range(n)]
    speakers = [f"spk{i % 50}" for i in range(n)]
    rows = c["info"]["planted_in"][3]                                                # query 3: 40 near-copies, levels cycle 0.99, 0.95, 0.92, 0.905
    keys = R.keys(c["db"][rows], c["q"][3:4], "COSINE")[0]
    order = rows[np.argsort(-keys)]
    for r in order[:12]:                                                             # the 12 best are stored copies of the query's own file
        paths[int(r)] = f"/train/seg{int(r)}/clip3.wav"
        speakers[int(r)] = "alice"
    renamed = int(order[12])                                                         # the 13th is the same audio under another name, another speaker's
    paths[renamed] = "/train/renamed_copy.wav"
    speakers[renamed] = "bob"
    labels = [i % 2 for i in range(n)]
    pipe.vector_db.add_vectors(c["db"], paths, labels, {"speaker_id": speakers})
    q = c["q"][:20]
    query_paths = [f"/eval/clip{j}.wav" for j in range(20)]
    M = 8
    default = pipe.near_duplicates(q, 0.9, max_per_query=M, query_paths=query_paths)
    assert isinstance(default, list) and default[3] == []                            # all 8 slots went to the file's own copies: nothing is left
    hits, counts = pipe.near_duplicates(q, 0.9, max_per_query=M, query_paths=query_paths, exact_exclusion=True)
    assert counts[3] == 28 and len(hits[3]) == M                                     # 40 within the radius, 12 of them the file itself
    assert hits[3][0][0] == "/train/renamed_copy.wav" and hits[3][0][1] == labels[renamed] and hits[3][0][2] > 0.9
    assert all("clip3.wav" not in h[0] for h in hits[3])
    assert [h[2] for h in hits[3]] == sorted((h[2] for h in hits[3]), reverse=True)
    np.testing.assert_array_equal(np.delete(counts, 3), np.delete([R.COUNTS[j % 4] for j in range(20)], 3))
    # leave-one-speaker-out: the same rows are alice's
    query_speakers = ["alice" if j == 3 else f"nobody{j}" for j in range(20)]
    hits_s, counts_s = pipe.near_duplicates(_dev(q, gpu), 0.9, max_per_query=M, exact_exclusion=True, exclude="speaker",
                                            query_speakers=query_speakers)
    assert counts_s[3] == 28 and hits_s[3][0][0] == "/train/renamed_copy.wav" and [h[0] for h in hits_s[3]] == [h[0] for h in hits[3]]
    with pytest.raises(ValueError):
        pipe.near_duplicates(q, 0.9, exact_exclusion=True)                           # no query_paths
    with pytest.raises(ValueError):
        pipe.near_duplicates(q, 0.9, exclude="label")
