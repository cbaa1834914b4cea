"""A vetoed tile's few live rows deferred to a dense tail (csrc/knn_hi.inc, k_knn_hi_abandon_defer / k_knn_hi_tail;
RADAD_KNN_OPT_ABANDON_DEFER).  Where a candidate's row is multiplied must change nothing at all.

Every case checks
  * ids == the float64 oracle over the rows as stored (cosine: the stored, normalised rows against radad_rownorm of the query), and
  * EVERYTHING array_equal to the same search on the same handle with the option off and the abandon on: ids, distances, float64 keys,
    radad_knn_last_emitted's counts and floors, the certificate's six statistics, and last_launch()["early_abandon"],
and then what the case is about: how many tile tasks were deferred and how many rows they listed.

Shapes: tests/test_gpu_knn_abandon.py's -- 20 000 rows (78 tiles and a partial one; the sample's tiles are 0, 9, ..., 63), random rows,
queries within cos 0.998 of each other, P near-duplicates planted at t 256 + 3 + 15 i, i < P, in every third tile t (26 tiles; the
sample then holds >= 16 of them for P >= 2, so the floor clears every random row).  On the host, with P = 8 and 16 at dims 128 and
512, the per-row rule leaves exactly the P planted rows live in every planted tile task and none elsewhere: the counts below are
asserted as equalities."""
import numpy as np
import pytest

from conftest import c_knn

pytestmark = pytest.mark.gpu

N0 = 20000
K = 10
MAX_ROWS = 16          # KNN_DEFER_MAX_ROWS
NONE = {"tile_tasks_deferred": 0, "rows_listed": 0, "tail_launches": 0}


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


def _planted(n, dim, nq, seed, per_tile):
    """(rows, queries, planted ids).  per_tile: {tile: P} or a function tile -> P; the rows of tile t are t 256 + 3 + 15 i, i < P"""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    ids = np.array([t * 256 + 3 + 15 * i for t, p in sorted(per_tile.items()) for i in range(p)], np.int64)
    assert len(ids) == 0 or ids.max() < n
    db[ids] = q[np.arange(len(ids)) % nq] + (0.03 * amp * rng.standard_normal((len(ids), dim))).astype(np.float32)
    return db, q, ids


def _every_third(p, n=N0):
    return {t: p for t in range(0, n // 256, 3)}


class _Index:
    """one handle; search() runs the batch with the option off and on (the abandon on both times) and returns the second observation"""

    def __init__(self, gpu, knn_oracle_lib, metric, rows, **kw):
        import torch
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
        self.gpu, self.lib, self.metric = gpu, knn_oracle_lib, metric
        self.idx = HipFlatIndex(rows.shape[1], {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric], 0, **kw)
        self.idx.add_device(_dev(rows, gpu))
        n = self.idx.ntotal
        self.stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(r0, min(n, r0 + 65536), device=gpu)).cpu().numpy()
                                      for r0 in range(0, n, 65536)])

    def observe(self, qt, begun=False):
        nq = qt.shape[0]
        if begun:
            self.idx.search_begin(qt, K)
            D, I, K64 = self.idx.search_finish(None, return_f64=True)
        else:
            D, I, K64 = self.idx.search_device(qt, K, return_f64=True)
        launch = self.idx.last_launch()
        counts, floors = self.idx.last_emitted(nq)
        return {"D": D.cpu().numpy(), "I": I.cpu().numpy(), "K64": K64.cpu().numpy(), "counts": counts, "floors": floors,
                "certificate": launch["certificate"], "abandon": launch["early_abandon"], "defer": launch["abandon_defer"], "launch": launch}

    def search(self, q, begun=False, oracle_rows=None):
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        self.idx.set_abandon(1)
        self.idx.set_abandon_defer(0)
        off = self.observe(qt, begun)
        self.idx.set_abandon_defer(1)
        on = self.observe(qt, begun)
        print(f"{self.metric} n={len(self.stored)} d={self.stored.shape[1]} nq={len(q)}: defer {on['defer']}, abandon {on['abandon']}, "
              f"launches {on['launch']['scan_launches']}, emitted mean {on['counts'].mean():.1f}, floors min {np.nanmin(on['floors']):.4f}")
        assert on["launch"]["scan_kind"] == "hi_tile", on["launch"]
        assert off["defer"] == NONE, off["defer"]
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(on[name], off[name], equal_nan=name in ("D", "K64", "floors")), f"{name} differs from the search with the option off"
        assert on["certificate"] == off["certificate"], (on["certificate"], off["certificate"])
        assert on["abandon"] == off["abandon"], (on["abandon"], off["abandon"])
        for name in ("query_tiles", "db_splits", "block_threads", "scan_launches", "scan_phases"):
            assert on["launch"][name] == off["launch"][name], name
        qo = _rownorm(self.gpu, q) if self.metric == "COSINE" else np.asarray(q, np.float32)
        fin = np.isfinite(qo).all(axis=1) if oracle_rows is None else oracle_rows
        _, oi = c_knn(self.lib, self.stored, qo[fin], K, "L2" if self.metric == "L2" else "IP")
        assert np.array_equal(on["I"][fin], oi), "ids differ from the float64 oracle"
        return on


def _qtiles(nq):
    return (nq + 255) // 256


@pytest.mark.parametrize("dim", [128, 512])
@pytest.mark.parametrize("p", [8, 16])
@pytest.mark.parametrize("nq", [17, 256, 300])
def test_deferred_tiles(gpu, knn_oracle_lib, dim, p, nq):
    db, q, _ = _planted(N0, dim, nq, 11 + dim + nq + p, _every_third(p))
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    ab, df = on["abandon"], on["defer"]
    assert ab["checked"] == ab["tasks"] and ab["checked"] - ab["skipped"] == 26 * _qtiles(nq), ab
    assert df["tile_tasks_deferred"] == 26 * _qtiles(nq) and df["rows_listed"] == 26 * p * _qtiles(nq) and df["tail_launches"] >= 1, df


def test_too_many_live_rows(gpu, knn_oracle_lib):
    db, q, _ = _planted(N0, 128, 300, 21, _every_third(MAX_ROWS + 1))
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["defer"]["tile_tasks_deferred"] == 0 and on["defer"]["rows_listed"] == 0, on["defer"]
    assert on["abandon"]["checked"] - on["abandon"]["skipped"] == 26 * 2, on["abandon"]


def test_mixed(gpu, knn_oracle_lib):
    """tiles of 3 and tiles of 17 planted rows in one store: only the former are deferred"""
    per_tile = {t: (3 if (t // 3) % 2 == 0 else MAX_ROWS + 1) for t in range(0, N0 // 256, 3)}
    few = sum(1 for v in per_tile.values() if v == 3)
    db, q, _ = _planted(N0, 128, 300, 23, per_tile)
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["defer"]["tile_tasks_deferred"] == few * 2 and on["defer"]["rows_listed"] == 3 * few * 2, (on["defer"], few)


def test_partial_last_tile(gpu, knn_oracle_lib):
    """planted rows in the store's last, partly filled tile, its last row among them: found, and no row >= n is listed (the tail would
    score it: the counts and the candidates would differ)"""
    dim, nq = 128, 40
    db, q, _ = _planted(N0, dim, nq, 31, _every_third(4))
    last_tile = N0 // 256
    assert N0 % 256 == 32
    rng = np.random.default_rng(5)
    amp = np.linalg.norm(q[0]) / np.sqrt(dim)
    for j, row in enumerate((last_tile * 256 + 5, N0 - 1)):
        db[row] = q[j] + (0.002 * amp * rng.standard_normal(dim)).astype(np.float32)
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["I"][0, 0] == last_tile * 256 + 5 and on["I"][1, 0] == N0 - 1, on["I"][:2]
    assert on["defer"]["tile_tasks_deferred"] == 27 and on["defer"]["rows_listed"] == 26 * 4 + 2, on["defer"]


def test_two_phases(gpu, knn_oracle_lib):
    """(tests/test_gpu_knn_abandon.py::test_two_phases' store.)  Two scan launches, each followed by its tail; the floors after phase 0
    come from candidates the first tail emitted -- they equal the option-off run's (search() compares the final floors and counts)"""
    n, dim, nq = 400000, 128, 300
    db, q, ids = _planted(n, dim, nq, 5, {t: 1 for t in range(0, n // 256, 6)})
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["launch"]["scan_launches"] == 2 and on["defer"]["tail_launches"] == 2, (on["launch"], on["defer"])
    assert on["defer"]["tile_tasks_deferred"] == len(ids) * 2 and on["defer"]["rows_listed"] == len(ids) * 2, on["defer"]


@pytest.mark.parametrize("dim", [128, 512])
@pytest.mark.parametrize("metric,kw", [("L2", {}), ("COSINE", {"store_f16": True})])
def test_l2_and_an_fp16_store(gpu, knn_oracle_lib, metric, kw, dim):
    db, q, _ = _planted(N0, dim, 300, 41 + dim, _every_third(8))
    s = _Index(gpu, knn_oracle_lib, metric, db, **kw)
    on = s.search(q)
    if metric == "L2":
        assert s.idx.plane_info()["one_scale"]          # RSC 3: the bias variant with one scale
    ab, df = on["abandon"], on["defer"]
    assert df["tile_tasks_deferred"] <= ab["checked"] - ab["skipped"] and df["rows_listed"] <= MAX_ROWS * df["tile_tasks_deferred"], (ab, df)
    # (raw L2 rows of dim 512: the tile-side gate stays shut for nearly every tile -- |y|^2 dominates the score -- and nothing is tested)
    if ab["checked"] == ab["tasks"]:
        assert df["tile_tasks_deferred"] == 26 * 2 and df["rows_listed"] == 26 * 8 * 2, (ab, df)


@pytest.mark.parametrize("dim", [128, 512])
def test_gate_shut(gpu, knn_oracle_lib, dim):
    rng = np.random.default_rng(3 + dim)
    db, q = rng.standard_normal((N0, dim)).astype(np.float32), rng.standard_normal((300, dim)).astype(np.float32)
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["abandon"]["tasks"] > 0 and on["abandon"]["checked"] == 0, on["abandon"]
    assert on["defer"]["tile_tasks_deferred"] == 0 and on["defer"]["rows_listed"] == 0, on["defer"]


def test_a_nan_query_row_and_a_floor_of_minus_infinity(gpu, knn_oracle_lib):
    """a NaN query (its floor is NaN) and an all-zero query in the SECOND query tile: nothing is deferred for that query tile; the first
    defers as ever"""
    dim, nq = 128, 300
    db, q, _ = _planted(N0, dim, nq, 51, _every_third(8))
    q[260] = 0.0
    q[270, 5] = np.nan
    ordinary = np.ones(nq, bool)
    ordinary[[260, 270]] = False
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q, oracle_rows=ordinary)
    assert on["defer"]["tile_tasks_deferred"] == 26 and on["defer"]["rows_listed"] == 26 * 8, on["defer"]


def test_search_begin_and_finish(gpu, knn_oracle_lib):
    db, q, _ = _planted(N0, 512, 40, 61, _every_third(8))
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q, begun=True)
    assert on["defer"]["tile_tasks_deferred"] == 26 and on["defer"]["rows_listed"] == 26 * 8, on["defer"]


def test_range_search(gpu, knn_oracle_lib):
    """every query's radius holds the planted rows and nothing else (cos > 0.9): one launch from the caller's floors, then its tail"""
    dim, nq, m, thr = 128, 40, 512, 0.9
    db, q, ids = _planted(N0, dim, nq, 71, _every_third(8))
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    qt = _dev(q, gpu)
    keys = s.stored.astype(np.float64) @ _rownorm(gpu, q).astype(np.float64).T
    assert np.abs(keys - thr).min() > 1e-3
    want = (keys > thr).sum(axis=0)
    assert want.min() == len(ids) and want.max() <= m
    out = {}
    for defer in (0, 1):
        s.idx.set_abandon_defer(defer)
        counts, D, I, K64 = s.idx.range_search_device(qt, thr, m, return_f64=True)
        out[defer] = (counts.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy(), K64.cpu().numpy(), s.idx.last_emitted(nq),
                      s.idx.last_abandon(), s.idx.last_range(), s.idx.last_abandon_defer())
    off, on = out[0], out[1]
    print(f"range: defer {on[7]}, abandon {on[5]}, route {on[6]}")
    assert on[6]["route"] == "tile" and on[6] == off[6], (on[6], off[6])
    for a, b in zip(on[:4], off[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(on[4][0], off[4][0]) and np.array_equal(on[4][1], off[4][1])
    assert np.array_equal(on[0], want)
    assert on[5] == off[5] and off[7] == NONE, (on[5], off[5], off[7])
    assert on[7]["tile_tasks_deferred"] == 26 and on[7]["rows_listed"] == 26 * 8 and on[7]["tail_launches"] == 1, on[7]


def test_floors_of_minus_infinity(gpu, knn_oracle_lib):
    """a range search with the radius -inf: every query's floor is -inf, every row is within it.  Nothing is deferred (no comparison
    against -inf is true: every row would be live), the results are equal"""
    dim, nq, m = 128, 40, 16
    db, q, _ = _planted(N0, dim, nq, 91, _every_third(8))
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    qt = _dev(q, gpu)
    out = {}
    for defer in (0, 1):
        s.idx.set_abandon_defer(defer)
        counts, D, I, K64 = s.idx.range_search_device(qt, -np.inf, m, return_f64=True)
        out[defer] = (counts.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy(), K64.cpu().numpy(), s.idx.last_abandon(), s.idx.last_abandon_defer())
    off, on = out[0], out[1]
    print(f"range -inf: defer {on[5]}, abandon {on[4]}")
    for a, b in zip(on[:4], off[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    assert (on[0] == N0).all() and on[4] == off[4]
    assert on[5]["tile_tasks_deferred"] == 0 and on[5]["rows_listed"] == 0, on[5]


def test_determinism(gpu, knn_oracle_lib):
    db, q, _ = _planted(N0, 128, 300, 81, _every_third(8))
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    first = s.search(q)
    qt = _dev(q, gpu)
    for _ in range(4):
        again = s.observe(qt)
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(again[name], first[name]), name
        assert again["defer"] == first["defer"] and again["abandon"] == first["abandon"] and again["certificate"] == first["certificate"]
