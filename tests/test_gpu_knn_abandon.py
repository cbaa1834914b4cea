"""Early abandon in the certified tile scan (csrc/knn_hi.inc, ABANDON; RADAD_KNN_OPT_ABANDON): a 256 x 256 tile is left after its
first K stages when no score of it can still reach its query's admission floor.  Results must not change at all.

Every case checks
  * ids == the float64 oracle over the rows as stored (under cosine: the stored, normalised rows against the device's radad_rownorm of
    the query -- as tests/test_gpu_knn_widths.py does), and
  * EVERYTHING array_equal to the same search on the same handle with the abandon switched off: ids, distances, float64 keys,
    radad_knn_last_emitted's counts and floors, the certificate's six statistics,
and then what the case is about: tiles were skipped, or none was even tested (the gate), or a particular row was found.

Shapes: the smallest the planner gives the tile scan -- 20 000 rows (78 tiles and a partial one; the sample pre-pass takes tiles 0, 9,
..., 63), dims 128 (checkpoint after 1 of 2 stages) and 512 (1 of 8), 17 / 256 / 300 queries (300: a second, partly filled query
tile) -- and one 400 000 x 128 store whose scan takes two phases.  The "benchmark in miniature": random rows, queries within cos
0.998 of each other, and near-duplicates of the queries planted 8 to a tile in every third tile (the sample's tiles among them): the
floor clears all random rows, two thirds of the tiles hold no planted row."""
import numpy as np
import pytest

from conftest import c_knn

pytestmark = pytest.mark.gpu

N0 = 20000
K = 10


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


def _checkpoint(dim):
    return max(1, dim // 64 // 8)


def _bench_like(n, dim, nq, seed, late=False, per_tile=8, every=3):
    """(rows, queries, ids of the planted rows: per_tile in every `every`-th tile).  late: the queries' energy sits behind the checkpoint (first 64 c elements x 0.02)"""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    if late:
        q[:, :64 * _checkpoint(dim)] *= np.float32(0.02)
    ids = np.array([t * 256 + 16 * i + 3 for t in range(0, n // 256, every) for i in range(per_tile)], np.int64)
    db[ids] = q[np.arange(len(ids)) % nq] + (0.03 * amp * rng.standard_normal((len(ids), dim))).astype(np.float32)
    return db, q, ids


class _Index:
    """one handle; search() runs the batch with the abandon on and off and returns both observations"""

    def __init__(self, gpu, knn_oracle_lib, metric, dim, **kw):
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
        self.gpu, self.lib, self.metric = gpu, knn_oracle_lib, metric
        self.idx = HipFlatIndex(dim, {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric], 0, **kw)

    def add(self, rows):
        self.idx.add_device(_dev(rows, self.gpu))

    def stored(self):
        import torch
        n = self.idx.ntotal
        return np.concatenate([self.idx.reconstruct_batch(torch.arange(r0, min(n, r0 + 65536), device=self.gpu)).cpu().numpy()
                               for r0 in range(0, n, 65536)])

    def observe(self, qt, k, begun=False):
        nq = qt.shape[0]
        if begun:
            self.idx.search_begin(qt, k)
            D, I, K64 = self.idx.search_finish(None, return_f64=True)
        else:
            D, I, K64 = self.idx.search_device(qt, k, return_f64=True)
        launch = self.idx.last_launch()
        counts, floors = self.idx.last_emitted(nq)
        return {"D": D.cpu().numpy(), "I": I.cpu().numpy(), "K64": K64.cpu().numpy(), "counts": counts, "floors": floors,
                "certificate": launch["certificate"], "abandon": launch["early_abandon"], "launch": launch}

    def search(self, q, k=K, begun=False, oracle_rows=None):
        """-> the observation with the abandon on, after the two checks every case makes"""
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        self.idx.set_abandon(0)
        off = self.observe(qt, k, begun)
        self.idx.set_abandon(1)
        on = self.observe(qt, k, begun)
        assert on["launch"]["scan_kind"] == "hi_tile", on["launch"]
        assert off["abandon"] == {"checked": 0, "skipped": 0, "tasks": 0}, off["abandon"]
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(on[name], off[name], equal_nan=name in ("D", "K64", "floors")), f"{name} differs from the search without the abandon"
        assert on["certificate"] == off["certificate"], (on["certificate"], off["certificate"])
        rows = self.stored()
        qo = _rownorm(self.gpu, q) if self.metric == "COSINE" else np.asarray(q, np.float32)
        fin = np.isfinite(qo).all(axis=1) if oracle_rows is None else oracle_rows
        _, oi = c_knn(self.lib, rows, qo[fin], k, "L2" if self.metric == "L2" else "IP")
        assert np.array_equal(on["I"][fin], oi), "ids differ from the float64 oracle"
        print(f"{self.metric} n={len(rows)} d={rows.shape[1]} nq={len(q)}: abandon {on['abandon']}, floors min {np.nanmin(on['floors']):.4f}, "
              f"emitted mean {on['counts'].mean():.1f}, launches {on['launch']['scan_launches']}")
        return on


@pytest.mark.parametrize("dim", [128, 512])
@pytest.mark.parametrize("nq", [17, 256, 300])
def test_the_benchmark_in_miniature_skips_tiles(gpu, knn_oracle_lib, dim, nq):
    db, q, _ = _bench_like(N0, dim, nq, 11 + dim + nq)
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    ab = s.search(q)["abandon"]
    assert ab["tasks"] == ((N0 + 255) // 256) * ((nq + 255) // 256)
    assert ab["skipped"] > 0 and ab["skipped"] <= ab["checked"] <= ab["tasks"], ab
    # two thirds of the tiles hold no planted row: most of those must go (a partly filled query tile -- nq = 300 -- included)
    assert ab["skipped"] >= ab["tasks"] // 3, ab
    # ... and the veto path: every tile is tested (flat query energy: the gate is open everywhere), and exactly the 26 row tiles that hold
    # planted rows -- candidates whose partial score at the checkpoint is still far below the floor -- survive the test
    assert ab["checked"] == ab["tasks"] and ab["checked"] - ab["skipped"] == 26 * ((nq + 255) // 256), ab


def test_two_phases(gpu, knn_oracle_lib):
    # (400 000 rows: the smallest round number the planner scans in two launches at k = 10 -- 16 n > a third of the candidate buffer x
    # the 16 384 sample rows; the sample's tiles are 0, 24, 48, ...: planted ones.  261 planted rows: every one of them is a candidate
    # of every query, the buffer holds 1024 and the re-rank takes 512)
    n, dim, nq = 400000, 128, 300
    db, q, _ = _bench_like(n, dim, nq, 5, per_tile=1, every=6)
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    on = s.search(q)
    assert on["launch"]["scan_launches"] == 2, on["launch"]
    assert on["abandon"]["tasks"] == ((n + 255) // 256) * 2 and on["abandon"]["skipped"] >= on["abandon"]["tasks"] // 3, on["abandon"]


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim", [128, 512])
def test_random_rows_and_queries_are_never_tested(gpu, knn_oracle_lib, metric, dim):
    """the gate: on unstructured queries no tile runs the test"""
    rng = np.random.default_rng(3 + dim)
    db, q = rng.standard_normal((N0, dim)).astype(np.float32), rng.standard_normal((300, dim)).astype(np.float32)
    s = _Index(gpu, knn_oracle_lib, metric, dim)
    s.add(db)
    ab = s.search(q)["abandon"]
    assert ab["tasks"] > 0 and ab["checked"] == 0 and ab["skipped"] == 0, ab


@pytest.mark.parametrize("dim", [128, 512])
def test_late_energy_row_is_found(gpu, knn_oracle_lib, dim):
    """in an otherwise skippable tile, one row whose first 64 c elements OPPOSE the query (its partial score at the checkpoint is
    negative) and whose remainder makes it one of the query's k nearest.  Such a row shuts the TILE-side gate (its suffix norm alone
    reaches the floor: full score <= partial + RQ RY), so its tile is not even tested; the veto of a TESTED tile
    is what test_the_benchmark_in_miniature_skips_tiles counts on the planted tiles"""
    nq = 40
    db, q, _ = _bench_like(N0, dim, nq, 23 + dim, late=True)
    c = 64 * _checkpoint(dim)
    special = 256 * 4 + 77                         # tile 4: no planted row, not a sample tile
    row = q[0].copy()
    row[:c] = -row[:c]
    db[special] = row
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    on = s.search(q)
    assert special in on["I"][0], on["I"][0]
    assert on["abandon"]["skipped"] > 0, on["abandon"]


def test_rows_at_the_floor_in_an_appended_partial_tile_and_a_snapshot(gpu, knn_oracle_lib, tmp_path):
    """rows whose score sits just below and just above a query's admission floor (read back from a first search), appended after the
    plane exists into the store's last, partial tile (the row count stays off a multiple of 256, the sample's tiles stay the same, so
    the floor stays where it was read); a true neighbour planted there too; then the same through a save / load round trip"""
    dim, nq = 128, 40
    db, q, _ = _bench_like(N0, dim, nq, 31)
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    first = s.search(q)
    qn = _rownorm(gpu, q).astype(np.float64)
    rng = np.random.default_rng(7)
    extra = []
    for j in (0, 5):                               # scores floor (1 + i 2^-23) and floor (1 + i 2^-12): a few ulp of fp32, a few of f16
        for rel in [i * 2.0 ** -23 for i in range(-3, 4)] + [i * 2.0 ** -12 for i in range(-4, 5)]:
            t = float(first["floors"][j]) * (1.0 + rel)
            r = rng.standard_normal(dim)
            r -= (r @ qn[j]) * qn[j]
            extra.append(t * qn[j] + np.sqrt(max(0.0, 1.0 - t * t)) * r / np.linalg.norm(r))
    extra.append(qn[7] + 1e-3 * rng.standard_normal(dim))          # the best neighbour of query 7
    extra = np.asarray(extra, np.float32)
    assert (N0 + len(extra)) // 256 == N0 // 256 and (N0 + len(extra)) % 256 != 0
    s.add(extra)
    on = s.search(q)
    assert np.array_equal(on["floors"], first["floors"])
    assert on["I"][7, 0] == N0 + len(extra) - 1
    assert on["abandon"]["skipped"] > 0, on["abandon"]
    path = str(tmp_path / "store.knn")
    s.idx.save(path)
    s2 = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s2.idx.load(path)
    on2 = s2.search(q)
    for name in ("I", "D", "K64", "counts", "floors"):
        assert np.array_equal(on2[name], on[name]), name
    assert on2["abandon"] == on["abandon"], (on2["abandon"], on["abandon"])


def test_zero_nan_and_inf_queries(gpu, knn_oracle_lib):
    dim, nq = 128, 40
    db, q, _ = _bench_like(N0, dim, nq, 41)
    q[3] = 0.0
    q[9, 5] = np.nan
    q[9, 70] = np.inf
    ordinary = np.ones(nq, bool)
    ordinary[[3, 9]] = False
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    s.search(q, oracle_rows=ordinary)


@pytest.mark.parametrize("metric,kw", [("L2", {}), ("COSINE", {"centre": 1})])
def test_l2_and_forced_centred_cosine(gpu, knn_oracle_lib, metric, kw):
    """the bias variants with one scale for all rows (RSC 3): the gate sees the accumulators' start (-|y|^2, mu.y); tiles are skipped"""
    dim, nq = 128, 300
    db, q, _ = _bench_like(N0, dim, nq, 51)
    s = _Index(gpu, knn_oracle_lib, metric, dim, **kw)
    s.add(db)
    on = s.search(q)
    info = s.idx.plane_info()
    assert info["one_scale"] and (metric == "L2" or info["centred"]), info
    assert on["abandon"]["tasks"] == 158 and on["abandon"]["skipped"] >= on["abandon"]["tasks"] // 3, on["abandon"]


def test_ip_rows_of_very_different_magnitudes_run_the_plain_scan(gpu, knn_oracle_lib):
    """per-row scales (RSC 1 / 2) are not covered: such a store launches the scan it launched before"""
    dim, nq = 128, 40
    db, q, _ = _bench_like(N0, dim, nq, 61)
    db *= np.exp2(np.random.default_rng(1).integers(-10, 11, (N0, 1))).astype(np.float32)
    s = _Index(gpu, knn_oracle_lib, "IP", dim, centre=0)
    s.add(db)
    on = s.search(q)
    assert not s.idx.plane_info()["one_scale"]
    assert on["abandon"] == {"checked": 0, "skipped": 0, "tasks": 0}, on["abandon"]


def test_fp16_store(gpu, knn_oracle_lib):
    dim, nq = 128, 300
    db, q, _ = _bench_like(N0, dim, nq, 71)
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim, store_f16=True)
    s.add(db)
    assert s.search(q)["abandon"]["skipped"] > 0


def test_search_begin_and_finish(gpu, knn_oracle_lib):
    dim, nq = 512, 40
    db, q, _ = _bench_like(N0, dim, nq, 81)
    s = _Index(gpu, knn_oracle_lib, "COSINE", dim)
    s.add(db)
    assert s.search(q, begun=True)["abandon"]["skipped"] > 0
