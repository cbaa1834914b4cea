"""The abandoning tile scan's row tiles dealt to the workgroups by ticket (csrc/knn_hi.inc, k_knn_hi_abandon_deal;
RADAD_KNN_OPT_ABANDON_DEAL).  Who multiplies a tile must change nothing at all.

Every case searches ONE handle with the deal off and on and, with it on, asserts
  * ids, distances, float64 keys, radad_knn_last_emitted's counts and floors array_equal, the certificate's statistics equal;
  * radad_knn_last_abandon's checked / skipped / tasks equal: whether a tile task is tested and skipped belongs to the task, not to the
    workgroup that computes it, so a tile computed twice or never shows here (and in the emitted counts);
  * ids == the float64 oracle over the rows as stored (as tests/test_gpu_knn_abandon.py does);
  * at least one launch was dealt (and none with the option off).

Shapes: the smallest at which a resident workgroup of a 256-CU part draws several granules -- 262 400 x 128 (1025 row tiles, the last
one partial; 17 / 256 / 300 queries, 300: a second, partly filled query tile), 140 000 x 512 (checkpoint after 1 of 8 stages) and
400 000 x 128 with 300 queries (two launches, each with its own counter set).  Planted rows: tests/test_gpu_knn_abandon.py's
_bench_like recipe, one row per planted tile so that the planted rows of a store fit the re-rank (512 candidates per query).
The 262 400 x 128 rows are drawn once and shared; every store is built once per module."""
import numpy as np
import pytest

from conftest import c_knn

pytestmark = pytest.mark.gpu

K = 10
N1, D1 = 262400, 128


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


def _bench_like(n, dim, nq, seed, tiles, per_tile=1):
    """(rows, queries): random rows, queries within cos 0.998 of each other, near-duplicates of the queries planted per_tile to each of `tiles`"""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim), dtype=np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    ids = np.array([t * 256 + 16 * i + 3 for t in tiles for i in range(per_tile)], np.int64)
    db[ids] = q[np.arange(len(ids)) % nq] + (0.03 * amp * rng.standard_normal((len(ids), dim))).astype(np.float32)
    return db, q


class _Store:
    """one handle with its rows as stored and, lazily, the oracle's ids for the queries it was made with"""

    def __init__(self, gpu, lib, metric, rows, q, **kw):
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
        import torch
        self.gpu, self.lib, self.metric, self.q = gpu, lib, metric, q
        self.idx = HipFlatIndex(rows.shape[1], {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric], 0, **kw)
        self.idx.add_device(_dev(rows, gpu))
        n = self.idx.ntotal
        stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(r0, min(n, r0 + 65536), device=gpu)).cpu().numpy()
                                 for r0 in range(0, n, 65536)])
        qo = _rownorm(gpu, q) if metric == "COSINE" else np.asarray(q, np.float32)
        _, self.oracle_ids = c_knn(lib, stored, qo, K, "L2" if metric == "L2" else "IP")      # once; a batch of the first nq queries reads its rows
        self.stored, self.qo = stored, qo

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
                "certificate": launch["certificate"], "abandon": launch["early_abandon"], "deal": launch["abandon_deal"], "launch": launch}

    def static(self, nq, begun=False):
        self.idx.set_abandon_deal(0)
        off = self.observe(_dev(self.q[:nq], self.gpu), begun)
        self.idx.set_abandon_deal(1)
        assert off["deal"] == {"launches": 0, "workgroups": 0, "granule": 0}, off["deal"]
        assert off["launch"]["scan_kind"] == "hi_tile" and off["abandon"]["tasks"] > 0, off["launch"]
        return off

    def dealt(self, nq, off, begun=False):
        """the first nq queries with the deal on, checked against `off` (the same batch with static chunks) and the oracle"""
        on = self.observe(_dev(self.q[:nq], self.gpu), begun)
        print(f"{self.metric} n={len(self.stored)} d={self.stored.shape[1]} nq={nq}: deal {on['deal']}, abandon {on['abandon']} (static {off['abandon']}), "
              f"launches {on['launch']['scan_launches']}, emitted mean {on['counts'].mean():.1f}")
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(on[name], off[name]), f"{name} differs from the search with static chunks"
        assert on["certificate"] == off["certificate"], (on["certificate"], off["certificate"])
        assert on["abandon"] == off["abandon"], (on["abandon"], off["abandon"])
        assert np.array_equal(on["I"], self.oracle_ids[:nq]), "ids differ from the float64 oracle"
        assert on["deal"]["launches"] >= 1 and on["deal"]["workgroups"] > 0 and on["deal"]["granule"] in (1, 2, 4), on["deal"]
        for name in ("query_tiles", "db_splits", "block_threads", "scan_launches", "scan_phases", "scan_kind"):
            assert on["launch"][name] == off["launch"][name], name
        return on

    def search(self, nq, begun=False):
        return self.dealt(nq, self.static(nq, begun), begun)


@pytest.fixture(scope="module")
def rows1():
    """262 400 x 128 with a near-duplicate planted in every third tile, and 300 queries"""
    return _bench_like(N1, D1, 300, 101, range(0, N1 // 256, 3))


@pytest.fixture(scope="module")
def store1(gpu, knn_oracle_lib, rows1):
    return _Store(gpu, knn_oracle_lib, "COSINE", rows1[0], rows1[1])


@pytest.mark.parametrize("nq", [17, 256, 300])
def test_the_benchmark_in_miniature(store1, nq):
    on = store1.search(nq)
    ab = on["abandon"]
    assert ab["tasks"] == ((N1 + 255) // 256) * ((nq + 255) // 256)
    assert ab["skipped"] >= ab["tasks"] // 3 and ab["skipped"] <= ab["checked"] <= ab["tasks"], ab


def test_checkpoint_one_of_eight_stages(gpu, knn_oracle_lib):
    n, dim = 140000, 512
    db, q = _bench_like(n, dim, 256, 103, range(0, n // 256, 3))
    on = _Store(gpu, knn_oracle_lib, "COSINE", db, q).search(256)
    assert on["abandon"]["skipped"] >= on["abandon"]["tasks"] // 3, on["abandon"]


def test_two_launches_each_with_its_own_counters(gpu, knn_oracle_lib):
    """(400 000 rows, 300 queries: tests/test_gpu_knn_abandon.py's two-phase store.  512 + 1051 row tiles, 2 query tiles: on a 256-CU part
    16 resident workgroups per (slot, query tile) draw 2 and 4 granules of two tiles -- both launches are dealt.  Were they to share
    counters the second would find them used up and scan nothing.)"""
    n, dim, nq = 400000, 128, 300
    db, q = _bench_like(n, dim, nq, 5, range(0, n // 256, 6))
    on = _Store(gpu, knn_oracle_lib, "COSINE", db, q).search(nq)
    assert on["launch"]["scan_launches"] == 2, on["launch"]
    assert on["deal"]["launches"] == 2, on["deal"]
    assert on["abandon"]["tasks"] == ((n + 255) // 256) * 2 and on["abandon"]["skipped"] >= on["abandon"]["tasks"] // 3, on["abandon"]


def test_a_cluster_ordered_store(gpu, knn_oracle_lib):
    """every planted row inside one contiguous eighth of the store (tiles 128 ... 255): the tiles that cannot be skipped are one static
    chunk's neighbours, and the deal spreads them over all eight slots"""
    db, q = _bench_like(N1, D1, 300, 107, range(128, 256), per_tile=2)
    s = _Store(gpu, knn_oracle_lib, "COSINE", db, q)
    on = s.search(300)
    ab = on["abandon"]
    assert ab["checked"] == ab["tasks"] and ab["tasks"] - ab["skipped"] <= 2 * (128 + 64), ab      # the planted tiles and the sample's survive, little else


@pytest.mark.parametrize("metric,kw", [("L2", {}), ("COSINE", {"store_f16": True})])
def test_l2_and_an_fp16_store(gpu, knn_oracle_lib, rows1, metric, kw):
    s = _Store(gpu, knn_oracle_lib, metric, rows1[0], rows1[1], **kw)
    on = s.search(300)
    assert on["abandon"]["skipped"] > 0, on["abandon"]
    if metric == "L2":
        assert s.idx.plane_info()["one_scale"]          # RSC 3: the bias variant with one scale


def test_counters_left_by_earlier_searches(store1):
    """the same search three times on one handle, then 17 -> 300 -> 17 queries: a counter left unzeroed makes the next search scan nothing"""
    off = {nq: store1.static(nq) for nq in (17, 300)}
    for nq in (300, 300, 300, 17, 300, 17):
        store1.dealt(nq, off[nq])


def test_search_begin_and_finish(store1):
    store1.search(300, begun=True)


def test_a_range_search_whose_one_launch_is_dealt(store1):
    """every query's radius holds the planted rows and nothing else: cos > 0.9 (planted ~0.997, random rows |cos| < 0.5 by 5 sigma).  The
    radius is the floor the abandon tests against: at 0.9 it stands clear of what half a random row can add (0.707 x 0.707), so the
    gate opens and tiles are skipped"""
    nq, m, thr = 17, 512, 0.9
    qt = _dev(store1.q[:nq], store1.gpu)
    keys = store1.stored.astype(np.float64) @ store1.qo[:nq].astype(np.float64).T        # [n, nq]
    assert np.abs(keys - thr).min() > 1e-3                                               # nothing near the radius: the count is beyond rounding
    want = (keys > thr).sum(axis=0)
    assert want.min() > 0 and want.max() <= m
    out = {}
    for deal in (0, 1):
        store1.idx.set_abandon_deal(deal)
        counts, D, I, K64 = store1.idx.range_search_device(qt, thr, m, return_f64=True)
        out[deal] = (counts.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy(), K64.cpu().numpy(), store1.idx.last_emitted(nq),
                     store1.idx.last_abandon(), store1.idx.last_abandon_deal(), store1.idx.last_range())
    store1.idx.set_abandon_deal(1)
    off, on = out[0], out[1]
    print(f"range: deal {on[6]}, abandon {on[5]} (static {off[5]}), route {on[7]}")
    assert on[7]["route"] == "tile" and on[7] == off[7], (on[7], off[7])
    for a, b in zip(on[:4], off[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(on[4][0], off[4][0]) and np.array_equal(on[4][1], off[4][1])
    assert on[5] == off[5] and on[5]["skipped"] > 0, (on[5], off[5])
    assert on[6]["launches"] == 1 and off[6]["launches"] == 0, (on[6], off[6])
    assert np.array_equal(on[0], want)
    for j in range(nq):
        order = np.lexsort((np.arange(len(keys)), -keys[:, j]))[:want[j]]
        assert np.array_equal(on[2][j, :want[j]], order), j


def test_random_rows_and_queries_are_never_tested(gpu, knn_oracle_lib):
    """the gate stays shut for every query tile: the dealt launch's workgroups run the plain body over their static chunks"""
    rng = np.random.default_rng(3)
    db, q = rng.standard_normal((N1, D1), dtype=np.float32), rng.standard_normal((300, D1)).astype(np.float32)
    on = _Store(gpu, knn_oracle_lib, "COSINE", db, q).search(300)
    assert on["abandon"]["tasks"] > 0 and on["abandon"]["checked"] == 0 and on["abandon"]["skipped"] == 0, on["abandon"]
