"""The next tile's head fetched at the abandon checkpoint (csrc/knn_hi.inc, ahead_on; RADAD_KNN_OPT_ABANDON_AHEAD).  What a stage
fetches, and when, must change nothing at all.

Every case searches ONE handle with the option off and on (abandon and deferral on unless the case says otherwise) and asserts
  * ids, distances, float64 keys, radad_knn_last_emitted's counts and floors array_equal, the certificate's statistics equal and no
    query rejected, last_launch()["early_abandon"] and ["abandon_defer"] equal;
  * ids == the float64 oracle over the rows as stored (the first 32 queries of a batch);
  * the counters: used + wasted and wasted EQUAL to what the host model (knn_ahead_walk, csrc/knn_plan.h, restated below) gives for
    the store's outcome pattern walked over the launch's chunks as the planner cuts them (radad_knn_scan_geometry), per query tile.

Shapes.  The 20 000-row stores of the other abandon tests give one tile per workgroup: nothing there has a next tile.  Here: 262 400 x
128 (1025 tiles, the last one of 64 rows), 140 000 x 512 (checkpoint after 1 of 8 stages) and a store of dim 1024 (checkpoint after 2
of 16) at the smallest row count at which 300 queries give two tiles per chunk.  All are ONE launch (asserted), so the launch's chunks
are radad_knn_scan_geometry(n, nq)'s, and every case asserts at least two tiles per chunk.

Patterns.  Random unit-scale rows, queries within cos 0.998 of each other (the benchmark's structure), so every workgroup's gate is open
and a tile of random rows is skipped.  On top of that:
  * a PLANTED tile holds one near-duplicate of a query: one live row, deferred (leaves) -- or, with the deferral off, stays.  Every
    fourth tile is planted, which covers every tile of the sample pre-pass: the floors stand clear of everything else.
  * a STAY tile holds 24 rows whose first 64 ck elements are 0.9 of the queries' common direction there and whose rest is noise: at the
    checkpoint their partial score (0.9 |q[:64 ck]|) lies above floor - |q[64 ck:]| max |y[64 ck:]| by more than 0.1 |q|, so they are
    live -- more than KNN_DEFER_MAX_ROWS of them: the tile stays -- and in full they score 0.9 |q[:64 ck]| + noise, far below the
    floor: they are no candidates and fill no buffer.
  * an UNTESTED tile (IP store of unit rows) holds one row of norm 3 pointing away from the queries in its elements from 64 ck on: the
    tile's suffix norm is three times its neighbours' and its gate is shut; the row scores far below every other.
Whether the store behaved as built is itself asserted, as equalities on the read-backs: tested = every tile that is not UNTESTED,
skipped = the plain tiles, deferred = the planted ones, stayed = the STAY tiles (x query tiles)."""
import ctypes as C

import numpy as np
import pytest

from conftest import c_knn

pytestmark = pytest.mark.gpu

K = 10
N1, D1 = 262400, 128
N2, D2 = 140000, 512
D3 = 1024
UNTESTED, LEAVE, STAY = 0, 1, 2
ORACLE_Q = 32


def checkpoint(dim):
    """knn_abandon_checkpoint (csrc/knn_plan.h; tests/abandon_ref.py)"""
    return max(1, dim // 64 // 8)


def ahead_walk(outcome, ahead_on=True):
    """knn_ahead_walk (csrc/knn_plan.h): one workgroup's tiles -> (used, wasted)"""
    used = wasted = 0
    pred = True
    for t, o in enumerate(outcome):
        if o == UNTESTED:
            continue
        spec = ahead_on and pred and t + 1 < len(outcome)
        left = o == LEAVE
        used += int(left and spec)
        wasted += int(not left and spec)
        pred = left
    return used, wasted


def geometry(n, nq):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    qt, ch, rows = C.c_int(), C.c_int(), C.c_int64()
    _lib.check(_lib.load().radad_knn_scan_geometry(n, nq, C.byref(qt), C.byref(ch), C.byref(rows)))
    assert rows.value % 256 == 0
    return qt.value, ch.value, rows.value // 256


def expected(outcome, n, nq):
    """(used, wasted) of a one-launch search: every query tile walks every chunk"""
    qt, chunks, per = geometry(n, nq)
    assert per >= 2, "the shape gives one tile per workgroup: nothing has a next tile"
    u = w = 0
    for c in range(chunks):
        a, b = ahead_walk(outcome[c * per:(c + 1) * per])
        u, w = u + a, w + b
    return u * qt, w * qt


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


def build(n, dim, nq, seed, stay=(), untested=(), unit=False):
    """(rows, queries, kind [tiles]: 'plain' | 'planted' | 'stay' | 'untested').  unit: rows and queries of norm 1 (L2 and IP stores then
    rank as the cosine ones do)"""
    rng = np.random.default_rng(seed)
    tiles = (n + 255) // 256
    db = rng.standard_normal((n, dim), dtype=np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    kind = np.array(["plain"] * tiles, dtype=object)
    stay, untested = set(stay), set(untested)
    assert not (stay & untested) and all(0 <= t < tiles for t in stay | untested)
    e0 = 64 * checkpoint(dim)
    head = base[:e0] / np.linalg.norm(base[:e0])
    scale = np.sqrt(dim)
    planted = 0
    for t in range(tiles):
        rows_t = min(256, n - t * 256)
        if t in stay:
            kind[t] = "stay"
            r = t * 256 + 1 + 2 * np.arange(24)
            assert r.max() < t * 256 + rows_t
            tailn = rng.standard_normal((24, dim - e0))
            tailn *= np.sqrt(1 - 0.81) / np.linalg.norm(tailn, axis=1, keepdims=True)
            db[r, :e0] = (scale * 0.9 * head[None, :]).astype(np.float32)
            db[r, e0:] = (scale * tailn).astype(np.float32)
        elif t in untested:
            kind[t] = "untested"
            db[t * 256 + 7] = 0.0
            db[t * 256 + 7, e0:] = (-3.0 * scale * base[e0:] / np.linalg.norm(base[e0:])).astype(np.float32)
        elif t % 4 == 0:
            kind[t] = "planted"
            db[t * 256 + 3] = q[planted % nq] + (0.03 * amp * rng.standard_normal(dim)).astype(np.float32)
            planted += 1
    if unit:
        norms = np.linalg.norm(db, axis=1, keepdims=True)
        big = norms[:, 0] > 2 * scale
        db = np.where(big[:, None], db / scale, db / norms).astype(np.float32)
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return db, q, kind


class _Index:
    def __init__(self, gpu, lib, metric, rows, **kw):
        import torch
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
        self.gpu, self.lib, self.metric = gpu, lib, metric
        self.idx = HipFlatIndex(rows.shape[1], {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric], 0, **kw)
        self.idx.add_device(_dev(rows, gpu))
        n = self.idx.ntotal
        self.stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(r0, min(n, r0 + 65536), device=gpu)).cpu().numpy()
                                      for r0 in range(0, n, 65536)])

    def observe(self, qt):
        nq = qt.shape[0]
        D, I, K64 = self.idx.search_device(qt, K, return_f64=True)
        launch = self.idx.last_launch()
        counts, floors = self.idx.last_emitted(nq)
        return {"D": D.cpu().numpy(), "I": I.cpu().numpy(), "K64": K64.cpu().numpy(), "counts": counts, "floors": floors,
                "certificate": launch["certificate"], "abandon": launch["early_abandon"], "defer": launch["abandon_defer"],
                "ahead": launch["abandon_ahead"], "launch": launch}

    def search(self, q, defer=1):
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        self.idx.set_abandon(1)
        self.idx.set_abandon_defer(defer)
        self.idx.set_abandon_ahead(0)
        off = self.observe(qt)
        self.idx.set_abandon_ahead(1)
        on = self.observe(qt)
        print(f"{self.metric} n={len(self.stored)} d={self.stored.shape[1]} nq={len(q)}: ahead {on['ahead']}, abandon {on['abandon']}, defer {on['defer']}, "
              f"grid {on['launch']['query_tiles']} x {on['launch']['db_splits']}, emitted mean {on['counts'].mean():.1f}")
        assert on["launch"]["scan_kind"] == "hi_tile" and on["launch"]["scan_launches"] == 1, on["launch"]
        assert off["ahead"] == {"used": 0, "wasted": 0}, off["ahead"]
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(on[name], off[name]), f"{name} differs from the search with the option off"
        assert on["certificate"] == off["certificate"] and on["certificate"]["rejected"] == 0, (on["certificate"], off["certificate"])
        assert on["abandon"] == off["abandon"], (on["abandon"], off["abandon"])
        assert on["defer"] == off["defer"], (on["defer"], off["defer"])
        for name in ("query_tiles", "db_splits", "block_threads", "scan_launches", "scan_phases"):
            assert on["launch"][name] == off["launch"][name], name
        m = min(len(q), ORACLE_Q)
        qo = _rownorm(self.gpu, q[:m]) if self.metric == "COSINE" else np.asarray(q[:m], np.float32)
        _, oi = c_knn(self.lib, self.stored, qo, K, "L2" if self.metric == "L2" else "IP")
        assert np.array_equal(on["I"][:m], oi), "ids differ from the float64 oracle"
        return on


def check(on, kind, n, nq, defer=1):
    """the store behaved as built, and the counters are the host model's"""
    qtiles = (nq + 255) // 256
    count = {k: int((kind == k).sum()) for k in ("plain", "planted", "stay", "untested")}
    ab, df, ah = on["abandon"], on["defer"], on["ahead"]
    assert ab["tasks"] == len(kind) * qtiles, ab
    assert ab["checked"] == (len(kind) - count["untested"]) * qtiles, (ab, count)
    assert ab["skipped"] == count["plain"] * qtiles, (ab, count)
    assert df["tile_tasks_deferred"] == (count["planted"] * qtiles if defer else 0), (df, count)
    leave = ("plain", "planted") if defer else ("plain",)
    outcome = [UNTESTED if k == "untested" else LEAVE if k in leave else STAY for k in kind]
    used, wasted = expected(outcome, n, nq)
    assert ah["used"] + ah["wasted"] == used + wasted and ah["wasted"] == wasted, (ah, used, wasted)
    return used, wasted


def run(gpu, lib, metric, n, dim, nq, seed, stay=(), untested=(), defer=1, **kw):
    db, q, kind = build(n, dim, nq, seed, stay, untested, unit=metric != "COSINE")
    s = _Index(gpu, lib, metric, db, **kw)
    on = s.search(q, defer)
    return s, q, on, kind, check(on, kind, n, nq, defer)


TILES1 = (N1 + 255) // 256


@pytest.mark.parametrize("nq", [17, 256, 300])
def test_every_tile_leaves(gpu, knn_oracle_lib, nq):
    _, _, on, _, (used, wasted) = run(gpu, knn_oracle_lib, "COSINE", N1, D1, nq, 7 + nq)
    assert wasted == 0 and on["ahead"]["wasted"] == 0 and used > 0


@pytest.mark.parametrize("nq", [17, 300])
def test_every_other_tile_stays(gpu, knn_oracle_lib, nq):
    _, _, _, _, (used, wasted) = run(gpu, knn_oracle_lib, "COSINE", N1, D1, nq, 11 + nq, stay=range(1, TILES1, 2))
    assert wasted > 0


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_stay_at_the_first_or_the_last_tile_of_some_chunks(gpu, knn_oracle_lib, where):
    """... and, for `last`, the store's partial last tile"""
    nq = 256
    _, chunks, per = geometry(N1, nq)
    stay = {c * per + (0 if where == "first" else per - 1) for c in range(1, chunks, 3) if c * per + per - 1 < TILES1}
    if where == "last":
        stay.add(TILES1 - 1)
    _, _, _, kind, (used, wasted) = run(gpu, knn_oracle_lib, "COSINE", N1, D1, nq, 13 + len(where), stay=stay)
    # (a chunk's last tile never speculates: a stay there wastes nothing; a stay at its first tile always does)
    assert wasted == (len(stay) if where == "first" else 0)


def test_a_stay_right_after_a_deferral_and_a_deferral_right_after_a_stay(gpu, knn_oracle_lib):
    """planted tiles are the multiples of 4: a stay at 4 j + 1 follows a deferral, a stay at 4 j + 3 precedes one"""
    stay = [t for t in range(TILES1 - 1) if t % 8 in (1, 7)]
    run(gpu, knn_oracle_lib, "COSINE", N1, D1, 300, 17, stay=stay)


def test_deferring_off_so_that_vetoed_tiles_stay(gpu, knn_oracle_lib):
    _, _, _, _, (used, wasted) = run(gpu, knn_oracle_lib, "COSINE", N1, D1, 300, 19, defer=0)
    assert wasted > 0


def test_checkpoint_one_of_eight_stages(gpu, knn_oracle_lib):
    run(gpu, knn_oracle_lib, "COSINE", N2, D2, 256, 23, stay=range(1, (N2 + 255) // 256, 2))


def test_checkpoint_two_of_sixteen_stages(gpu, knn_oracle_lib):
    """dim 1024 at the smallest row count at which 300 queries give two tiles per chunk, a partial last tile"""
    nq = 300
    tiles = next(t for t in range(8, 4096) if geometry(t * 256, nq)[2] >= 2)
    n = tiles * 256 - 48
    assert geometry(n, nq)[2] >= 2 and geometry(n - 256, nq)[2] == 1
    run(gpu, knn_oracle_lib, "COSINE", n, D3, nq, 29, stay=range(1, tiles, 2))


def test_l2(gpu, knn_oracle_lib):
    s, _, _, _, _ = run(gpu, knn_oracle_lib, "L2", N1, D1, 300, 31, stay=range(1, TILES1, 2))
    assert s.idx.plane_info()["one_scale"]          # RSC 3: the bias variant with one scale


def test_an_fp16_store(gpu, knn_oracle_lib):
    run(gpu, knn_oracle_lib, "COSINE", N1, D1, 256, 37, stay=range(1, TILES1, 2), store_f16=True)


def test_tiles_whose_gate_is_shut_between_tested_neighbours(gpu, knn_oracle_lib):
    """an IP store with one huge-norm row in some tiles: those tiles are not tested, neither consult nor update the prediction, and run
    today's fetch pattern"""
    untested = [t for t in range(TILES1 - 1) if t % 8 == 2]
    stay = [t for t in range(TILES1 - 1) if t % 8 == 5]
    run(gpu, knn_oracle_lib, "IP", N1, D1, 300, 41, stay=stay, untested=untested)


def test_random_queries_shut_the_workgroups_gate(gpu, knn_oracle_lib):
    rng = np.random.default_rng(43)
    db, q = rng.standard_normal((N1, D1), dtype=np.float32), rng.standard_normal((300, D1), dtype=np.float32)
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    qt = _dev(q, gpu)
    s.idx.set_abandon_ahead(1)
    on = s.observe(qt)
    assert on["abandon"]["tasks"] > 0 and on["abandon"]["checked"] == 0, on["abandon"]
    assert on["ahead"] == {"used": 0, "wasted": 0}, on["ahead"]
    _, oi = c_knn(knn_oracle_lib, s.stored, _rownorm(gpu, q[:ORACLE_Q]), K, "IP")
    assert np.array_equal(on["I"][:ORACLE_Q], oi)


def test_determinism(gpu, knn_oracle_lib):
    """the alternating pattern ten times on one handle with the option on: a race on the LDS words a leaving tile's second barrier used
    to protect (s_veto, the live-row masks, the accumulator starts) shows here, or as a tile emitted twice or never"""
    s, q, first, _, _ = run(gpu, knn_oracle_lib, "COSINE", N1, D1, 300, 47, stay=range(1, TILES1, 2))
    qt = _dev(q, gpu)
    for _ in range(10):
        again = s.observe(qt)
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(again[name], first[name]), name
        for name in ("ahead", "defer", "abandon", "certificate"):
            assert again[name] == first[name], (name, again[name], first[name])
