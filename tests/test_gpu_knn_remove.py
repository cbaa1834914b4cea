"""Removing rows from a flat store in place (radad_knn_remove_ids, csrc/knn_remove.inc; HipFlatIndex.remove_ids,
VectorDatabase.remove_vectors / remove_files, HotPathPipeline.remove_files).

What a removal must leave: the kept rows bit for bit, in their old order, at positions 0 ... ntotal - 1; the old -> new id map of the
numpy model (tests/knn_remove_ref.py); and a store every search path answers exactly -- ids equal to the float64 oracle over
rows[keep], distances within 1e-6 relative and absolute (the tolerance of tests/test_gpu_knn_exact_batches.py).  The removal patterns
run with remove_stage_rows at its minimum (64), so that a 5 000-row store spans 79 slabs and both kinds of launch (staged and direct)
move rows; a subset runs at the default stage size."""
import os

import numpy as np
import pytest

import excl_per_query_ref as P
import exclusion_ref as E
import knn_remove_ref as M
import range_ref as RG
from conftest import c_knn

pytestmark = pytest.mark.gpu

METRICS = ("L2", "IP", "COSINE")
S_MIN = M.MIN_STAGE_ROWS


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _index(metric, dim, f16=False, id_base=0, **kw):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    return HipFlatIndex(dim, {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric], 0, id_base, store_f16=f16, **kw)


def _stored(idx, gpu):
    import torch
    n = idx.ntotal
    if n == 0:
        return np.zeros((0, idx.d), np.float32)
    return idx.reconstruct_batch(idx.id_base + torch.arange(n, device=gpu)).cpu().numpy()


def _rownorm(gpu, q):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    qt = _dev(np.asarray(q, np.float32), gpu)
    out = torch.empty_like(qt)
    _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), out.data_ptr(), qt.shape[0], qt.shape[1], gpu.index or 0, _lib.stream_ptr(gpu)))
    return out.cpu().numpy()


def _oracle(lib, gpu, metric, rows, q, k, id_base=0):
    """the C float64 oracle over `rows` (as stored); cosine: stored rows against the device's normalised queries, as an inner product"""
    qo = _rownorm(gpu, q) if metric == "COSINE" else np.asarray(q, np.float32)
    return c_knn(lib, rows, qo, k, "L2" if metric == "L2" else "IP", id_base)


def _check_search(idx, lib, gpu, metric, rows, q, k, what):
    D, I = idx.search_device(_dev(q, gpu), k)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    ed, ei = _oracle(lib, gpu, metric, rows, q, k, idx.id_base)
    assert np.array_equal(I, ei), f"{what}: ids differ from the float64 oracle in {int((I != ei).any(axis=1).sum())} of {len(q)} queries"
    assert (np.abs(D - ed) <= 1e-6 + 1e-6 * np.abs(ed)).all(), f"{what}: distances beyond 1e-6"


# ---- stored rows ------------------------------------------------------------------------------------------------------------------------
def _id_lists(n, S, id_base, rng):
    """(name, id list): every pattern of the plan's check as ascending global ids, then one unsorted list with duplicates, negative
    ids and ids at and beyond ntotal"""
    for pat in M.PATTERNS:
        yield pat, id_base + np.flatnonzero(M.pattern_flags(pat, n, S)).astype(np.int64)
    pos = rng.choice(n, max(1, n // 3), replace=False).astype(np.int64)
    messy = np.concatenate([id_base + pos, id_base + pos[: len(pos) // 2 + 1], [-1, -7, id_base - 1, id_base + n, id_base + n + 5, 2 ** 62]])
    yield "messy", rng.permutation(messy)


def _remove_and_check(gpu, metric, dim, f16, n, name, ids, id_base, stage_rows, rows_in):
    import torch
    idx = _index(metric, dim, f16, id_base, remove_stage_rows=stage_rows)
    idx.add_device(_dev(rows_in, gpu))
    before = _stored(idx, gpu)                      # (cosine / fp16: the rows as stored, not as handed in)
    keep, omap, removed = M.removal(n, ids, id_base)
    got, dmap = idx.remove_ids(_dev(ids, gpu) if len(ids) % 2 else ids, return_map=True)       # (device tensors and numpy arrays both)
    what = f"{metric} dim {dim} {'f16' if f16 else 'f32'} n {n} {name} base {id_base} stage {stage_rows}"
    assert got == removed, f"{what}: n_removed {got}, the model says {removed}"
    assert idx.ntotal == n - removed, what
    assert np.array_equal(dmap.cpu().numpy(), omap), f"{what}: old_to_new differs from the model"
    after = _stored(idx, gpu)
    assert after.shape == (n - removed, dim) and np.array_equal(after.view(np.uint32), before[keep].view(np.uint32)), f"{what}: stored rows are not rows[keep] bit for bit"
    if metric == "L2" and n - removed > 0:          # the squared norms moved with their rows: an L2 search of a kept row finds it at 0
        j = int(np.flatnonzero(keep)[-1])
        D, I = idx.search_device(_dev(before[j:j + 1], gpu), 1)
        assert int(I[0, 0]) == int(omap[j]), what
        assert abs(float(D[0, 0])) <= 1e-3 * max(1.0, float((before[j] ** 2).sum())), what
    return idx


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [4, 100, 512])
@pytest.mark.parametrize("metric", METRICS)
def test_stored_rows_after_every_pattern(gpu, metric, dim, f16):
    """dim 100 on an fp16 store: rows of 200 bytes, every second one only 8-byte aligned, source and destination of either parity"""
    rng = np.random.default_rng(1000 + dim + 7 * f16 + METRICS.index(metric))
    for n in (1, 257, 5000):
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        for name, ids in _id_lists(n, S_MIN, 0, rng):
            _remove_and_check(gpu, metric, dim, f16, n, name, ids, 0, S_MIN, rows)
    n = 5000
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for name, ids in _id_lists(n, S_MIN, 10 ** 9, rng):
        if name in ("random30", "every_other", "run", "messy"):
            _remove_and_check(gpu, metric, dim, f16, n, name, ids, 10 ** 9, S_MIN, rows)
    for name, ids in _id_lists(n, M.stage_rows(dim * (2 if f16 else 4)), 0, rng):          # the default stage size: one slab
        if name in ("random30", "every_other", "last", "messy"):
            _remove_and_check(gpu, metric, dim, f16, n, name, ids, 0, None, rows)


def test_the_minimum_stage_spans_many_slabs_and_an_empty_list_changes_nothing(gpu):
    rng = np.random.default_rng(5)
    n, dim = 5000, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    flags = M.pattern_flags("random30", n, S_MIN)
    idx = _index("L2", dim, remove_stage_rows=1)                 # below the minimum: raised to 64
    idx.add_device(_dev(rows, gpu))
    before = _stored(idx, gpu)
    for empty in ([], np.zeros(0, np.int64), _dev(np.zeros(0, np.int64), gpu), [-5, n, n + 1]):
        got, dmap = idx.remove_ids(empty, return_map=True)
        assert got == 0 and idx.ntotal == n and np.array_equal(dmap.cpu().numpy(), np.arange(n))
        assert np.array_equal(_stored(idx, gpu).view(np.uint32), before.view(np.uint32))
        assert idx.last_remove() == {"launches": 0, "bytes_moved": 0}
    assert idx.remove_ids(np.flatnonzero(flags)) == int(flags.sum())
    p = M.plan(n, dim * 4, flags, 1, l2=True)
    assert len(p["slabs"]) == 79 and any(s[4] for s in p["slabs"]) and not all(s[4] for s in p["slabs"])
    assert idx.last_remove() == {"launches": len(p["launches"]), "bytes_moved": p["bytes_moved"]}
    assert np.array_equal(_stored(idx, gpu).view(np.uint32), before[~flags].view(np.uint32))
    # the same removal at the default stage size: one staged slab, the same store
    idx2 = _index("L2", dim)
    idx2.add_device(_dev(rows, gpu))
    idx2.remove_ids(np.flatnonzero(flags))
    assert idx2.last_remove()["launches"] == 2
    assert np.array_equal(_stored(idx2, gpu).view(np.uint32), _stored(idx, gpu).view(np.uint32))


def test_many_slabs_with_grouped_direct_launches(gpu):
    """200 000 rows in slabs of 1024: once 1024 rows have gone the slabs go direct, and the launches grow with the rows removed in front
    of them (several slabs each)"""
    import torch
    n, dim = 200_000, 32
    g = torch.Generator(device=gpu).manual_seed(11)
    rows = torch.randn((n, dim), device=gpu, generator=g)
    flags = (torch.rand((n,), device=gpu, generator=g) < 0.2).cpu().numpy()
    for metric in ("L2", "IP"):
        idx = _index(metric, dim, remove_stage_rows=1024)
        idx.add_device(rows)
        got, dmap = idx.remove_ids(np.flatnonzero(flags), return_map=True)
        p = M.plan(n, dim * 4, flags, 1024, l2=metric == "L2")
        assert got == int(flags.sum()) and idx.last_remove() == {"launches": len(p["launches"]), "bytes_moved": p["bytes_moved"]}
        assert sum(1 for l in p["launches"] if l[0] == M.DIRECT and l[2] > 4 * 1024) > 5 and sum(1 for l in p["launches"] if l[0] == M.GATHER) >= 4
        assert np.array_equal(dmap.cpu().numpy(), M.removal(n, np.flatnonzero(flags))[1])
        assert torch.equal(idx.reconstruct_batch(torch.arange(idx.ntotal, device=gpu)), rows[_dev(~flags, gpu)])
        if metric == "L2":       # the norms moved with the rows: |row - row| = 0 at the row's new id, for rows from every part of the store
            probe = np.flatnonzero(~flags)[:: 9973]
            D, I = idx.search_device(rows[_dev(probe, gpu)], 1)
            assert np.array_equal(I.cpu().numpy()[:, 0], dmap.cpu().numpy()[probe]) and float(D.abs().max()) < 1e-3


def test_a_store_beyond_four_gibibytes(gpu):
    """2.2 M x 512 fp32 rows are 4.5 GB: byte offsets of sources, destinations and launches beyond 2^31 and 2^32, at the default
    stage size (69 slabs of 32 768 rows).  Compared on the device."""
    import torch
    n, dim = 2_200_000, 512
    g = torch.Generator(device=gpu).manual_seed(12)
    rows = torch.randn((n, dim), device=gpu, generator=g)
    drop = torch.rand((n,), device=gpu, generator=g) < 0.2
    drop[-3:] = torch.tensor([False, True, False], device=gpu)
    idx = _index("IP", dim)
    idx.add_device(rows)
    got = idx.remove_ids(torch.nonzero(drop).reshape(-1))
    assert got == int(drop.sum()) and idx.ntotal == n - got
    assert idx.last_remove()["launches"] > 6
    kept = rows[~drop]
    del rows
    assert torch.equal(idx.reconstruct_batch(torch.arange(idx.ntotal, device=gpu)), kept)


# ---- searches after a removal -----------------------------------------------------------------------------------------------------------
ROUTES = {   # name: (n, dim, nq, k, metric, scan kind the search must report)
    "dense": (5000, 64, 32, 10, "L2", "f32_dense"),
    "reg_list": (5000, 64, 32, 10, "IP", None),
    "smallq_plane": (20000, 512, 4, 10, "COSINE", "hi_smallq"),
    "tile_k10": (20000, 512, 32, 10, "IP", "hi_tile"),
    "tile_k130": (20000, 512, 32, 130, "L2", None),
}
_cache = {}


def _route_data(name):
    if name not in _cache:
        n, dim, nq, k, metric, kind = ROUTES[name]
        rng = np.random.default_rng(sorted(ROUTES).index(name) + 77)
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        # 5 000-row stores lose 30 % of their rows; the 20 000-row stores 10 %, so that the 18 000 or so that stay still take the
        # route the case is about (the plane's small-batch stream needs 16 384 rows, the tile scan 64 row tiles)
        flags = M.pattern_flags("random30", n, S_MIN) if n <= 5000 else rng.random(n) < 0.1
        flags[:3] = [False, True, False]                 # the first removed row is row 1: the whole plane is brought up to date
        _cache[name] = rows, q, flags
    return _cache[name]


@pytest.mark.parametrize("order", ["plane_first", "removal_first"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_search_after_a_removal(gpu, knn_oracle_lib, route, order):
    n, dim, nq, k, metric, kind = ROUTES[route]
    rows, q, flags = _route_data(route)
    kw = {"dense": 0} if route == "reg_list" else {}
    idx = _index(metric, dim, remove_stage_rows=S_MIN, **kw)
    idx.add_device(_dev(rows, gpu))
    if order == "plane_first":
        _check_search(idx, knn_oracle_lib, gpu, metric, _stored(idx, gpu), q, k, f"{route} before the removal")
    before = _stored(idx, gpu)
    assert idx.remove_ids(np.flatnonzero(flags)) == int(flags.sum())
    kept = _stored(idx, gpu)
    assert np.array_equal(kept.view(np.uint32), before[~flags].view(np.uint32))
    _check_search(idx, knn_oracle_lib, gpu, metric, kept, q, k, f"{route} after the removal ({order})")
    launch = idx.last_launch()
    if kind is not None:
        assert launch["scan_kind"] == kind, launch["scan_kind"]
    if metric == "L2":
        # the squared norms moved with their rows: the certificate sees what it sees on a new store of the kept rows (a norm left
        # behind would still give exact results -- through rejected queries and the exact kernel)
        fresh = _index(metric, dim, **kw)
        fresh.add_device(_dev(kept, gpu))
        _check_search(fresh, knn_oracle_lib, gpu, metric, kept, q, k, f"{route}: a new store of the kept rows")
        assert launch["certificate"]["rejected"] == fresh.last_launch()["certificate"]["rejected"], (launch["certificate"], fresh.last_launch()["certificate"])
    # ... and again: the second search finds everything up to date
    _check_search(idx, knn_oracle_lib, gpu, metric, kept, q, k, f"{route}, second search after the removal ({order})")


def test_removing_the_tail_does_not_rebuild_the_plane(gpu, knn_oracle_lib):
    rows, q, _ = _route_data("tile_k10")
    idx = _index("IP", 512, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    _check_search(idx, knn_oracle_lib, gpu, "IP", rows, q, 10, "before")
    info = idx.plane_info()
    assert info["built"]
    assert idx.remove_ids(np.arange(19000, 20000)) == 1000
    assert idx.last_remove() == {"launches": 0, "bytes_moved": 0}        # nothing behind the removed rows: nothing moves
    _check_search(idx, knn_oracle_lib, gpu, "IP", rows[:19000], q, 10, "after removing the last 1000 rows")
    assert idx.last_launch()["scan_kind"] == "hi_tile"
    assert idx.plane_info() == info, (idx.plane_info(), info)             # built, centring, scale and the rebuild count: unchanged


def _bench_like(n, dim, nq, seed, per_tile=8, every=3):
    """random rows, queries within a narrow cone, near-duplicates of the queries planted per_tile to a tile in every `every`-th tile:
    the admission floor clears every random row, so most tiles are abandoned"""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    ids = np.array([t * 256 + 16 * i + 3 for t in range(0, n // 256, every) for i in range(per_tile)], np.int64)
    db[ids] = q[np.arange(len(ids)) % nq] + (0.03 * amp * rng.standard_normal((len(ids), dim))).astype(np.float32)
    return db, q


def test_the_abandoning_scan_after_the_last_row_of_a_full_tile_went(gpu, knn_oracle_lib):
    n, dim, nq = 79 * 256, 128, 256
    db, q = _bench_like(n, dim, nq, 31)
    idx = _index("COSINE", dim, remove_stage_rows=S_MIN)
    idx.add_device(_dev(db, gpu))
    stored = _stored(idx, gpu)
    _check_search(idx, knn_oracle_lib, gpu, "COSINE", stored, q, 10, "before")
    ab = idx.last_abandon()
    assert ab["tasks"] == 79 and ab["skipped"] > 0, ab
    assert idx.remove_ids([n - 1]) == 1                                   # the last row of the full last tile
    _check_search(idx, knn_oracle_lib, gpu, "COSINE", stored[:n - 1], q, 10, "after the last row went")
    ab = idx.last_abandon()
    assert ab["tasks"] == 79 and ab["skipped"] > 0, ab                    # ceil(20223 / 256) row tiles x one query tile
    assert idx.remove_ids(np.arange(78 * 256, n - 1)) == 255              # ... and the rest of that tile
    _check_search(idx, knn_oracle_lib, gpu, "COSINE", stored[:78 * 256], q, 10, "after the last tile went")
    ab = idx.last_abandon()
    assert ab["tasks"] == 78 and ab["skipped"] > 0, ab
    # a row out of the MIDDLE of a tile that holds planted rows: the tiles behind it shift by one row, their terms are recomputed
    mid = 30 * 256 + 19
    assert idx.remove_ids([mid]) == 1
    keep = np.ones(78 * 256, bool)
    keep[mid] = False
    _check_search(idx, knn_oracle_lib, gpu, "COSINE", stored[:78 * 256][keep], q, 10, "after a row in the middle went")
    assert idx.last_abandon()["tasks"] == 78 and idx.last_abandon()["skipped"] > 0


# ---- remove, then append ----------------------------------------------------------------------------------------------------------------
def test_remove_then_append(gpu, knn_oracle_lib):
    rows, q, flags = _route_data("tile_k10")
    rng = np.random.default_rng(99)
    extra = rng.standard_normal((3000, 512)).astype(np.float32)
    idx = _index("IP", 512, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    _check_search(idx, knn_oracle_lib, gpu, "IP", rows, q, 10, "before")
    removed = idx.remove_ids(np.flatnonzero(flags))
    idx.add_device(_dev(extra, gpu))
    assert idx.ntotal == 20000 - removed + 3000
    both = np.concatenate([rows[~flags], extra])
    assert np.array_equal(_stored(idx, gpu).view(np.uint32), both.view(np.uint32))      # the new rows' ids start at the new ntotal
    _check_search(idx, knn_oracle_lib, gpu, "IP", both, q, 10, "after remove + append")
    assert idx.last_launch()["scan_kind"] == "hi_tile"
    _check_search(idx, knn_oracle_lib, gpu, "IP", both, q[:4], 10, "small batch after remove + append")


def test_rows_of_another_magnitude_appended_after_a_removal_are_noticed(gpu, knn_oracle_lib):
    """60 % of 20 000 rows go, then 12 000 rows scaled by 2^10 come: as many rows as before, and half again the rows the plane's
    decision still stands for -- the tuning must see an append (KnnTuning::rows_removed) and decide the plane again"""
    rows, q, _ = _route_data("tile_k10")
    rng = np.random.default_rng(123)
    gone = rng.choice(20000, 12000, replace=False)
    extra = (rng.standard_normal((12000, 512)) * 1024.0).astype(np.float32)
    idx = _index("L2", 512, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    _check_search(idx, knn_oracle_lib, gpu, "L2", rows, q, 10, "before")
    rebuilds = idx.plane_info()["rebuilds"]
    assert idx.remove_ids(gone) == 12000
    keep = np.ones(20000, bool)
    keep[gone] = False
    _check_search(idx, knn_oracle_lib, gpu, "L2", rows[keep], q, 10, "after the removal")
    assert idx.plane_info()["rebuilds"] == rebuilds
    idx.add_device(_dev(extra, gpu))
    both = np.concatenate([rows[keep], extra])
    qq = np.concatenate([q[:16], (q[16:] * 1024.0).astype(np.float32)])
    _check_search(idx, knn_oracle_lib, gpu, "L2", both, qq, 10, "after the scaled append")
    assert idx.plane_info()["rebuilds"] == rebuilds + 1, idx.plane_info()
    print("certificate after the scaled append:", idx.last_launch()["certificate"])


# ---- exclusion and range searches -------------------------------------------------------------------------------------------------------
def test_exclusion_and_range_searches_after_a_removal(gpu, knn_oracle_lib):
    import torch
    rows, q, flags = _route_data("tile_k10")
    n = len(rows)
    rng = np.random.default_rng(321)
    tags = (100 + np.arange(n) % 125).astype(np.int64)
    idx = _index("IP", 512, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    _check_search(idx, knn_oracle_lib, gpu, "IP", rows, q, 10, "before")
    removed, omap = idx.remove_ids(np.flatnonzero(flags), return_map=True)
    # the caller's own column, compacted through old_to_new on the device
    tags_old = _dev(tags, gpu)
    tags_new = torch.empty((n - removed,), dtype=torch.int64, device=gpu)
    alive = omap >= 0
    tags_new[omap[alive]] = tags_old[alive]
    kept, tags_kept = rows[~flags], tags[~flags]
    assert np.array_equal(tags_new.cpu().numpy(), tags_kept)
    qd = _dev(q, gpu)
    excl = np.sort(100 + rng.choice(125, 60, replace=False)).astype(np.int64)
    D, I = idx.search_excluding_in_scan(qd, 10, tags_new, _dev(excl, gpu))
    ed, ei = E.expected_excluding(kept, tags_kept, excl, q, 10, "IP")
    assert idx.last_excl_scan()["route"] == "tile"
    assert np.array_equal(I.cpu().numpy(), ei) and (np.abs(D.cpu().numpy() - ed) <= 1e-6 + 1e-6 * np.abs(ed)).all()
    qtags = np.stack([100 + rng.choice(125, 8, replace=False) for _ in range(len(q))]).astype(np.int64)
    D, I = idx.search_excluding_per_query(qd, 10, tags_new, _dev(qtags, gpu))
    ed, ei = P.expected_pq(kept, tags_kept, qtags, None, q, 10, "IP")
    assert np.array_equal(I.cpu().numpy(), ei) and (np.abs(D.cpu().numpy() - ed) <= 1e-6 + 1e-6 * np.abs(ed)).all()
    radius, cap = 62.0, 128
    counts, D, I, K64 = idx.range_search_device(qd, radius, cap, return_f64=True)
    ec, ei, ek, boundary = RG.expected_range(kept, q, radius, "IP", cap)
    assert not boundary.any() and 0 < ec.max() <= cap and ec.sum() > 100
    assert np.array_equal(counts.cpu().numpy(), ec) and np.array_equal(I.cpu().numpy(), ei)
    f = ei >= 0
    assert np.allclose(K64.cpu().numpy()[f], ek[f], rtol=1e-9, atol=0) and np.isnan(K64.cpu().numpy()[~f]).all()


# ---- remove everything; snapshot; state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_remove_everything(gpu, knn_oracle_lib, metric):
    rng = np.random.default_rng(8)
    base = 10 ** 9 if metric == "L2" else 0
    rows = rng.standard_normal((20000, 512)).astype(np.float32)
    q = rng.standard_normal((32, 512)).astype(np.float32)
    idx = _index(metric, 512, id_base=base, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    _check_search(idx, knn_oracle_lib, gpu, metric, _stored(idx, gpu), q, 5, "before")
    assert idx.remove_ids(base + np.arange(20000)) == 20000 and idx.ntotal == 0
    fresh = _index(metric, 512, id_base=base)
    for handle in (idx, fresh):                              # the emptied handle answers as a new empty one does
        D, I = handle.search_device(_dev(q, gpu), 5)
        assert (I.cpu().numpy() == -1).all() and not np.isfinite(D.cpu().numpy()).any()
    again = rng.standard_normal((20000, 512)).astype(np.float32)
    idx.add_device(_dev(again, gpu))
    assert idx.ntotal == 20000
    stored = _stored(idx, gpu)                               # ids restart at id_base
    if metric == "L2":
        assert np.array_equal(stored, again)
    _check_search(idx, knn_oracle_lib, gpu, metric, stored, q, 5, "after the store was emptied and filled again")
    assert idx.last_launch()["scan_kind"] == "hi_tile"


def test_snapshot_after_a_removal(gpu, knn_oracle_lib, tmp_path):
    rows, q, flags = _route_data("dense")
    idx = _index("L2", 64, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    idx.remove_ids(np.flatnonzero(flags))
    path = str(tmp_path / "after_removal.knn")
    idx.save(path)
    other = _index("L2", 64)
    other.load(path)
    assert other.ntotal == idx.ntotal == int((~flags).sum())
    assert np.array_equal(_stored(other, gpu).view(np.uint32), rows[~flags].view(np.uint32))
    a, b = idx.search_device(_dev(q, gpu), 10), other.search_device(_dev(q, gpu), 10)
    assert np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy()) and np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())
    _check_search(other, knn_oracle_lib, gpu, "L2", rows[~flags], q, 10, "the loaded snapshot")


@pytest.mark.parametrize("end", ["finish", "abort"])
def test_a_pending_search_refuses_the_removal(gpu, knn_oracle_lib, end):
    rows, q, flags = _route_data("dense")
    idx = _index("L2", 64, remove_stage_rows=S_MIN)
    idx.add_device(_dev(rows, gpu))
    idx.search_begin(_dev(q, gpu), 10)
    with pytest.raises(ValueError, match="begun search"):
        idx.remove_ids([1, 2, 3])
    assert idx.ntotal == len(rows)
    if end == "finish":
        D, I = idx.search_finish(None)
        _, ei = _oracle(knn_oracle_lib, gpu, "L2", rows, q, 10)
        assert np.array_equal(I.cpu().numpy(), ei)
    else:
        idx.search_abort()
    assert np.array_equal(_stored(idx, gpu), rows)                       # the store is unchanged ...
    assert idx.remove_ids(np.flatnonzero(flags)) == int(flags.sum())     # ... and a later removal succeeds
    _check_search(idx, knn_oracle_lib, gpu, "L2", rows[~flags], q, 10, "after the refused and the accepted removal")


# ---- the shell --------------------------------------------------------------------------------------------------------------------------
def _pipeline(gpu, tmp_path, index_type="L2"):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, feature_dim=32, tpp_levels=[1, 2], top_k=5, vector_db_index_type=index_type,
               vector_db_path=str(tmp_path / ("vdb_" + index_type)), knn_remove_stage_rows=S_MIN)

    class NoExtractor:
        feature_dim = 32

        def extract_features(self, segments):
            raise AssertionError("not used")
    if index_type == "IVF":
        cfg.ivf_nlist = 64
    return R.HotPathPipeline(cfg, feature_extractor=NoExtractor()), cfg


def test_remove_files_through_the_shell(gpu, tmp_path):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    pipe, cfg = _pipeline(gpu, tmp_path)
    vdb = pipe.vector_db
    D = pipe.tpp.get_output_dim()
    rng = np.random.default_rng(17)
    n = 3000
    db = rng.standard_normal((n, D)).astype(np.float32)
    paths = [f"/train/f{i}.wav" for i in range(n)]
    paths[700] = "/train/copies/f5.wav"                       # two rows share the basename f5.wav
    labels = [i % 2 for i in range(n)]
    vdb.add_vectors(db, paths, labels, {"speaker_id": [f"s{i % 40}" for i in range(n)]})
    pipe.training_file_ids.update(os.path.basename(p) for p in paths)
    assert vdb.index.options["remove_stage_rows"] == S_MIN
    tags0 = vdb.row_tags_device().cpu().numpy()
    gone = ["/somewhere/else/f5.wav", "f1234.wav", "/train/f2999.wav", "no_such_file.wav"]
    assert pipe.remove_files(gone) == 4
    keep = np.ones(n, bool)
    keep[[5, 700, 1234, 2999]] = False
    assert vdb.index.ntotal == n - 4 == len(vdb.vector_paths) == len(vdb.vector_labels) == len(vdb.vector_metadata["speaker_id"])
    assert vdb.vector_paths == [p for p, k_ in zip(paths, keep) if k_]
    assert vdb.vector_labels == [l for l, k_ in zip(labels, keep) if k_]
    assert vdb.vector_metadata["speaker_id"] == [f"s{i % 40}" for i in range(n) if keep[i]]
    assert not ({"f5.wav", "f1234.wav", "f2999.wav"} & pipe.training_file_ids) and "f6.wav" in pipe.training_file_ids
    assert np.array_equal(vdb.row_tags_device().cpu().numpy(), tags0[keep])
    assert np.array_equal(_stored(vdb.index, gpu), db[keep])
    # the removed rows themselves as queries: none of their paths comes back, and the hits are the kept rows' own neighbours
    q = _dev(db[[5, 700, 1234, 2999]], gpu)
    vec, lbl, rp = pipe.retrieve_similar_vectors(q, query_paths=None, exclude_self=False, return_info=True)
    names = {os.path.basename(p) for row in rp for p in row}
    assert names and not (names & {"f5.wav", "f1234.wav", "f2999.wav"})
    # remove m rows, add m others: the cached device columns have the old length and must not be served
    m_paths = [f"/new/g{i}.wav" for i in range(4)]
    vdb.add_vectors(rng.standard_normal((4, D)).astype(np.float32), m_paths, [1, 1, 0, 0], {"speaker_id": ["t"] * 4})
    assert len(vdb.vector_paths) == n
    assert np.array_equal(vdb.row_tags_device().cpu().numpy(), np.array([path_tag(p) for p in vdb.vector_paths], np.int64))
    assert np.array_equal(vdb.labels_device().cpu().numpy(), np.array(vdb.vector_labels, np.float32))
    # remove_vectors by id, with ids that name nothing
    assert vdb.remove_vectors([0, 0, -3, 10 ** 7, n - 1]) == 2
    assert vdb.vector_paths[0] == "/train/f1.wav" and vdb.vector_paths[-1] == "/new/g2.wav" and vdb.index.ntotal == n - 2
    assert np.array_equal(vdb.row_tags_device().cpu().numpy(), np.array([path_tag(p) for p in vdb.vector_paths], np.int64))


def test_an_ivf_store_refuses_and_stays_as_it_was(gpu, tmp_path):
    pipe, cfg = _pipeline(gpu, tmp_path, index_type="IVF")
    vdb = pipe.vector_db
    D = pipe.tpp.get_output_dim()
    rng = np.random.default_rng(18)
    n = 4096
    db = rng.standard_normal((n, D)).astype(np.float32)
    paths = [f"/train/f{i}.wav" for i in range(n)]
    vdb.add_vectors(db, paths, [0] * n, {})
    pipe.training_file_ids.update(os.path.basename(p) for p in paths)
    q = _dev(db[:8], gpu)
    d0, i0 = vdb.search_batch(q, k=5)
    for call in (lambda: vdb.index.remove_ids([1, 2]), lambda: vdb.remove_vectors([1, 2]), lambda: vdb.remove_files(["f7.wav"]),
                 lambda: vdb.remove_files(["no_such.wav"]), lambda: pipe.remove_files(["f7.wav"])):
        with pytest.raises(ValueError, match="rebuild"):
            call()
    assert vdb.index.ntotal == n and len(vdb.vector_paths) == n and "f7.wav" in pipe.training_file_ids
    d1, i1 = vdb.search_batch(q, k=5)
    assert np.array_equal(i0.cpu().numpy(), i1.cpu().numpy()) and np.array_equal(d0.cpu().numpy(), d1.cpu().numpy())
