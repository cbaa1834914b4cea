"""The row tail of a deferring launch (csrc/knn_hi.inc, k_knn_hi_rowtail): the listed rows scored in 16-row groups by every CU instead of
256-row tiles.  Stores, helpers and the check of tests/test_gpu_knn_abandon_defer.py -- EVERYTHING array_equal to the same search with
the option off (ids, distances, float64 keys, emitted counts, floors, certificate, abandon counters), ids equal to the float64 oracle --
on what the group form can newly get wrong: list lengths around a group, an empty list beside a filled one, row widths of one stage
(which never defers), four K steps, one step pair more than a register block (16 steps = 512 elements) and two blocks plus one, the widest row, more groups than workgroups,
nearly empty query blocks and query tiles, a candidate buffer that overflows in the tail, two phases, determinism.

A tile of P <= 16 planted near-duplicates defers P rows; a tile of 17 stays (test_mixed of the deferral's tests).  The sample pre-pass
reads tiles 0, 9, ..., 63 of a 20 000-row store and the floor is its 16th best score, so the cases that list only a few rows plant 17
rows in tiles 0 and 9 as well: those tiles are scanned in full and the floor clears every random row."""
import numpy as np
import pytest

from test_gpu_knn_abandon_defer import K, MAX_ROWS, N0, _Index, _dev, _every_third, _planted, _qtiles

pytestmark = pytest.mark.gpu

FLOOR_TILES = {0: MAX_ROWS + 1, 9: MAX_ROWS + 1}       # sample tiles that stay: 34 rows above every random one


def _own_duplicates(n, dim, nq, seed, tiles, sample_stride):
    """A store whose planted tiles defer 16 rows each without crowding any candidate buffer or certificate: the queries are 0.08 off a
    common direction b; the first two planted rows of every SAMPLE tile (every sample_stride-th tile, 64 of them) are 0.005 off b --
    every floor comes from those 128 rows, cos 0.9968 -- and every other planted row is a near-duplicate of ONE query, 0.01 ... 0.03 off
    it: >= 0.9995 to its own query (emitted, and alive at the checkpoint because of it), 0.9934 to the others (below their floors)."""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.08 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    tiles = np.asarray(tiles)
    where = (tiles[:, None] * 256 + 3 + 15 * np.arange(MAX_ROWS)[None, :]).reshape(-1)
    off = rng.uniform(0.01, 0.03, len(where))[:, None]
    own = q[np.arange(len(where)) % nq] + (off * amp * rng.standard_normal((len(where), dim))).astype(np.float32)
    common = (base[None, :] + 0.005 * amp * rng.standard_normal((len(where), dim))).astype(np.float32)
    in_sample = (tiles % sample_stride == 0) & (tiles // sample_stride < 64)
    is_common = (in_sample[:, None] & (np.arange(MAX_ROWS)[None, :] < 2)).reshape(-1)
    db[where] = np.where(is_common[:, None], common, own)
    return db, q, where


@pytest.mark.parametrize("name,lists", [("1", {3: 1}), ("15", {3: 15}), ("16", {3: 16}), ("16+1", {3: 16, 6: 1}), ("2x16+1", {3: 16, 6: 16, 12: 1})])
@pytest.mark.parametrize("nq", [40, 300])
def test_list_lengths_around_a_group(gpu, knn_oracle_lib, name, lists, nq):
    """lists of 1, 15, 16, 17 and 33 entries per query tile: one partly filled group, one full, a full one and a single entry, two and one"""
    db, q, _ = _planted(N0, 128, nq, 100 + sum(lists.values()) + nq, {**FLOOR_TILES, **lists})
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    df = on["defer"]
    assert df["tile_tasks_deferred"] == len(lists) * _qtiles(nq) and df["rows_listed"] == sum(lists.values()) * _qtiles(nq) and df["tail_launches"] == 1, df


def test_one_list_empty(gpu, knn_oracle_lib):
    """300 queries, a NaN query in the second query tile: that tile lists nothing (every comparison with its floor fails), the first
    lists 26 x 8 rows -- the workgroups of the second leave at the count, the first's results are what they are without it"""
    dim, nq = 128, 300
    db, q, _ = _planted(N0, dim, nq, 151, _every_third(8))
    q[270, 5] = np.nan
    ordinary = np.ones(nq, bool)
    ordinary[270] = False
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q, oracle_rows=ordinary)
    assert on["defer"]["tile_tasks_deferred"] == 26 and on["defer"]["rows_listed"] == 26 * 8, on["defer"]


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim", [64, 128, 1088, 2112])
def test_widths(gpu, knn_oracle_lib, dim, metric):
    """dim 64: two 32-element MFMA steps, ONE stage of the scan -- the abandon has no checkpoint there (knn_abandon_checkpoint returns 0),
    so no launch of that width defers and the row tail never sees it: the case pins that, and that the search is the option-off one.
    The narrowest rows that reach the row tail are dim 128 = 4 steps (no whole register block: the rest-of-row path alone); 1088 = 34
    steps: two blocks of 16 and a rest of 2; 2112 = 66: four and 2.  Every width >= 128 must list rows, cosine (RSC 0) and L2 (RSC 3).
    (300 queries: with one query tile a 79-tile store of rows >= 1024 wide is K-split, and a K-split launch neither abandons nor defers.)"""
    db, q, _ = _planted(N0, dim, 300, 200 + dim, _every_third(8))
    s = _Index(gpu, knn_oracle_lib, metric, db)
    on = s.search(q)
    ab, df = on["abandon"], on["defer"]
    assert df["tile_tasks_deferred"] <= ab["checked"] - ab["skipped"] and df["rows_listed"] <= MAX_ROWS * df["tile_tasks_deferred"], (ab, df)
    if dim == 64:
        assert ab["checked"] == 0 and df["rows_listed"] == 0, (ab, df)
    elif metric == "COSINE":
        # the designed number: the 26 planted tiles x 2 query tiles, kept alive by exactly their 8 planted rows
        assert ab["checked"] == ab["tasks"] and df["tile_tasks_deferred"] == 26 * 2 and df["rows_listed"] == 26 * 8 * 2, (ab, df)
    else:
        # raw L2 rows: |y|^2 varies from tile to tile, the tile-side gate stays shut for some tiles, and a tile WITHOUT planted rows may
        # be kept alive by one or two random rows and defer those: no designed number.  A deferred task lists 1 ... 16 rows, and at
        # least one tile task must defer (a run that lists nothing does not run the kernel under test)
        assert s.idx.plane_info()["one_scale"]
        assert df["tile_tasks_deferred"] > 0 and df["rows_listed"] >= df["tile_tasks_deferred"], (ab, df)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim", [4096, 16320])
def test_the_widest_rows(gpu, knn_oracle_lib, metric, dim):
    """dim 16 320 = 510 steps, the widest multiple of 64 a store takes (31 register blocks and a rest of 14), and 4096 = 128 steps (8
    blocks, no rest).  64 row tiles (the fewest the tile scan takes) and 3 query tiles (with fewer the launch is K-split: 64 x 2 <= 128
    workgroups).  Built on the device; the float64 oracle checks the first 8 queries.  Launches of both widths defer, cosine and L2:
    the 32 planted tiles x 3 query tiles list their 8 planted rows each."""
    import torch
    n, nq = 16384, 513
    g = torch.Generator(device=gpu).manual_seed(7)
    rows = torch.randn((n, dim), device=gpu, generator=g)
    base = torch.randn(dim, device=gpu, generator=g)
    q = base[None, :] + 0.05 * torch.randn((nq, dim), device=gpu, generator=g)
    # (every second tile: all 8 tiles of the sample -- 0, 8, ..., 56 -- are among them, and a sample tile keeps the best two scores of each
    # of its 8 row holders: 4 of a tile's 8 planted rows, 32 in all for the floor's rank 16)
    ids = torch.tensor([t * 256 + 3 + 15 * i for t in range(0, 64, 2) for i in range(8)], device=gpu)
    rows[ids] = q[torch.arange(len(ids), device=gpu) % nq] + 0.03 * torch.randn((len(ids), dim), device=gpu, generator=g)

    class _OnDevice(_Index):
        def __init__(self, gpu, lib, metric, rows_t):
            from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
            self.gpu, self.lib, self.metric = gpu, lib, metric
            self.idx = HipFlatIndex(rows_t.shape[1], {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric], 0)
            self.idx.add_device(rows_t)
            self.stored = self.idx.reconstruct_batch(torch.arange(0, n, device=gpu)).cpu().numpy()

    s = _OnDevice(gpu, knn_oracle_lib, metric, rows)
    del rows
    first = np.zeros(nq, bool)
    first[:8] = True
    on = s.search(q.cpu().numpy(), oracle_rows=first)
    ab, df = on["abandon"], on["defer"]
    assert ab["checked"] == ab["tasks"] == 64 * 3, ab
    assert df["tile_tasks_deferred"] == 32 * 3 and df["rows_listed"] == 32 * 8 * 3, (ab, df)


def test_a_long_list_takes_the_tile_tail(gpu, knn_oracle_lib):
    """a list longer than KNN_ROWTAIL_MAX_ENTRIES = 4096 is left by the row tail and scored by the tile tail (k_knn_hi_tail): 160 000 rows =
    625 tiles, every one defers 16 rows, one launch, one query tile: 10 000 entries (_own_duplicates: 50 candidates of its own per
    query, the sample's tiles are every 9th)."""
    n, dim, nq = 160000, 128, 200
    db, q, where = _own_duplicates(n, dim, nq, 501, np.arange(n // 256), 9)
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    print(f"long list: launches {on['launch']['scan_launches']}, defer {on['defer']}, emitted max {on['counts'].max()}")
    assert on["counts"].max() < 1024, on["counts"].max()
    assert on["defer"]["rows_listed"] == len(where) and len(where) > 4096 * on["launch"]["scan_launches"], (on["defer"], on["launch"]["scan_launches"])


def test_more_groups_than_workgroups(gpu, knn_oracle_lib):
    """every whole tile of the store defers 16 rows: 78 x 16 = 1248 entries = 78 groups per query tile; with 8 query tiles the grid has
    2 x CUs / 8 workgroups per query tile in eights (64 on 256 CUs: tests/knn_row_tail_plan_check.cpp), so the persistent loop takes a
    second round.  (1248 rows near EVERY query would overflow every candidate buffer and the handle would widen them between the two
    searches.  So the sample's tiles hold 16 rows near the queries' common direction b -- every floor comes from them: cos(q_j, b) =
    0.9968 with the queries 0.08 off b -- and the other tiles 16 near-duplicates of one query each, 0.02 off it: 0.9998 to their own
    query, 0.9934 to everybody else -- below the floor, never emitted -- and alive at the checkpoint of dim 512 for EVERY query tile:
    the bound there is the score plus 7/8 (1 - cos) = 0.9992 > 0.9968.  Random rows: 0.875 + ~0.1.)  The oracle checks every 16th query."""
    nq, dim = 1800, 512
    tiles = N0 // 256
    rng = np.random.default_rng(301)
    db = rng.standard_normal((N0, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.08 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    for t in range(tiles):
        ids = t * 256 + 3 + 15 * np.arange(MAX_ROWS)
        if t % 9 == 0 and t < 64:
            db[ids] = (base[None, :] + 0.005 * amp * rng.standard_normal((MAX_ROWS, dim))).astype(np.float32)
        else:
            db[ids] = q[(t * MAX_ROWS + np.arange(MAX_ROWS)) % nq] + (0.02 * amp * rng.standard_normal((MAX_ROWS, dim))).astype(np.float32)
    some = np.zeros(nq, bool)
    some[::16] = True
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q, oracle_rows=some)
    assert _qtiles(nq) == 8 and on["launch"]["query_tiles"] == 8, on["launch"]
    assert on["counts"].max() < 1024, on["counts"].max()
    assert on["defer"]["tile_tasks_deferred"] == tiles * 8 and on["defer"]["rows_listed"] == tiles * MAX_ROWS * 8, on["defer"]


@pytest.mark.parametrize("nq", [17, 257])
def test_nearly_empty_query_blocks_and_tiles(gpu, knn_oracle_lib, nq):
    """17 queries: the second 16-query block of wave 0 holds one query, waves 1-3 none; 257: the second query tile holds one.  A slot past
    nq never emits: the real queries' counts are the option-off run's (search() compares them)"""
    db, q, _ = _planted(N0, 128, nq, 400 + nq, _every_third(16))
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["defer"]["tile_tasks_deferred"] == 26 * _qtiles(nq) and on["defer"]["rows_listed"] == 26 * 16 * _qtiles(nq), on["defer"]
    assert len(on["counts"]) == nq and (on["counts"] > 0).all()


def test_candidate_overflow_in_the_tail(gpu, knn_oracle_lib):
    """One query's candidate buffer overflows from rows only the tail scores.  (A floor of -inf cannot do it: such a query keeps every
    row of every tile alive and its query tile defers nothing.)  Query X is 0.3 of a noise vector off the others' common direction.  The
    sample's tiles hold 16 rows near the COMMON direction -- everybody's floor comes from them, X's is ~0.96, the others' ~0.998 -- and
    the 70 other whole tiles hold 16 near-duplicates of X each: 1120 rows above X's floor and below everybody else's, alive at the
    checkpoint because of X alone, listed, and scored by the tail: X's count passes the buffer's 1024 entries, X is rejected and answered
    by the exact pass; its neighbours' buffers lie right behind its own and their candidates, counts and ids are what they are with the
    option off, and the oracle's."""
    dim, nq, x = 128, 40, 20
    rng = np.random.default_rng(77)
    db = rng.standard_normal((N0, dim)).astype(np.float32)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = (base[None, :] + 0.05 * amp * rng.standard_normal((nq, dim))).astype(np.float32)
    q[x] = (base + 0.3 * amp * rng.standard_normal(dim)).astype(np.float32)
    sample_tiles = list(range(0, 64, 9))
    for t in range(N0 // 256):
        ids = t * 256 + 3 + 15 * np.arange(MAX_ROWS)
        centre = base if t in sample_tiles else q[x].astype(np.float64)
        db[ids] = (centre[None, :] + 0.03 * amp * rng.standard_normal((MAX_ROWS, dim))).astype(np.float32)
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    on = s.search(q)
    cap = 1024             # knn_finish_plan: emit_cap = max(1024 cap_boost, 32 (k + 6)), cap_boost 1 on a handle nothing has widened
    print(f"overflow: counts[x] {on['counts'][x]}, other counts max {np.delete(on['counts'], x).max()}, rechecked {on['launch']['rechecked_queries']}, defer {on['defer']}")
    assert on["defer"]["rows_listed"] >= (N0 // 256 - len(sample_tiles)) * MAX_ROWS, on["defer"]
    assert on["counts"][x] > cap and np.delete(on["counts"], x).max() < cap, on["counts"]
    assert on["launch"]["rechecked_queries"] >= 1, on["launch"]
    # the neighbours, directly: X's buffer is [x cap, (x + 1) cap), query x + 1's begins right behind it
    s.idx.set_abandon_defer(0)
    off = s.observe(_dev(q, gpu))
    s.idx.set_abandon_defer(1)
    for j in (x - 1, x + 1):
        assert on["counts"][j] == off["counts"][j] and 0 < on["counts"][j] < cap, (j, on["counts"][j], off["counts"][j])
        for name in ("I", "D", "K64"):
            assert np.array_equal(on[name][j], off[name][j]), (name, j)


def test_two_phases(gpu, knn_oracle_lib):
    """(the deferral's two-phase store size, 16 rows in every 6th tile: _own_duplicates, the sample's tiles are every 24th.)  Both launches
    list rows, each tail runs in front of the floors raised after phase 0: they equal the option-off run's (search() compares floors
    and counts).  The second launch's capacity is past the row tail's share, so both tail kernels are launched there and the tile tail
    leaves the short list alone."""
    n, dim, nq = 400000, 128, 200
    db, q, where = _own_duplicates(n, dim, nq, 5, np.arange(0, n // 256, 6), 24)
    on = _Index(gpu, knn_oracle_lib, "COSINE", db).search(q)
    assert on["launch"]["scan_launches"] == 2 and on["defer"]["tail_launches"] == 2, (on["launch"], on["defer"])
    assert on["counts"].max() < 1024 and on["defer"]["rows_listed"] == len(where), (on["counts"].max(), on["defer"])


def test_determinism(gpu, knn_oracle_lib):
    db, q, _ = _planted(N0, 512, 300, 181, _every_third(16))
    s = _Index(gpu, knn_oracle_lib, "COSINE", db)
    first = s.search(q)
    assert first["defer"]["rows_listed"] == 26 * 16 * 2, first["defer"]
    qt = _dev(q, gpu)
    for _ in range(2):
        again = s.observe(qt)
        for name in ("I", "D", "K64", "counts", "floors"):
            assert np.array_equal(again[name], first[name]), name
        assert again["defer"] == first["defer"] and again["abandon"] == first["abandon"] and again["certificate"] == first["certificate"]
