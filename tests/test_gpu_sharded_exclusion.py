"""Exclusion-aware search over row shards (radad_knn_search_excl_begin / _finish, radad_excl_merge_certify,
ShardedSearch.search_excluding): the exact top k of the WHOLE store among the rows whose tag is not excluded, with one certificate
across the shards, so that the exact pass runs only for queries nobody can prove.

One process, G = 2 or 3 handles with id_base on one device, the exchange done by torch.stack; then two processes on one GPU through
ShardedSearch itself.  Reference: expected_excluding (tests/exclusion_ref.py) over the rows AS STORED; the `unproved` vector is that
of the numpy model (tests/sharded_excl_ref.py, checked on the CPU by tests/test_sharded_excl_model.py) and is asserted with
equality: both sides rank by exact float64 keys, ties to the lower id.  Distances and keys: as tests/test_gpu_knn_exclusion.py
(1e-4 absolute on unit-norm data, 1e-6 on raw L2; out_dist is the key rounded once).  Shapes: the smallest that reach each scan path
at dim 64 -- 2 x 20 000 rows with 48 queries (certified f16 tile scan), 3 x 1 000 rows with 5 queries (small batch), 2 x 5 000 rows
with 40 queries (fp32 rows: at dim 64 a store of <= 6144 rows takes the dense fp32 kernel, so one case at dim 36 and 2 x 20 000 rows
reaches the fp32 tile kernel as well)."""
import functools
import os
import socket
import sys
import time

import numpy as np
import pytest

import sharded_excl_ref as M
from exclusion_ref import crowded, expected_exact, expected_excluding

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@functools.lru_cache(maxsize=None)
def _store(name):
    """(db, q, tags, excl, info, sizes) of the stores below, built once"""
    if name == "a":
        sizes = [20000, 20000]
        return M.store_a(sizes, 64, 48, 12, 30, 9110) + (sizes,)
    if name == "b":
        sizes = [5000, 5000]
        return M.store_b(sizes, 64, 40, 5, 9120) + (sizes,)
    if name == "c":
        sizes = [1000, 8, 300]
        return M.store_c(sizes, 64, 5, 9130) + (sizes,)
    if name == "d":
        sizes = [1000, 1000, 1000]
        return M.store_d(sizes, 64, 5, 9140) + (sizes,)
    if name == "crowded_small":                              # 60 excluded duplicates in front of 3 of the 5 queries, all in shard 0
        sizes = [1000, 1000, 1000]
        return M.store_a(sizes, 64, 5, 3, 60, 9150) + (sizes,)
    if name == "crowded_tile":                               # dim 36: no f16 plane, and too many rows for the dense kernel
        return crowded(40000, 36, 40, 8, 30, 9170) + ([20000, 20000],)
    if name == "crowded_f32":                                # 150 in front of 4 of the 40
        return crowded(10000, 64, 40, 4, 150, 9160) + ([5000, 5000],)
    raise KeyError(name)


class _Shards:
    """G handles with id_base on one device, their rows as stored, tags and exclusion set"""

    def __init__(self, gpu, metric, db, q, tags, excl, sizes, f16=False):
        import torch
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
        self.metric, self.q, self.tags, self.excl, self.gpu, self.sizes = metric, q, np.asarray(tags, np.int64), excl, gpu, sizes
        self.m = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric]
        self.b = M.bases_of(sizes)
        self.idx, self.tags_t, stored = [], [], []
        for g in range(len(sizes)):
            lo, hi = int(self.b[g]), int(self.b[g + 1])
            ix = HipFlatIndex(db.shape[1], self.m, 0, lo, store_f16=f16)
            ix.add(db[lo:hi])
            stored.append(ix.reconstruct_batch(torch.arange(lo, hi, device=gpu)).cpu().numpy())
            self.idx.append(ix)
            self.tags_t.append(_dev(self.tags[lo:hi], gpu))
        self.stored = np.concatenate(stored)
        self.excl_t = None if excl is None or len(excl) == 0 else _dev(np.asarray(excl, np.int64), gpu)
        self.qt = _dev(q, gpu)

    def run(self, k, k_fetch):
        """begin on every shard, certificate, finish / abort, merge; compare ids, distances, keys and the unproved vector with the
        references -> (unproved [nq], [last_excl()["exact"] per shard])"""
        import torch
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
        from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge
        begun = [ix.search_excluding_begin(self.qt, k, t, self.excl_t, k_fetch) for ix, t in zip(self.idx, self.tags_t)]
        K, I, FK, FI = (torch.stack([x[c] for x in begun]) for c in range(4))
        D, Im, K64, U = HipFlatIndex.excl_merge_certify(self.m, K, I, FK, FI)
        unproved = U.cpu().numpy()
        # the model's begin, per shard, on the rows as stored
        for g, ix in enumerate(self.idx):
            lo, hi = int(self.b[g]), int(self.b[g + 1])
            mk, mi, mfk, mfi = M.shard_begin(self.stored[lo:hi], self.tags[lo:hi], self.excl, self.q, k, k_fetch, self.metric, lo)
            np.testing.assert_array_equal(I[g].cpu().numpy(), mi)
            # the frontier: which case applies is exact; its id is compared where it is one of the survivors.  A frontier that is the
            # last of the k_fetch hits may be one of many excluded near-duplicates whose float64 keys lie closer together than the
            # fp32 rounding of a cosine store's row norms (the oracle normalises the stored rows again): there the KEY is compared,
            # with the tolerance of the distances
            fi, fk = FI[g].cpu().numpy(), FK[g].cpu().numpy()
            np.testing.assert_array_equal(fi < 0, mfi < 0)
            full = mi[:, -1] >= 0
            np.testing.assert_array_equal(fi[full], mi[full, -1])
            assert np.all((fi[fi >= 0] >= lo) & (fi[fi >= 0] < hi))
            assert np.all(np.isnan(fk[mfi < 0]))
            tol = dict(rtol=0, atol=1e-4) if self.metric == "COSINE" else dict(rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(fk[mfi >= 0], mfk[mfi >= 0], **tol)
        _, _, want = M.sharded_search_excluding(self.stored, self.tags, self.excl, self.q, k, k_fetch, self.metric, self.sizes)
        print(f"unproved {int(unproved.sum())} of {len(unproved)} (model {int(want.sum())}), scans "
              f"{[ix.last_launch()['scan_kind'] for ix in self.idx]}")
        np.testing.assert_array_equal(unproved, want)
        if unproved.any():
            done = [ix.search_excluding_finish(U, return_f64=True) for ix in self.idx]
            K2, I2 = torch.stack([x[2] for x in done]), torch.stack([x[1] for x in done])
            D, Im = hip_merge(self.m, K2, I2, k)
            D = D.masked_fill(Im < 0, float("nan"))
            K64 = None
        else:
            for ix in self.idx:
                ix.search_abort()
        exact = [ix.last_excl() for ix in self.idx]
        assert all(e["queries"] == len(self.q) for e in exact), exact
        ed, ei = expected_excluding(self.stored, self.tags, self.excl, self.q, k, self.metric)
        Dn, In = D.cpu().numpy(), Im.cpu().numpy()
        np.testing.assert_array_equal(In, ei)
        f = ei >= 0
        if self.metric == "COSINE":
            np.testing.assert_allclose(Dn[f], ed[f], rtol=0, atol=1e-4)
        else:
            np.testing.assert_allclose(Dn[f], ed[f], rtol=1e-6, atol=1e-6)
        assert np.all(np.isnan(Dn[~f]))
        if K64 is not None:
            Kn = K64.cpu().numpy()
            assert np.all(np.isnan(Kn[~f]))
            np.testing.assert_array_equal(Kn[f].astype(np.float32), Dn[f])          # out_dist is the key, rounded once
        return unproved, [e["exact"] for e in exact]


# ---- (a) crowding duplicates all in one shard: those queries are unproved ------------------------------------------------------------
@pytest.mark.parametrize("metric,f16", [("L2", False), ("COSINE", False), ("L2", True)])
def test_a_duplicates_in_one_shard(gpu, metric, f16):
    db, q, tags, excl, which, sizes = _store("a")
    rows = np.flatnonzero(np.isin(tags, excl))
    assert rows.max() < sizes[0] and len(rows) == 12 * 30
    s = _Shards(gpu, metric, db, q, tags, excl, sizes, f16=f16)
    unproved, exact = s.run(5, 15)
    assert np.all(unproved[which] == 1)
    if not f16:
        assert [ix.last_launch()["scan_kind"] for ix in s.idx] == ["hi_tile", "hi_tile"]
    # shard 1 holds 5 survivors for every query: its lists already are its exact admissible top 5 and it lists nobody
    assert exact[0] >= 12 and exact[1] == 0, exact


# ---- (b) one shard mostly excluded, the other holds the neighbours: the global certificate lists nobody -----------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_b_one_shard_mostly_excluded(gpu, metric):
    db, q, tags, excl, planted, sizes = _store("b")
    gone = np.isin(tags, excl)
    assert 0.89 < gone[:5000].mean() <= 0.9 and not gone[5000:].any() and planted.min() >= 5000
    s = _Shards(gpu, metric, db, q, tags, excl, sizes)
    alone = int(expected_exact(s.stored[:5000], tags[:5000], excl, q, 5, 15, metric).sum())
    assert alone > 0
    unproved, exact = s.run(5, 15)
    assert unproved.sum() == 0 and exact == [0, 0]
    assert all(ix.last_launch()["scan_kind"].startswith("f32") for ix in s.idx)
    s.idx[0].search_excluding(s.qt, 5, s.tags_t[0], s.excl_t, k_fetch=15)          # the single-handle call on shard 0 alone
    assert s.idx[0].last_excl() == {"queries": 40, "exact": alone}


# ---- (c) a shard smaller than k_fetch, a shard without admissible rows; (d) everything excluded --------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_c_small_shard_and_shard_without_admissible_rows(gpu, metric):
    db, q, tags, excl, gone, sizes = _store("c")
    assert sizes[1] < 15 and gone[1008:].all() and not gone[1000:1008].any()
    s = _Shards(gpu, metric, db, q, tags, excl, sizes)
    s.run(5, 15)
    s.run(10, 15)                                            # more than the small shard's 8 rows: its frontier is "nothing unseen"


def test_d_everything_excluded(gpu):
    db, q, tags, excl, _, sizes = _store("d")
    assert np.isin(tags, excl).all()
    s = _Shards(gpu, "L2", db, q, tags, excl, sizes)
    unproved, exact = s.run(5, 15)
    assert np.all(unproved == 1) and exact == [5, 5, 5]


# ---- nothing excluded: the plain search over the whole store -------------------------------------------------------------------------
def test_no_exclusion(gpu):
    db, q, tags, excl, which, sizes = _store("a")
    s = _Shards(gpu, "L2", db, q, tags, None, sizes)
    unproved, exact = s.run(5, 15)
    assert unproved.sum() == 0 and exact == [0, 0]


# ---- longer lists ----------------------------------------------------------------------------------------------------------------------
def test_k30_small_batch(gpu):
    db, q, tags, excl, which, sizes = _store("crowded_small")
    s = _Shards(gpu, "L2", db, q, tags, excl, sizes)
    unproved, _ = s.run(30, 40)
    assert unproved.sum() >= 1


def test_fp32_tile_kernel(gpu):
    db, q, tags, excl, which, sizes = _store("crowded_tile")
    s = _Shards(gpu, "L2", db, q, tags, excl, sizes)
    s.run(5, 15)
    assert [ix.last_launch()["scan_kind"] for ix in s.idx] == ["f32_tile", "f32_tile"]


def test_k130_fp32_shape(gpu):
    db, q, tags, excl, which, sizes = _store("crowded_f32")
    s = _Shards(gpu, "L2", db, q, tags, excl, sizes)
    unproved, _ = s.run(130, 140)
    assert unproved.sum() >= 1
    assert all(ix.last_launch()["scan_kind"].startswith("f32") for ix in s.idx)


# ---- state rules ------------------------------------------------------------------------------------------------------------------------
def test_state_rules(gpu):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    db, q, tags, excl, which, sizes = _store("crowded_f32")
    s = _Shards(gpu, "L2", db, q, tags, excl, sizes)
    ix, tg = s.idx[0], s.tags_t[0]
    D0, I0 = ix.search_device(s.qt, 5)
    with pytest.raises(ValueError):                                   # _finish without _begin
        ix.search_excluding_finish()
    nq = len(q)
    bufs = [torch.empty((nq, 5), device=gpu, dtype=torch.float32), torch.empty((nq, 5), device=gpu, dtype=torch.int64)]
    with pytest.raises(ValueError):                                   # ... in the library too
        _lib.check(_lib.load().radad_knn_search_excl_finish(ix._h, None, bufs[0].data_ptr(), bufs[1].data_ptr(), None, _lib.stream_ptr(gpu)))
    for bad_k, bad_fetch in ((5, 4), (1025, 1025), (0, 15), (5, 1025)):
        with pytest.raises(ValueError):
            ix.search_excluding_begin(s.qt, bad_k, tg, s.excl_t, bad_fetch)
    empty = HipFlatIndex(64, _lib.METRIC_L2, 0, 0)
    with pytest.raises(ValueError):                                   # an empty store
        empty.search_excluding_begin(s.qt, 5, None, None)
    D1, I1 = ix.search_device(s.qt, 5)                                # the refused calls left no begun search behind
    assert torch.equal(I1, I0) and torch.equal(D1, D0)

    K, I, FK, FI = ix.search_excluding_begin(s.qt, 5, tg, s.excl_t, 15)
    with pytest.raises(ValueError):                                   # a begun search owns the handle
        ix.search_device(s.qt, 5)
    with pytest.raises(ValueError):
        ix.search_excluding(s.qt, 5, tg, s.excl_t, k_fetch=15)
    with pytest.raises(ValueError):
        ix.search_excluding_begin(s.qt, 5, tg, s.excl_t, 15)
    with pytest.raises(ValueError):
        ix.search_begin(s.qt, 5)
    with pytest.raises(ValueError):
        ix.add(db[:4])
    assert ix.ntotal == sizes[0]
    ix.search_abort()                                                 # abort, then a normal search works
    D1, I1 = ix.search_device(s.qt, 5)
    assert torch.equal(I1, I0) and torch.equal(D1, D0)
    with pytest.raises(ValueError):                                   # the aborted search cannot be finished
        ix.search_excluding_finish()
    ix.search_begin(s.qt, 5)                                          # at most one begun search, of either kind
    with pytest.raises(ValueError):
        ix.search_excluding_begin(s.qt, 5, tg, s.excl_t, 15)
    ix.search_abort()

    # _begin + _finish with the shard's OWN flags is search_excluding, bit for bit
    want = ix.search_excluding(s.qt, 5, tg, s.excl_t, k_fetch=15, return_f64=True)
    n_exact = ix.last_excl()["exact"]
    assert n_exact >= 1
    K, I, FK, FI = ix.search_excluding_begin(s.qt, 5, tg, s.excl_t, 15)
    own = ((I[:, -1] < 0) & (FI >= 0)).to(torch.int32)
    assert int(own.sum()) == n_exact
    assert ix.last_excl() == {"queries": nq, "exact": 0}
    got = ix.search_excluding_finish(own, return_f64=True)
    assert ix.last_excl() == {"queries": nq, "exact": n_exact}
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    # ... and with no flags the rows come through as _begin left them
    K, I, FK, FI = ix.search_excluding_begin(s.qt, 5, tg, s.excl_t, 15)
    D2, I2, K2 = ix.search_excluding_finish(None, return_f64=True)
    assert torch.equal(I2, I) and torch.equal(_bits(K2), _bits(K)) and torch.equal(_bits(D2), _bits(K.float()))


# ---- two processes on one GPU: ShardedSearch.search_excluding itself ----------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, store, metric_name, nq_locals, exchange, out):
    sys.path[:0] = [ROOT, TESTS]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    rccl = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if rccl else 0)
    torch.cuda.set_device(dev)
    if rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    metric = {"L2": _lib.METRIC_L2, "COSINE": _lib.METRIC_COSINE}[metric_name]
    db, q_all, tags, excl, _, sizes = _store(store)
    b = M.bases_of(sizes)
    lo, hi = int(b[rank]), int(b[rank + 1])
    idx = HipFlatIndex(db.shape[1], metric, dev.index, id_base=lo)
    idx.add(db[lo:hi])
    local = idx.reconstruct_batch(torch.arange(lo, hi, device=dev))    # every rank needs the whole store AS STORED for the reference
    local = local if rccl else local.cpu()
    parts = [torch.empty_like(local) for _ in range(world)]            # (the shards of these stores are equal)
    dist.all_gather(parts, local)
    stored = np.concatenate([p.cpu().numpy() for p in parts])
    tags_t = torch.from_numpy(tags[lo:hi]).to(dev)
    s = ShardedSearch(None, metric, uneven=len(set(nq_locals)) > 1, exchange=exchange, excluding=idx.sharded_excluding(tags_t))
    starts = np.concatenate([[0], np.cumsum(nq_locals)])
    sl = slice(int(starts[rank]), int(starts[rank + 1]))
    q = q_all[:int(starts[-1])]
    mine = torch.from_numpy(excl[rank::world].copy()).to(dev)          # every rank excludes a part: the union is what counts
    d, i = s.search_excluding(torch.from_numpy(q[sl]).to(dev), 5, mine, 15)
    ed, ei = expected_excluding(stored, tags, excl, q, 5, metric_name)
    _, _, want = M.sharded_search_excluding(stored, tags, excl, q, 5, 15, metric_name, sizes)
    f = ei[sl] >= 0
    dn = d.cpu().numpy()
    tol = dict(rtol=0, atol=1e-4) if metric_name == "COSINE" else dict(rtol=1e-6, atol=1e-6)
    ok = (np.array_equal(i.cpu().numpy(), ei[sl]) and tuple(d.shape) == (nq_locals[rank], 5) and np.allclose(dn[f], ed[sl][f], **tol)
          and np.all(np.isnan(dn[~f])))
    info = idx.last_excl()
    # nobody unproved: the begun search was given up and no shard entered the exact pass
    n_searched = world * max(nq_locals)                              # (uneven batches are padded to the largest)
    checks = [ok, info["queries"] == n_searched, bool(want.any()) or info["exact"] == 0, store != "b" or not want.any()]
    if not all(checks):
        print(f"rank {rank}: {checks} {info} ids equal {np.array_equal(i.cpu().numpy(), ei[sl])}", flush=True)
    ok = all(checks)
    D1, I1 = idx.search_device(torch.from_numpy(q[sl]).to(dev), 5)     # the handle accepts searches again
    out[rank] = bool(ok and tuple(I1.shape) == (nq_locals[rank], 5))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("store,metric,nq_locals,exchange", [
    ("b", "L2", [20, 20], "all_to_all"),
    ("b", "COSINE", [20, 20], "all_gather"),
    ("crowded_f32", "COSINE", [20, 20], "all_to_all"),
    ("crowded_f32", "L2", [33, 7], "all_gather"),            # query counts differ per rank
])
def test_two_ranks_one_gpu(gpu, store, metric, nq_locals, exchange):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(2, _free_port(), store, metric, nq_locals, exchange, out), nprocs=2, join=False)
    deadline = time.monotonic() + 180                     # a worker that raises ends the join at once; a hung one is killed here
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a worker did not finish")
    assert dict(out) == {0: True, 1: True}
