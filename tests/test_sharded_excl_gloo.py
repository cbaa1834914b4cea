"""CPU, 2 and 4 processes, gloo: the collective structure of ShardedSearch.search_excluding (union of the ranks' exclusion sets,
all-gather of the queries, begin on the shard, exchange of lists + frontiers, certificate, all-gather of the flags, finish, second
exchange, merge), with oracle stand-ins for begin / finish and the numpy model's certificate and merge (tests/sharded_excl_ref.py)
-- the pattern of tests/test_sharded_gloo.py.  The result must be expected_excluding over the WHOLE store with the UNION of the
ranks' exclusion sets.  On the GPU box tests/test_gpu_sharded_exclusion.py runs the same class on HipFlatIndex handles."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(store, world, metric):
    sys.path[:0] = [p for p in (ROOT, TESTS) if p not in sys.path]
    import sharded_excl_ref as M
    from exclusion_ref import crowded
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import shard_bounds
    n, nq_max = 1203, 16
    sizes = [shard_bounds(n, world, r)[1] - shard_bounds(n, world, r)[0] for r in range(world)]
    if store == "crowded":
        db, q, tags, excl, _ = crowded(n, 16, nq_max, 6, 30, 8101)
    elif store == "b":
        db, q, tags, excl, _ = M.store_b(sizes, 16, nq_max, 5, 8102)
    elif store == "d":
        db, q, tags, excl, _ = M.store_d(sizes, 16, nq_max, 8103)
    else:
        raise KeyError(store)
    return db, q, tags, excl, sizes


def _worker(rank, world, port, store, metric, nq_locals, exchange, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    db, q_all, tags, excl, sizes = _data(store, world, metric)
    import sharded_excl_ref as M
    from exclusion_ref import expected_excluding
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    k, k_fetch = 5, 15
    b = M.bases_of(sizes)
    lo, hi = int(b[rank]), int(b[rank + 1])
    shard, stags = db[lo:hi], tags[lo:hi]
    state = {"begun": None, "finished": 0, "aborted": 0, "excl": None}

    def begin(q, kk, ex, kf):                    # oracle stand-in for HipFlatIndex.search_excluding_begin on the shard
        assert state["begun"] is None, "the previous begin on this handle has not been finished"
        ex = ex.numpy()
        assert np.all(np.diff(ex) > 0)                                 # sorted ascending, no duplicates
        state["excl"] = ex
        K, I, FK, FI = M.shard_begin(shard, stags, ex, q.numpy(), kk, kf, metric, lo)
        state["begun"] = (q.numpy(), kk, ex, K, I)
        return tuple(torch.from_numpy(x) for x in (K, I, FK, FI))

    def finish(flags):                           # ... and for search_excluding_finish
        qn, kk, ex, K, I = state["begun"]
        state["begun"] = None
        state["finished"] += 1
        fl = np.zeros(len(qn), np.int32) if flags is None else flags.numpy()
        K, I = M.shard_finish(shard, stags, ex, qn, kk, metric, lo, K, I, fl)
        return torch.from_numpy(K), torch.from_numpy(I)

    def abort():
        state["begun"] = None
        state["aborted"] += 1

    def certify(m, K, I, FK, FI):
        md, mi, un = M.certify(metric, K.numpy(), I.numpy(), FK.numpy(), FI.numpy())
        return torch.from_numpy(md).float(), torch.from_numpy(mi), torch.from_numpy(md), torch.from_numpy(un)

    def merge(m, K, I, kk):
        md, mi = M.merge(metric, K.numpy(), I.numpy(), kk)
        return torch.from_numpy(np.where(mi < 0, np.inf if metric == "L2" else -np.inf, md)), torch.from_numpy(mi)    # (the plain merge's padding)

    uneven = len(set(nq_locals)) > 1
    s = ShardedSearch(None, 0 if metric == "L2" else 1, merge=merge, uneven=uneven, exchange=exchange,
                      excluding=(begin, finish, abort), certify=certify)
    starts = np.concatenate([[0], np.cumsum(nq_locals)])
    sl = slice(int(starts[rank]), int(starts[rank + 1]))
    q = q_all[:int(starts[-1])]
    # the exclusion set is dealt out over the ranks, unevenly, unsorted and with overlaps; one rank may hold none
    holders = [r for r in range(world) if r != 1]
    deal = lambda r: np.concatenate([excl[holders.index(r)::len(holders)], excl[:3]])[::-1].copy()
    mine = deal(rank) if rank != 1 else excl[:0]
    union = np.unique(np.concatenate([deal(r) for r in holders]))
    assert np.array_equal(union, excl)
    d, i = s.search_excluding(torch.from_numpy(q[sl]), k, torch.from_numpy(mine), k_fetch)
    ed, ei = expected_excluding(db, tags, union, q, k, metric)
    _, _, want_unproved = M.sharded_search_excluding(db, tags, union, q, k, k_fetch, metric, sizes)
    f = ei[sl] >= 0
    ok = (np.array_equal(i.numpy(), ei[sl]) and d.shape == (nq_locals[rank], k) and d.dtype == torch.float32
          and np.allclose(d.numpy()[f], ed[sl][f], rtol=1e-6, atol=1e-6) and np.all(np.isnan(d.numpy()[~f]))
          and np.array_equal(state["excl"], union) and state["begun"] is None
          # the exact pass ran on this rank iff SOME rank's query was unproved; otherwise the begun search was given up
          and (state["finished"], state["aborted"]) == ((1, 0) if want_unproved.any() else (0, 1)))
    try:
        s.search_excluding(torch.from_numpy(q[sl]), k, None, k_fetch, return_all=True)
        ok = False
    except ValueError:
        pass
    out[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,store,metric,nq_locals,exchange", [
    (2, "crowded", "L2", [8, 8], "all_to_all"),
    (2, "crowded", "COSINE", [5, 2], "all_gather"),          # query counts differ per rank
    (2, "b", "L2", [8, 8], "all_gather"),                    # nobody is unproved: no second exchange, the begun search is aborted
    (4, "crowded", "COSINE", [4, 4, 4, 4], "all_gather"),
    (4, "crowded", "L2", [3, 0, 5, 1], "all_to_all"),        # ... and one rank has none
    (4, "d", "L2", [2, 2, 2, 2], "all_to_all"),              # everything excluded: -1 / NaN on every rank
])
def test_sharded_search_excluding(world, store, metric, nq_locals, exchange):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), store, metric, nq_locals, exchange, out), nprocs=world, join=True)
    assert dict(out) == {r: True for r in range(world)}


def _worker_failing(rank, world, port, out):
    """the certificate throws on every rank: the begun search must be given up and the error re-raised"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ShardedSearch
    state = {"begun": False, "aborted": 0, "finished": 0}

    def begin(q, k, ex, kf):
        assert not state["begun"]
        state["begun"] = True
        n = len(q)
        return (torch.zeros((n, k), dtype=torch.float64), torch.zeros((n, k), dtype=torch.int64), torch.zeros(n, dtype=torch.float64),
                torch.zeros(n, dtype=torch.int64))

    def finish(flags):
        state["begun"] = False
        state["finished"] += 1
        return torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int64)

    def abort():
        state["begun"] = False
        state["aborted"] += 1

    def certify(*a):
        raise ValueError("radad_excl_merge_certify: bad shape")

    ok = True
    for ex in ((begin, finish, abort), (begin, finish)):
        s = ShardedSearch(None, 1, excluding=ex, certify=certify)
        try:
            s.search_excluding(torch.zeros((2, 8)), 3, None, 13)
            ok = False
        except ValueError:
            pass
        ok = ok and not state["begun"]
    out[rank] = bool(ok and state["aborted"] == 1 and state["finished"] == 1)
    dist.barrier()
    dist.destroy_process_group()


def test_a_failed_certificate_does_not_leave_the_shard_begun():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_failing, args=(2, _free_port(), out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}


def test_replicated_and_single_rank_forms():
    sys.path.insert(0, ROOT)
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ReplicatedSearch, ShardedSearch
    calls = []

    def local(q, k, ex, kf):
        calls.append((tuple(q.shape), k, None if ex is None else ex.tolist(), kf))
        return torch.zeros((len(q), k), dtype=torch.float64), torch.zeros((len(q), k), dtype=torch.int64)
    q = torch.zeros((3, 8))
    d, i = ReplicatedSearch(None, local_search_excluding=local).search_excluding(q, 4, torch.tensor([9, 2]), 14)
    assert d.dtype == torch.float32 and d.shape == i.shape == (3, 4)
    d, i = ShardedSearch(None, 0, local_search_excluding=local).search_excluding(q, 4, None)      # world == 1: the one-piece call
    assert calls == [((3, 8), 4, [9, 2], 14), ((3, 8), 4, None, None)]
    with pytest.raises(ValueError):
        ReplicatedSearch(None).search_excluding(q, 4)
    with pytest.raises(ValueError):
        ShardedSearch(None, 0).search_excluding(q, 4)
    with pytest.raises(ValueError):
        ShardedSearch(None, 0, local_search_excluding=local).search_excluding(q, 4, return_all=True)
