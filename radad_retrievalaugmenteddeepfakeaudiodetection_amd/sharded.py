"""Row-sharded retrieval across the GPUs of one node (one process per GPU, torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" in the CPU tests).

The reference is single-GPU (vector_database.py:23 `device_id = 0`).  The store shards naturally: rank r owns a
contiguous row range [base_r, base_r + n_r) and reports GLOBAL ids (id_base = base_r).  A search is
  1. all_gather the per-rank query blocks            [Q_r, D] -> [Q, D]            (embeds are data-parallel)
  2. local brute-force top-k of ALL queries on the shard                            (no communication)
  3. all_gather the per-shard (dist, id) lists       2 x [Q, k] per rank          (12*Q*k bytes per rank: latency bound)
  4. merge the G sorted lists per query by (distance, id)                          (radad_topk_merge)
Both collectives are tiny, so on a fully connected xGMI node they are one-hop all-gathers.

With `bounded=(begin, finish)` (HipFlatIndex.search_begin / search_finish) step 2 is split around one more tiny collective:
  2a. scan the shard; per query lower bounds of the exact scores of its k best rows          (radad_knn_search_begin)
  2b. all_gather of the bounds                       [Q, k] float32 per rank (4*Q*k bytes); the k-th largest of a query's G*k
      values is a lower bound of the exact k-th best score of the WHOLE store
  2c. float64 re-rank of only those candidates that can still be among the GLOBAL k best      (radad_knn_search_finish)
Without it every shard certifies ITS OWN top k: on G shards the node re-ranks G times what one GPU would (rehearsed at G = 8:
143 candidates per query and shard against 151 per query on one GPU), and the re-rank does not scale.
"""
import ctypes as C
from typing import Callable, Optional, Tuple

import numpy as np

from . import _lib


def shard_bounds(n_total: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced row range of `rank`: the first n_total % world_size ranks get one extra row."""
    q, r = divmod(int(n_total), int(world_size))
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def hip_merge(metric: int, dists, idxs, k: int):
    """dists/idxs: [G, Q, k] CUDA tensors -> merged ([Q,k] f32, [Q,k] i64).  float64 `dists` (the keys
    radad_knn_search_f64 returns) are merged on float64 so no cross-shard pair is decided by fp32 rounding."""
    import torch
    lib = _lib.load()
    G, Q, kk = dists.shape
    assert kk == k
    out_d = torch.empty((Q, k), device=dists.device, dtype=torch.float32)
    out_i = torch.empty((Q, k), device=dists.device, dtype=torch.int64)
    d, i = dists.contiguous(), idxs.contiguous()
    with torch.cuda.device(dists.device):
        if d.dtype == torch.float64:
            _lib.check(lib.radad_topk_merge_f64(metric, d.data_ptr(), i.data_ptr(), G, Q, k, out_d.data_ptr(), out_i.data_ptr(),
                                                None, dists.device.index, _lib.stream_ptr(dists.device)), "radad_topk_merge_f64")
        else:
            _lib.check(lib.radad_topk_merge(metric, d.float().data_ptr() if d.dtype != torch.float32 else d.data_ptr(),
                                            i.data_ptr(), G, Q, k, out_d.data_ptr(), out_i.data_ptr(), dists.device.index,
                                            _lib.stream_ptr(dists.device)), "radad_topk_merge")
    return out_d, out_i


def _hip_certify(metric, keys, ids, fkeys, fids):
    from .vector_database import HipFlatIndex
    return HipFlatIndex.excl_merge_certify(metric, keys, ids, fkeys, fids)


class _Halves:
    """a (begin, finish[, abort]) triple.  Between begin and finish the shard holds a begun search: whatever goes wrong in between (a
    collective that throws, a kernel that refuses its shape), the second half must still run -- or be given up -- or every later
    search on the index fails with "has not been finished"."""

    def __init__(self, triple):
        self.begin, self.finish = triple[0], triple[1]
        self.abort = triple[2] if len(triple) > 2 else None

    def give_up(self):
        if self.abort is not None:
            self.abort()
        else:
            self.finish(None)              # (the shard's own result: a valid, if unbounded, second half)


class ShardedSearch:
    """Collective search over per-rank shards.

    local_search(q [Q,D], k) -> (dist [Q,k], gid [Q,k]) must return GLOBAL ids (HipFlatIndex with id_base does);
    dist may be float64 (HipFlatIndex.search_device(..., return_f64=True)[2]) -- it is what gets merged.
    merge(metric, dists [G,Q,k], idxs [G,Q,k], k) -> ([Q,k],[Q,k]); defaults to the HIP merge kernel.
    Every rank must call `search` with the same k.  uneven=False (default): every rank passes the same number of local
    queries.  uneven=True: the counts may differ (or be zero); one extra tiny all-gather of the counts per search, local
    blocks are padded to the largest.
    exchange: how the per-shard lists travel -- "all_to_all" (each rank receives only the lists of its own queries: 1/world
    of an all-gather's traffic; RCCL and gloo both implement it) or "all_gather" (+ slice).  It is fixed HERE, identically on
    every rank: a collective is never retried with a different primitive (a rank that failed alone would leave the others
    inside the first one).
    """

    def __init__(self, local_search: Callable, metric: int, group=None, merge: Optional[Callable] = None,
                 uneven: bool = False, exchange: str = "all_to_all", bounded=None, timing: bool = False, excluding=None,
                 certify: Optional[Callable] = None, local_search_excluding: Optional[Callable] = None,
                 excluding_per_query=None, local_search_excluding_per_query: Optional[Callable] = None):
        import torch.distributed as dist
        if exchange not in ("all_to_all", "all_gather"):
            raise ValueError("exchange must be 'all_to_all' or 'all_gather'")
        self.local_search = local_search
        self.metric = int(metric)
        self.group = group
        self.merge = merge or hip_merge
        self.uneven = bool(uneven)
        self.exchange = exchange
        # bounded = (begin, finish[, abort]): begin(q [Q,D], k) -> float32 [Q, k] lower bounds of the exact scores of this shard's k best
        # rows (or [Q]: of its k-th best alone); finish(global_lb [Q] or None) -> (dist [Q,k] (float64 keys), gid [Q,k]), rows short of
        # k are -1 filled; abort() gives the begun search up when the exchange fails (without it finish(None) is called).  Same on
        # every rank.
        self.bounded = bounded
        # excluding = (begin, finish[, abort]) of search_excluding (HipFlatIndex.sharded_excluding): begin(q [Q,D], k, exclude_tags
        # sorted int64 [n], k_fetch) -> (key f64 [Q,k], gid [Q,k], frontier key f64 [Q], frontier gid [Q]); finish(unproved int32 [Q] or
        # None) -> (key f64 [Q,k], gid [Q,k]); abort() gives the begun search up (without it finish(None) is called).  certify(metric,
        # keys [G,q,k], gids [G,q,k], fkeys [G,q], fgids [G,q]) -> (dist, gid, key, unproved [q]) defaults to
        # HipFlatIndex.excl_merge_certify; local_search_excluding(q, k, exclude_tags, k_fetch) -> (dist, gid) serves a world of one.
        self.excluding = excluding
        self.certify = certify or _hip_certify
        self.local_search_excluding = local_search_excluding
        # excluding_per_query = (begin, finish[, abort]) of search_excluding(query_tags_local=...) (HipFlatIndex.
        # sharded_excluding_per_query): begin(q [Q,D], k, query_tags int64 [Q,m], query_tag_counts int32 [Q], k_fetch) -> as above;
        # finish / abort as above.  local_search_excluding_per_query(q, k, query_tags, query_tag_counts, k_fetch) -> (dist, gid)
        # serves a world of one (HipFlatIndex.search_excluding_per_query bound to the store's row tags).
        self.excluding_per_query = excluding_per_query
        self.local_search_excluding_per_query = local_search_excluding_per_query
        self.timing = bool(timing)       # record (collective_ms, rerank_ms) of every search (CUDA events; read with timings())
        self._events = []
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # gloo moves host memory: device tensors are staged through the host (CPU tests; rehearsing ranks on one GPU)
        self.staged = dist.is_initialized() and dist.get_backend(group) == "gloo"

    def _all_gather(self, t):
        """[n, ...] per rank -> [world*n, ...] (rank-major)."""
        import torch
        import torch.distributed as dist
        t = t.contiguous()
        out = torch.empty((self.world * t.shape[0],) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        if t.is_cuda and self.staged:
            host = torch.empty(out.shape, dtype=t.dtype)
            dist.all_gather_into_tensor(host, t.cpu(), group=self.group)
            out.copy_(host)
        else:
            dist.all_gather_into_tensor(out, t, group=self.group)
        return out

    def _exchange(self, t, qr: int):
        """t [world*qr, k]: this shard's lists for ALL queries, rank-major -> [world, qr, k]: every shard's lists for THIS
        rank's queries."""
        import torch
        import torch.distributed as dist
        t = t.contiguous()
        k = t.shape[1]
        if self.exchange == "all_gather":
            sl = slice(self.rank * qr, (self.rank + 1) * qr)
            return self._all_gather(t).view(self.world, self.world * qr, k)[:, sl].contiguous()
        if t.is_cuda and self.staged:
            host_out = torch.empty((self.world * qr, k), dtype=t.dtype)
            dist.all_to_all_single(host_out, t.cpu(), group=self.group)
            return host_out.to(t.device).view(self.world, qr, k)
        out = torch.empty((self.world * qr, k), device=t.device, dtype=t.dtype)
        dist.all_to_all_single(out, t, group=self.group)
        return out.view(self.world, qr, k)

    def _all_reduce_max(self, t):
        import torch.distributed as dist
        if t.is_cuda and self.staged:
            host = t.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.MAX, group=self.group)
            t.copy_(host)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return t

    def timings(self):
        """[(collective_ms, rerank_ms)] of the searches since the last call (synchronises); needs timing=True and CUDA tensors"""
        out = []
        for ev in self._events:
            ev[-1].synchronize()
            coll = sum(a.elapsed_time(b) for a, b in ev[0])
            out.append((coll, ev[1][0].elapsed_time(ev[1][1]) if ev[1] else 0.0))
        self._events = []
        return out

    def gather_queries(self, q_local):
        return q_local if self.world == 1 else self._all_gather(q_local)

    def _pad_uneven(self, q_local):
        """-> (q_local, rows per rank, counts): with uneven=True one all-gather of the ranks' query counts, and the local block padded
        to the largest with zero queries (their results are dropped by the caller); else as it came, counts None"""
        import torch
        qr = q_local.shape[0]
        if not self.uneven:
            return q_local, qr, None
        c = torch.tensor([qr], dtype=torch.int64, device=q_local.device)
        counts = [int(x) for x in self._all_gather(c).cpu().tolist()]
        qmax = max(max(counts), 1)
        if qr < qmax:
            pad = torch.zeros((qmax - qr,) + tuple(q_local.shape[1:]), device=q_local.device, dtype=q_local.dtype)
            q_local = torch.cat([q_local, pad])
        return q_local, qmax, counts

    def _gather_exclusion(self, excl_local, device):
        """the ranks' exclusion tags -> their sorted union [n] int64 on `device` (counts first, then blocks padded to the largest)"""
        import torch
        e = torch.empty(0, dtype=torch.int64, device=device) if excl_local is None else excl_local.to(device=device, dtype=torch.int64).reshape(-1)
        counts = self._all_gather(torch.tensor([e.numel()], dtype=torch.int64, device=device)).cpu().tolist()
        emax = max(counts)
        if emax == 0:
            return e
        block = torch.zeros(emax, dtype=torch.int64, device=device)
        block[:e.numel()] = e
        blocks = self._all_gather(block).view(self.world, emax)
        return torch.unique(torch.cat([blocks[r, :c] for r, c in enumerate(counts)]))         # (sorted ascending)

    def _gather_query_tags(self, qtags_local, qcnt_local, qr: int, qr_pad: int, device):
        """the rank's per-query tags [qr, m] (or [qr]) and counts [qr] / None -> (tags int64 [world * qr_pad, m], counts int32
        [world * qr_pad]) in the order of the gathered queries.  They travel as ONE block of fixed width m + 1 (the count rides as
        the last column), so m must be the same on every rank; padding queries get count 0."""
        import torch
        t = torch.as_tensor(qtags_local, dtype=torch.int64).to(device)
        if t.dim() == 1:
            t = t.reshape(-1, 1)
        if t.dim() != 2 or t.shape[0] != qr:
            raise ValueError(f"query_tags_local must be [Q_r, m] (or [Q_r]) with Q_r = {qr}, got {tuple(t.shape)}")
        m = t.shape[1]
        if m > 64:
            raise ValueError(f"query_tags_local lists {m} tags per query; a per-query exclusion set holds at most 64")
        c = torch.full((qr,), m, dtype=torch.int64, device=device) if qcnt_local is None else \
            torch.as_tensor(qcnt_local).to(device=device, dtype=torch.int64).reshape(-1).clamp(0, m)
        if c.numel() != qr:
            raise ValueError("query_tag_counts_local must hold one count per local query")
        block = torch.zeros((qr_pad, m + 1), dtype=torch.int64, device=device)
        block[:qr, :m] = t
        block[:qr, m] = c
        allb = self._all_gather(block)
        return allb[:, :m].contiguous(), allb[:, m].to(torch.int32).contiguous()

    def search_excluding_in_scan(self, *args, **kwargs):
        raise ValueError("search_excluding_in_scan has no sharded form of its own: a shard's result of HipFlatIndex.search_excluding_in_scan "
                         "is already its exact admissible top k, so ShardedSearch(local_search=<that call with return_f64>).search(q, k) "
                         "merges the shards' lists exactly (INTEGRATION.md); search_excluding is the certified over-fetch over shards")

    def search_excluding_per_query_in_scan(self, *args, **kwargs):
        raise ValueError("search_excluding_per_query_in_scan has no sharded form of its own: a shard's result of "
                         "HipFlatIndex.search_excluding_per_query_in_scan is already its exact admissible top k, so "
                         "ShardedSearch(local_search=<that call with return_f64>).search(q, k) merges the shards' lists exactly "
                         "(INTEGRATION.md); search_excluding with query_tags_local is the certified over-fetch over shards")

    def range_search(self, *args, **kwargs):
        raise ValueError("range_search has no sharded form of its own: a shard's result of HipFlatIndex.range_search is already every "
                         "row of that shard within the radius, so concatenating the shards' lists per query (and adding their counts) "
                         "is the merge")

    def range_search_excluding(self, *args, **kwargs):
        raise ValueError("range_search_excluding has no sharded form of its own: a shard's result of HipFlatIndex.range_search_excluding "
                         "is already every admissible row of that shard within the radius, so concatenating the shards' lists per query "
                         "(and adding their counts) is the merge")

    def range_search_excluding_per_query(self, *args, **kwargs):
        raise ValueError("range_search_excluding_per_query has no sharded form of its own: a shard's result of "
                         "HipFlatIndex.range_search_excluding_per_query is already every admissible row of that shard within the radius, so "
                         "concatenating the shards' lists per query (and adding their counts) is the merge")

    def search_excluding(self, q_local, k: int, exclude_tags_local=None, k_fetch=None, return_all: bool = False,
                         query_tags_local=None, query_tag_counts_local=None):
        """The exclusion-aware search (HipFlatIndex.search_excluding) over the row shards: q_local [Q_r, D], exclude_tags_local int64
        tensor (any order, may be None / empty) -> this rank's rows ([Q_r,k] float32 distances, [Q_r,k] global ids): per query the k
        nearest rows of the WHOLE store whose tag no rank excluded, -1 / NaN where fewer exist.  Needs excluding=(begin, finish[,
        abort]); every rank passes the same k and k_fetch (None = k + 10, per shard).
          1. the ranks' exclusion tags are all-gathered (counts, then padded blocks) and unioned: the excluded set is that of the
             batch all ranks form together ("no clip of the batch retrieves a clip of the batch", pipeline.py:491-509)
          2. the queries are all-gathered as in search
          3. begin on the shard: certified search at k_fetch, admissible hits + frontier per query
          4. lists and frontiers travel by the configured primitive: each rank holds every shard's lists for its own queries
          5. certify (radad_excl_merge_certify): merged rows + one flag per query the shards together cannot prove
          6. the flags are all-gathered: every rank holds the same [Q] vector
          7. no flag set: the merged rows are the result and the begun search is given up.  Otherwise finish(flags) runs the
             row-filtered exact pass for the flagged queries on every shard, the lists travel a second time and are merged
             (radad_topk_merge_f64).
        The "any flag set?" test of step 7 is one 4-byte host read of the all-gathered vector.  It is the ONLY host synchronisation
        this search adds (beyond the count exchanges of step 1 and of uneven=True), and its value is identical on every rank, so
        every rank takes the same sequence of collectives.  A failure between begin and finish gives the begun search up.
        return_all is refused: each rank certifies its own queries only.
        query_tags_local int64 [Q_r, m] (or [Q_r]; m <= 64, the same on every rank) with query_tag_counts_local [Q_r] or None selects
        the PER-QUERY form instead (HipFlatIndex.search_excluding_per_query): query j excludes the first count_j of its own tags and
        nothing else.  The tags travel with the queries, all-gathered at the fixed width m; step 1 is skipped, no union is formed, and
        the result of a query depends neither on the batch nor on the world size.  Steps 2 - 7 are the same sequence.  Needs
        excluding_per_query=(begin, finish[, abort]); passing both kinds of set is refused (one call takes one admission rule)."""
        import torch
        if return_all:
            raise ValueError("search_excluding returns a rank's own rows only (return_all is not supported: each rank certifies its own queries)")
        per_query = query_tags_local is not None
        if per_query and exclude_tags_local is not None:
            raise ValueError("search_excluding takes exclude_tags_local (one set for the batch) or query_tags_local (one set per query), "
                             "not both: a batch-wide set cannot be combined with per-query sets in one call")
        if query_tag_counts_local is not None and not per_query:
            raise ValueError("query_tag_counts_local needs query_tags_local")
        if self.world == 1 and per_query:
            if self.local_search_excluding_per_query is None:
                raise ValueError("search_excluding(query_tags_local=...) on one rank needs local_search_excluding_per_query "
                                 "(HipFlatIndex.search_excluding_per_query)")
            d_loc, i_loc = self.local_search_excluding_per_query(q_local, k, query_tags_local, query_tag_counts_local, k_fetch)[:2]
            return d_loc.float(), i_loc
        if self.world == 1:
            if self.local_search_excluding is None:
                raise ValueError("search_excluding on one rank needs local_search_excluding (HipFlatIndex.search_excluding)")
            d_loc, i_loc = self.local_search_excluding(q_local, k, exclude_tags_local, k_fetch)[:2]
            return d_loc.float(), i_loc
        if per_query and self.excluding_per_query is None:
            raise ValueError("search_excluding(query_tags_local=...) needs excluding_per_query=(begin, finish[, abort]) "
                             "(HipFlatIndex.sharded_excluding_per_query)")
        if not per_query and self.excluding is None:
            raise ValueError("search_excluding needs excluding=(begin, finish[, abort]) (HipFlatIndex.sharded_excluding)")
        halves = _Halves(self.excluding_per_query if per_query else self.excluding)
        k = int(k)
        excl = None if per_query else self._gather_exclusion(exclude_tags_local, q_local.device)
        qr = q_local.shape[0]
        q_local, qr_pad, _ = self._pad_uneven(q_local)
        q_all = self._all_gather(q_local)
        if per_query:
            qtags_all, qcnt_all = self._gather_query_tags(query_tags_local, query_tag_counts_local, qr, qr_pad, q_local.device)
            key, gid, fkey, fgid = halves.begin(q_all, k, qtags_all, qcnt_all, k_fetch)
        else:
            key, gid, fkey, fgid = halves.begin(q_all, k, excl, k_fetch)
        done = False
        try:
            # frontiers ride as column k of the lists: two exchanges instead of four
            xk = self._exchange(torch.cat([key, fkey.view(-1, 1)], dim=1), qr_pad)
            xi = self._exchange(torch.cat([gid, fgid.view(-1, 1)], dim=1), qr_pad)
            md, mi, _, flags = self.certify(self.metric, xk[:, :, :k].contiguous(), xi[:, :, :k].contiguous(),
                                            xk[:, :, k].contiguous(), xi[:, :, k].contiguous())
            flags = flags.to(torch.int32)
            flags[qr:] = 0                                  # (padding queries need no proof)
            flags_all = self._all_gather(flags)
            if int(flags_all.max().item()) == 0:            # the one host read; the same value on every rank
                halves.give_up()
                done = True
                return md[:qr].float(), mi[:qr]
            done = True
            key2, gid2 = halves.finish(flags_all)
        except BaseException:
            if not done:
                halves.give_up()
            raise
        md, mi = self.merge(self.metric, self._exchange(key2, qr_pad), self._exchange(gid2, qr_pad), k)
        md = md.float().masked_fill(mi < 0, float("nan"))   # the exclusion family's padding (the plain merge pads with +-inf)
        return md[:qr], mi[:qr]

    def search(self, q_local, k: int, return_all: bool = False):
        """q_local [Q_r, D] -> this rank's rows of the merged result ([Q_r,k] distances, [Q_r,k] global ids);
        `return_all` returns the rows of all ranks' queries instead (rank-major; with uneven=True: padded blocks removed)."""
        import torch
        if self.world == 1:
            d_loc, i_loc = self.local_search(q_local, k)
            return d_loc.float(), i_loc
        qr = q_local.shape[0]
        q_local, qr_pad, counts = self._pad_uneven(q_local)
        import contextlib
        rec = self.timing and q_local.is_cuda
        coll_ev, rr_ev = [], None

        @contextlib.contextmanager
        def timed(kind):
            if not rec:
                yield
                return
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            yield
            b.record()
            if kind == "c":
                coll_ev.append((a, b))
            else:
                nonlocal rr_ev
                rr_ev = (a, b)

        with timed("c"):
            q_all = self._all_gather(q_local)
        if self.bounded is not None:
            halves = _Halves(self.bounded)
            lb = halves.begin(q_all, k)
            try:
                with timed("c"):
                    if lb.dim() == 2:      # the k best of every shard: the k-th largest of the union bounds the global k-th best
                        allb = self._all_gather(lb).view(self.world, lb.shape[0], lb.shape[1])
                        from .vector_database import HipFlatIndex
                        lb = HipFlatIndex.global_bound(allb, k)       # (torch.topk on the CPU or beyond the kernel's 1280 values per query)
                    else:
                        lb = self._all_reduce_max(lb)
            except BaseException:
                halves.give_up()
                raise
            with timed("r"):
                d_loc, i_loc = halves.finish(lb)
        else:
            d_loc, i_loc = self.local_search(q_all, k)
        Q = q_all.shape[0]
        if return_all:
            d_all = self._all_gather(d_loc).view(self.world, Q, k)
            i_all = self._all_gather(i_loc).view(self.world, Q, k)
            md, mi = self.merge(self.metric, d_all, i_all, k)
            if counts is not None:
                keep = torch.cat([torch.arange(r * qr_pad, r * qr_pad + c) for r, c in enumerate(counts)]).to(md.device)
                md, mi = md[keep], mi[keep]
            return md, mi
        with timed("c"):
            xd, xi = self._exchange(d_loc, qr_pad), self._exchange(i_loc, qr_pad)
        md, mi = self.merge(self.metric, xd, xi, k)
        if rec:
            self._events.append((coll_ev, rr_ev, coll_ev[-1][1]))
        return md[:qr], mi[:qr]


class ReplicatedSearch:
    """The other way to use G GPUs (SURVEY 8e's tuning option; the reference is single-GPU, vector_database.py:23): every rank holds
    the WHOLE store and searches only its own queries -- no collective in the data path, a rank's step is the one-GPU step.  Every
    BASELINE store fits one 288 GB MI355X (1 M x 512: 3 GB with its f16 plane; 10 M x 512: 30 GB; 50 M x 256 fp16: 26 GB); sharding
    (ShardedSearch, north_star's partitioning) is for stores that do not, and costs every rank the scan of ALL queries plus G re-ranks.
    Same call surface as ShardedSearch: search(q_local, k) -> this rank's rows; return_all=True gathers every rank's rows (rank-major;
    the only collective, and not part of a search)."""

    def __init__(self, local_search: Callable, group=None, local_search_excluding: Optional[Callable] = None):
        import torch.distributed as dist
        self.local_search = local_search
        self.local_search_excluding = local_search_excluding
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.timing = False
        self._gather = ShardedSearch(None, 0, group=group)._all_gather

    def timings(self):
        return []

    def range_search(self, *args, **kwargs):
        raise ValueError("range_search has no replicated form of its own: every rank holds the whole store, so "
                         "HipFlatIndex.range_search on the rank's store with the rank's own queries is the answer")

    def range_search_excluding(self, *args, **kwargs):
        raise ValueError("range_search_excluding has no replicated form of its own: every rank holds the whole store, so "
                         "HipFlatIndex.range_search_excluding on the rank's store with the rank's own queries and set is the answer")

    def range_search_excluding_per_query(self, *args, **kwargs):
        raise ValueError("range_search_excluding_per_query has no replicated form of its own: every rank holds the whole store, so "
                         "HipFlatIndex.range_search_excluding_per_query on the rank's store with the rank's own queries is the answer")

    def search_excluding(self, q_local, k: int, exclude_tags_local=None, k_fetch=None):
        """local_search_excluding(q_local, k, exclude_tags_local, k_fetch) on the rank's own queries with the rank's OWN exclusion set
        (HipFlatIndex.search_excluding): every rank holds the whole store, so there is nothing to certify across ranks."""
        if self.local_search_excluding is None:
            raise ValueError("search_excluding needs local_search_excluding (HipFlatIndex.search_excluding on the rank's store)")
        d, i = self.local_search_excluding(q_local, k, exclude_tags_local, k_fetch)[:2]
        return d.float(), i

    def search(self, q_local, k: int, return_all: bool = False):
        d, i = self.local_search(q_local, k)
        d = d.float()
        if not return_all or self.world == 1:
            return d, i
        return self._gather(d), self._gather(i)
