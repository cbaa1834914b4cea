"""VectorDatabase -- same call surface as the reference's vector_database.py:8-272, with the faiss index
object replaced by `HipFlatIndex`, a thin handle on the HBM-resident store in libradad_hip.so.

What callers of the reference rely on and still find here:
  * VectorDatabase(config): .add_vectors / .add_vectors_batch / .search_batch / .search / .save / .load,
    attributes .vector_paths / .vector_labels / .vector_metadata, and the raw `.index`
    (pipeline.py:445-446,480,495-506; app.py:67-76).
  * .index.ntotal / .d / .is_trained / .add(np) / .search(np,k) / .reconstruct(i)  (faiss.IndexFlat surface
    used at vector_database.py:124,138,151,169,181 and pipeline.py:465,503).
Index types: 'L2' -> squared-L2 ascending; 'IP' -> inner product descending, with rows and queries
L2-normalised first when config.normalize_for_ip (default True) i.e. cosine (vector_database.py:61-64,97,100-105).
'IVF' (vector_database.py:65-70) -> HipIVFFlatIndex (k-means coarse quantiser + list scan, csrc/ivf.inc; k <= 128: above 26 the exact scan
of the same rows answers).
Device-resident variants (`search_device`, `reconstruct_batch`) let the pipeline skip the D2H/H2D hops.
"""
import ctypes as C
import hashlib
import logging
import os
import pickle
from typing import Dict, List, Tuple

import numpy as np

from . import _lib


def path_tag(path: str) -> int:
    """Stable 63-bit tag of a file's basename: the device-side stand-in for the strings the reference compares in
    retrieve_similar_vectors (pipeline.py:463,495-502)."""
    h = hashlib.blake2b(os.path.basename(path).encode("utf-8", "surrogatepass"), digest_size=8).digest()
    return int.from_bytes(h, "little") & 0x7FFFFFFFFFFFFFFF


# ---- faiss IndexFlat file interchange -------------------------------------------------------------------------------
# The reference persists its store with faiss.write_index (vector_database.py:203) -> `faiss_index.bin`.  faiss is not
# available here, so this reader/writer follows the published on-disk layout of a flat index from upstream faiss
# (impl/index_write.cpp: fourcc 'IxF2' (L2) / 'IxFI' (IP), then the index header d:int32, ntotal:int64, two int64
# dummies, is_trained:uint8, metric_type:int32 [+ metric_arg:float32 if metric_type > 1], then the row data as a
# uint64 count of 4-byte words followed by ntotal*d float32).  UNVERIFIED against a real faiss build (none in this
# image): round-trips through this module only; treat as best effort for migrating an existing RADAD deployment.
def read_faiss_flat(path: str):
    """-> (metric 'L2'|'IP', d, rows float32 [ntotal, d]); raises ValueError if the file is not a flat faiss index."""
    with open(path, "rb") as f:
        fourcc = f.read(4)
        if fourcc not in (b"IxF2", b"IxFI"):
            raise ValueError(f"{path}: not a faiss IndexFlat file (fourcc {fourcc!r})")
        d = int(np.frombuffer(f.read(4), "<i4")[0])
        ntotal = int(np.frombuffer(f.read(8), "<i8")[0])
        f.read(16)                                   # two int64 dummies
        f.read(1)                                    # is_trained
        metric_type = int(np.frombuffer(f.read(4), "<i4")[0])
        if metric_type > 1:
            f.read(4)                                # metric_arg
        nwords = int(np.frombuffer(f.read(8), "<u8")[0])
        if d <= 0 or ntotal < 0 or nwords != ntotal * d:
            raise ValueError(f"{path}: inconsistent faiss header (d={d}, ntotal={ntotal}, words={nwords})")
        rows = np.fromfile(f, "<f4", nwords).reshape(ntotal, d)
    return ("L2" if fourcc == b"IxF2" else "IP"), d, rows


def write_faiss_flat(path: str, rows: np.ndarray, metric: str):
    rows = np.ascontiguousarray(rows, "<f4")
    n, d = rows.shape
    with open(path, "wb") as f:
        f.write(b"IxF2" if metric.upper() == "L2" else b"IxFI")
        f.write(np.int32(d).tobytes()); f.write(np.int64(n).tobytes())
        f.write(np.int64(1 << 20).tobytes() * 2)
        f.write(b"\x01")
        f.write(np.int32(1 if metric.upper() == "L2" else 0).tobytes())     # faiss MetricType: 0 = IP, 1 = L2
        f.write(np.uint64(n * d).tobytes())
        rows.tofile(f)


def knn_options_from_config(config):
    """the optional scan knobs, read the way the reference reads its own optional ones (getattr with a default,
    vector_database.py:43,67,80): knn_hi_plane, knn_centre, knn_smallq_hi, knn_wide_min_q, knn_dense, knn_abandon, knn_abandon_defer, knn_abandon_ahead, knn_range_smallq, knn_remove_stage_rows; absent / None = the library's default.
    knn_live_floor is still recognised, but only None / 0 (the default): the one-launch scan form it selected was removed"""
    if getattr(config, "knn_live_floor", None) not in (None, 0):
        raise ValueError("knn_live_floor: the one-launch scan form was measured slower and removed (DESIGN §4.1); "
                         "leave it None / 0 for the default, one launch per phase")
    opts = dict(hi_plane=getattr(config, "knn_hi_plane", None), centre=getattr(config, "knn_centre", None),
                smallq_hi=getattr(config, "knn_smallq_hi", None), wide_min_q=getattr(config, "knn_wide_min_q", None),
                dense=getattr(config, "knn_dense", None), abandon=getattr(config, "knn_abandon", None),
                range_smallq=getattr(config, "knn_range_smallq", None), abandon_defer=getattr(config, "knn_abandon_defer", None),
                abandon_ahead=getattr(config, "knn_abandon_ahead", None),
                remove_stage_rows=getattr(config, "knn_remove_stage_rows", None))
    return {k: v for k, v in opts.items() if v is not None}


def _prep_queries(q, d: int):
    """q -> (q, q_dtype): a contiguous [nq, d] CUDA tensor as the library reads it (bfloat16 as it is, anything else as float32)"""
    import torch
    _lib.require_cuda(q, "q")
    bf16 = q.dtype == torch.bfloat16
    q = q.contiguous() if bf16 else q.contiguous().float()
    if q.dim() != 2 or q.shape[1] != d:
        raise ValueError(f"search expects [nq, {d}], got {tuple(q.shape)}")
    return q, _lib.Q_BF16 if bf16 else _lib.Q_F32


def _prep_tags(row_tags, exclude_tags, ntotal: int):
    """-> (row_tags, exclude_tags, n_excl): flat contiguous int64 CUDA tensors, one tag per stored row; (None, None, 0) when nothing
    is excluded (the row tags are not looked at then)"""
    import torch
    n_excl = 0 if exclude_tags is None else int(exclude_tags.numel())
    if not n_excl:
        return None, None, 0
    _lib.require_cuda(exclude_tags, "exclude_tags")
    _lib.require_cuda(row_tags, "row_tags")
    exclude_tags = exclude_tags.contiguous().to(torch.int64).reshape(-1)
    row_tags = row_tags.contiguous().to(torch.int64).reshape(-1)
    if row_tags.numel() != ntotal:
        raise ValueError(f"row_tags must hold one tag per stored row ({ntotal}), got {row_tags.numel()}")
    return row_tags, exclude_tags, n_excl


def _prep_query_tags(row_tags, query_tags, query_tag_counts, nq: int, ntotal: int):
    """-> (row_tags [ntotal], query_tags [nq, m], counts int32 [nq] or None, m): contiguous CUDA tensors of the per-query exclusion
    (radad_knn_search_excl_pq); a 1-D [nq] query_tags is m = 1; (None, None, None, 0) when no query lists a tag.  A tensor on the CPU,
    a wrong shape or m above the limit is a ValueError here: the library would only see a pointer."""
    import torch
    if query_tags is None:
        return None, None, None, 0
    if not isinstance(query_tags, torch.Tensor) or not query_tags.is_cuda:
        raise ValueError("query_tags must be an int64 CUDA (ROCm) tensor [nq, m]: the HIP path has no CPU fallback")
    if query_tags.dim() == 1:
        query_tags = query_tags.reshape(-1, 1)
    if query_tags.dim() != 2 or query_tags.shape[0] != nq:
        raise ValueError(f"query_tags must be [nq, m] (or [nq] for one tag per query) with nq = {nq}, got {tuple(query_tags.shape)}")
    m = int(query_tags.shape[1])
    if m > _lib.EXCL_PQ_MAX_TAGS:
        raise ValueError(f"query_tags lists {m} tags per query; a per-query exclusion set holds at most {_lib.EXCL_PQ_MAX_TAGS} "
                         "(one wave compares them)")
    if m == 0:
        return None, None, None, 0
    if not isinstance(row_tags, torch.Tensor) or not row_tags.is_cuda:
        raise ValueError("row_tags must be an int64 CUDA (ROCm) tensor [ntotal]: the HIP path has no CPU fallback")
    query_tags = query_tags.contiguous().to(torch.int64)
    row_tags = row_tags.contiguous().to(torch.int64).reshape(-1)
    if row_tags.numel() != ntotal:
        raise ValueError(f"row_tags must hold one tag per stored row ({ntotal}), got {row_tags.numel()}")
    if query_tag_counts is not None:
        if not isinstance(query_tag_counts, torch.Tensor) or not query_tag_counts.is_cuda:
            raise ValueError("query_tag_counts must be a CUDA (ROCm) tensor [nq]: the HIP path has no CPU fallback")
        query_tag_counts = query_tag_counts.contiguous().to(torch.int32).reshape(-1)
        if query_tag_counts.numel() != nq:
            raise ValueError(f"query_tag_counts must hold one count per query ({nq}), got {query_tag_counts.numel()}")
    return row_tags, query_tags, query_tag_counts, m


def _alloc_out(q, k: int, f64: bool = False):
    """-> (D f32, I i64, K64 f64 or None), each [nq, k] on q's device"""
    import torch
    D = torch.empty((q.shape[0], k), device=q.device, dtype=torch.float32)
    I = torch.empty((q.shape[0], k), device=q.device, dtype=torch.int64)
    K64 = torch.empty((q.shape[0], k), device=q.device, dtype=torch.float64) if f64 else None
    return D, I, K64


def _ptr(t):
    return t.data_ptr() if t is not None else None


class HipFlatIndex:
    """Flat (exhaustive) index living in HBM.  Mirrors the slice of faiss.IndexFlat{L2,IP} the reference uses."""

    is_trained = True   # flat indexes need no training (vector_database.py:124)

    def __init__(self, d: int, metric: int, device: int = 0, id_base: int = 0, store_f16: bool = False, hi_plane=None, centre=None,
                 smallq_hi=None, wide_min_q=None, dense=None, abandon=None, range_smallq=None, abandon_defer=None, abandon_ahead=None,
                 remove_stage_rows=None):
        """hi_plane / centre / smallq_hi / wide_min_q / dense / abandon / range_smallq / abandon_defer / abandon_ahead: kernel choices of the handle (radad_knn_set_option;
        None = the library's default).  They change speed, never results: A/B measurements and the parity tests select kernels through
        them.  range_smallq (default off): range searches of <= 16 queries stream the f16 plane instead of the float64 exact kernel.
        remove_stage_rows: slab size of remove_ids in rows (None = 64 MiB of rows; at least 64)."""
        self._lib = _lib.load()
        self.d = int(d)
        self.metric = int(metric)
        self.device = int(device)
        self.id_base = int(id_base)
        self.store_f16 = bool(store_f16)      # config.use_float16 (vector_database.py:80): rows kept as IEEE fp16
        h = C.c_void_p()
        _lib.check(self._lib.radad_knn_create_ex(self.d, self.metric, _lib.STORE_F16 if self.store_f16 else _lib.STORE_F32,
                                                 self.device, self.id_base, C.byref(h)), "radad_knn_create")
        self._h = h
        self.options = dict(hi_plane=hi_plane, centre=centre, smallq_hi=smallq_hi, wide_min_q=wide_min_q, dense=dense, abandon=abandon,
                            range_smallq=range_smallq, abandon_defer=abandon_defer, abandon_ahead=abandon_ahead,
                            remove_stage_rows=remove_stage_rows)
        for opt, val in ((_lib.KNN_OPT_HI_PLANE, hi_plane), (_lib.KNN_OPT_CENTRE, centre), (_lib.KNN_OPT_SMALLQ_HI, smallq_hi),
                         (_lib.KNN_OPT_WIDE_MIN_Q, wide_min_q), (_lib.KNN_OPT_DENSE, dense), (_lib.KNN_OPT_ABANDON, abandon),
                         (_lib.KNN_OPT_RANGE_SMALLQ, range_smallq), (_lib.KNN_OPT_ABANDON_DEFER, abandon_defer),
                         (_lib.KNN_OPT_ABANDON_AHEAD, abandon_ahead), (_lib.KNN_OPT_REMOVE_STAGE_ROWS, remove_stage_rows)):
            if val is not None:
                _lib.check(self._lib.radad_knn_set_option(self._h, opt, int(val)), "radad_knn_set_option")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.radad_knn_destroy(h)
            except Exception:
                pass

    @property
    def ntotal(self) -> int:
        n = C.c_int64()
        _lib.check(self._lib.radad_knn_ntotal(self._h, C.byref(n)))
        return n.value

    def reserve(self, capacity: int):
        _lib.check(self._lib.radad_knn_reserve(self._h, int(capacity)), "radad_knn_reserve")

    # ---- host (numpy) surface: what faiss offers ---------------------------------------------------------
    def add(self, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}] float32, got {x.shape}")
        _lib.check(self._lib.radad_knn_add_host(self._h, x.ctypes.data, x.shape[0]), "radad_knn_add_host")

    def search(self, x: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}] float32, got {x.shape}")
        D = np.empty((x.shape[0], k), np.float32)
        I = np.empty((x.shape[0], k), np.int64)
        _lib.check(self._lib.radad_knn_search_host(self._h, x.ctypes.data, x.shape[0], int(k), D.ctypes.data, I.ctypes.data),
                   "radad_knn_search_host")
        return D, I

    def reconstruct(self, i: int) -> np.ndarray:
        idx = np.asarray([int(i)], np.int64)
        out = np.empty((1, self.d), np.float32)
        _lib.check(self._lib.radad_knn_reconstruct_host(self._h, idx.ctypes.data, 1, out.ctypes.data))
        return out[0]

    # ---- device (torch) surface ---------------------------------------------------------------------------
    def add_device(self, x):
        import torch
        _lib.require_cuda(x, "x")
        x = x.contiguous().float()
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}], got {tuple(x.shape)}")
        with torch.cuda.device(x.device):
            _lib.check(self._lib.radad_knn_add(self._h, x.data_ptr(), x.shape[0], _lib.stream_ptr(x.device)), "radad_knn_add")

    def remove_ids(self, ids, return_map: bool = False):
        """Remove the rows with these GLOBAL ids (id_base + position) in place, on the device, as faiss IndexFlat.remove_ids does: the
        kept rows keep their bits and their order and hold positions 0 ... ntotal - 1 afterwards (radad_knn_remove_ids).  ids: a list, a
        numpy array or a CPU / CUDA int64 tensor, in any order; repeats and ids that name no stored row are ignored.  -> the number of
        distinct rows removed; with return_map also an int64 CUDA tensor [ntotal before]: the new global id of every old position, -1
        for a removed one (to compact per-row columns of the caller's own).  On a row shard (id_base != 0) only ids of the shard's own
        range count, and ids shift inside the shard only.  Synchronises; a ValueError while a search_begin awaits its finish."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(ids, torch.Tensor):
            t = ids.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))).to(dev)
        omap = torch.empty((self.ntotal,), device=dev, dtype=torch.int64) if return_map else None
        removed = C.c_int64(0)
        with torch.cuda.device(dev):
            _lib.check(self._lib.radad_knn_remove_ids(self._h, t.data_ptr() if t.numel() else None, int(t.numel()), _ptr(omap),
                                                      C.byref(removed), _lib.stream_ptr(dev)), "radad_knn_remove_ids")
        return (int(removed.value), omap) if return_map else int(removed.value)

    def last_remove(self):
        """{"launches", "bytes_moved"} of the last remove_ids: the move launches of its plan and the bytes they read + wrote"""
        n, b = C.c_int(), C.c_int64()
        _lib.check(self._lib.radad_knn_last_remove(self._h, C.byref(n), C.byref(b)))
        return {"launches": n.value, "bytes_moved": b.value}

    def search_device(self, q, k: int, return_f64: bool = False):
        """q [nq, d] CUDA tensor (float32, or bfloat16 = BASELINE config 5's bf16 embeddings, handed to the library as
        they are) -> (D f32 [nq,k], I i64 [nq,k]) on the device; with return_f64 also the float64 distances the ranking
        was made on (used by the sharded merge)."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        D, I, K64 = _alloc_out(q, k, return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_ex(self._h, q.data_ptr(), q_dtype, q.shape[0], int(k), D.data_ptr(), I.data_ptr(),
                                                     _ptr(K64), _lib.stream_ptr(q.device)), "radad_knn_search")
        return (D, I, K64) if return_f64 else (D, I)

    def search_excluding(self, q, k: int, row_tags, exclude_tags, k_fetch=None, return_f64: bool = False):
        """The k nearest rows whose tag is not excluded, exactly (radad_knn_search_excl): q [nq, d] CUDA tensor (float32 or bfloat16),
        row_tags int64 CUDA tensor [ntotal] (indexed by id - id_base), exclude_tags int64 CUDA tensor sorted ascending, or None /
        empty -> (D f32 [nq,k], I i64 [nq,k][, K64 f64 [nq,k]]) on the device; slots beyond the admissible rows hold -1 / NaN.
        k_fetch (None = k + 10, the reference's over-fetch) is the size of the certified search in front: a query that does not find
        k admissible rows among its k_fetch hits is answered by the float64 scan of the admissible rows (last_excl()["exact"])."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        k = int(k)
        k_fetch = min(k + 10, _lib.KNN_MAX_K) if k_fetch is None else int(k_fetch)
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        D, I, K64 = _alloc_out(q, max(k, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl(self._h, q.data_ptr(), q_dtype, q.shape[0], k, k_fetch, _ptr(row_tags),
                                                       _ptr(exclude_tags), n_excl, D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                       _lib.stream_ptr(q.device)), "radad_knn_search_excl")
        return (D, I, K64) if return_f64 else (D, I)

    def search_excluding_per_query(self, q, k: int, row_tags, query_tags, query_tag_counts=None, k_fetch=None, return_f64: bool = False):
        """search_excluding with one exclusion set PER QUERY (radad_knn_search_excl_pq; leave-one-out): row r is admissible for query
        j iff row_tags[r] is not among the first query_tag_counts[j] entries of query_tags[j].  query_tags int64 CUDA tensor [nq, m],
        m <= 64, any order, duplicates allowed ([nq] = one tag per query; None or m = 0 = nothing excluded); query_tag_counts int32
        CUDA tensor [nq], clamped to [0, m] on the device, None = m for every query.  Everything else as search_excluding: the result
        of a query does not depend on what the other queries of the batch exclude.  If no tag is carried by more than c rows,
        k_fetch >= k + m * c proves every query in the fast pass (last_excl()["exact"] == 0)."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        k = int(k)
        k_fetch = min(k + 10, _lib.KNN_MAX_K) if k_fetch is None else int(k_fetch)
        row_tags, query_tags, counts, m = _prep_query_tags(row_tags, query_tags, query_tag_counts, q.shape[0], self.ntotal)
        D, I, K64 = _alloc_out(q, max(k, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_pq(self._h, q.data_ptr(), q_dtype, q.shape[0], k, k_fetch, _ptr(row_tags),
                                                          _ptr(query_tags), m, _ptr(counts), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                          _lib.stream_ptr(q.device)), "radad_knn_search_excl_pq")
        return (D, I, K64) if return_f64 else (D, I)

    def last_excl(self):
        """{"queries", "exact"} of the most recent search_excluding: its batch size and how many of its queries the exact float64 pass
        answered (radad_knn_last_excl; synchronises with that search)"""
        nq, ex = C.c_int64(), C.c_int()
        _lib.check(self._lib.radad_knn_last_excl(self._h, C.byref(nq), C.byref(ex)), "radad_knn_last_excl")
        return {"queries": nq.value, "exact": ex.value}

    def search_excluding_in_scan(self, q, k: int, row_tags, exclude_tags, return_f64: bool = False):
        """search_excluding's result without a k_fetch (radad_knn_search_excl_scan): the admission test sits inside the certified tile
        scan, so the cost does not depend on how much of the store is excluded -- the call for exclusion sets that cover most of it
        (the reference's training_file_ids mode, pipeline.py:500-502).  Arguments and outputs as search_excluding.  Batches the
        plain search would not give to the tile scan (<= 16 queries, small stores, k > 128, dim % 64 != 0) take the row-filtered
        float64 pass for every query: last_excl_scan()["route"]."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        k = int(k)
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        D, I, K64 = _alloc_out(q, max(k, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_scan(self._h, q.data_ptr(), q_dtype, q.shape[0], k, _ptr(row_tags),
                                                            _ptr(exclude_tags), n_excl, D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                            _lib.stream_ptr(q.device)), "radad_knn_search_excl_scan")
        return (D, I, K64) if return_f64 else (D, I)

    def search_excluding_per_query_in_scan(self, q, k: int, row_tags, query_tags, query_tag_counts=None, return_f64: bool = False):
        """search_excluding_per_query's result without a k_fetch (radad_knn_search_excl_scan_pq): the plain certified tile scan, with
        each query's excluded rows cleared out of the scan's buffers before every floor and before the re-rank -- the call for tags
        carried by hundreds or thousands of rows (leave-one-speaker-out), where no k_fetch proves a query.  Arguments and outputs as
        search_excluding_per_query.  Batches the plain search would not give to the tile scan (<= 16 queries, small stores, k > 128,
        dim % 64 != 0) take the per-query float64 pass for every query: last_excl_scan()["route"]."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        k = int(k)
        row_tags, query_tags, counts, m = _prep_query_tags(row_tags, query_tags, query_tag_counts, q.shape[0], self.ntotal)
        D, I, K64 = _alloc_out(q, max(k, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_scan_pq(self._h, q.data_ptr(), q_dtype, q.shape[0], k, _ptr(row_tags),
                                                               _ptr(query_tags), m, _ptr(counts), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                               _lib.stream_ptr(q.device)), "radad_knn_search_excl_scan_pq")
        return (D, I, K64) if return_f64 else (D, I)

    def last_excl_scan(self):
        """{"queries", "route", "exact"} of the most recent search_excluding_in_scan or search_excluding_per_query_in_scan: its batch
        size, "tile" or "exact", and how many of its queries the exact float64 kernel answered (radad_knn_last_excl_scan; synchronises
        with that search)"""
        nq, route, ex = C.c_int64(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_last_excl_scan(self._h, C.byref(nq), C.byref(route), C.byref(ex)), "radad_knn_last_excl_scan")
        return {"queries": nq.value, "route": "tile" if route.value == _lib.EXCL_SCAN_TILE else "exact", "exact": ex.value}

    def range_search_device(self, q, thresh: float, max_per_query: int = 128, return_f64: bool = False):
        """Every stored row within `thresh` of each query, exactly (radad_knn_range_search): squared L2 < thresh, or inner product /
        cosine > thresh, strictly, decided on the float64 key.  q [nq, d] CUDA tensor (float32 or bfloat16) ->
        (counts i32 [nq], D f32 [nq, M], I i64 [nq, M]) on the device, M = max_per_query: counts are the EXACT numbers of rows within
        the radius, also beyond M; each query's first min(count, M) slots hold its best rows in (key, lower id) order, the rest
        -1 / NaN.  With return_f64 also the float64 keys."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        m = int(max_per_query)
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, max(m, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_range_search(self._h, q.data_ptr(), q_dtype, q.shape[0], float(thresh), m, counts.data_ptr(),
                                                        D.data_ptr(), I.data_ptr(), _ptr(K64), _lib.stream_ptr(q.device)),
                       "radad_knn_range_search")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    def range_search(self, x, thresh: float, max_per_query: int = 128, return_counts: bool = False):
        """faiss's index.range_search: -> (lims int64 [nq + 1], D float32 [lims[-1]], I int64 [lims[-1]]), query i's rows at
        lims[i]:lims[i + 1], best first.  Unlike faiss a query's list is cut to its `max_per_query` (<= 1024) best rows; a warning is
        logged once per call when any query was cut, and with return_counts the exact int32 counts (cut or not) come back as a fourth
        value.  numpy in -> numpy out; a CUDA tensor in -> CUDA tensors out."""
        return self._range_csr(x, max_per_query, return_counts, lambda q: self.range_search_device(q, thresh, max_per_query))

    def _range_csr(self, x, max_per_query: int, return_counts: bool, run):
        """range_search's packing of a padded device result: run(q) -> (counts, D, I) for the device queries q"""
        import torch
        is_dev = hasattr(x, "is_cuda") and x.is_cuda
        q = x if is_dev else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.device("cuda", self.device))
        counts, D, I = run(q)
        kept = counts.to(torch.int64).clamp(max=int(max_per_query))
        lims = torch.zeros((q.shape[0] + 1,), dtype=torch.int64, device=q.device)
        lims[1:] = torch.cumsum(kept, 0)
        n_cut = int((counts.to(torch.int64) > kept).sum().item())
        if n_cut:
            logging.warning(f"range_search: {n_cut} of {q.shape[0]} queries have more than max_per_query={int(max_per_query)} rows "
                            "within the radius; their lists were cut to the best (the counts are exact)")
        mask = torch.arange(D.shape[1], device=q.device).unsqueeze(0) < kept.unsqueeze(1)
        out = (lims, D[mask], I[mask]) + ((counts,) if return_counts else ())
        return out if is_dev else tuple(t.cpu().numpy() for t in out)

    def range_search_excluding_device(self, q, thresh: float, row_tags, exclude_tags, max_per_query: int = 128, return_f64: bool = False):
        """range_search_device among the rows whose tag is not in ONE set for the batch (radad_knn_range_search_excl): row_tags int64
        CUDA tensor [ntotal] (indexed by id - id_base), exclude_tags int64 CUDA tensor sorted ascending, or None / empty.  The counts
        are the exact numbers of ADMISSIBLE rows within the radius; an excluded row is never counted and never takes a slot."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        m = int(max_per_query)
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, max(m, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_range_search_excl(self._h, q.data_ptr(), q_dtype, q.shape[0], float(thresh), m, _ptr(row_tags),
                                                             _ptr(exclude_tags), n_excl, counts.data_ptr(), D.data_ptr(), I.data_ptr(),
                                                             _ptr(K64), _lib.stream_ptr(q.device)), "radad_knn_range_search_excl")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    def range_search_excluding_per_query_device(self, q, thresh: float, row_tags, query_tags, query_tag_counts=None, max_per_query: int = 128,
                                                return_f64: bool = False):
        """range_search_device with one exclusion set PER QUERY (radad_knn_range_search_excl_pq; leave-one-file-out, leave-one-speaker-
        out): row r is admissible for query j iff row_tags[r] is not among the first query_tag_counts[j] entries of query_tags[j].
        Tag arguments as search_excluding_per_query (m <= 64 tags per query, any order, repeats allowed, counts clamped to [0, m],
        None = m)."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        m = int(max_per_query)
        row_tags, query_tags, tag_counts, n_tags = _prep_query_tags(row_tags, query_tags, query_tag_counts, q.shape[0], self.ntotal)
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, max(m, 0), return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_range_search_excl_pq(self._h, q.data_ptr(), q_dtype, q.shape[0], float(thresh), m, _ptr(row_tags),
                                                                _ptr(query_tags), n_tags, _ptr(tag_counts), counts.data_ptr(), D.data_ptr(),
                                                                I.data_ptr(), _ptr(K64), _lib.stream_ptr(q.device)),
                       "radad_knn_range_search_excl_pq")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    def range_search_excluding(self, x, thresh: float, row_tags, exclude_tags, max_per_query: int = 128, return_counts: bool = False):
        """range_search among the rows whose tag is not in exclude_tags (one set for the batch): the same CSR result, the counts those
        of the admissible rows.  The tags are CUDA tensors, as for search_excluding_in_scan."""
        return self._range_csr(x, max_per_query, return_counts,
                               lambda q: self.range_search_excluding_device(q, thresh, row_tags, exclude_tags, max_per_query))

    def range_search_excluding_per_query(self, x, thresh: float, row_tags, query_tags, query_tag_counts=None, max_per_query: int = 128,
                                         return_counts: bool = False):
        """range_search with one exclusion set per query: the same CSR result, the counts those of each query's admissible rows.  The
        tags are CUDA tensors, as for search_excluding_per_query_in_scan."""
        return self._range_csr(x, max_per_query, return_counts,
                               lambda q: self.range_search_excluding_per_query_device(q, thresh, row_tags, query_tags, query_tag_counts,
                                                                                      max_per_query))

    def last_range(self):
        """{"queries", "route", "exact"} of the most recent range search: its batch size, "tile", "stream" (<= 16 queries with
        range_smallq) or "exact", and how many of its queries the exact float64 kernel answered (radad_knn_last_range; synchronises
        with that search)"""
        nq, route, ex = C.c_int64(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_last_range(self._h, C.byref(nq), C.byref(route), C.byref(ex)), "radad_knn_last_range")
        name = {_lib.RANGE_TILE: "tile", _lib.RANGE_STREAM: "stream"}.get(route.value, "exact")
        return {"queries": nq.value, "route": name, "exact": ex.value}

    def search_excluding_begin(self, q, k: int, row_tags, exclude_tags, k_fetch=None):
        """first half of search_excluding over a ROW SHARD (radad_knn_search_excl_begin; sharded.ShardedSearch.search_excluding): the
        certified search at k_fetch on this shard and the compaction -> (K64 f64 [nq,k], I i64 [nq,k], FK f64 [nq], FI i64 [nq]): the
        first <= k admissible hits (-1 / NaN padded) and per query the frontier (key, id) behind which every admissible row of the
        shard that is not listed ranks; FI -1 (FK NaN) = the list is all the shard has.  Arguments as search_excluding.  The index
        then holds a begun search until search_excluding_finish or search_abort; q, row_tags and exclude_tags are kept alive."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        if q.shape[0] == 0:
            raise ValueError("search_excluding_begin needs at least one query")
        k = int(k)
        k_fetch = min(k + 10, _lib.KNN_MAX_K) if k_fetch is None else int(k_fetch)
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        nq = q.shape[0]
        K64 = torch.empty((nq, max(k, 0)), device=q.device, dtype=torch.float64)
        I = torch.empty((nq, max(k, 0)), device=q.device, dtype=torch.int64)
        FK = torch.empty((nq,), device=q.device, dtype=torch.float64)
        FI = torch.empty((nq,), device=q.device, dtype=torch.int64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_begin(self._h, q.data_ptr(), q_dtype, nq, k, k_fetch, _ptr(row_tags),
                                                             _ptr(exclude_tags), n_excl, K64.data_ptr(), I.data_ptr(), FK.data_ptr(),
                                                             FI.data_ptr(), _lib.stream_ptr(q.device)), "radad_knn_search_excl_begin")
        self._begun_excl = (q, k, row_tags, exclude_tags)
        return K64, I, FK, FI

    def search_excluding_per_query_begin(self, q, k: int, row_tags, query_tags, query_tag_counts=None, k_fetch=None):
        """first half of search_excluding_per_query over a ROW SHARD (radad_knn_search_excl_pq_begin) -> (K64, I, FK, FI) as
        search_excluding_begin, with the per-query admission test.  It is finished by search_excluding_finish (the begun search
        remembers its rule) or given up by search_abort; q, the tags and the counts are kept alive until then."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        if q.shape[0] == 0:
            raise ValueError("search_excluding_per_query_begin needs at least one query")
        k = int(k)
        k_fetch = min(k + 10, _lib.KNN_MAX_K) if k_fetch is None else int(k_fetch)
        nq = q.shape[0]
        row_tags, query_tags, counts, m = _prep_query_tags(row_tags, query_tags, query_tag_counts, nq, self.ntotal)
        K64 = torch.empty((nq, max(k, 0)), device=q.device, dtype=torch.float64)
        I = torch.empty((nq, max(k, 0)), device=q.device, dtype=torch.int64)
        FK = torch.empty((nq,), device=q.device, dtype=torch.float64)
        FI = torch.empty((nq,), device=q.device, dtype=torch.int64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_pq_begin(self._h, q.data_ptr(), q_dtype, nq, k, k_fetch, _ptr(row_tags),
                                                                _ptr(query_tags), m, _ptr(counts), K64.data_ptr(), I.data_ptr(),
                                                                FK.data_ptr(), FI.data_ptr(), _lib.stream_ptr(q.device)),
                       "radad_knn_search_excl_pq_begin")
        self._begun_excl = (q, k, row_tags, query_tags, counts)
        return K64, I, FK, FI

    def search_excluding_finish(self, unproved=None, return_f64: bool = False):
        """second half: unproved int32 CUDA tensor [nq] (non-zero = no combination of the shards proved the query,
        excl_merge_certify; None = none) -> (D, I[, K64]) as search_excluding: the flagged queries' rows are this shard's exact
        admissible top k (the row-filtered float64 pass where the shard's list could still change; last_excl()["exact"] counts
        them), the others as search_excluding_begin left them."""
        import torch
        if getattr(self, "_begun_excl", None) is None:
            raise ValueError("search_excluding_finish: no exclusion-aware search was begun on this index (search_excluding_begin "
                             "first; a begun search is finished once)")
        q, k = self._begun_excl[:2]
        if unproved is not None:
            _lib.require_cuda(unproved, "unproved")
            unproved = unproved.contiguous().to(torch.int32).reshape(-1)
            if unproved.numel() != q.shape[0]:
                raise ValueError("unproved must hold one flag per query")
        D, I, K64 = _alloc_out(q, k, return_f64)
        keep = self._begun_excl                # (alive until the call below has been enqueued on this stream)
        self._begun_excl = None
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_excl_finish(self._h, _ptr(unproved), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                              _lib.stream_ptr(q.device)), "radad_knn_search_excl_finish")
        del keep
        return (D, I, K64) if return_f64 else (D, I)

    @staticmethod
    def excl_merge_certify(metric: int, keys, ids, fkeys, fids):
        """keys f64 / ids i64 [G, nq, k] and fkeys f64 / fids i64 [G, nq]: every shard's search_excluding_begin result for the same
        queries -> (D f32 [nq,k], I i64 [nq,k], K64 f64 [nq,k], unproved i32 [nq]): the merged admissible top k (-1 / NaN padded)
        and, per query, 1 where the shards together cannot prove it (radad_excl_merge_certify)"""
        import torch
        _lib.require_cuda(keys, "keys")
        G, nq, k = keys.shape
        if tuple(ids.shape) != (G, nq, k) or tuple(fkeys.shape) != (G, nq) or tuple(fids.shape) != (G, nq):
            raise ValueError("excl_merge_certify expects keys / ids [G, nq, k] and frontiers [G, nq]")
        keys, ids = keys.contiguous().to(torch.float64), ids.contiguous().to(torch.int64)
        fkeys, fids = fkeys.contiguous().to(torch.float64), fids.contiguous().to(torch.int64)
        D = torch.empty((nq, k), device=keys.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=keys.device, dtype=torch.int64)
        K64 = torch.empty((nq, k), device=keys.device, dtype=torch.float64)
        U = torch.empty((nq,), device=keys.device, dtype=torch.int32)
        with torch.cuda.device(keys.device):
            _lib.check(_lib.load().radad_excl_merge_certify(int(metric), keys.data_ptr(), ids.data_ptr(), fkeys.data_ptr(), fids.data_ptr(),
                                                            G, nq, k, D.data_ptr(), I.data_ptr(), K64.data_ptr(), U.data_ptr(),
                                                            keys.device.index, _lib.stream_ptr(keys.device)), "radad_excl_merge_certify")
        return D, I, K64, U

    def sharded_excluding(self, row_tags):
        """the (begin, finish, abort) triple sharded.ShardedSearch(excluding=...) takes, for this shard and its rows' tags"""
        def finish(unproved):
            _, I, K64 = self.search_excluding_finish(unproved, return_f64=True)
            return K64, I
        return (lambda q, k, exclude_tags, k_fetch=None: self.search_excluding_begin(q, k, row_tags, exclude_tags, k_fetch)), finish, \
            self.search_abort

    def sharded_excluding_per_query(self, row_tags):
        """the (begin, finish, abort) triple sharded.ShardedSearch(excluding_per_query=...) takes, for this shard and its rows' tags:
        begin(q, k, query_tags [Q, m], query_tag_counts [Q] or None, k_fetch)"""
        def finish(unproved):
            _, I, K64 = self.search_excluding_finish(unproved, return_f64=True)
            return K64, I
        return (lambda q, k, query_tags, query_tag_counts=None, k_fetch=None:
                self.search_excluding_per_query_begin(q, k, row_tags, query_tags, query_tag_counts, k_fetch)), finish, self.search_abort

    def search_begin(self, q, k: int):
        """first half of a search over a row shard (sharded.py): prepares the queries and scans this shard; returns a float32 CUDA
        tensor [nq, k] -- per query lower bounds of the exact scores of this shard's k best rows (q.y / -|q - y|^2; -inf where
        there is none).  The caller gathers them from all shards; the k-th largest of a query's G k values (global_bound below) is
        what search_finish takes."""
        import torch
        q, q_dtype = _prep_queries(q, self.d)
        lb = torch.empty((q.shape[0], int(k)), device=q.device, dtype=torch.float32)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_begin(self._h, q.data_ptr(), q_dtype, q.shape[0], int(k),
                                                        lb.data_ptr(), _lib.stream_ptr(q.device)), "radad_knn_search_begin")
        self._begun = (q, int(k))          # (keeps the queries alive until the second half has read them)
        return lb

    @staticmethod
    def global_bound(lb_all, k: int):
        """lb_all [G, nq, k] (every shard's search_begin result) -> [nq]: the k-th largest of each query's G k lower bounds = a lower
        bound of the exact k-th best score over all shards"""
        import torch
        G, nq, kk = lb_all.shape
        if G * kk > HipFlatIndex.KTH_MAX_VALUES or not lb_all.is_cuda:     # beyond the selection kernel's reach (8 ranks x k > 160): torch
            # (NaN ranks lowest, as in the kernel; torch.topk alone ranks it highest)
            vals = torch.nan_to_num(lb_all.permute(1, 0, 2).reshape(nq, -1).float(), nan=float("-inf"), posinf=float("inf"),
                                    neginf=float("-inf"))
            return torch.topk(vals, int(k), dim=1).values[:, int(k) - 1].contiguous()
        flat = lb_all.contiguous().float()                 # [G][nq][k] as gathered: the kernel reads that layout
        out = torch.empty((nq,), device=flat.device, dtype=torch.float32)
        with torch.cuda.device(flat.device):
            _lib.check(_lib.load().radad_kth_largest(flat.data_ptr(), nq, G, kk, int(k), out.data_ptr(), flat.device.index,
                                                     _lib.stream_ptr(flat.device)), "radad_kth_largest")
        return out

    def search_finish(self, global_lb=None, return_f64: bool = False):
        """second half: float64 re-rank of what can still be among the GLOBAL k best (global_lb: the element-wise maximum of the
        shards' search_begin bounds; None = this shard's own top k), then the exact kernel for uncertified queries.
        -> (D, I[, K64]) as search_device; with a bound a row may hold fewer than k real entries (-1 filled)."""
        import torch
        if getattr(self, "_begun", None) is None:
            raise ValueError("search_finish: no search was begun on this index (search_begin first; a begun search is finished once)")
        q, k = self._begun
        self._begun = None
        D, I, K64 = _alloc_out(q, k, return_f64)
        if global_lb is not None:
            _lib.require_cuda(global_lb, "global_lb")
            global_lb = global_lb.contiguous().float()
            if global_lb.numel() != q.shape[0]:
                raise ValueError("global_lb must hold one bound per query")
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_knn_search_finish(self._h, _ptr(global_lb), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                         _lib.stream_ptr(q.device)), "radad_knn_search_finish")
        return (D, I, K64) if return_f64 else (D, I)

    def search_abort(self):
        """gives up a begun search of either kind, search_begin or search_excluding_begin (the exchange between the shards failed, or
        every query was proved): the index accepts searches again"""
        self._begun = None
        self._begun_excl = None
        _lib.check(self._lib.radad_knn_search_abort(self._h), "radad_knn_search_abort")

    KTH_MAX_VALUES = 1280        # radad_kth_largest: groups x per_group values per query (csrc/knn.hip KTH_PER_LANE x 64)

    def reconstruct_batch(self, idx):
        """idx: int64 CUDA tensor of any shape -> [*idx.shape, d]; negative ids give zero rows."""
        import torch
        _lib.require_cuda(idx, "idx")
        flat = idx.contiguous().to(torch.int64).reshape(-1)
        out = torch.empty((flat.numel(), self.d), device=idx.device, dtype=torch.float32)
        with torch.cuda.device(idx.device):
            _lib.check(self._lib.radad_knn_reconstruct(self._h, flat.data_ptr(), flat.numel(), out.data_ptr(),
                                                       _lib.stream_ptr(idx.device)), "radad_knn_reconstruct")
        return out.reshape(*idx.shape, self.d)

    def plane_info(self):
        """{"built", "centred", "one_scale", "rebuilds"} of the f16 plane the certified scans read (radad_knn_plane_info, _plane_rebuilds)"""
        b, c, o, r = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_plane_info(self._h, C.byref(b), C.byref(c), C.byref(o)))
        _lib.check(self._lib.radad_knn_plane_rebuilds(self._h, C.byref(r)))
        return {"built": bool(b.value), "centred": bool(c.value), "one_scale": bool(o.value), "rebuilds": r.value}

    def last_emitted(self, nq: int):
        """(candidates emitted per query int32 [nq], final admission floors float32 [nq]) of the last tile-scan search (radad_knn_last_emitted)"""
        c = np.empty(nq, np.int32)
        f = np.empty(nq, np.float32)
        _lib.check(self._lib.radad_knn_last_emitted(self._h, c.ctypes.data, f.ctypes.data, int(nq)), "radad_knn_last_emitted")
        return c, f

    def set_abandon(self, value):
        """RADAD_KNN_OPT_ABANDON at any time: 1 = the tile scan leaves tiles that cannot reach the admission floor (default), 0 = never
        (same results; A/B measurements and the parity tests)"""
        _lib.check(self._lib.radad_knn_set_option(self._h, _lib.KNN_OPT_ABANDON, int(value)), "radad_knn_set_option")
        self.options["abandon"] = int(value)

    def last_abandon(self):
        """{"checked", "skipped", "tasks"}: of the (query tile, row tile) tasks the last search's abandoning scan launches covered, how
        many ran the abandon test and how many were left after it (radad_knn_last_abandon; all 0 when no launch abandoned)"""
        c, s, t = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self._lib.radad_knn_last_abandon(self._h, C.byref(c), C.byref(s), C.byref(t)), "radad_knn_last_abandon")
        return {"checked": c.value, "skipped": s.value, "tasks": t.value}

    def set_abandon_deal(self, value):
        """RADAD_KNN_OPT_ABANDON_DEAL at any time: 1 = abandoning launches that qualify deal their row tiles to the workgroups by ticket,
        0 = every launch walks static chunks (the default; same results; A/B measurements and the parity tests)"""
        _lib.check(self._lib.radad_knn_set_option(self._h, _lib.KNN_OPT_ABANDON_DEAL, int(value)), "radad_knn_set_option")
        self.options["abandon_deal"] = int(value)

    def last_abandon_deal(self):
        """{"launches", "workgroups", "granule"}: how many abandoning launches of the last search were dealt by ticket, and the grid and
        the row tiles per granule of the last of them (radad_knn_last_abandon_deal; all 0 when none was)"""
        n, w, g = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_last_abandon_deal(self._h, C.byref(n), C.byref(w), C.byref(g)), "radad_knn_last_abandon_deal")
        return {"launches": n.value, "workgroups": w.value, "granule": g.value}

    def set_abandon_defer(self, value):
        """RADAD_KNN_OPT_ABANDON_DEFER at any time: 1 = a vetoed tile with at most 16 live rows lists them for the launch's tail and is
        left as a skipped one, 0 = a vetoed tile is multiplied in full (same results; A/B measurements and the parity tests)"""
        _lib.check(self._lib.radad_knn_set_option(self._h, _lib.KNN_OPT_ABANDON_DEFER, int(value)), "radad_knn_set_option")
        self.options["abandon_defer"] = int(value)

    def last_abandon_defer(self):
        """{"tile_tasks_deferred", "rows_listed", "tail_launches"} of the last search's deferring launches
        (radad_knn_last_abandon_defer; all 0 when none deferred)"""
        t, r, n = C.c_int64(), C.c_int64(), C.c_int()
        _lib.check(self._lib.radad_knn_last_abandon_defer(self._h, C.byref(t), C.byref(r), C.byref(n)), "radad_knn_last_abandon_defer")
        return {"tile_tasks_deferred": t.value, "rows_listed": r.value, "tail_launches": n.value}

    def set_abandon_ahead(self, value):
        """RADAD_KNN_OPT_ABANDON_AHEAD at any time: 1 = the checkpoint stage of a tile expected to leave fetches the next tile's head,
        0 = it fetches the tile's own next stage (same results; A/B measurements and the parity tests)"""
        _lib.check(self._lib.radad_knn_set_option(self._h, _lib.KNN_OPT_ABANDON_AHEAD, int(value)), "radad_knn_set_option")
        self.options["abandon_ahead"] = int(value)

    def last_abandon_ahead(self):
        """{"used", "wasted"}: tile tasks of the last search that left into a head fetched ahead, and tile tasks that stayed and threw
        one away (radad_knn_last_abandon_ahead; both 0 when no launch fetched ahead)"""
        u, w = C.c_int64(), C.c_int64()
        _lib.check(self._lib.radad_knn_last_abandon_ahead(self._h, C.byref(u), C.byref(w)), "radad_knn_last_abandon_ahead")
        return {"used": u.value, "wasted": w.value}

    def tuning_info(self):
        """{"cap_boost", "fp32_searches_left", "reports_consumed"} (radad_knn_tuning_info): read without synchronising"""
        a, b, n = C.c_int(), C.c_int(), C.c_int64()
        _lib.check(self._lib.radad_knn_tuning_info(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return {"cap_boost": a.value, "fp32_searches_left": b.value, "reports_consumed": n.value}

    def last_launch(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_last_launch(self._h, C.byref(a), C.byref(b), C.byref(c)))
        st, nq = (C.c_int * 6)(), C.c_int64()
        _lib.check(self._lib.radad_knn_last_certificate(self._h, C.byref(nq), st))
        kind, nl, nph = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_knn_last_scan_kind(self._h, C.byref(kind)))
        _lib.check(self._lib.radad_knn_last_scan_launches(self._h, C.byref(nl)))
        _lib.check(self._lib.radad_knn_last_scan_phases(self._h, C.byref(nph)))
        return {"query_tiles": a.value, "db_splits": b.value, "block_threads": c.value, "rechecked_queries": st[0],
                "scan_launches": nl.value, "scan_phases": nph.value, "early_abandon": self.last_abandon(),
                "abandon_deal": self.last_abandon_deal(), "abandon_defer": self.last_abandon_defer(),
                "abandon_ahead": self.last_abandon_ahead(),
                "scan_kind": ("f32_tile", "hi_tile", "f32_smallq", "hi_smallq", "f16_tile", "f32_dense")[kind.value],
                "certificate": {"queries": nq.value, "rejected": st[0], "candidates_rescored": st[1],
                                "rejected_buffer_full": st[2], "rejected_list_used_up": st[3],
                                "rejected_floor_above_threshold": st[4], "rejected_scan_dropped": st[5]}}

    def profile(self, enable: bool = True, every: int = 1):
        """record HIP events around every scan-kernel launch (ring of 64) of every `every`-th search"""
        _lib.check(self._lib.radad_knn_profile(self._h, max(1, int(every)) if enable else 0), "radad_knn_profile")

    def profile_read(self):
        """scan-kernel durations in ms (synchronises on the recorded events)"""
        buf = (C.c_float * 64)()
        n = C.c_int()
        _lib.check(self._lib.radad_knn_profile_read(self._h, buf, 64, C.byref(n)), "radad_knn_profile_read")
        return [float(buf[i]) for i in range(n.value)]

    def save(self, path: str):
        _lib.check(self._lib.radad_knn_save(self._h, os.fsencode(path)), "radad_knn_save")

    def load(self, path: str, row0: int = 0, n_rows: int = -1):
        """replace the contents with rows [row0, row0+n_rows) of a snapshot (default: all of it).  A rank of a sharded
        run loads its own slice of one shared file: HipFlatIndex.load_shard."""
        _lib.check(self._lib.radad_knn_load_range(self._h, os.fsencode(path), int(row0), int(n_rows)), "radad_knn_load")

    @staticmethod
    def snapshot_info(path: str) -> dict:
        """header of a snapshot file: {"d", "metric", "store_f16", "ntotal"}"""
        d, m, t, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        _lib.check(_lib.load().radad_knn_snapshot_info(os.fsencode(path), C.byref(d), C.byref(m), C.byref(t), C.byref(n)),
                   "radad_knn_snapshot_info")
        return {"d": d.value, "metric": m.value, "store_f16": t.value == _lib.STORE_F16, "ntotal": n.value}

    @classmethod
    def load_shard(cls, path: str, rank: int, world_size: int, device: int = 0):
        """this rank's row shard of a snapshot written by any number of GPUs: rows shard_bounds(ntotal, world, rank),
        ids reported globally (id_base = first row).  Only the shard's byte range of the file is read."""
        from .sharded import shard_bounds
        info = cls.snapshot_info(path)
        lo, hi = shard_bounds(info["ntotal"], world_size, rank)
        index = cls(info["d"], info["metric"], device=device, id_base=lo, store_f16=info["store_f16"])
        index.load(path, lo, hi - lo)
        return index


class HipIVFFlatIndex:
    """faiss.IndexIVFFlat(IndexFlatL2(d), d, nlist, METRIC_L2) on the GPU: the slice of its surface the reference uses
    (vector_database.py:65-70,124-128,138,174-181; pipeline.py:503): d, nlist, nprobe, is_trained, ntotal, train, add,
    search, reconstruct."""

    def __init__(self, d: int, nlist: int, device: int = 0, niter: int = 10, hi_scan=None, pq_filter=None):
        """hi_scan: 0 keeps the list scans on the fp32 rows (radad_ivf_set_option; None = the library's default, the certified f16 scan);
        2 (tests) sends every query through the exact float64 list scan that answers the queries a certificate rejects.
        pq_filter: 0 (tests) makes search_probed_excluding_per_query treat every row as suspect (RADAD_IVF_OPT_PQ_FILTER; same results)"""
        self._lib = _lib.load()
        self.d, self.nlist, self.device, self.niter = int(d), int(nlist), int(device), int(niter)
        self.nprobe = 1                      # faiss default; the reference sets it from config.vector_db_nprobe (:177)
        self.id_base = 0
        self.metric = _lib.METRIC_L2
        self.store_f16 = False
        h = C.c_void_p()
        _lib.check(self._lib.radad_ivf_create(self.d, self.nlist, self.device, C.byref(h)), "radad_ivf_create")
        self._h = h
        if hi_scan is not None:
            _lib.check(self._lib.radad_ivf_set_option(self._h, _lib.IVF_OPT_HI_SCAN, int(hi_scan)), "radad_ivf_set_option")
        if pq_filter is not None:
            self.set_pq_filter(pq_filter)

    def set_pq_filter(self, value):
        """RADAD_IVF_OPT_PQ_FILTER: 1 = the suspect pre-pass of search_probed_excluding_per_query (default), 0 (tests) = every row suspect"""
        _lib.check(self._lib.radad_ivf_set_option(self._h, _lib.IVF_OPT_PQ_FILTER, int(value)), "radad_ivf_set_option")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.radad_ivf_destroy(h)
            except Exception:
                pass

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    @property
    def is_trained(self) -> bool:
        t = C.c_int()
        _lib.check(self._lib.radad_ivf_is_trained(self._h, C.byref(t)))
        return bool(t.value)

    @property
    def ntotal(self) -> int:
        n = C.c_int64()
        _lib.check(self._lib.radad_ivf_ntotal(self._h, C.byref(n)))
        return n.value

    def _to_dev(self, x):
        import torch
        if isinstance(x, torch.Tensor):
            return _lib.require_cuda(x, "x").contiguous().float()
        return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self._dev())

    def train(self, x):
        import torch
        t = self._to_dev(x)
        with torch.cuda.device(t.device):
            _lib.check(self._lib.radad_ivf_train(self._h, t.data_ptr(), t.shape[0], self.niter, _lib.stream_ptr(t.device)), "radad_ivf_train")

    def set_centroids(self, c):
        import torch
        t = self._to_dev(c)
        if tuple(t.shape) != (self.nlist, self.d):
            raise ValueError(f"centroids must be [{self.nlist}, {self.d}]")
        with torch.cuda.device(t.device):
            _lib.check(self._lib.radad_ivf_set_centroids(self._h, t.data_ptr(), _lib.stream_ptr(t.device)), "radad_ivf_set_centroids")

    def centroids(self) -> np.ndarray:
        import torch
        out = torch.empty((self.nlist, self.d), device=self._dev())
        with torch.cuda.device(out.device):
            _lib.check(self._lib.radad_ivf_centroids(self._h, out.data_ptr(), _lib.stream_ptr(out.device)))
        return out.cpu().numpy()

    def assignments(self) -> np.ndarray:
        out = np.empty(self.ntotal, np.int32)
        _lib.check(self._lib.radad_ivf_assignments_host(self._h, out.ctypes.data, out.size))
        return out

    def add(self, x):
        import torch
        t = self._to_dev(x)
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}], got {tuple(t.shape)}")
        with torch.cuda.device(t.device):
            _lib.check(self._lib.radad_ivf_add(self._h, t.data_ptr(), t.shape[0], _lib.stream_ptr(t.device)), "radad_ivf_add")

    add_device = add

    def remove_ids(self, ids, return_map: bool = False):
        raise ValueError("HipIVFFlatIndex.remove_ids: an IVF store keeps list-major copies of its rows, which cannot be compacted in "
                         "place; rebuild the index from the rows that stay (or keep the store flat: HipFlatIndex.remove_ids)")

    MAX_K = 128    # csrc/ivf.inc: up to k = 26 the probed lists are scanned (k + 6 candidates per (query, list) in 32-entry register
                    # lists); 27..128 is answered by the exact certified scan of the same rows (recall 1.0, the flat scan's cost)

    def search_device(self, q, k: int):
        import torch
        if k > self.MAX_K:      # faiss accepts k up to 2048; refusing loudly beats the silent empty result a swallowed error gives
            raise ValueError(f"HipIVFFlatIndex supports k <= {self.MAX_K} (asked for {k}); use a flat index for larger k")
        q = self._to_dev(q)
        D = torch.empty((q.shape[0], k), device=q.device, dtype=torch.float32)
        I = torch.empty((q.shape[0], k), device=q.device, dtype=torch.int64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_search(self._h, q.data_ptr(), q.shape[0], int(k), int(self.nprobe), D.data_ptr(), I.data_ptr(),
                                                  _lib.stream_ptr(q.device)), "radad_ivf_search")
        ex = C.c_int()
        _lib.check(self._lib.radad_ivf_last_search_exact(self._h, C.byref(ex)))
        self.last_search_exact = bool(ex.value)
        if self.last_search_exact and not getattr(self, "_warned_exact", False):
            self._warned_exact = True
            logging.getLogger(__name__).warning(
                "HipIVFFlatIndex: k=%d > 26 is answered by the exact scan of all rows (a superset of the nprobe=%d lists' rows, at the "
                "flat search's cost); faiss.IndexIVFFlat would return rows of the probed lists only", k, self.nprobe)
        return D, I

    def search(self, x, k: int):
        D, I = self.search_device(x, k)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_excluding(self, *args, **kwargs):
        raise ValueError("exclusion-aware search is flat and single-handle only: an IVF search sees the probed lists, not the store")

    def search_excluding_per_query(self, *args, **kwargs):
        raise ValueError("search_excluding_per_query is the flat store's search: an IVF search sees the probed lists, not the store "
                         "(search_probed_excluding_per_query takes one set per query, search_probed_excluding one for the batch)")

    def search_excluding_in_scan(self, *args, **kwargs):
        raise ValueError("search_excluding_in_scan is the flat store's search: an IVF index has the admission test inside its own list "
                         "scans (search_probed_excluding)")

    def search_excluding_per_query_in_scan(self, *args, **kwargs):
        raise ValueError("search_excluding_per_query_in_scan is the flat store's search: an IVF index has the per-(row, query) test "
                         "inside its own list scans (search_probed_excluding_per_query)")

    def range_search(self, *args, **kwargs):
        raise ValueError("range_search is the flat store's search: an IVF search sees the probed lists, not the store, so it cannot "
                         "say that no other row is within the radius")

    def range_search_excluding(self, *args, **kwargs):
        raise ValueError("range_search_excluding is the flat store's search: an IVF search sees the probed lists, not the store, so it "
                         "cannot say that no other admissible row is within the radius")

    def range_search_excluding_per_query(self, *args, **kwargs):
        raise ValueError("range_search_excluding_per_query is the flat store's search: an IVF search sees the probed lists, not the "
                         "store, so it cannot say that no other admissible row is within the radius")

    def range_search_probed_device(self, q, thresh: float, max_per_query: int = 128, return_f64: bool = False):
        """Every row of the self.nprobe probed lists within `thresh` of each query, exactly (radad_ivf_range_search): squared L2 <
        thresh, strictly, decided on the float64 key -- the exact range search restricted to the probed lists, as search is the exact
        top-k restricted to them (nprobe == nlist: HipFlatIndex.range_search on the same rows).  q [nq, d] float32 CUDA tensor ->
        (counts i32 [nq], D f32 [nq, M], I i64 [nq, M]) on the device, M = max_per_query <= 128: counts are the EXACT numbers of
        members, also beyond M; each query's first min(count, M) slots hold its best members in (key, lower insertion id) order, the
        rest -1 / NaN.  With return_f64 also the float64 keys."""
        import torch
        m = self._range_probed_m(thresh, max_per_query)
        q = self._to_dev(q)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_search_probed expects [nq, {self.d}], got {tuple(q.shape)}")
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, m, return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_range_search(self._h, q.data_ptr(), q.shape[0], int(self.nprobe), float(thresh), m,
                                                        counts.data_ptr(), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                        _lib.stream_ptr(q.device)), "radad_ivf_range_search")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    @staticmethod
    def _range_probed_m(thresh, max_per_query) -> int:
        """the argument checks of range_search_probed*, before anything goes to the device"""
        m = int(max_per_query)
        if not 1 <= m <= _lib.IVF_MAX_K:
            raise ValueError(f"range_search_probed supports 1 <= max_per_query <= {_lib.IVF_MAX_K} (asked for {m}); the count is exact: "
                             "narrow the radius")
        if thresh != thresh:
            raise ValueError("range_search_probed: the radius is NaN")
        return m

    _range_csr = HipFlatIndex._range_csr      # the packing of a padded device result into faiss's CSR form (it reads self.device)

    def range_search_probed(self, x, thresh: float, max_per_query: int = 128, return_counts: bool = False):
        """range_search_probed_device in faiss's CSR form, as HipFlatIndex.range_search: -> (lims int64 [nq + 1], D float32
        [lims[-1]], I int64 [lims[-1]]) (+ the exact int32 counts with return_counts); numpy in -> numpy out, CUDA in -> CUDA out."""
        self._range_probed_m(thresh, max_per_query)
        return self._range_csr(x, max_per_query, return_counts, lambda q: self.range_search_probed_device(q, thresh, max_per_query))

    def range_search_probed_excluding_device(self, q, thresh: float, row_tags, exclude_tags, max_per_query: int = 128,
                                             return_f64: bool = False):
        """range_search_probed_device among the rows whose tag is not in ONE set for the batch (radad_ivf_range_search_excl): row_tags
        int64 CUDA tensor [ntotal] by insertion id, exclude_tags int64 CUDA tensor sorted ascending, or None / empty.  The counts are
        the exact numbers of ADMISSIBLE members of the probed lists; an excluded row is never counted, never takes one of the M slots
        and never takes a slot of a query's candidate buffer inside the list scan."""
        import torch
        m = self._range_probed_m(thresh, max_per_query)
        q = self._to_dev(q)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_search_probed_excluding expects [nq, {self.d}], got {tuple(q.shape)}")
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, m, return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_range_search_excl(self._h, q.data_ptr(), q.shape[0], int(self.nprobe), float(thresh), m,
                                                             _ptr(row_tags), _ptr(exclude_tags), n_excl, counts.data_ptr(), D.data_ptr(),
                                                             I.data_ptr(), _ptr(K64), _lib.stream_ptr(q.device)),
                       "radad_ivf_range_search_excl")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    def range_search_probed_excluding_per_query_device(self, q, thresh: float, row_tags, query_tags, query_tag_counts=None,
                                                       max_per_query: int = 128, return_f64: bool = False):
        """range_search_probed_device with one exclusion set PER QUERY (radad_ivf_range_search_excl_pq; leave-one-file-out, leave-one-
        speaker-out): row r is admissible for query j iff row_tags[r] is not among the first query_tag_counts[j] entries of
        query_tags[j].  Tag arguments as search_probed_excluding_per_query (m <= 64 tags per query, any order, repeats allowed, counts
        clamped to [0, m], None = m)."""
        import torch
        m = self._range_probed_m(thresh, max_per_query)
        q = self._to_dev(q)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_search_probed_excluding_per_query expects [nq, {self.d}], got {tuple(q.shape)}")
        row_tags, query_tags, tag_counts, n_tags = _prep_query_tags(row_tags, query_tags, query_tag_counts, q.shape[0], self.ntotal)
        counts = torch.empty((q.shape[0],), device=q.device, dtype=torch.int32)
        D, I, K64 = _alloc_out(q, m, return_f64)
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_range_search_excl_pq(self._h, q.data_ptr(), q.shape[0], int(self.nprobe), float(thresh), m,
                                                                _ptr(row_tags), _ptr(query_tags), n_tags, _ptr(tag_counts),
                                                                counts.data_ptr(), D.data_ptr(), I.data_ptr(), _ptr(K64),
                                                                _lib.stream_ptr(q.device)), "radad_ivf_range_search_excl_pq")
        return (counts, D, I, K64) if return_f64 else (counts, D, I)

    def range_search_probed_excluding(self, x, thresh: float, row_tags, exclude_tags, max_per_query: int = 128, return_counts: bool = False):
        """range_search_probed_excluding_device in faiss's CSR form, as range_search_probed; the tags are CUDA tensors."""
        self._range_probed_m(thresh, max_per_query)
        return self._range_csr(x, max_per_query, return_counts,
                               lambda q: self.range_search_probed_excluding_device(q, thresh, row_tags, exclude_tags, max_per_query))

    def range_search_probed_excluding_per_query(self, x, thresh: float, row_tags, query_tags, query_tag_counts=None, max_per_query: int = 128,
                                                return_counts: bool = False):
        """range_search_probed_excluding_per_query_device in faiss's CSR form, as range_search_probed; the tags are CUDA tensors."""
        self._range_probed_m(thresh, max_per_query)
        return self._range_csr(x, max_per_query, return_counts,
                               lambda q: self.range_search_probed_excluding_per_query_device(q, thresh, row_tags, query_tags,
                                                                                             query_tag_counts, max_per_query))

    def last_range(self) -> dict:
        """{"queries", "route": "hi_lists" | "exact_lists", "exact": queries the exact float64 list scan answered, "max_emitted": the
        largest number of positions one query's f16 scan emitted (0 on the exact route; admissible (row, query) pairs only after an
        exclusion-aware call)} of the most recent range_search_probed* call
        (radad_ivf_last_range; synchronises with it; a ValueError when the most recent search was not a range search)"""
        nq, route, ex, me = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_ivf_last_range(self._h, C.byref(nq), C.byref(route), C.byref(ex), C.byref(me)), "radad_ivf_last_range")
        return {"queries": nq.value, "route": _lib.IVF_RANGE_ROUTES[route.value], "exact": ex.value, "max_emitted": me.value}

    MAX_K_PROBED = 26  # csrc/ivf.inc: the largest k the list scans hold (k + 6 <= 32 entries per (query, list))

    def search_probed_excluding(self, q, k: int, row_tags, exclude_tags):
        """The k nearest rows of the nprobe probed lists whose tag is not excluded, exactly (radad_ivf_search_excl: the admission test
        sits inside the list scans, so the cost does not depend on how many excluded rows crowd a query): q [nq, d] CUDA tensor,
        row_tags int64 CUDA tensor [ntotal] by insertion id, exclude_tags int64 CUDA tensor sorted ascending, or None / empty
        -> (D f32 [nq,k], I i64 [nq,k]) on the device, ordered by (float64 distance, lower id); slots beyond the admissible rows of the
        probed lists hold -1 / NaN.  Uses self.nprobe.  k <= 26: a larger k is NOT forwarded to the flat store as search does."""
        import torch
        k = int(k)
        if k > self.MAX_K_PROBED:
            raise ValueError(f"search_probed_excluding supports k <= {self.MAX_K_PROBED}, the range the list scans hold (asked for {k})")
        q = self._to_dev(q)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}], got {tuple(q.shape)}")
        row_tags, exclude_tags, n_excl = _prep_tags(row_tags, exclude_tags, self.ntotal)
        D, I, _ = _alloc_out(q, max(k, 0))
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_search_excl(self._h, q.data_ptr(), q.shape[0], k, int(self.nprobe), _ptr(row_tags),
                                                       _ptr(exclude_tags), n_excl, D.data_ptr(), I.data_ptr(),
                                                       _lib.stream_ptr(q.device)), "radad_ivf_search_excl")
        self.last_search_exact = False
        return D, I

    def search_probed_excluding_per_query(self, q, k: int, row_tags, query_tags, query_tag_counts=None):
        """search_probed_excluding with one exclusion set PER QUERY (radad_ivf_search_excl_pq; leave-one-out): row r is admissible for
        query j iff row_tags[r] is not among the first query_tag_counts[j] entries of query_tags[j].  query_tags int64 CUDA tensor
        [nq, m], m <= 64, any order, duplicates allowed ([nq] = one tag per query; None or m = 0 = nothing excluded); query_tag_counts
        int32 CUDA tensor [nq], clamped to [0, m] on the device, None = m for every query.  Everything else as search_probed_excluding;
        the result of a query does not depend on what the other queries of the batch exclude."""
        import torch
        k = int(k)
        if k > self.MAX_K_PROBED:
            raise ValueError(f"search_probed_excluding_per_query supports k <= {self.MAX_K_PROBED}, the range the list scans hold (asked for {k})")
        q = self._to_dev(q)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}], got {tuple(q.shape)}")
        row_tags, query_tags, counts, m = _prep_query_tags(row_tags, query_tags, query_tag_counts, q.shape[0], self.ntotal)
        D, I, _ = _alloc_out(q, max(k, 0))
        with torch.cuda.device(q.device):
            _lib.check(self._lib.radad_ivf_search_excl_pq(self._h, q.data_ptr(), q.shape[0], k, int(self.nprobe), _ptr(row_tags),
                                                          _ptr(query_tags), m, _ptr(counts), D.data_ptr(), I.data_ptr(),
                                                          _lib.stream_ptr(q.device)), "radad_ivf_search_excl_pq")
        self.last_search_exact = False
        return D, I

    def last_search_info(self) -> dict:
        """{"scan": "f32_lists" | "hi_lists" | "exact_flat", "rejected": queries the list scan's certificate could not certify,
        "exact": queries the exact float64 list scan answered (the rejected ones)} of the most recent search (synchronises with it)"""
        kind, rej, ex = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.radad_ivf_last_search_info(self._h, C.byref(kind), C.byref(rej)), "radad_ivf_last_search_info")
        _lib.check(self._lib.radad_ivf_last_search_counts(self._h, C.byref(rej), C.byref(ex)), "radad_ivf_last_search_counts")
        return {"scan": _lib.IVF_SCAN_KINDS[kind.value], "rejected": rej.value, "exact": ex.value}

    SNAPSHOT_CHUNK = 1 << 18

    def save(self, path: str):
        """rows in insertion order as a native flat snapshot at `path` (gathered on the device chunk by chunk into a scratch
        flat store and streamed out by radad_knn_save: the store never exists in host memory), centroids at path + '.ivf.npz'"""
        import torch
        flat = HipFlatIndex(self.d, _lib.METRIC_L2, device=self.device)
        n = self.ntotal
        flat.reserve(max(n, 1))
        for s0 in range(0, n, self.SNAPSHOT_CHUNK):
            ids = torch.arange(s0, min(n, s0 + self.SNAPSHOT_CHUNK), device=self._dev())
            flat.add_device(self.reconstruct_batch(ids))
        flat.save(path)
        with open(path + ".ivf.npz", "wb") as f:
            np.savez(f, kind="radad_ivf", centroids=self.centroids(), nlist=self.nlist, ntotal=n)

    def load(self, path: str):
        """inverse of save(): the centroids are installed as they were, the rows are re-added in insertion order (so ids and list
        contents come out as before); the snapshot is streamed to the device by radad_knn_load"""
        import torch
        z = np.load(path + ".ivf.npz")
        centroids = z["centroids"]
        if centroids.shape != (self.nlist, self.d):
            raise ValueError(f"snapshot has {centroids.shape[0]} lists of dimension {centroids.shape[1]}, index has {self.nlist} x {self.d}")
        if self.ntotal:
            raise ValueError("load() needs an empty IVF index")
        self.set_centroids(centroids)
        flat = HipFlatIndex(self.d, _lib.METRIC_L2, device=self.device)
        flat.load(path)
        if flat.ntotal != int(z["ntotal"]):
            raise ValueError(f"{path} holds {flat.ntotal} rows, its sidecar says {int(z['ntotal'])}")
        for s0 in range(0, flat.ntotal, self.SNAPSHOT_CHUNK):
            ids = torch.arange(s0, min(flat.ntotal, s0 + self.SNAPSHOT_CHUNK), device=self._dev())
            self.add(flat.reconstruct_batch(ids))

    def reconstruct_batch(self, idx):
        import torch
        _lib.require_cuda(idx, "idx")
        flat = idx.contiguous().to(torch.int64).reshape(-1)
        out = torch.empty((flat.numel(), self.d), device=idx.device, dtype=torch.float32)
        with torch.cuda.device(idx.device):
            _lib.check(self._lib.radad_ivf_reconstruct(self._h, flat.data_ptr(), flat.numel(), out.data_ptr(), _lib.stream_ptr(idx.device)))
        return out.reshape(*idx.shape, self.d)

    def reconstruct(self, i: int) -> np.ndarray:
        import torch
        return self.reconstruct_batch(torch.tensor([int(i)], device=self._dev()))[0].cpu().numpy()


class VectorDatabase:
    """Store of clip embeddings + brute-force retrieval (vector_database.py:8-272)."""

    def __init__(self, config):
        self.config = config
        self.index = None
        self.vector_paths: List[str] = []
        self.vector_labels: List = []
        self.vector_metadata: Dict[str, list] = {}
        self.db_path = os.path.join(config.vector_db_path, "faiss_index.bin")   # file names kept (vector_database.py:18-19)
        self.metadata_path = os.path.join(config.vector_db_path, "metadata.pkl")
        self.device_id = 0
        os.makedirs(config.vector_db_path, exist_ok=True)
        self._cosine = False
        self._tags_host: List[int] = []      # path_tag of every stored row (device copy built lazily)
        self._tag_names: Dict[int, str] = {}  # tag -> basename, to assert the tags are collision-free
        self._tags_dev = None
        self._labels_dev = None
        import torch
        dev = torch.device(getattr(config, "device", "cuda"))
        if dev.type == "cuda":
            self.device_id = dev.index if dev.index is not None else torch.cuda.current_device()

    # vector_database.py:56-97
    def create_index(self, dimension: int, id_base: int = 0):
        index_type = self.config.vector_db_index_type.upper()
        self._cosine = (index_type == "IP") and bool(getattr(self.config, "normalize_for_ip", True))
        if index_type == "L2":
            metric = _lib.METRIC_L2
        elif index_type == "IP":
            metric = _lib.METRIC_COSINE if self._cosine else _lib.METRIC_IP
        elif index_type == "IVF":
            nlist = max(64, int(getattr(self.config, "ivf_nlist", 4096)))                     # vector_database.py:67-68
            self.index = HipIVFFlatIndex(dimension, nlist, self.device_id)
            logging.info(f"Created HIP IVF-flat index on device {self.device_id} dim={dimension} nlist={nlist}")
            return
        else:
            raise ValueError(f"Unsupported index type: {index_type}")
        self.index = HipFlatIndex(dimension, metric, self.device_id, id_base,
                                  store_f16=bool(getattr(self.config, "use_float16", False)),
                                  **knn_options_from_config(self.config))          # vector_database.py:80
        logging.info(f"Created HIP flat index on device {self.device_id} dim={dimension} type={index_type}")

    # vector_database.py:108-151
    def add_vectors_batch(self, vectors, paths: List[str], labels: List[int], metadata: Dict, batch_size: int = 10000):
        if vectors.shape[0] == 0:
            logging.warning("No vectors to add to database")
            return
        if self.index is None:
            self.create_index(vectors.shape[1])
        is_dev = hasattr(vectors, "is_cuda") and vectors.is_cuda
        if not is_dev:
            vectors = np.ascontiguousarray(np.asarray(vectors).astype(np.float32, copy=False))
        try:     # IVF: train once, on a representative prefix, before adding (vector_database.py:122-130)
            if hasattr(self.index, "is_trained") and not self.index.is_trained:
                logging.info("Training IVF index...")
                self.index.train(vectors[:min(50000, vectors.shape[0])])
        except Exception as e:
            logging.warning(f"Index training skipped/failed: {e}")
        total = vectors.shape[0]
        added = 0
        for start in range(0, total, batch_size):
            end = min(start + batch_size, total)
            # the 63-bit tags stand in for the basename strings the reference compares (pipeline.py:495-502): two distinct
            # basenames must never share one.  Checked before anything is added (a collision is a hard error, not a skipped batch).
            batch_tags = []
            for p_ in paths[start:end]:
                t_, b_ = path_tag(p_), os.path.basename(p_)
                if self._tag_names.setdefault(t_, b_) != b_:
                    raise RuntimeError(f"path_tag collision between {self._tag_names[t_]!r} and {b_!r}")
                batch_tags.append(t_)
            try:
                if is_dev:
                    self.index.add_device(vectors[start:end])
                else:
                    self.index.add(vectors[start:end])     # normalisation for cosine happens in the add kernel
                added += end - start
                self._tags_host.extend(batch_tags)
                self._tags_dev = self._labels_dev = None
                self.vector_paths.extend(paths[start:end])
                self.vector_labels.extend(labels[start:end])
                for key, values in metadata.items():
                    self.vector_metadata.setdefault(key, [])
                    vals = values[start:end] if hasattr(values, "__getitem__") else [values] * (end - start)
                    self.vector_metadata[key].extend(vals)
            except Exception as e:   # log-and-skip, as vector_database.py:147-149
                logging.error(f"Error adding batch {start}-{end}: {e}")
                continue
        logging.info(f"Added {added}/{total} vectors. Index ntotal={self.index.ntotal}")

    # vector_database.py:154-157
    def add_vectors(self, vectors, paths: List[str], labels: List[int], metadata: Dict):
        self.add_vectors_batch(vectors, paths, labels, metadata, getattr(self.config, "vector_add_batch_size", 10000))

    # ---- acting on an audit: forget rows (faiss remove_ids; the reference's VectorDatabase never got one) ------------------------
    def remove_vectors(self, ids) -> int:
        """Remove the rows with these ids (as search_batch returns them) from a flat store, in place on the device, and cut
        vector_paths, vector_labels and every vector_metadata column to the rows that stay: row i stays aligned with vector_paths[i].
        ids: list / numpy / int64 tensor, any order; repeats and ids that name no row are ignored.  -> rows removed.  An IVF store
        raises ValueError and is left as it was.  On a row shard (load(shard=...)) only ids of the shard's own range count and ids
        shift inside the shard only: the global id space then has a gap in front of the next shard."""
        if self.index is None:
            raise ValueError("Vector database is empty. Build the database first.")
        n_before = self.index.ntotal
        removed, omap = self.index.remove_ids(ids, return_map=True)       # (HipIVFFlatIndex raises before anything changes)
        if removed == 0:
            return 0
        keep = np.flatnonzero(omap.cpu().numpy() >= 0)
        assert len(keep) == n_before - removed == self.index.ntotal
        self.vector_paths = [self.vector_paths[i] for i in keep]
        self.vector_labels = [self.vector_labels[i] for i in keep]
        if isinstance(self.vector_metadata, dict):
            self.vector_metadata = {key: ([vals[i] for i in keep] if hasattr(vals, "__getitem__") and len(vals) == n_before else vals)
                                    for key, vals in self.vector_metadata.items()}
        # The device columns are dropped, not patched: row_tags_device() / labels_device() take an equal LENGTH as proof that their
        # cache is current, and a removal followed by an add of as many rows has that length with other rows behind it.  The host
        # tags are cut like the paths (or dropped when they were not current: row_tags_device() then takes them from the paths).
        # _tag_names (tag -> basename, the collision check) is LEFT as it is: a basename that is gone keeps its tag reserved, which
        # can only make the check stricter, and the same file added again finds its own entry.
        self._tags_host = [self._tags_host[i] for i in keep] if len(self._tags_host) == n_before else []
        self._tags_dev = self._labels_dev = None
        return removed

    def remove_files(self, paths) -> int:
        """Remove every stored row whose BASENAME equals that of one of `paths` (the match the exclusion makes, pipeline.py:495-502;
        two rows that share a basename both go).  -> rows removed."""
        if self.index is None:
            raise ValueError("Vector database is empty. Build the database first.")
        names = {os.path.basename(p_) for p_ in ([paths] if isinstance(paths, str) else paths)}
        base = getattr(self.index, "id_base", 0)
        ids = [base + i for i, p_ in enumerate(self.vector_paths) if os.path.basename(p_) in names]
        if not ids and not isinstance(self.index, HipFlatIndex):
            self.index.remove_ids(ids)           # an IVF store refuses whether or not a name matched
        return self.remove_vectors(ids) if ids else 0

    # vector_database.py:159-182
    def search_batch(self, query_vectors, k: int = None):
        """numpy in -> (float32 [B,k], int64 [B,k]) numpy out, as the reference; a CUDA tensor in -> CUDA tensors out."""
        if self.index is None:
            raise ValueError("Vector database is empty. Build the database first.")
        k = int(k if k is not None else getattr(self.config, "top_k", 5))
        is_dev = hasattr(query_vectors, "is_cuda") and query_vectors.is_cuda
        if not is_dev:
            query_vectors = np.asarray(query_vectors)
        if query_vectors.ndim == 1:
            query_vectors = query_vectors.reshape(1, -1)
        k = min(k, self.index.ntotal)
        if k <= 0:
            logging.warning("No vectors available for search")
            if is_dev:
                import torch
                return (torch.zeros((len(query_vectors), 0), dtype=torch.float32, device=query_vectors.device),
                        torch.zeros((len(query_vectors), 0), dtype=torch.int64, device=query_vectors.device))
            return np.zeros((len(query_vectors), 0), dtype=np.float32), np.zeros((len(query_vectors), 0), dtype=np.int64)
        try:     # IVF: tune nprobe (vector_database.py:174-179)
            if hasattr(self.index, "nprobe") and hasattr(self.config, "vector_db_nprobe"):
                self.index.nprobe = int(self.config.vector_db_nprobe)
        except Exception:
            pass
        if is_dev:
            return self.index.search_device(query_vectors, k)
        return self.index.search(query_vectors.astype(np.float32, copy=False), k)

    def range_search_batch(self, query_vectors, thresh: float, max_per_query: int = 128, return_counts: bool = False):
        """Every stored row within `thresh` of each query, exactly, in faiss's CSR form (HipFlatIndex.range_search): -> (lims int64
        [B + 1], D, I), with return_counts also the exact int32 counts.  Inputs as search_batch: numpy in -> numpy out, a CUDA tensor
        in -> CUDA tensors out, a 1-d query is one query; an empty store returns empty results.  Flat stores only."""
        query_vectors, empty = self._range_front("range_search_batch", query_vectors, return_counts)
        if empty is not None:
            return empty
        return self.index.range_search(query_vectors, thresh, max_per_query=max_per_query, return_counts=return_counts)

    def range_search_probed_batch(self, query_vectors, thresh: float, max_per_query: int = 128, return_counts: bool = False):
        """IVF stores: every row of the probed lists (config.vector_db_nprobe, vector_database.py:174-179) within `thresh` (squared L2,
        strictly) of each query, exactly, in the CSR form of range_search_batch (HipIVFFlatIndex.range_search_probed): the exact
        range search restricted to the probed lists.  max_per_query <= 128.  Inputs and the empty-store result as range_search_batch."""
        query_vectors, empty = self._range_front("range_search_probed_batch", query_vectors, return_counts, probed=True)
        if empty is not None:
            return empty
        if hasattr(self.config, "vector_db_nprobe"):        # vector_database.py:174-179
            self.index.nprobe = int(self.config.vector_db_nprobe)
        return self.index.range_search_probed(query_vectors, thresh, max_per_query=max_per_query, return_counts=return_counts)

    def _range_front(self, name: str, query_vectors, return_counts: bool, probed: bool = False, flat_name: str = "range_search_batch"):
        """the front of the range searches -> (query_vectors [B, d], None), or (query_vectors, the empty result of an empty store)"""
        if self.index is None:
            raise ValueError("Vector database is empty. Build the database first.")
        if probed:
            if not isinstance(self.index, HipIVFFlatIndex):
                raise ValueError(f"{name} is the IVF store's range search (vector_db_index_type 'IVF'); a flat store has {flat_name}")
        elif not isinstance(self.index, HipFlatIndex):
            raise ValueError(f"{name} is flat and single-handle only (vector_db_index_type 'L2' or 'IP'): an IVF search "
                             "sees the probed lists, not the store")
        is_dev = hasattr(query_vectors, "is_cuda") and query_vectors.is_cuda
        if not is_dev:
            query_vectors = np.asarray(query_vectors)
        if query_vectors.ndim == 1:
            query_vectors = query_vectors.reshape(1, -1)
        if self.index.ntotal <= 0:
            logging.warning("No vectors available for search")
            nq = len(query_vectors)
            if is_dev:
                import torch
                dev = query_vectors.device
                out = (torch.zeros((nq + 1,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                       torch.zeros((0,), dtype=torch.int64, device=dev))
                return query_vectors, out + ((torch.zeros((nq,), dtype=torch.int32, device=dev),) if return_counts else ())
            out = (np.zeros((nq + 1,), np.int64), np.zeros((0,), np.float32), np.zeros((0,), np.int64))
            return query_vectors, out + ((np.zeros((nq,), np.int32),) if return_counts else ())
        return query_vectors, None

    def range_search_excluding_batch(self, query_vectors, thresh: float, exclude_tags=None, max_per_query: int = 128,
                                     return_counts: bool = False, row_tags=None):
        """range_search_batch among the rows whose tag is not in `exclude_tags` -- ONE set for the batch
        (HipFlatIndex.range_search_excluding): the counts are the exact numbers of admissible rows within the radius, and an excluded
        row never takes one of the max_per_query slots.  exclude_tags: int64 tensor / sequence of tags, or None / empty.  row_tags:
        None = the basename tags (path_tag) kept per row, or an int64 [ntotal] column of the caller's own.  Flat stores only."""
        import torch
        query_vectors, empty = self._range_front("range_search_excluding_batch", query_vectors, return_counts)
        if empty is not None:
            return empty
        dev = torch.device("cuda", self.device_id)
        excl = None
        if exclude_tags is not None and len(exclude_tags) > 0:
            excl = torch.unique(torch.as_tensor(exclude_tags, dtype=torch.int64).to(dev).reshape(-1))       # sorted, as the kernel's search needs
        tags = None if excl is None else (self.row_tags_device() if row_tags is None else torch.as_tensor(row_tags, dtype=torch.int64).to(dev))
        return self.index.range_search_excluding(query_vectors, thresh, tags, excl, max_per_query=max_per_query, return_counts=return_counts)

    def range_search_excluding_per_query_batch(self, query_vectors, thresh: float, query_tags=None, query_tag_counts=None,
                                               max_per_query: int = 128, return_counts: bool = False, row_tags=None):
        """range_search_batch with one exclusion set PER QUERY (HipFlatIndex.range_search_excluding_per_query; leave-one-file-out,
        leave-one-speaker-out): query i excludes the rows whose tag is among the first query_tag_counts[i] entries of query_tags[i].
        query_tags: int64 tensor / nested sequence [B, m] (or [B]), m <= 64, None = nothing excluded; query_tag_counts: [B] or None.
        row_tags: None = the basename tags (path_tag) kept per row, or an int64 [ntotal] column of the caller's own.  Flat stores
        only."""
        import torch
        query_vectors, empty = self._range_front("range_search_excluding_per_query_batch", query_vectors, return_counts)
        if empty is not None:
            return empty
        dev = torch.device("cuda", self.device_id)
        if query_tags is not None:
            query_tags = torch.as_tensor(query_tags, dtype=torch.int64).to(dev)
        if query_tag_counts is not None:
            query_tag_counts = torch.as_tensor(query_tag_counts, dtype=torch.int32).to(dev)
        tags = None if query_tags is None else (self.row_tags_device() if row_tags is None else torch.as_tensor(row_tags, dtype=torch.int64).to(dev))
        return self.index.range_search_excluding_per_query(query_vectors, thresh, tags, query_tags, query_tag_counts,
                                                           max_per_query=max_per_query, return_counts=return_counts)

    def range_search_probed_excluding_batch(self, query_vectors, thresh: float, exclude_tags=None, max_per_query: int = 128,
                                            return_counts: bool = False):
        """IVF stores: range_search_probed_batch among the rows whose basename tag (path_tag) is not in `exclude_tags` -- ONE set for the
        batch (HipIVFFlatIndex.range_search_probed_excluding): the counts are the exact numbers of admissible members of the probed
        lists, and an excluded row never takes one of the max_per_query (<= 128) slots.  exclude_tags: int64 tensor / sequence of tags,
        or None / empty.  The IVF twin of range_search_excluding_batch; a flat store raises."""
        import torch
        query_vectors, empty = self._range_front("range_search_probed_excluding_batch", query_vectors, return_counts, probed=True,
                                                 flat_name="range_search_excluding_batch")
        if empty is not None:
            return empty
        dev = torch.device("cuda", self.device_id)
        excl = None
        if exclude_tags is not None and len(exclude_tags) > 0:
            excl = torch.unique(torch.as_tensor(exclude_tags, dtype=torch.int64).to(dev).reshape(-1))       # sorted, as the kernel's search needs
        tags = None if excl is None else self.row_tags_device()
        if hasattr(self.config, "vector_db_nprobe"):        # vector_database.py:174-179
            self.index.nprobe = int(self.config.vector_db_nprobe)
        return self.index.range_search_probed_excluding(query_vectors, thresh, tags, excl, max_per_query=max_per_query,
                                                        return_counts=return_counts)

    def range_search_probed_excluding_per_query_batch(self, query_vectors, thresh: float, query_tags=None, query_tag_counts=None,
                                                      max_per_query: int = 128, return_counts: bool = False, row_tags=None):
        """IVF stores: range_search_probed_batch with one exclusion set PER QUERY (HipIVFFlatIndex.range_search_probed_excluding_per_query;
        leave-one-file-out, leave-one-speaker-out): query i excludes the rows whose tag is among the first query_tag_counts[i] entries
        of query_tags[i].  query_tags: int64 tensor / nested sequence [B, m] (or [B]), m <= 64, None = nothing excluded;
        query_tag_counts: [B] or None.  row_tags: None = the basename tags (path_tag) kept per row, or an int64 [ntotal] column of the
        caller's own.  The IVF twin of range_search_excluding_per_query_batch; a flat store raises."""
        import torch
        query_vectors, empty = self._range_front("range_search_probed_excluding_per_query_batch", query_vectors, return_counts, probed=True,
                                                 flat_name="range_search_excluding_per_query_batch")
        if empty is not None:
            return empty
        dev = torch.device("cuda", self.device_id)
        if query_tags is not None:
            query_tags = torch.as_tensor(query_tags, dtype=torch.int64).to(dev)
        if query_tag_counts is not None:
            query_tag_counts = torch.as_tensor(query_tag_counts, dtype=torch.int32).to(dev)
        tags = None if query_tags is None else (self.row_tags_device() if row_tags is None else torch.as_tensor(row_tags, dtype=torch.int64).to(dev))
        if hasattr(self.config, "vector_db_nprobe"):        # vector_database.py:174-179
            self.index.nprobe = int(self.config.vector_db_nprobe)
        return self.index.range_search_probed_excluding_per_query(query_vectors, thresh, tags, query_tags, query_tag_counts,
                                                                  max_per_query=max_per_query, return_counts=return_counts)

    def _excluding_args(self, index_cls, wrong_index: str, query_vectors, k, exclude_tags, k_fetch=None):
        """the front of search_excluding / search_probed_excluding -> (query_vectors [B, d], k clamped to ntotal, k_fetch, row tags,
        exclusion set sorted and unique, as the kernels' binary search needs; both None when nothing is excluded); k == 0: nothing
        to search"""
        import torch
        if self.index is None:
            raise ValueError("Vector database is empty. Build the database first.")
        if not isinstance(self.index, index_cls):
            raise ValueError(wrong_index)
        _lib.require_cuda(query_vectors, "query_vectors")
        if query_vectors.dim() == 1:
            query_vectors = query_vectors.reshape(1, -1)
        k = int(k if k is not None else getattr(self.config, "top_k", 5))
        k_fetch = k + 10 if k_fetch is None else int(k_fetch)
        if k_fetch < k:
            raise ValueError(f"k_fetch={k_fetch} must be at least k={k}")
        k = min(k, self.index.ntotal)
        if k <= 0:
            logging.warning("No vectors available for search")
            return query_vectors, 0, k_fetch, None, None
        if exclude_tags is None or len(exclude_tags) == 0:
            return query_vectors, k, k_fetch, None, None
        excl = torch.unique(torch.as_tensor(exclude_tags, dtype=torch.int64).to(query_vectors.device).reshape(-1))
        return query_vectors, k, k_fetch, self.row_tags_device(), excl

    @staticmethod
    def _no_hits(query_vectors):
        import torch
        return (torch.zeros((len(query_vectors), 0), dtype=torch.float32, device=query_vectors.device),
                torch.zeros((len(query_vectors), 0), dtype=torch.int64, device=query_vectors.device))

    def search_excluding(self, query_vectors, k: int = None, exclude_tags=None, k_fetch=None):
        """The k nearest rows whose basename tag (path_tag) is not in `exclude_tags`, exactly, however many excluded rows precede them
        (HipFlatIndex.search_excluding; the reference's K + 10 over-fetch, pipeline.py:478,491-515, pads instead).  query_vectors: CUDA
        tensor [B, d]; exclude_tags: int64 tensor / sequence of tags, or None / empty -> (D f32 [B,k], I i64 [B,k]) on the device, -1 / NaN
        where fewer than k admissible rows exist.  k is clamped to ntotal as in search_batch.  Flat stores only."""
        q, k, k_fetch, tags, excl = self._excluding_args(
            HipFlatIndex, "exclusion-aware search is flat and single-handle only (vector_db_index_type 'L2' or 'IP')",
            query_vectors, k, exclude_tags, k_fetch)
        if k <= 0:
            return self._no_hits(q)
        return self.index.search_excluding(q, k, tags, excl, k_fetch=min(k_fetch, _lib.KNN_MAX_K))

    def search_excluding_in_scan(self, query_vectors, k: int = None, exclude_tags=None):
        """search_excluding's result with the admission test inside the certified tile scan (HipFlatIndex.search_excluding_in_scan): no
        k_fetch, and a cost that does not depend on how much of the store is excluded -- the call when `exclude_tags` covers most of
        it (training_file_ids, pipeline.py:500-502).  Arguments and outputs as search_excluding.  Flat stores only: an IVF store has
        search_probed_excluding, a row-sharded one merges its shards' results."""
        q, k, _, tags, excl = self._excluding_args(
            HipFlatIndex, "search_excluding_in_scan is flat and single-handle only (vector_db_index_type 'L2' or 'IP'); an IVF store has "
            "search_probed_excluding", query_vectors, k, exclude_tags)
        if k <= 0:
            return self._no_hits(q)
        return self.index.search_excluding_in_scan(q, k, tags, excl)

    def search_excluding_per_query(self, query_vectors, k: int = None, query_tags=None, query_tag_counts=None, k_fetch=None):
        """search_excluding with one exclusion set PER QUERY (HipFlatIndex.search_excluding_per_query; leave-one-out): query i excludes
        the rows whose basename tag (path_tag) is among the first query_tag_counts[i] entries of query_tags[i] and nothing else, so its
        result does not depend on the rest of the batch.  query_vectors: CUDA tensor [B, d]; query_tags: int64 tensor / nested sequence
        [B, m] (or [B]: one tag per query), m <= 64, None = nothing excluded; query_tag_counts: [B] or None = m for every query
        -> (D f32 [B,k], I i64 [B,k]) on the device, -1 / NaN where fewer than k admissible rows exist.  Flat stores only; a
        batch-wide set cannot be combined with it in one call."""
        import torch
        q, k, k_fetch, _, _ = self._excluding_args(
            HipFlatIndex, "search_excluding_per_query is flat and single-handle only (vector_db_index_type 'L2' or 'IP'); an IVF store has "
            "search_probed_excluding_per_query", query_vectors, k, None, k_fetch)
        if k <= 0:
            return self._no_hits(q)
        if query_tags is not None:
            query_tags = torch.as_tensor(query_tags, dtype=torch.int64).to(q.device)
        if query_tag_counts is not None:
            query_tag_counts = torch.as_tensor(query_tag_counts, dtype=torch.int32).to(q.device)
        return self.index.search_excluding_per_query(q, k, self.row_tags_device(), query_tags, query_tag_counts,
                                                     k_fetch=min(k_fetch, _lib.KNN_MAX_K))

    def search_excluding_per_query_in_scan(self, query_vectors, k: int = None, query_tags=None, query_tag_counts=None):
        """search_excluding_per_query's result on the certified tile scan (HipFlatIndex.search_excluding_per_query_in_scan): no k_fetch
        -- the call when one basename tag is carried by hundreds or thousands of rows (a query excluding its own speaker's files).
        Arguments and outputs as search_excluding_per_query.  Flat stores only: an IVF store has search_probed_excluding_per_query, a
        row-sharded one merges its shards' results."""
        import torch
        q, k, _, _, _ = self._excluding_args(
            HipFlatIndex, "search_excluding_per_query_in_scan is flat and single-handle only (vector_db_index_type 'L2' or 'IP'); an IVF "
            "store has search_probed_excluding_per_query", query_vectors, k, None)
        if k <= 0:
            return self._no_hits(q)
        if query_tags is not None:
            query_tags = torch.as_tensor(query_tags, dtype=torch.int64).to(q.device)
        if query_tag_counts is not None:
            query_tag_counts = torch.as_tensor(query_tag_counts, dtype=torch.int32).to(q.device)
        return self.index.search_excluding_per_query_in_scan(q, k, self.row_tags_device(), query_tags, query_tag_counts)

    def search_probed_excluding(self, query_vectors, k: int = None, exclude_tags=None):
        """IVF stores: the k nearest rows of the probed lists (config.vector_db_nprobe, vector_database.py:174-179) whose basename tag
        (path_tag) is not in `exclude_tags`, exactly, however many excluded rows precede them
        (HipIVFFlatIndex.search_probed_excluding; the reference's K + 10 over-fetch, pipeline.py:478,491-515, pads instead).
        query_vectors: CUDA tensor [B, d]; exclude_tags: int64 tensor / sequence of tags, or None / empty -> (D f32 [B,k], I i64 [B,k])
        on the device, -1 / NaN where the probed lists hold fewer than k admissible rows.  k is clamped to ntotal as in search_batch."""
        q, k, _, tags, excl = self._excluding_args(
            HipIVFFlatIndex, "search_probed_excluding is the IVF store's exclusion-aware search (vector_db_index_type 'IVF'); "
            "a flat store has search_excluding", query_vectors, k, exclude_tags)
        if k <= 0:
            return self._no_hits(q)
        if hasattr(self.config, "vector_db_nprobe"):        # vector_database.py:174-179
            self.index.nprobe = int(self.config.vector_db_nprobe)
        return self.index.search_probed_excluding(q, k, tags, excl)

    def search_probed_excluding_per_query(self, query_vectors, k: int = None, query_tags=None, query_tag_counts=None):
        """IVF stores: search_probed_excluding with one exclusion set PER QUERY (HipIVFFlatIndex.search_probed_excluding_per_query;
        leave-one-out): query i excludes the rows whose basename tag (path_tag) is among the first query_tag_counts[i] entries of
        query_tags[i] and nothing else, so its result does not depend on the rest of the batch.  Arguments and result as
        search_excluding_per_query, among the rows of the probed lists (config.vector_db_nprobe)."""
        import torch
        q, k, _, _, _ = self._excluding_args(
            HipIVFFlatIndex, "search_probed_excluding_per_query is the IVF store's per-query exclusion-aware search (vector_db_index_type "
            "'IVF'); a flat store has search_excluding_per_query", query_vectors, k, None)
        if k <= 0:
            return self._no_hits(q)
        if query_tags is not None:
            query_tags = torch.as_tensor(query_tags, dtype=torch.int64).to(q.device)
        if query_tag_counts is not None:
            query_tag_counts = torch.as_tensor(query_tag_counts, dtype=torch.int32).to(q.device)
        if hasattr(self.config, "vector_db_nprobe"):        # vector_database.py:174-179
            self.index.nprobe = int(self.config.vector_db_nprobe)
        return self.index.search_probed_excluding_per_query(q, k, self.row_tags_device(), query_tags, query_tag_counts)

    # ---- device-side columns for retrieve_similar_vectors ------------------------------------------------------
    def row_tags_device(self):
        """int64 [ntotal] CUDA tensor: path_tag(vector_paths[i]).  (The cache is trusted by its length: whatever changes rows without
        changing their number -- remove_vectors followed by an add -- resets it.)"""
        import torch
        if self._tags_dev is None or self._tags_dev.numel() != len(self.vector_paths):
            if len(self._tags_host) != len(self.vector_paths):          # e.g. after load()
                self._tags_host, self._tag_names = [], {}
                for p_ in self.vector_paths:
                    t_, b_ = path_tag(p_), os.path.basename(p_)
                    if self._tag_names.setdefault(t_, b_) != b_:
                        raise RuntimeError(f"path_tag collision between {self._tag_names[t_]!r} and {b_!r}")
                    self._tags_host.append(t_)
            self._tags_dev = torch.tensor(self._tags_host, dtype=torch.int64, device=torch.device("cuda", self.device_id))
        return self._tags_dev

    def labels_device(self):
        """float32 [ntotal] CUDA tensor of vector_labels (the reference stacks them as float32, pipeline.py:523)"""
        import torch
        if self._labels_dev is None or self._labels_dev.numel() != len(self.vector_labels):
            self._labels_dev = torch.tensor([float(l) for l in self.vector_labels], dtype=torch.float32,
                                            device=torch.device("cuda", self.device_id))
        return self._labels_dev

    def filter_hits(self, dists, idxs, k_keep: int, exclude_tags=None):
        """first k_keep hits per row whose tag is not excluded; (-1, NaN) padded.  All on the device."""
        import torch
        lib = _lib.load()
        B, k_in = idxs.shape
        out_d = torch.empty((B, k_keep), device=idxs.device, dtype=torch.float32)
        out_i = torch.empty((B, k_keep), device=idxs.device, dtype=torch.int64)
        n_excl = 0 if exclude_tags is None else int(exclude_tags.numel())
        tags = self.row_tags_device() if n_excl else None
        d, i = dists.contiguous().float(), idxs.contiguous()
        with torch.cuda.device(idxs.device):
            _lib.check(lib.radad_filter_topk(d.data_ptr(), i.data_ptr(), B, k_in, k_keep, tags.data_ptr() if n_excl else None,
                                             self.index.ntotal, self.index.id_base, exclude_tags.data_ptr() if n_excl else None,
                                             n_excl, out_d.data_ptr(), out_i.data_ptr(), idxs.device.index,
                                             _lib.stream_ptr(idxs.device)), "radad_filter_topk")
        return out_d, out_i

    # vector_database.py:185-188
    def search(self, query_vector, k: int = None):
        distances, indices = self.search_batch(query_vector.reshape(1, -1), k)
        return (distances[0] if len(distances) > 0 else np.array([]), indices[0] if len(indices) > 0 else np.array([]))

    # vector_database.py:190-216 (own snapshot format instead of faiss.write_index; same metadata keys)
    def save(self):
        try:
            if self.index is None:
                logging.warning("No index to save.")
                return
            # IVF: rows in insertion order as a NATIVE flat snapshot (streamed from HBM by radad_knn_save, no host copy of the
            # store), centroids in a small sidecar; assignments are recomputed on load (deterministic: nearest centroid)
            self.index.save(self.db_path)
            if not isinstance(self.index, HipIVFFlatIndex) and os.path.exists(self.db_path + ".ivf.npz"):
                os.remove(self.db_path + ".ivf.npz")      # centroids of an IVF store saved here earlier: not this store's
            meta = {"paths": self.vector_paths, "labels": self.vector_labels, "metadata": self.vector_metadata,
                    "index_type": self.config.vector_db_index_type, "dimension": self.index.d}
            with open(self.metadata_path, "wb") as f:
                pickle.dump(meta, f)
            logging.info(f"Saved index to {self.db_path} with {self.index.ntotal} vectors")
        except Exception as e:
            logging.error(f"Error saving vector database: {e}")

    # vector_database.py:218-242
    def load(self, shard=None):
        """shard=(rank, world_size): keep only this rank's row shard of the saved store (native snapshots only) -- the index
        reads just its byte range of the file and reports global ids; paths / labels / metadata are cut to the same rows."""
        try:
            if not (os.path.exists(self.db_path) and os.path.exists(self.metadata_path)):
                logging.warning("No saved vector database found")
                return
            with open(self.metadata_path, "rb") as f:
                meta = pickle.load(f)
            self.vector_paths, self.vector_labels, self.vector_metadata = meta["paths"], meta["labels"], meta["metadata"]
            self._tags_host, self._tags_dev, self._labels_dev = [], None, None      # device columns follow the new rows
            with open(self.db_path, "rb") as f:
                magic = f.read(8)
            if shard is not None and magic != b"RADADKNN":
                raise ValueError("sharded load is only available for native flat snapshots")
            # which kind of store the snapshot holds is what save() recorded (meta["index_type"]), not whether a centroid sidecar
            # happens to lie beside it (files written before the key existed: the sidecar decides, as it used to)
            saved_type = str(meta.get("index_type", "IVF" if os.path.exists(self.db_path + ".ivf.npz") else "")).upper()
            if magic == b"RADADKNN" and saved_type == "IVF":      # an IVF store written by save() above
                if shard is not None:
                    raise ValueError("sharded load is only available for flat stores")
                self.create_index(int(meta["dimension"]))
                if not isinstance(self.index, HipIVFFlatIndex):
                    raise ValueError("saved IVF store does not match config (index type)")
                self.index.load(self.db_path)
            elif magic[:2] == b"PK":                    # numpy .npz: an IVF store written by an earlier version of save()
                z = np.load(self.db_path)
                centroids, rows = z["centroids"], z["rows"]        # NpzFile re-reads an array on every access: read once
                self.create_index(int(centroids.shape[1]))
                if not isinstance(self.index, HipIVFFlatIndex) or self.index.nlist != centroids.shape[0]:
                    raise ValueError("saved IVF store does not match config (index type / ivf_nlist)")
                self.index.set_centroids(centroids)
                for s0 in range(0, len(rows), 1 << 18):
                    self.index.add(rows[s0:s0 + (1 << 18)])
            elif magic[:4] in (b"IxF2", b"IxFI"):
                # a store written by the reference itself (faiss.write_index).  For cosine the reference had normalised
                # the rows before adding them (vector_database.py:118); adding them again re-normalises unit rows, which
                # changes them by at most one ulp.
                file_metric, d, rows = read_faiss_flat(self.db_path)
                want = self.config.vector_db_index_type.upper()
                if want in ("L2", "IP") and want != file_metric:     # faiss.read_index keeps the file's metric; so do we
                    raise ValueError(f"{self.db_path} holds a faiss Index{file_metric} store but config asks for {want}")
                self.create_index(d)
                for s0 in range(0, len(rows), 1 << 18):
                    self.index.add(rows[s0:s0 + (1 << 18)])
            elif shard is not None:
                from .sharded import shard_bounds
                rank, world = int(shard[0]), int(shard[1])
                self.create_index(int(meta["dimension"]))
                if not isinstance(self.index, HipFlatIndex):
                    raise ValueError("sharded load needs a flat store")
                lo, hi = shard_bounds(HipFlatIndex.snapshot_info(self.db_path)["ntotal"], world, rank)
                self.index = HipFlatIndex(self.index.d, self.index.metric, device=self.device_id, id_base=lo,
                                          store_f16=self.index.store_f16, **{k: v for k, v in getattr(self.index, "options", {}).items() if v is not None})
                self.index.load(self.db_path, lo, hi - lo)
                self.vector_paths, self.vector_labels = self.vector_paths[lo:hi], self.vector_labels[lo:hi]
                if isinstance(self.vector_metadata, dict):
                    self.vector_metadata = {key: vals[lo:hi] for key, vals in self.vector_metadata.items()}
            else:
                self.create_index(int(meta["dimension"]))
                self.index.load(self.db_path)
            logging.info(f"Loaded index; ntotal={self.index.ntotal}")
        except Exception as e:
            logging.error(f"Error loading vector database: {e}")

    # vector_database.py:245-256
    def get_gpu_memory_usage(self):
        try:
            import torch
            if torch.cuda.is_available():
                free, total = torch.cuda.mem_get_info(self.device_id)
                used = total - free
                return {"used": int(used), "total": int(total), "utilization": float(used / total)}
        except Exception:
            pass
        return None
