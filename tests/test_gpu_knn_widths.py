"""Flat searches at row widths 4 .. 16380 against the float64 C oracle, on the designed stores of tests/knn_width_ref.py.

Which scan answers is decided by the residues of the width (csrc/knn_plan.h), and a scan that mishandles the last partial K step of
a width is repaired by the re-rank or the exact kernel on random rows.  On a tail_store the designated column group decides the
answer and a correct scan has nothing to reject (tests/test_knn_width_cases.py shows both on the CPU), so every search here checks
the route (radad_knn_last_launch), ids, distances, float64 keys AND that the certificate rejected no query.

Isolation: the oracle runs on what the store holds (reconstruct_batch) and, under cosine, on the device's radad_rownorm of the
queries; ingest is held to a host model at these widths by tests/test_gpu_store_contents.py.  The queries are handed over as the first
nq rows of a tensor whose remaining rows are NaN: a kernel that reads a neighbouring query row into a live lane poisons its result.
Query j of a batch is centre j % P of the store, so the reference is computed once per centre and compared with every query.

Key bounds (derived, not measured): the device and the oracle both sum `dim` float64 terms, in different orders.  L2: the terms are
non-negative, each sum is within (dim + 2) 2^-53 of the exact value relatively -- tests/test_gpu_store_contents.py::_key_rtol(dim),
relative to the key.  IP / cosine: the same factor times sum |q_i y_i|.  D is float32(K64), bit for bit."""
import time

import numpy as np
import pytest

import knn_width_ref as W
from conftest import c_knn
from test_gpu_store_contents import _key_rtol

pytestmark = pytest.mark.gpu

WORST = {}          # class -> worst |K64 - oracle| / bound seen by the tail-store tests (printed per store)


def _lib():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib as L
    return L


def _mk(gpu, metric, dim, f16=False):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    L = _lib()
    return HipFlatIndex(dim, {"L2": L.METRIC_L2, "IP": L.METRIC_IP, "COSINE": L.METRIC_COSINE}[metric], gpu.index or 0, 0, store_f16=f16)


def _held(idx, n, gpu):
    import torch
    out = [idx.reconstruct_batch(torch.arange(r0, min(n, r0 + 4096), device=gpu)).cpu().numpy() for r0 in range(0, n, 4096)]
    return np.concatenate(out)


def _rownorm(gpu, x):
    import torch
    L = _lib()
    out = torch.empty_like(x)
    L.check(L.load().radad_rownorm(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], gpu.index or 0, L.stream_ptr(gpu)))
    return out


def _padded(gpu, q, pad=3):
    """the queries as the first rows of a tensor whose other rows are NaN -> (the view of the first nq rows, the whole tensor)"""
    import torch
    buf = torch.full((len(q) + pad, q.shape[1]), float("nan"), device=gpu, dtype=torch.float32)
    buf[:len(q)] = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(gpu)
    return buf[:len(q)], buf


class Store:
    """a designed store on the device and the float64 oracle over what it holds, for the store's distinct queries (the centres)"""

    def __init__(self, gpu, lib, rows, centres, metric, f16, k_ref):
        import torch
        self.gpu, self.metric, self.dim, self.n = gpu, metric, rows.shape[1], len(rows)
        self.idx = _mk(gpu, metric, self.dim, f16)
        self.idx.add(rows)
        self.stored = _held(self.idx, self.n, gpu)
        ct = torch.from_numpy(np.ascontiguousarray(centres, np.float32)).to(gpu)
        self.qq = _rownorm(gpu, ct).cpu().numpy() if metric == "COSINE" else np.ascontiguousarray(centres, np.float32)
        self.k_ref = min(k_ref, self.n)
        self.od, self.oi = c_knn(lib, self.stored, self.qq, self.k_ref, "L2" if metric == "L2" else "IP")
        hit = self.stored[self.oi].astype(np.float64)                                  # [P, k_ref, dim]
        mass = np.abs(self.od) if metric == "L2" else (np.abs(hit) * np.abs(self.qq.astype(np.float64))[:, None, :]).sum(-1)
        self.bound = _key_rtol(self.dim) * mass
        gaps = np.abs(np.diff(self.od, axis=1))
        self.decidable = gaps > 4 * self.bound[:, 1:]                                  # rank r and r + 1 are told apart by the keys

    def check(self, D, I, K, centre_of, k, what):
        """ids, float64 keys within the bound, D == float32(K64) in bits; -> worst key error / bound"""
        import torch
        assert torch.equal(D, K.float()), f"{what}: D is not float32(K64)"
        I, K = I.cpu().numpy(), K.cpu().numpy()
        oi, od, bound = self.oi[centre_of, :k], self.od[centre_of, :k], self.bound[centre_of, :k]
        bad = I != oi
        assert not bad.any(), (f"{what}: {int(bad.any(1).sum())} of {len(I)} queries differ from the oracle, first query "
                               f"{int(np.flatnonzero(bad.any(1))[0])}: got {I[bad.any(1)][0][:12]} want {oi[bad.any(1)][0][:12]}")
        err = np.abs(K - od)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        r = float(ratio.max())
        assert r <= 1.0, f"{what}: worst |K64 - oracle| / bound = {r:.3f}"
        return r


def _assert_route_and_certificate(idx, case, nq, what, rejected=0):
    info = idx.last_launch()
    assert info["scan_kind"] == W.expected_kind(case), f"{what}: scan {info['scan_kind']}, planned {W.expected_kind(case)}"
    cert = info["certificate"]
    assert cert["queries"] == nq, f"{what}: {info}"
    if rejected == 0:
        assert cert["rejected"] == 0, f"{what}: the certificate rejected queries of a store with nothing to reject: {cert}"
    return info


@pytest.mark.parametrize("width,n,f16,metric,rot", W.store_params(), ids=lambda v: str(v))
def test_tail_store_searches(gpu, knn_oracle_lib, width, n, f16, metric, rot):
    """every (nq, k) of W.SEARCHES on one designed store: the planned route, the oracle's ids (ties to the lower id), float64 keys
    within the summation bound, D == float32(K64), NaN rows behind the queries, and NO rejected query at any k <= k_max"""
    t0 = time.time()
    rows, _, info = W.tail_store(width, n, 1, W.K_MAX, W.STORE_SEED, rot)
    C, P = info["centre_rows"], info["centres"]
    st = Store(gpu, knn_oracle_lib, rows, C, metric, f16, W.K_MAX + 8)
    # the store is what the CPU test vouched for: the oracle's top k_max + 8 over the STORED rows are the centre's neighbours
    for a in range(P):
        assert set(st.oi[a]) == set(info["neighbours"][a]), (width, n, f16, metric, a)
    assert st.decidable[:, :W.K_MAX].all(), "the keys of adjacent ranks must be further apart than their error bounds"
    worst = 0.0
    for nq, k in W.SEARCHES:
        case = (width, n, f16, metric, nq, k)
        what = f"width {width} n {n} {'fp16' if f16 else 'fp32'} {metric} groups {info['groups']} nq {nq} k {k}"
        centre_of = np.arange(nq) % P
        qv, buf = _padded(gpu, C[centre_of])
        D, I, K = st.idx.search_device(qv, k, return_f64=True)
        _assert_route_and_certificate(st.idx, case, nq, what)
        worst = max(worst, st.check(D, I, K, centre_of, k, what))
    cls = W.CLASS_OF[width]
    WORST[cls] = max(WORST.get(cls, 0.0), worst)
    print(f"width {width} (class {cls}) n {n} {'fp16' if f16 else 'fp32'} {metric} groups {info['groups']}: worst |K64 - oracle| / bound = "
          f"{worst:.3f} (class so far {WORST[cls]:.3f}), {time.time() - t0:.2f} s")


DUP_STORES = [(w, n, f16, m) for (w, n, f16) in ((12, 1500, False), (12, 1500, True), (16, 1500, False), (48, 1500, False), (48, 1500, True),
                                                 (68, 1500, True), (32, 20000, False), (36, 20000, False), (64, 1500, True),
                                                 (64, 20000, False), (1024, 20000, False), (1040, 1500, False), (16380, 1500, False))
              for m in ("L2", "COSINE")]
DUP_SEARCHES = ((1, 10), (16, 10), (17, 10), (300, 10), (17, 26), (300, 150))


@pytest.mark.parametrize("width,n,f16,metric", DUP_STORES, ids=lambda v: str(v))
def test_dup_store_searches(gpu, knn_oracle_lib, width, n, f16, metric):
    """100 exact copies of one neighbour per centre, adjacent in the store, at ranks 4 .. 103: the ids are the oracle's, the copies in
    ascending id order, whichever kernel answers.  Whether the route certifies the query or hands it to the exact kernel, as observed
    on an MI355X and as the candidate capacities say:
      f32_dense                      rejects at k = 10 and 26 (k + 32 candidates, 100 rows tie with the k-th), certifies k = 150
      f32_tile, f16_tile, f32_smallq, hi_smallq
                                     reject at k = 10 and 26 (lists of k + 6 <= 32 per chunk, all 100 copies in one or two chunks),
                                     certify k = 150 (a list of 156 holds them)
      hi_tile                        certifies every k (the emit buffer lists all copies, the re-rank orders the ties by id)
    Only the first two lines are asserted: the rejection is the exact kernel at this width (nv = dim / 4 lanes live in
    k_exact_scan_any, a group of up to 8 queries per workgroup)."""
    rows, _, info = W.dup_store(width, n, 1, W.K_MAX, W.STORE_SEED)
    C, P = info["centre_rows"], info["centres"]
    st = Store(gpu, knn_oracle_lib, rows, C, metric, f16, W.K_MAX + 108)
    for a in range(P):
        assert list(st.oi[a, 3:103]) == list(info["copies"][a]), "the oracle itself must list the copies in id order"
    seen = {}
    for nq, k in DUP_SEARCHES:
        case = (width, n, f16, metric, nq, k)
        what = f"dup store width {width} n {n} {'fp16' if f16 else 'fp32'} {metric} nq {nq} k {k}"
        centre_of = np.arange(nq) % P
        qv, buf = _padded(gpu, C[centre_of])
        D, I, K = st.idx.search_device(qv, k, return_f64=True)
        launch = _assert_route_and_certificate(st.idx, case, nq, what, rejected=None)
        st.check(D, I, K, centre_of, k, what)
        rej = launch["certificate"]["rejected"]
        seen.setdefault((launch["scan_kind"], k), []).append((nq, rej))
        if launch["scan_kind"] != "hi_tile" and k + 6 <= 32:
            assert rej == nq, f"{what}: every query has 100 rows tied with its k-th, {rej} of {nq} took the exact kernel: {launch}"
    print(f"dup store width {width} n {n} {'fp16' if f16 else 'fp32'} {metric}: (kind, k) -> (nq, rejected): {seen}")


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("width,f16", [(12, True), (20, False), (48, False), (68, True)])
def test_k_beyond_ntotal_at_tail_widths(gpu, knn_oracle_lib, width, f16, metric):
    """k = 150 over the 40 rows nearest the stores' planted ones: all 40 in the oracle's order, then id -1 with +inf (L2) / -inf"""
    rows, _, info = W.dup_store(width, W.N_SMALL, 1, W.K_MAX, W.STORE_SEED)
    keep = np.sort(np.concatenate([info["neighbours"][0][:25], info["copies"][0][:15]]))
    C = info["centre_rows"][:1]
    st = Store(gpu, knn_oracle_lib, rows[keep], C, metric, f16, 40)
    for nq in W.NQ_LIST:
        qv, buf = _padded(gpu, np.repeat(C, nq, axis=0))
        D, I, K = st.idx.search_device(qv, 150, return_f64=True)
        what = f"width {width} {'fp16' if f16 else 'fp32'} {metric} nq {nq}: 40 rows, k 150"
        st.check(D[:, :40].contiguous(), I[:, :40], K[:, :40].contiguous(), np.zeros(nq, np.int64), 40, what)
        tail = np.inf if metric == "L2" else -np.inf
        assert bool((I[:, 40:] == -1).all()) and np.all(D[:, 40:].cpu().numpy() == tail) and np.all(K[:, 40:].cpu().numpy() == tail), what


# ---- the exclusion family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("width,f16", [(12, True), (48, False), (68, True), (16380, False)])
def test_exclusion_family_at_tail_widths(gpu, width, f16, metric):
    """search_excluding and search_excluding_per_query with k_fetch = k on a tail_store whose decoys -- and the centre's three best
    neighbours -- carry the excluded tag: fewer than k of the k_fetch hits are admissible, so the row-filtered exact passes
    (k_exact_scan_excl, k_exact_scan_excl_pq) answer, at a width whose last K step is partial.  Reference: the float64 brute force
    over the admissible rows (tests/exclusion_ref.py, tests/excl_per_query_ref.py)."""
    import torch
    from exclusion_ref import expected_excluding
    from excl_per_query_ref import expected_pq
    rot = len(W.column_groups(width)) - 2 if width > 12 else 1          # a centre in the last partial step (12: the last group)
    rows, _, info = W.tail_store(width, W.N_SMALL, 1, W.K_MAX, W.STORE_SEED, rot)
    n, C = len(rows), info["centre_rows"]
    idx = _mk(gpu, metric, width, f16)
    idx.add(rows)
    stored = _held(idx, n, gpu)
    # (cosine: the inner product of the stored rows with the device's own normalisation of the query, as in every test here)
    qq = _rownorm(gpu, torch.from_numpy(C).to(gpu)).cpu().numpy() if metric == "COSINE" else C
    om = "L2" if metric == "L2" else "IP"
    tags = 1000 + np.arange(n, dtype=np.int64)
    tags[info["decoys"][0]] = 7
    s, _ = W.scores64(stored, qq, om)
    best = W.topk64(s, 3)[0]
    tags[best] = 7
    tags_t = torch.from_numpy(tags).to(gpu)
    nq = 17
    qv, buf = _padded(gpu, np.repeat(C, nq, axis=0))
    for k in (10, 150):
        what = f"width {width} {'fp16' if f16 else 'fp32'} {metric} k {k}"
        od, oi = expected_excluding(stored, tags, [7], qq, k, om)
        D, I, K = idx.search_excluding(qv, k, tags_t, torch.tensor([7], device=gpu), k_fetch=k, return_f64=True)
        assert idx.last_excl() == {"queries": nq, "exact": nq}, f"{what}: {idx.last_excl()}"
        np.testing.assert_array_equal(I.cpu().numpy(), np.repeat(oi, nq, axis=0), err_msg=f"{what}: search_excluding")
        np.testing.assert_allclose(K.cpu().numpy(), np.repeat(od, nq, axis=0), rtol=1e-11, atol=1e-11, err_msg=what)
        assert torch.equal(D, K.float())
        # per query: even queries exclude tag 7 and the 4th best row, odd queries nothing (count 0): the plain search
        t4 = int(tags[W.topk64(s, 4)[0, 3]])
        qt = np.tile(np.array([[7, t4]], np.int64), (nq, 1))
        cnt = np.where(np.arange(nq) % 2 == 0, 2, 0).astype(np.int32)
        od2, oi2 = expected_pq(stored, tags, qt[:2], cnt[:2], np.repeat(qq, 2, axis=0), k, om)
        D, I, K = idx.search_excluding_per_query(qv, k, tags_t, torch.from_numpy(qt).to(gpu), torch.from_numpy(cnt).to(gpu), k_fetch=k,
                                                 return_f64=True)
        assert idx.last_excl() == {"queries": nq, "exact": (nq + 1) // 2}, f"{what}: {idx.last_excl()}"
        np.testing.assert_array_equal(I.cpu().numpy(), oi2[np.arange(nq) % 2], err_msg=f"{what}: search_excluding_per_query")
        np.testing.assert_allclose(K.cpu().numpy(), od2[np.arange(nq) % 2], rtol=1e-11, atol=1e-11, err_msg=what)
        assert torch.equal(D, K.float())


# ---- bf16 queries on an fp16 store -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("width", [12, 48, 68])
def test_bf16_queries_on_fp16_store_at_tail_widths(gpu, width, metric):
    """bf16 queries are decoded exactly: ids, distances and float64 keys of the same values handed over as fp32 (the generic kernel's
    fp16 branch at a width with a partial K step, every batch size of the query preparation)"""
    import torch
    rows, _, info = W.tail_store(width, W.N_SMALL, 1, W.K_MAX, W.STORE_SEED, 1)
    idx = _mk(gpu, metric, width, True)
    idx.add(rows)
    for nq in W.NQ_LIST:
        q = torch.from_numpy(np.repeat(info["centre_rows"], nq, axis=0)).to(gpu)
        q = (q * torch.linspace(0.5, 1.5, nq, device=gpu)[:, None]).to(torch.bfloat16)
        for k in (10, 150):
            a = idx.search_device(q, k, return_f64=True)
            b = idx.search_device(q.float(), k, return_f64=True)
            for x, y, name in zip(a, b, ("D", "I", "K64")):
                assert torch.equal(x, y), f"width {width} {metric} nq {nq} k {k}, bf16 vs the same queries as fp32: {name} differs"
            assert int(a[1].min()) >= 0


# ---- the width x k limit (include/radad_hip.h, radad_knn_create) ---------------------------------------------------------------------------
def _ladder_store(width, n, seed):
    """n rows at strictly growing distance from one query (W's neighbour ladder over the whole store), then 100 exact copies of the
    row of rank 990 stored at the ranks 990 .. 1089: 65 rows tie with the 1024-th beyond it, more than the k + 32 candidates the
    re-rank takes at k = 1024 -- the query cannot be certified"""
    rng = np.random.default_rng([seed, width])
    C = W._centres(width, [width // 8], rng)
    y = W._neighbours(width, C, 0, width // 8, n, rng).astype(np.float32)
    y[990:1090] = y[990]
    perm = rng.permutation(n)
    rows = np.empty_like(y)
    rows[perm] = y
    return rows, C.astype(np.float32)


def _raw_search(idx, q, k, D, I, K, excl=None):
    """the C entry points on caller-owned output tensors -> status code"""
    L = _lib()
    lib = L.load()
    if excl is None:
        return lib.radad_knn_search_ex(idx._h, q.data_ptr(), L.Q_F32, q.shape[0], k, D.data_ptr(), I.data_ptr(), K.data_ptr(), L.stream_ptr(q.device))
    tags, ex = excl
    return lib.radad_knn_search_excl(idx._h, q.data_ptr(), L.Q_F32, q.shape[0], k, k, tags.data_ptr(), ex.data_ptr(), ex.numel(), D.data_ptr(),
                                     I.data_ptr(), K.data_ptr(), L.stream_ptr(q.device))


@pytest.mark.parametrize("excluding", [False, True], ids=["search", "search_excluding"])
def test_widest_rows_at_k_1024_and_the_refusal_beyond(gpu, knn_oracle_lib, excluding):
    """dim * 4 + 96 k + 16 <= 163840.  At 16380 x 1024 (exactly 160 KB, one query per workgroup of the exact kernel) the ids are the
    oracle's and the exact kernel answered (until this test the launch asked for the formula's 16 spare bytes as dynamic LDS beside
    the kernel's static flag and was refused by the runtime: RADAD_EHIP after the scan, and HIP's last error left for the next call).  At 16384 x 1024 the search is refused with ValueError BEFORE anything is enqueued: NaN
    prefilled outputs are untouched, and the next search at k = 10 on the same handle is the oracle's."""
    import torch
    L = _lib()
    n, nq = 1500, 3
    for width, fits in ((16380, True), (16384, False)):
        rows, C = _ladder_store(width, n, 4300)
        idx = _mk(gpu, "L2", width)
        idx.add(rows)
        stored = _held(idx, n, gpu)
        q = torch.from_numpy(np.repeat(C, nq, axis=0)).to(gpu)
        tags = torch.arange(n, device=gpu, dtype=torch.int64) + 50
        od_all, oi_all = c_knn(knn_oracle_lib, stored, C, 1100, "L2")
        drop = oi_all[0, [0, 5, 1000]]                                          # the excluded rows: two near ones and one of the copies
        ex = torch.sort(tags[torch.from_numpy(drop).to(gpu)])[0]
        if excluding:
            keep = ~np.isin(oi_all[0], drop)
            od_all, oi_all = od_all[:, keep], oi_all[:, keep]
        for k in (1024, 10):
            D = torch.full((nq, k), float("nan"), device=gpu)
            I = torch.full((nq, k), -7, device=gpu, dtype=torch.int64)
            K = torch.full((nq, k), float("nan"), device=gpu, dtype=torch.float64)
            rc = _raw_search(idx, q, k, D, I, K, (tags, ex) if excluding else None)
            what = f"width {width} k {k}"
            if k == 1024 and not fits:
                assert rc == L.RADAD_EINVAL, f"{what}: status {rc}"
                with pytest.raises(ValueError, match="too large for the exact kernel"):
                    L.check(rc)
                torch.cuda.synchronize()
                assert bool(torch.isnan(D).all()) and bool((I == -7).all()) and bool(torch.isnan(K).all()), f"{what}: a refused search wrote its outputs"
                with pytest.raises(ValueError, match="too large for the exact kernel"):
                    (idx.search_excluding(q, k, tags, ex, k_fetch=k) if excluding else idx.search_device(q, k))
                continue
            L.check(rc)
            np.testing.assert_array_equal(I.cpu().numpy(), np.repeat(oi_all[:, :k], nq, axis=0), err_msg=what)
            np.testing.assert_allclose(K.cpu().numpy(), np.repeat(od_all[:, :k], nq, axis=0), rtol=_key_rtol(width), atol=0, err_msg=what)
            assert torch.equal(D, K.float())
            if k == 1024 and fits:
                if excluding:
                    assert idx.last_excl() == {"queries": nq, "exact": nq}, idx.last_excl()       # 3 of the k_fetch = k hits are excluded
                else:
                    assert idx.last_launch()["certificate"]["rejected"] == nq, idx.last_launch()
