"""The bounded two-half search over row shards -- radad_knn_search_begin -> k-th largest of the G k lower bounds ->
radad_knn_search_finish(global_lb) -> radad_topk_merge_f64 -- on the designed stores of tests/sharded_bound_ref.py, against its float64
model: one process, G HipFlatIndex handles on one GPU with id_base set, no collectives.

Every case asserts, in this order: the scan kind of every shard (so that a dispatch change cannot silently take a kernel out of the
test); A the reported values ARE lower bounds of the shard's j-th best exact scores, with zero tolerance; B global_bound is the host's
k-th largest; C what search_finish returns for two bounds -- the one the shards' own values give and the tightest valid one, the
largest float32 not above the exact global k-th best score -- is well formed, exact in key and distance, and holds every row of the
global top k the shard owns; D the merged lists are the oracle's over the whole store; E begin + finish(None) is search_device bit for
bit; F the bound prunes where the store was designed for it (and is not applied where the scan's scores do not compare across shards);
G the exact kernel is not what makes the results right."""
import numpy as np
import pytest

import sharded_bound_ref as M
from conftest import c_knn
from test_gpu_knn_large_k import _check, _gpu_unit, _mk, _stored

pytestmark = pytest.mark.gpu

MAX_K = 128


def _kinds(name, k):
    """the scan every shard was designed to run (csrc/knn.hip knn_plan_scan).  The certified f16 tile scan needs more than 16 queries,
    16 384 rows and 2 (k + 6) entries in its sample lists -- 16 entries x 8 sample tiles on a 16 640-row shard (k <= 58), x 16 on the
    40 000-row one (k <= 122); beyond that the fp32 tile kernels filter.  <= 16 queries stream the f16 plane while k + 6 <= 32.  An
    fp32 shard of <= 6144 rows takes the dense kernel, one between that and 16 384 rows the fp32 tile kernel."""
    if name == "S4":
        return ("hi_tile" if k <= 122 else "f32_tile", "f32_tile", "f32_dense", "f32_dense")
    if name == "S5":
        return ("hi_smallq" if k <= 26 else "f32_tile",) * 3
    return ("hi_tile" if k <= 58 else "f32_tile",) * 3


@pytest.fixture(scope="module")
def shards(gpu, knn_oracle_lib):
    """(store, metric) -> the G handles, the rows as stored, the queries as prepared, the model and the C oracle's top 128 over the
    whole store; one entry is kept (the cases of a store and metric follow one another)"""
    cache = {}

    def get(name, metric):
        if (name, metric) not in cache:
            cache.clear()
            db, q, sizes, info = M.STORES[name]()
            b = M.bases_of(sizes)
            idx, stored = [], []
            for g in range(len(sizes)):
                s = _mk(metric, M.DIM, name in M.F16, id_base=int(b[g]))
                s.add(db[b[g]:b[g + 1]])
                idx.append(s)
                stored.append(_stored(s, sizes[g], gpu))
            stored = np.concatenate(stored)
            qq = _gpu_unit(q, gpu) if metric == "COSINE" else np.ascontiguousarray(q, np.float32)
            od, oi = c_knn(knn_oracle_lib, stored, qq, MAX_K, "L2" if metric == "L2" else "IP")
            cache[(name, metric)] = dict(idx=idx, stored=stored, q=q, qq=qq, sizes=sizes, bases=b, info=info, od=od, oi=oi,
                                         model=M.Model(stored, qq, metric, sizes))
        return cache[(name, metric)]
    yield get
    cache.clear()


def _check_shard_list(c, g, k, metric, D, I, K64, ctx):
    """C: one shard's result of search_finish"""
    m, lo, hi = c["model"], c["bases"][g], c["bases"][g + 1]
    tail = np.inf if metric == "L2" else -np.inf
    filled = I >= 0
    assert np.all(filled[:, :-1] >= filled[:, 1:]), ctx                                  # filled entries first
    assert np.all(I[~filled] == -1) and np.all(D[~filled] == tail) and np.all(K64[~filled] == tail), ctx
    assert np.all((I[filled] >= lo) & (I[filled] < hi)), ctx
    assert not np.isnan(K64).any() and not np.isnan(D).any(), ctx
    sc = -K64 if metric == "L2" else K64                                                 # larger is better
    both = filled[:, :-1] & filled[:, 1:]
    ahead = (sc[:, :-1] > sc[:, 1:]) | ((sc[:, :-1] == sc[:, 1:]) & (I[:, :-1] < I[:, 1:]))
    assert np.all(ahead | ~both), ctx                                                    # strictly ordered by (key, id)
    want = np.take_along_axis(m.S, np.where(filled, I, 0), 1)
    want = -want if metric == "L2" else want
    scale = max(1.0, float(np.abs(c["od"]).max()))
    np.testing.assert_allclose(K64[filled], want[filled], rtol=1e-12, atol=1e-12 * scale, err_msg=str(ctx))
    assert np.array_equal(D[filled], K64[filled].astype(np.float32)), ctx                # the correctly rounded distance
    for j, need in enumerate(m.must_return(g, k)):
        missing = np.setdiff1d(need, I[j])
        assert len(missing) == 0, dict(ctx, query=j, missing=missing.tolist(), scores=m.S[j, missing].tolist(), kth=float(m.kth(k)[j]))


CASES = ([("S1", m, k) for m in ("L2", "COSINE") for k in (1, 10, 128)]
         + [("S2", "L2", 1), ("S2", "L2", 10), ("S2", "COSINE", 10)]
         + [("S3", m, k) for m in ("L2", "COSINE", "IP") for k in (4, 7)]
         + [("S4", "L2", 1), ("S4", "L2", 10), ("S4", "L2", 128), ("S4", "COSINE", 10), ("S4", "COSINE", 128),
            ("S4", "IP", 1), ("S4", "IP", 10), ("S4", "IP", 128)]
         + [("S5", "L2", 1), ("S5", "L2", 10), ("S5", "COSINE", 10), ("S5", "COSINE", 128)]
         + [("S6", "L2", 10), ("S6", "COSINE", 1), ("S6", "COSINE", 10), ("S6", "COSINE", 128)])


@pytest.mark.parametrize("name,metric,k", CASES)
def test_bounded_search_on_designed_store(gpu, shards, name, metric, k):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge
    c = shards(name, metric)
    idx, m, sizes = c["idx"], c["model"], c["sizes"]
    G, nq = len(idx), m.nq
    kinds = _kinds(name, k)
    qd = torch.from_numpy(c["q"]).to(gpu)
    ctx0 = dict(store=name, metric=metric, k=k)

    def two_halves(bound):
        """-> (lbs [G] tensors, results [G] of (D, I, K64) tensors, certificates [G]); the scan kind is asserted on the way"""
        lbs = [s.search_begin(qd, k) for s in idx]
        out, certs = [], []
        for g, s in enumerate(idx):
            out.append(s.search_finish(bound, return_f64=True))
            info = s.last_launch()
            assert info["scan_kind"] == kinds[g], dict(ctx0, shard=g, info=info)
            assert info["certificate"]["queries"] == nq, dict(ctx0, shard=g, info=info)
            certs.append(info["certificate"])
        return lbs, out, certs

    # ---- E: begin + finish(None) == search_device, bit for bit ------------------------------------------------------------------
    plain = [s.search_device(qd, k, return_f64=True) for s in idx]
    lbs, own, cert_none = two_halves(None)
    for g in range(G):
        for a, b, what in zip(own[g], plain[g], "DIK"):
            assert torch.equal(a, b), dict(ctx0, shard=g, what=what)

    # ---- A: the bound is a bound ----------------------------------------------------------------------------------------------------
    lb_np = np.stack([x.cpu().numpy() for x in lbs])
    assert lb_np.dtype == np.float32 and lb_np.shape == (G, nq, k) and not np.isnan(lb_np).any(), ctx0
    for g in range(G):
        got = -np.sort(-lb_np[g], axis=1)
        if kinds[g] != "hi_tile":                                    # fp32 tile, dense, small batch: no bound is reported
            assert np.all(got == -np.inf), dict(ctx0, shard=g)
            continue
        have = min(k, sizes[g])
        exact = m.shard_sorted(g)[:, :have]
        over = got[:, :have].astype(np.float64) > exact
        assert not over.any(), dict(ctx0, shard=g, first=np.argwhere(over)[:5].tolist(), got=got[:, :have][over][:5].tolist(),
                                    exact=exact[over][:5].tolist())
        assert np.all(got[:, have:] == -np.inf), dict(ctx0, shard=g)

    # ---- B: global_bound == the host's k-th largest of the same values ------------------------------------------------------------------
    glb = HipFlatIndex.global_bound(torch.stack(lbs), k)
    glb_np = glb.cpu().numpy()
    assert np.array_equal(glb_np, M.host_kth_largest(lb_np, k)), ctx0
    assert np.all(glb_np.astype(np.float64) <= m.kth(k)), ctx0       # (follows from A: the k-th largest of valid bounds of G k rows)

    # ---- C, D, F, G for both bounds -----------------------------------------------------------------------------------------------------
    tight = torch.from_numpy(m.tightest_bound(k)).to(gpu)
    od, oi = c["od"][:, :k], c["oi"][:, :k]
    for which, bound in (("global_bound", glb), ("tightest", tight)):
        ctx = dict(ctx0, bound=which)
        _, res, certs = two_halves(bound)
        res = [tuple(t.cpu().numpy() for t in r) for r in res]
        for g in range(G):
            D, I, K64 = res[g]
            cg = dict(ctx, shard=g, kind=kinds[g], certificate=certs[g])
            _check_shard_list(c, g, k, metric, D, I, K64, cg)
            if name == "S2" and g != 1:
                # F: nothing of shards 0 and 2 can be among the global k best, by a gap hundreds of times any eps
                back = np.argwhere(I >= 0)
                assert len(back) == 0, dict(cg, rows=[(int(j), int(I[j, t]), float(K64[j, t]), float(bound[j])) for j, t in back[:5]])
            if name == "S1":
                assert certs[g]["candidates_rescored"] <= cert_none[g]["candidates_rescored"], dict(cg, unbounded=cert_none[g])
            if name == "S4" and metric == "L2" and kinds[g] != "hi_tile":
                # F: the fp32 kernels' L2 scores lack |q|^2: the bound does not apply to them, the shard returns its own top k
                want = np.full((nq, k), -1, np.int64)
                top = m.shard_topk(g, k)
                want[:, :top.shape[1]] = top
                assert np.array_equal(I, want), cg
            if name in ("S1", "S2", "S5"):
                assert certs[g]["rejected"] <= max(1, nq // 50), cg                      # G
        md, mi = hip_merge(idx[0].metric, torch.stack([torch.from_numpy(r[2]) for r in res]).to(gpu),
                           torch.stack([torch.from_numpy(r[1]) for r in res]).to(gpu), k)
        ctx["rejected"] = [x["rejected"] for x in certs]
        # (S3's expected ids are exact under every metric: bit-equal rows, bit-equal keys -- no multiset fallback there)
        _check(md.cpu().numpy(), mi.cpu().numpy(), od, oi, c["stored"], c["qq"], "IP" if name == "S3" and metric == "COSINE" else metric,
               ctx=ctx)
        assert np.array_equal(oi, m.topk(k)[1]) or metric == "COSINE", ctx               # the two oracles agree
