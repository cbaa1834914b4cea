"""k_merge_lists<float|double> (radad_topk_merge, radad_topk_merge_f64 with its out_key), k_excl_merge_certify
(radad_excl_merge_certify) and k_kth_largest (radad_kth_largest, HipFlatIndex.global_bound) on synthetic lists straight through the
C ABI, against oracle.merge_topk, sharded_excl_ref.certify and a host k-th largest: part counts around and far beyond the 64 lanes that
stride over them (up to the documented 4096), k up to 1024, ties between parts of one lane, signed zeros, runs of more than k equal
keys, empty parts and empty queries."""
import numpy as np
import pytest

import sharded_bound_ref as B
import sharded_excl_ref as X
from oracle import radad_oracle as O

pytestmark = pytest.mark.gpu

ID0 = 1 << 40                      # ids beyond 32 bits


def _lists(G, nq, k, metric, f64, seed):
    """-> (K [G, nq, k] float32 / float64, I [G, nq, k] int64): sorted lists in the metric's order with (key, lower id) among equals, -1
    only at the tail, padding key +inf (L2) / -inf.  Designed in: parts of every length 0..k; part G // 2 empty for every query (G >= 3);
    the last query without any entry (nq >= 5); query 1 all one key (a run of G k > k equal keys, G >= 2); query 2 short in total (fewer
    than k entries over all parts); discrete keys with +0.0 and -0.0, and -- float64 only -- keys that differ below float32 resolution;
    for G >= 65 the best key of query 0 sits at the head of parts 0 and 64 (one lane reads both), the lower id in part 64."""
    rng = np.random.default_rng(seed)
    l2 = metric == 0
    kt = np.float64 if f64 else np.float32
    K = np.full((G, nq, k), np.inf if l2 else -np.inf, kt)
    I = np.full((G, nq, k), -1, np.int64)
    for j in range(nq):
        ids = ID0 + rng.permutation(3 * G * k)[:G * k].reshape(G, k)
        if nq >= 5 and j == nq - 1:
            continue
        left = k - 1 if j == 2 else None                                  # query 2: fewer than k entries in all
        for g in range(G):
            if G >= 3 and g == G // 2:
                continue
            n = int(rng.integers(0, k + 1)) if rng.integers(4) else int(rng.choice([0, k]))
            if (G >= 65 and j == 0 and g in (0, 64)) or j == 1:
                n = k if j == 1 else max(n, 1)
            if left is not None:
                n = min(n, left, 2)
                left -= n
            if n == 0:
                continue
            key = (rng.integers(-3, 4, n) / 4.0).astype(kt)             # seven levels: ties everywhere, +-0.0 among them
            cont = rng.random(n) < 0.3
            key[cont] = rng.standard_normal(int(cont.sum())).astype(np.float32)
            if f64:
                key[cont] += 1e-12 * rng.integers(-3, 4, int(cont.sum()))      # equal as float32, ordered as float64
            key[(key == 0) & (rng.random(n) < 0.5)] = -0.0
            if j == 1:
                key[:] = 0.5
            order = np.lexsort((ids[g, :n], key if l2 else -key))
            K[g, j, :n], I[g, j, :n] = key[order], ids[g, :n][order]
        if G >= 65 and j == 0:
            best = kt(-7.0 if l2 else 7.0)
            K[0, j, 0], K[64, j, 0] = best, best
            I[0, j, 0], I[64, j, 0] = ID0 + 3 * G * k + 9, ID0 + 3 * G * k + 8
    return K, I


def _design_is_there(K, I, G, nq, k):
    filled = I >= 0
    assert np.all(filled[:, :, :-1] >= filled[:, :, 1:])
    if G >= 3:
        assert not filled[G // 2].any()
    if nq >= 5:
        assert not filled[:, nq - 1].any()
    if nq >= 3:
        assert filled[:, 2].sum() < k
    if G >= 2 and nq >= 2:
        assert filled[:, 1].sum() > k and len(np.unique(K[:, 1][filled[:, 1]])) == 1
    if G >= 65:
        assert K[0, 0, 0] == K[64, 0, 0] and I[64, 0, 0] < I[0, 0, 0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _run_merge(gpu, metric, K, I, want_key):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    G, nq, k = K.shape
    kd, idd = torch.from_numpy(K).to(gpu), torch.from_numpy(I).to(gpu)
    od = torch.full((nq, k), 123.0, device=gpu, dtype=torch.float32)
    oi = torch.full((nq, k), -7, device=gpu, dtype=torch.int64)
    ok = torch.full((nq, k), 123.0, device=gpu, dtype=torch.float64) if want_key else None
    with torch.cuda.device(gpu):
        if K.dtype == np.float64:
            _lib.check(lib.radad_topk_merge_f64(metric, kd.data_ptr(), idd.data_ptr(), G, nq, k, od.data_ptr(), oi.data_ptr(),
                                                ok.data_ptr() if want_key else None, gpu.index, _lib.stream_ptr(gpu)), "radad_topk_merge_f64")
        else:
            _lib.check(lib.radad_topk_merge(metric, kd.data_ptr(), idd.data_ptr(), G, nq, k, od.data_ptr(), oi.data_ptr(), gpu.index,
                                            _lib.stream_ptr(gpu)), "radad_topk_merge")
    return od.cpu().numpy(), oi.cpu().numpy(), ok.cpu().numpy() if want_key else None


# (G, k, nq, metric): every G, k, nq and metric of the grid at least twice; k = 1024 at G <= 65 only, G = 4096 at k <= 15 only
SHAPES = [(1, 1, 1, 0), (1, 15, 5, 1), (2, 15, 7, 0), (2, 128, 64, 2), (2, 1024, 7, 1), (63, 15, 5, 0), (63, 128, 7, 1), (64, 1, 7, 2),
          (64, 15, 64, 0), (64, 1024, 1, 2), (65, 15, 7, 1), (65, 128, 5, 0), (65, 1024, 5, 0), (130, 1, 5, 1), (130, 15, 64, 2),
          (130, 128, 7, 0), (4096, 1, 5, 1), (4096, 15, 7, 0)]


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("G,k,nq,metric", SHAPES)
def test_merge_lists(gpu, G, k, nq, metric, f64):
    K, I = _lists(G, nq, k, metric, f64, 1000 * G + k + nq)
    _design_is_there(K, I, G, nq, k)
    wd, wi = O.merge_topk(list(K), list(I), k, "L2" if metric == 0 else "IP")
    wd = wd.astype(K.dtype)                                               # (merge_topk carries float64; the values are the inputs')
    od, oi, ok = _run_merge(gpu, metric, K, I, want_key=f64)
    ctx = dict(G=G, k=k, nq=nq, metric=metric, f64=f64)
    assert np.array_equal(oi, wi), dict(ctx, bad_rows=np.flatnonzero((oi != wi).any(1))[:10].tolist())
    pad = wi < 0
    tail = np.inf if metric == 0 else -np.inf
    assert np.all(od[pad] == tail) and np.all(oi[pad] == -1), ctx
    if f64:
        assert np.array_equal(_bits(ok), _bits(wd)), ctx                  # the input keys, bit for bit (signed zeros included)
        assert np.array_equal(_bits(od), _bits(wd.astype(np.float32))), ctx
        assert np.all(ok[pad] == tail), ctx
        od2, oi2, _ = _run_merge(gpu, metric, K, I, want_key=False)       # out_key_dev == NULL: the same lists
        assert np.array_equal(oi2, oi) and np.array_equal(_bits(od2), _bits(od)), ctx
    else:
        assert np.array_equal(_bits(od), _bits(wd)), ctx                  # the input distances, bit for bit


def _frontiers(K, I, metric_name, rng):
    """designed frontiers [G, nq] for lists with -1 / NaN padding, by query j % 7:
      0 none (every id -1);  1 M[k-1] itself;  2 M[k-1]'s key with a LOWER id (ranks ahead of it: not proved);  3 its key with a HIGHER
      id;  4 a key far ahead of M[k-1] under id -1 (no frontier);  5 a frontier strictly behind M[k-1], in the last part (>= 64 when
      G >= 65);  6 one strictly ahead of it, in the last part.  Where the merged list is short (M[k-1] is padding) designs 1-3, 5 and 6
      place a real frontier all the same: short + frontier = not proved."""
    G, nq, k = K.shape
    md, mi = X.merge(metric_name, K, I, k)
    FK, FI = np.full((G, nq), np.nan), np.full((G, nq), -1, np.int64)
    worse = 1.0 if metric_name == "L2" else -1.0
    for j in range(nq):
        d, p = j % 7, (j * 37) % G
        short = mi[j, k - 1] < 0
        key, gid = (0.25, ID0 + 5) if short else (md[j, k - 1], mi[j, k - 1])
        if d == 1:
            FK[p, j], FI[p, j] = key, gid
        elif d == 2:
            FK[p, j], FI[p, j] = key, gid - 1
        elif d == 3:
            FK[p, j], FI[p, j] = key, gid + 1
        elif d == 4:
            FK[p, j], FI[p, j] = key - 100.0 * worse, -1
        elif d == 5:
            FK[G - 1, j], FI[G - 1, j] = key + 0.125 * worse, ID0
        elif d == 6:
            FK[G - 1, j], FI[G - 1, j] = key - 0.125 * worse, ID0 + (1 << 20)
        if d in (1, 3) and G > 1 and not short and rng.integers(2):       # a second, harmless frontier elsewhere
            FK[(p + 1) % G, j], FI[(p + 1) % G, j] = key + 1.0 * worse, ID0 + 1
    return FK, FI


@pytest.mark.parametrize("G,k,nq,metric", SHAPES)
def test_excl_merge_certify(gpu, G, k, nq, metric):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    name = "L2" if metric == 0 else "IP"
    K, I = _lists(G, nq, k, metric, True, 2000 * G + k + nq)
    K[I < 0] = np.nan                                                     # the exclusion family's padding
    FK, FI = _frontiers(K, I, name, np.random.default_rng(G + k))
    wk, wi, wu = X.certify(name, K, I, FK, FI)
    if nq >= 7:
        short = wi[:, k - 1] < 0
        assert wu.min() == 0 and wu.max() == 1                            # the design holds proved and unproved queries ...
        assert np.all(wu[np.arange(nq) % 7 == 2] == 1) and np.all(wu[(np.arange(nq) % 7 == 3) & ~short] == 0)
        assert np.all(wu[np.arange(nq) % 7 == 6] == 1) and np.all(wu[(np.arange(nq) % 7 == 5) & ~short] == 0)
        assert wu[2] == 1 and short[2]                                    # ... and a short list beside a frontier
    D, Iout, K64, U = HipFlatIndex.excl_merge_certify(metric, *(torch.from_numpy(x).to(gpu) for x in (K, I, FK, FI)))
    D, Iout, K64, U = D.cpu().numpy(), Iout.cpu().numpy(), K64.cpu().numpy(), U.cpu().numpy()
    ctx = dict(G=G, k=k, nq=nq, metric=metric)
    assert np.array_equal(Iout, wi), ctx
    f = wi >= 0
    assert np.array_equal(_bits(K64[f]), _bits(wk[f])) and np.array_equal(_bits(D[f]), _bits(wk[f].astype(np.float32))), ctx
    assert np.all(np.isnan(K64[~f])) and np.all(np.isnan(D[~f])) and np.all(Iout[~f] == -1), ctx
    assert np.array_equal(U, wu), dict(ctx, got=U.tolist(), want=wu.tolist())


def _kth_input(groups, n, per, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((groups, n, per)).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.inf
    x[rng.random(x.shape) < 0.05] = -np.inf
    x[rng.random(x.shape) < 0.05] = np.nan
    x[rng.random(x.shape) < 0.1] = 0.25                                   # equal values: a round drops ONE copy
    if n > 1:
        x[:, 1, :] = np.nan                                               # a query with nothing but NaN: -inf
    if n > 2:
        x[:, 2, :] = np.inf
    return x


@pytest.mark.parametrize("groups,per,n", [(1, 1280, 5), (1, 1, 3), (1, 77, 9), (10, 128, 7), (40, 32, 6), (3, 10, 1), (7, 15, 130)])
def test_kth_largest_layouts_and_limits(gpu, groups, per, n):
    """groups = 1 is the plain [n][m] layout; 1 x 1280, 10 x 128 and 40 x 32 are the 1280-value limit; k = 1, k = m and between;
    +inf, -inf and NaN entries; n not a multiple of the 4 rows of a workgroup"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    x = _kth_input(groups, n, per, 31 * groups + per)
    xd = torch.from_numpy(x).to(gpu)
    m = groups * per
    for k in sorted(k for k in {1, 2, m // 2 + 1, m - 1, m} if 1 <= k <= m):
        out = torch.full((n,), 123.0, device=gpu, dtype=torch.float32)
        with torch.cuda.device(gpu):
            _lib.check(lib.radad_kth_largest(xd.data_ptr(), n, groups, per, k, out.data_ptr(), gpu.index, _lib.stream_ptr(gpu)),
                       "radad_kth_largest")
        assert np.array_equal(out.cpu().numpy(), B.host_kth_largest(x, k)), (groups, per, n, k)


@pytest.mark.parametrize("G,kk,nq", [(11, 128, 7), (10, 128, 7), (3, 1024, 5)])
def test_global_bound_fallback_ranks_like_the_kernel(gpu, G, kk, nq):
    """beyond 1280 values per query (11 x 128, 3 x 1024) and for CPU tensors HipFlatIndex.global_bound takes torch.topk, which ranks
    NaN HIGHEST; the kernel it stands in for (10 x 128) ranks it lowest.  One function, one rule."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    x = _kth_input(G, nq, kk, 77 + G)
    for k in (1, kk // 2, kk):
        want = B.host_kth_largest(x, k)
        assert np.array_equal(HipFlatIndex.global_bound(torch.from_numpy(x).to(gpu), k).cpu().numpy(), want), (G, kk, k, "device")
        assert np.array_equal(HipFlatIndex.global_bound(torch.from_numpy(x), k).numpy(), want), (G, kk, k, "host tensors")
