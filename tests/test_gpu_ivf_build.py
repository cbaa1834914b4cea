"""The BUILD side of the inverted-file index (csrc/ivf.inc: radad_ivf_train, radad_ivf_add) against a float64 Lloyd
(oracle/radad_oracle.py: kmeans_init, kmeans_assign, kmeans_step).  The search tests take an index's centroids and assignments as
given; here they are what is checked.

  initialisation  niter = 0 centroids are bit-equal to the training rows (c * n) // nlist
  Lloyd           one step at a time from the device's own state: C_t = train(niter = t).centroids() is reproducible, so C_{t+1} is
                  compared with kmeans_step(rows, C_t) -- a flipped near-tie cannot make two trajectories drift apart
  assignment      set_centroids + add at the batch sizes the product uses, on every scan the quantiser (a flat k = 1 search of the
                  centroid store with the added rows as queries) can take; exact against the C float64 oracle on a sample, and
                  over the full width against itself (a row's list must not depend on the batch it arrived in)
  non-finite rows refused by add and train with ValueError, the index left exactly as it was

Tolerances.  Assignments and initial centroids: exact equality.  Means: the worst-case bound of the kernel's arithmetic
(k_centroid_update: a sequential fp32 sum of the list's m rows, one fp32 division), u = 2^-24, gamma_k = k u / (1 - k u):

    |C[c, j] - mean| <= gamma_(m-1) (sum_r |x[r, j]|) / m + u |mean|

with no multiplier.  The condition under which "the float64 argmin" is the only defensible list is ASSERTED on the CPU (assert_gap):
no row has its two nearest distinct-valued centroids closer than 1e-12 (|x|^2 + |c|^2) apart.  Identical centroids are legitimate
(n < nlist, planted duplicates): all their rows go to the lower id, the higher id stays empty and unmoved."""

import numpy as np
import pytest

from conftest import c_knn
from oracle import radad_oracle as O
from oracle import synth

U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# ---- CPU side ---------------------------------------------------------------------------------------------------------------------
def _knn_fn(lib):
    return lambda db, q, k: c_knn(lib, db, q, k, "L2")


def assert_gap(lib, rows, cent, what):
    """no row's two nearest DISTINCT-VALUED centroids are closer than 1e-12 (|x|^2 + |c|^2) apart in float64; returns the rows'
    distance to their nearest centroid"""
    uniq = np.unique(np.asarray(cent, np.float32), axis=0)
    d, i = c_knn(lib, uniq, rows, min(2, len(uniq)), "L2")
    if len(uniq) > 1:
        x2 = (np.asarray(rows, np.float64) ** 2).sum(1)
        c2 = (uniq.astype(np.float64) ** 2).sum(1)
        scale = x2 + np.maximum(c2[i[:, 0]], c2[i[:, 1]])
        bad = np.flatnonzero(d[:, 1] - d[:, 0] <= 1e-12 * scale)
        assert len(bad) == 0, f"{what}: {len(bad)} rows (first {bad[:5]}) have two centroids {d[bad[0], 1] - d[bad[0], 0]:.3e} apart: pick another seed"
    return d[:, 0]


def mean_bound(rows, assign, counts, mean):
    """the derived bound of a sequential fp32 sum of m rows and one fp32 division, per (list, column); 0 for empty lists"""
    nlist = len(counts)
    s_abs = np.zeros((nlist, rows.shape[1]))
    np.add.at(s_abs, assign, np.abs(rows.astype(np.float64)))
    m = np.maximum(counts, 1)[:, None].astype(np.float64)
    return np.where(counts[:, None] > 0, gamma(m - 1) * s_abs / m + U * np.abs(mean), 0.0)


def last_rows(rows, assign, counts):
    """the last row (in insertion order) of every list; zeros for empty lists"""
    last = np.zeros((len(counts), rows.shape[1]))
    idx = np.full(len(counts), -1, np.int64)
    idx[assign] = np.arange(len(rows))                      # (later rows overwrite earlier ones)
    last[idx >= 0] = rows[idx[idx >= 0]].astype(np.float64)
    return last


def assert_sharp(rows, assign, counts, mean, bound, what):
    """the bound tells a mean from one that left a row out: for every list of two or more rows, the sum without the list's last row
    divided by m (what a loop that stops one row early computes) and the mean of the other m - 1 rows both miss it somewhere --
    unless all the list's rows equal the last one, where the second is the same mean.  Guards against a later change of a generator
    that blunts the test."""
    last = last_rows(rows, assign, counts)
    m = np.maximum(counts, 2)[:, None].astype(np.float64)
    short = np.abs(last) / m                                 # |(s - x) / m - s / m|
    loo = np.abs(mean - last) / (m - 1)                      # |(s - x) / (m - 1) - s / m|
    for c in np.flatnonzero(counts >= 2):
        assert (short[c] > bound[c]).any(), f"{what}: list {c} ({counts[c]} rows): a sum one row short stays within the bound"
        if loo[c].max() > 0:
            assert (loo[c] > bound[c]).any(), f"{what}: list {c} ({counts[c]} rows): a mean without the last row stays within the bound"


def _blobs(n, dim, n_clusters, seed, spread=3.0):
    centers = synth.rows(0, n_clusters, dim, seed) * np.float32(spread)
    which = (np.arange(n) * 7919) % n_clusters
    return (centers[which] + synth.rows(0, n, dim, seed + 1)).astype(np.float32)


def _embedding_like(n, dim, seed):
    """one large positive common component, individual parts an order of magnitude smaller: 2 x.c - |c|^2 cancels, and a quantity
    centred on the wrong mean goes wrong"""
    base = np.abs(synth.rows(0, 1, dim, seed)) + np.float32(0.5)
    return (base + np.float32(0.3) * synth.rows(0, n, dim, seed + 1)).astype(np.float32)


def training_set(kind, n, dim, seed):
    if kind == "blobs":
        return _blobs(n, dim, 50, seed)
    if kind == "embedding_like":
        return _embedding_like(n, dim, seed)
    if kind == "many_clusters":                              # clusters far outnumber the lists
        return _blobs(n, dim, 400, seed, spread=2.0)
    if kind == "few_distinct":
        # fewer distinct rows than lists: the initial centroids repeat.  The values are multiples of 1/16 below 16: a list of m <= 3000
        # copies of x sums and divides exactly in fp32, so its centroid stays x.  (With arbitrary values the lower id's centroid moves by a
        # rounding error while the empty higher id keeps x exactly: two distinct centroids ~1e-10 apart, inside the gap condition's band.)
        distinct = (np.round(_blobs(40, dim, 40, seed) * np.float32(16)) / np.float32(16)).astype(np.float32)
        return distinct[(np.arange(n) * 7) % 40]
    raise KeyError(kind)


def _train(gpu, rows, nlist, niter):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    idx = R.HipIVFFlatIndex(rows.shape[1], nlist, gpu.index or 0, niter=niter)
    idx.train(rows)
    assert idx.is_trained
    return idx


# ---- initialisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 96, 5376])
@pytest.mark.parametrize("n,nlist", [(640, 64), (1000, 64), (1001, 48), (64, 64), (20, 64), (1, 64)])
def test_initial_centroids_are_the_strided_rows(gpu, dim, n, nlist):
    """niter = 0: centroid c is training row (c * n) // nlist, bit for bit -- n a multiple of nlist, not a multiple, n == nlist,
    n < nlist (rows repeat), one row"""
    rows = _blobs(n, dim, 7, 3100 + n)
    cent = _train(gpu, rows, nlist, 0).centroids()
    want = O.kmeans_init(rows, nlist)
    assert cent.shape == want.shape and cent.dtype == np.float32
    assert cent.tobytes() == want.tobytes(), np.flatnonzero((cent != want).any(1))[:8]
    if n % nlist and n > 1:
        assert not np.array_equal(want, rows[np.arange(nlist) * (n // nlist)])      # (the case tells the rule from c * (n // nlist))


# ---- Lloyd, step by step from the device's own state ------------------------------------------------------------------------------
def _lloyd_check(gpu, lib, rows, nlist, steps, what, sharp):
    knn_fn = _knn_fn(lib)
    n, dim = rows.shape
    cents = [_train(gpu, rows, nlist, t).centroids() for t in range(steps + 1)]
    assert cents[0].tobytes() == O.kmeans_init(rows, nlist).tobytes(), what
    nearest = assert_gap(lib, rows, cents[0], f"{what} t=0")
    saw_duplicates = False
    for t in range(steps):
        ct, cn = cents[t], cents[t + 1]
        w = f"{what} t={t}"
        mean, assign, counts = O.kmeans_step(rows, ct, knn_fn)
        # identical centroids: every row goes to the lowest id among them, the others stay empty (and, below, unmoved)
        uniq, first, inv = np.unique(ct, axis=0, return_index=True, return_inverse=True)
        higher = np.flatnonzero(first[inv.reshape(-1)] != np.arange(nlist))
        saw_duplicates |= len(higher) > 0
        assert counts[higher].sum() == 0, (w, higher[:8])
        empty = counts == 0
        assert cn[empty].tobytes() == ct[empty].tobytes(), f"{w}: an empty list's centroid moved: {np.flatnonzero(empty & (cn != ct).any(1))[:8]}"
        bound = mean_bound(rows, assign, counts, mean)
        if sharp:
            assert counts.max() <= 2000, (w, counts.max())
            assert_sharp(rows, assign, counts, mean, bound, w)
        err = np.abs(cn.astype(np.float64) - mean)
        over = err > bound
        print(f"{w}: lists {int((~empty).sum())}/{nlist} non-empty, largest {counts.max()}, max err/bound "
              f"{np.max(err[~empty] / np.maximum(bound[~empty], 1e-300)):.3g}")
        assert not over.any(), f"{w}: {over.sum()} elements of {np.unique(np.nonzero(over)[0])[:8]} beyond the fp32 mean's bound: " \
                               f"err {err[over].max():.3e} vs bound {bound[over].min():.3e}"
        # Lloyd's monotonicity in float64: the exact means cannot raise the cost; a mean moved by delta raises its list's cost by
        # m |delta|^2, |delta_j| <= bound.  (The evaluation's own float64 rounding: n sums of dim squares, (n + dim) 2^-53 relative.)
        nearest_next = assert_gap(lib, rows, cn, f"{what} t={t + 1}")
        cost_t, cost_n = nearest.sum(), nearest_next.sum()
        slack = (counts * (bound ** 2).sum(1)).sum() + 2 * (n + dim) * 2.0 ** -53 * cost_t
        assert cost_n <= cost_t + slack, f"{w}: cost rose from {cost_t!r} to {cost_n!r} (allowed {slack:.3e})"
        nearest = nearest_next
    return saw_duplicates


LLOYD_CASES = [("blobs", 64, 8000, 64), ("embedding_like", 512, 4000, 64), ("embedding_like", 96, 6000, 48),
               ("many_clusters", 96, 6000, 32), ("few_distinct", 64, 3000, 64), ("blobs", 512, 5000, 100),
               ("blobs", 5376, 1500, 32), ("blobs", 64, 40, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dim,n,nlist", LLOYD_CASES)
def test_lloyd_steps_match_the_float64_mean(gpu, knn_oracle_lib, kind, dim, n, nlist):
    """four Lloyd steps, each from the centroids the device holds: C_{t+1} within the derived bound of the float64 mean of the float64
    assignment to C_t, empty lists bit-equal, duplicates to the lower id, the float64 cost not rising"""
    rows = training_set(kind, n, dim, 3200 + dim + nlist)
    dup = _lloyd_check(gpu, knn_oracle_lib, rows, nlist, 4, f"{kind} dim {dim} n {n} nlist {nlist}", sharp=True)
    if kind == "few_distinct" or n < nlist:
        assert dup, "the case was built to start from repeated centroids"


@pytest.mark.gpu
def test_lloyd_long_lists(gpu, knn_oracle_lib):
    """lists of ~25 000 rows.  The worst-case bound grows with the list (gamma_(m-1)): here it is LOOSE -- a row left out of a mean
    errs by |x| / m, which is inside it.  This case checks indexing (offsets and the permutation of long lists, the column blocks),
    not rounding."""
    rows = _blobs(100000, 64, 4, 3301)
    _lloyd_check(gpu, knn_oracle_lib, rows, 4, 2, "long lists", sharp=False)


# ---- assignment at the batch sizes the product uses ------------------------------------------------------------------------------------
def _assign_store(nlist, dim, n, kind, seed):
    if kind == "embedding_like":
        cent = _embedding_like(nlist, dim, seed)
        base = cent - np.float32(0.3) * synth.rows(0, nlist, dim, seed + 1)       # (the shared component again, to rounding)
        rows = (base[(np.arange(n) * 7919) % nlist] + np.float32(0.3) * synth.rows(0, n, dim, seed + 2)).astype(np.float32)
    else:       # rows near the boundary between two centroids: w c_a + (1 - w) c_b + noise, w = 0.5 +- a few per cent
        cent = synth.rows(0, nlist, dim, seed).astype(np.float32)
        i = np.arange(n, dtype=np.int64)
        a, b = (i * 7919) % nlist, (i * 104729 + 1) % nlist
        w = np.float32(0.5) + np.float32(0.02) * synth.rows(0, n, 1, seed + 3)
        rows = (w * cent[a] + (np.float32(1) - w) * cent[b] + np.float32(0.05) * synth.rows(0, n, dim, seed + 2)).astype(np.float32)
    return cent, rows


def _sample(n, m=8192):
    """m rows spread evenly, plus the first and last 256 of the batch (ragged first and last query tiles)"""
    return np.unique(np.concatenate([np.arange(min(256, n)), np.arange(max(0, n - 256), n), np.linspace(0, n - 1, min(m, n)).astype(np.int64)]))


# nlist, dim, batch, store, the scan a flat k = 1 search of that batch takes over that many centroids (knn_plan_scan):
#   dense     <= 6144 centroids and batch x nlist <= 2^24 scores
#   f32_tile  past either limit (10 000 x 4096 is what VectorDatabase appends at nlist 4096); k_knn_f32_reg: radad_ivf_create takes
#             dim % 32 == 0 only, so the generic tile kernel (dim % 32 != 0, or lists longer than 32) is out of the quantiser's reach
#   hi_tile   >= 16 384 centroids, dim % 64 == 0: the certified f16 tile scan, hundreds of query tiles
ASSIGN_CASES = [(64, 128, 100000, "unit", "f32_dense"), (64, 128, 300000, "unit", "f32_tile"), (4096, 512, 10000, "embedding_like", "f32_tile"),
                (1024, 96, 50000, "unit", "f32_tile"), (16384, 64, 200000, "unit", "hi_tile")]


@pytest.mark.gpu
@pytest.mark.parametrize("nlist,dim,n,kind,scan", ASSIGN_CASES)
def test_assignment_at_product_batch_sizes(gpu, knn_oracle_lib, nlist, dim, n, kind, scan):
    """set_centroids + add: the scan the batch takes (flat twin, whose ids must equal assignments() in full), the float64 argmin on
    a sample with the first and last query tile, and the same lists whatever batches the rows arrive in.  The certificate's count of
    rejected queries is printed, not bounded (which queries it rejected is not exposed)."""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    what = f"nlist {nlist} dim {dim} batch {n}"
    cent, rows = _assign_store(nlist, dim, n, kind, 3400 + nlist)
    if nlist == 64:
        cent[5] = cent[2]                                    # planted duplicate: list 5 must stay empty
    rows_d = torch.from_numpy(rows).to(gpu)

    def index_with(batches):
        idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
        idx.set_centroids(cent)
        s = 0
        for b in batches:
            idx.add(rows_d[s:s + b])
            s += b
        assert s == n and idx.ntotal == n
        return idx

    idx = index_with([n])
    assign = idx.assignments()
    np.testing.assert_array_equal(idx.centroids(), cent)
    assert assign.dtype == np.int32 and assign.min() >= 0 and assign.max() < nlist
    # the scan the batch took, on a flat twin of the (private) quantiser: same centroids, same batch, k = 1
    twin = R.HipFlatIndex(dim, _lib.METRIC_L2, gpu.index or 0)
    twin.add(cent)
    kinds = {}
    for b in (n, 10000, 17, 16, 1):
        D, I = twin.search_device(rows_d[:b], 1)
        launch = twin.last_launch()
        kinds[b] = launch["scan_kind"]
        np.testing.assert_array_equal(I[:, 0].cpu().numpy(), assign[:b], err_msg=f"{what}: the twin's search of the first {b} rows")
        if b == n:
            cert = launch["certificate"]
    print(f"{what}: scan kind per batch size {kinds}; certificate of the full batch {cert}")
    assert kinds[n] == scan, (what, kinds)
    assert cert["queries"] == n and 0 <= cert["rejected"] <= n, cert
    # exact against the C float64 oracle on a sample that holds the first and the last query tile
    sel = _sample(n)
    assert len(sel) >= 4096 and sel[0] == 0 and sel[-1] == n - 1
    assert_gap(knn_oracle_lib, rows[sel], cent, what)
    want = O.kmeans_assign(rows[sel], cent, _knn_fn(knn_oracle_lib))
    wrong = np.flatnonzero(assign[sel] != want)
    assert len(wrong) == 0, f"{what}: {len(wrong)} of {len(sel)} sampled rows in another list than the float64 argmin, first rows {sel[wrong[:8]]}: " \
                            f"{assign[sel][wrong[:8]]} vs {want[wrong[:8]]}"
    if nlist == 64:
        assert (assign == 5).sum() == 0 and (assign == 2).sum() > 0
    # full width, no oracle: a row's list does not depend on the batch it arrived in
    per_10k = [10000] * (n // 10000) + ([n % 10000] if n % 10000 else [])
    for name, batches in (("batches of 10 000", per_10k), ("1 + 16 + 17 + the rest", [1, 16, 17, n - 34])):
        if batches == [n]:
            continue
        other = index_with(batches).assignments()
        diff = np.flatnonzero(other != assign)
        assert len(diff) == 0, f"{what}: {len(diff)} rows change their list when added as {name}, first {diff[:8]}"


# ---- non-finite rows ---------------------------------------------------------------------------------------------------------------------
def _state(idx, q):
    idx.nprobe = 4
    D, I = idx.search(q, 5)
    return idx.ntotal, idx.assignments().copy(), idx.centroids().copy(), D, I


def _assert_state(idx, q, state, what):
    n, assign, cent, D, I = state
    n2, assign2, cent2, D2, I2 = _state(idx, q)
    assert n2 == n, (what, n2, n)
    assert assign2.tobytes() == assign.tobytes() and cent2.tobytes() == cent.tobytes(), what
    assert np.array_equal(I2, I) and D2.tobytes() == D.tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("nlist,dim,batch,scan", [(64, 64, 2000, "f32_dense"), (6400, 64, 3000, "f32_tile"), (64, 96, 17, "f32_dense"), (64, 64, 5, "f32_dense")])
def test_add_refuses_non_finite_rows(gpu, knn_oracle_lib, nlist, dim, batch, scan):
    """one NaN or infinity in one added row: ValueError naming the row, nothing appended, nothing changed, the index still usable.
    (faiss counts such a row in ntotal and puts it in no list; here a row without a list is refused: INTEGRATION.md.)"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    cent, rows = _assign_store(nlist, dim, 2000 + 2 * batch + 40, "unit", 3500 + nlist)
    q = rows[-40:]
    twin = R.HipFlatIndex(dim, _lib.METRIC_L2, gpu.index or 0)
    twin.add(cent)
    twin.search(rows[:batch], 1)
    assert twin.last_launch()["scan_kind"] == scan
    idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    idx.set_centroids(cent)
    idx.add(rows[:1000])
    added = [rows[:1000]]
    state = _state(idx, q)
    s = 1000
    for value in (np.nan, np.inf, -np.inf):
        for pos in (0, batch // 2, batch - 1):
            bad = rows[s:s + batch].copy()
            bad[pos, 3 if value != value else dim - 1] = value
            what = f"{value} at row {pos} of {batch}"
            with pytest.raises(ValueError, match=rf"row {pos} "):
                idx.add(bad)
            _assert_state(idx, q, state, what)
            clean = rows[s:s + 100]
            idx.add(clean)                                    # a clean add afterwards works
            added.append(clean)
            s += 100
            state = _state(idx, q)
            assert state[0] == sum(len(a) for a in added), what
    whole = rows[s:s + batch].copy()
    whole[batch // 3] = np.nan                               # a row of NaNs, and a second bad row behind it: the FIRST is named
    whole[batch - 1, 0] = np.inf
    with pytest.raises(ValueError, match=rf"row {batch // 3} "):
        idx.add(whole)
    _assert_state(idx, q, state, "a row of NaNs")
    db = np.concatenate(added)
    np.testing.assert_array_equal(idx.assignments(), O.kmeans_assign(db, cent, _knn_fn(knn_oracle_lib)))
    od, oi = O.ivf_search(db, idx.assignments(), cent, q, 5, 4)
    np.testing.assert_array_equal(state[4], oi)


@pytest.mark.gpu
@pytest.mark.parametrize("niter", [0, 3])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_train_refuses_non_finite_rows(gpu, knn_oracle_lib, niter, value):
    """a non-finite training row: ValueError, a fresh index stays untrained, a trained one keeps its centroids and its quantiser.
    niter = 0 looks only at the rows it picks as centroids: one of THOSE is refused (row (c * n) // nlist), another is never read."""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    dim, nlist, n = 64, 64, 4000
    rows = _blobs(n + 500, dim, 50, 3601)
    train, extra, q = rows[:n], rows[n:], rows[n:n + 30]
    picked = (17 * n) // nlist                               # the initial centroid of list 17
    for pos in (0, picked, n - 1) if niter else (0, picked):
        bad = train.copy()
        bad[pos, 7] = value
        fresh = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, niter=niter)
        with pytest.raises(ValueError, match=rf"row {pos} "):
            fresh.train(bad)
        assert not fresh.is_trained and fresh.ntotal == 0
        with pytest.raises(ValueError):
            fresh.add(extra)                                 # still untrained
        fresh.train(train)                                   # and still trainable
        good = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, niter=niter)
        good.train(train)
        assert fresh.centroids().tobytes() == good.centroids().tobytes()
        # a trained index with rows keeps everything
        good.add(extra)
        state = _state(good, q)
        with pytest.raises(ValueError, match=rf"row {pos} "):
            good.train(bad)
        assert good.is_trained
        _assert_state(good, q, state, f"{value} at training row {pos}")
        good.add(train[:300])                                # the quantiser it kept still assigns
        want = O.kmeans_assign(np.concatenate([extra, train[:300]]), state[2], _knn_fn(knn_oracle_lib))
        np.testing.assert_array_equal(good.assignments(), want)
    if niter == 0:
        bad = train.copy()
        bad[picked + 1, 7] = value                           # not an initial centroid: niter = 0 never reads it
        idx = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0, niter=0)
        idx.train(bad)
        assert idx.centroids().tobytes() == O.kmeans_init(train, nlist).tobytes()


# ---- CPU: the sharpness argument without a GPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,nlist", [c for c in LLOYD_CASES if c[1] <= 512])
def test_cpu_the_bound_tells_a_mean_from_one_a_row_short(knn_oracle_lib, kind, dim, n, nlist):
    """no GPU: on every sharp training set, from the initial centroids, leaving the last row out of any list's mean breaks the
    bound, lists stay at or below 2000 rows, and the gap condition holds"""
    rows = training_set(kind, n, dim, 3200 + dim + nlist)
    cent = O.kmeans_init(rows, nlist)
    assert_gap(knn_oracle_lib, rows, cent, kind)
    mean, assign, counts = O.kmeans_step(rows, cent, _knn_fn(knn_oracle_lib))
    assert counts.max() <= 2000 and counts.sum() == n
    bound = mean_bound(rows, assign, counts, mean)
    assert_sharp(rows, assign, counts, mean, bound, kind)
    assert (np.abs(mean.astype(np.float32).astype(np.float64) - mean) <= bound).all()      # (and the rounded float64 mean is inside it)
