"""CPU: the per-row rule of the deferring tile scan (tests/abandon_defer_ref.py) in fp32.  The rows it flags live are a SUPERSET of the
rows with a pair whose full fp32 sum reaches the floor -- for sequential, pairwise and blocked accumulation of the partial and of the
full sum, at dims 128, 512 and 5376, with floors set ON full scores so that the comparison is decided by the last bits -- and a NaN
or -inf floor keeps every row live.  And it is not vacuous: on a tile shaped like the benchmark's, the planted rows are live and no
other row is."""
import numpy as np
import pytest

import abandon_defer_ref as D
import abandon_ref as A

DIMS = (128, 512, 5376)
ROWS, QUERIES = 40, 6


def _f16(x):
    return np.clip(x, -65504.0, 65504.0).astype(np.float16)


def _tile(dim, rng, bias):
    """queries close to each other, random rows, five rows near a query (one of them with its energy behind the checkpoint)"""
    e0 = 64 * A.checkpoint(dim)
    base = rng.standard_normal(dim)
    q = base[None, :] + 0.05 * rng.standard_normal((QUERIES, dim))
    y = rng.standard_normal((ROWS, dim))
    near = [3, 11, 12, 29, 39]
    for i, r in enumerate(near):
        y[r] = q[i % QUERIES] + 0.03 * rng.standard_normal(dim)
    y[29, :e0] *= 0.01
    qh, yh = _f16(q * 3000.0), _f16(y * 3000.0)
    c0 = (rng.standard_normal(ROWS) * 0.05 * np.max(A.norm_f32(qh)) * np.max(A.norm_f32(yh))).astype(np.float32) if bias else np.zeros(ROWS, np.float32)
    return qh, yh, c0, e0, near


def _scores(qh, yh, c0, e0):
    """partial sums at the checkpoint and full sums, [order][ROWS, QUERIES]"""
    pq, py = D.pairs(qh, yh)
    pc = np.repeat(c0, QUERIES)
    dim = qh.shape[1]
    partial = {o: f(pq, py, pc, 0, e0) for o, f in A.ORDERS.items()}
    full = {o: f(pq, py, pc, 0, dim) for o, f in A.ORDERS.items()}
    for o, p in partial.items():
        full["continued_" + o] = A.acc_sequential(pq, py, p, e0, dim)
    shape = lambda d: {o: v.reshape(ROWS, QUERIES) for o, v in d.items()}
    return shape(partial), shape(full)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("bias", [False, True])
def test_live_rows_cover_every_row_that_reaches_the_floor(dim, bias):
    rng = np.random.default_rng(3 * dim + bias)
    qh, yh, c0, e0, near = _tile(dim, rng, bias)
    partial, full = _scores(qh, yh, c0, e0)
    rq, ry, sl = D.tile_terms(qh, yh, c0, e0)
    ref = full["sequential"]
    # floors: exactly the score of a near row (it reaches its floor by equality), one ulp above and below it, and the tile's median
    floors = []
    for r in near:
        for step in (0, 1, -1):
            at = ref[r].copy()
            for _ in range(abs(step)):
                at = np.nextafter(at, np.float32(np.inf if step > 0 else -np.inf))
            floors.append(at)
    floors.append(np.median(ref, axis=0).astype(np.float32))
    for at in floors:
        reach = np.zeros(ROWS, bool)
        for f in full.values():
            reach |= (f >= at[None, :]).any(axis=1)
        for po, p in partial.items():
            live = D.live_rows(p, rq, ry, sl, at)
            assert not (reach & ~live).any(), f"dim {dim} partial {po}: rows {np.nonzero(reach & ~live)[0]} reach the floor and are not live"


@pytest.mark.parametrize("dim", DIMS)
def test_nan_and_minus_infinity_floors_keep_every_row_live(dim):
    rng = np.random.default_rng(dim)
    qh, yh, c0, e0, _ = _tile(dim, rng, False)
    partial, _ = _scores(qh, yh, c0, e0)
    rq, ry, sl = D.tile_terms(qh, yh, c0, e0)
    high = np.full(QUERIES, np.float32(3.0e38))
    assert not D.live_rows(partial["sequential"], rq, ry, sl, high).any()          # (the other floors: nothing is live)
    for bad in (np.nan, -np.inf):
        for j in range(QUERIES):
            at = high.copy()
            at[j] = bad
            for p in partial.values():
                assert D.live_rows(p, rq, ry, sl, at).all(), (dim, bad, j)
    nan_term = sl.copy()
    nan_term[2] = np.nan
    assert D.live_rows(partial["sequential"], rq, ry, nan_term, high).all()        # a NaN in a term, too


@pytest.mark.parametrize("dim", (128, 512))
@pytest.mark.parametrize("planted", (8, 16, 17))
def test_the_benchmark_in_miniature_lists_the_planted_rows_only(dim, planted):
    """a 256-row tile of the GPU tests' store: unit-norm rows x 2^14, near-duplicates of the queries at 3 + 15 i, the floor just below
    the weakest of them: exactly the planted rows are live, so the tile is deferred up to 16 of them and continues at 17"""
    rng = np.random.default_rng(dim + planted)
    e0 = 64 * A.checkpoint(dim)
    base = rng.standard_normal(dim)
    amp = np.linalg.norm(base) / np.sqrt(dim)
    q = base[None, :] + 0.05 * amp * rng.standard_normal((QUERIES, dim))
    y = rng.standard_normal((256, dim))
    ids = np.array([3 + 15 * i for i in range(planted)])
    y[ids] = q[np.arange(planted) % QUERIES] + 0.03 * amp * rng.standard_normal((planted, dim))
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    qh, yh = _f16(unit(q) * 2.0 ** 14), _f16(unit(y) * 2.0 ** 14)
    c0 = np.zeros(256, np.float32)
    acc_c = (qh[:, :e0].astype(np.float32) @ yh[:, :e0].astype(np.float32).T).T            # [rows, queries]
    full = (qh.astype(np.float64) @ yh.astype(np.float64).T).T
    at = (full[ids].min(axis=0) - 0.001 * 2.0 ** 28).astype(np.float32)                    # cos 0.001 below the weakest planted row
    rq, ry, sl = D.tile_terms(qh, yh, c0, e0)
    live = D.live_rows(acc_c.astype(np.float32), rq, ry, sl, at)
    assert np.array_equal(np.nonzero(live)[0], ids), (np.nonzero(live)[0], ids)
    assert D.decision(live) == ("defer" if planted <= D.MAX_ROWS else "continue")
    assert D.decision(live, rowlimit=3) == "continue" and D.decision(np.zeros(256, bool)) == "skip"
