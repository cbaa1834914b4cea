"""numpy model of the per-row rule of the deferring tile scan (csrc/knn_hi.inc, DEFER; csrc/knn_plan.h, knn_abandon_defer), on top of
tests/abandon_ref.py.

A wave that vetoes its tile at the checkpoint says which rows are LIVE: row i is live iff for some query j the abandon's own comparison

    acc_c[i, j] + fmaf(RQ_j, RY (1 + 2^-10), slack_j)  <  at_j

is NOT true -- the same terms as the tile-level test, RY tile-wide (the largest suffix norm of the tile's rows), slack_j over the tile's
largest row, so a NaN anywhere keeps the row live.  A tile with 1 ... KNN_DEFER_MAX_ROWS live rows hands them to the tail and is left;
that is sound iff every row with a pair whose fp32-accumulated FULL score reaches at_j -- whatever order the accumulation takes -- is
live.  Everything in float32 the way the device computes it."""
import numpy as np

import abandon_ref as A

F = np.float32
MAX_ROWS = 16          # KNN_DEFER_MAX_ROWS


def pairs(qh, yh):
    """all (row, query) pairs of a tile as abandon_ref's pair lists: -> (qh [R Q, dim], yh [R Q, dim]), pair r Q + j = (row r, query j)"""
    r, q = yh.shape[0], qh.shape[0]
    return np.tile(qh, (r, 1)), np.repeat(yh, q, axis=0)


def tile_terms(qh, yh, c0, e0):
    """the terms of the comparison: RQ [Q], the tile-wide RY (1 + 2^-10), slack [Q] over the tile's largest row and start value"""
    dim = qh.shape[1]
    rq = A.norm_f32(qh[:, e0:])
    ry = F(np.max(A.norm_f32(yh[:, e0:]))) * A.INFL
    ymax, cmax = F(np.max(A.norm_f32(yh))), F(np.max(np.abs(c0))) if len(c0) else F(0)
    sl = (F(2.0) * F(dim) * F(2.0 ** -23) * (A.norm_f32(qh) * ymax + cmax) * A.INFL).astype(F)
    return rq, ry, sl


def live_rows(acc_c, rq, ry, sl, at):
    """acc_c [R, Q] partial sums at the checkpoint, at [Q] the epilogue's thresholds -> bool [R]: the rows the kernel lists"""
    t = (rq.astype(np.float64) * np.float64(ry) + sl).astype(F)           # fmaf: one rounding
    with np.errstate(invalid="ignore"):
        ok = (acc_c + t[None, :]).astype(F) < at[None, :].astype(F)       # a NaN compares false: live
    return ~ok.all(axis=1)


def decision(live, rowlimit=None):
    """-> "skip" (no wave vetoes: no row is live), "defer" (1 ... MAX_ROWS live rows below rowlimit) or "continue" """
    n = int(live[:rowlimit].sum())
    if not live.any():
        return "skip"
    return "defer" if 1 <= n <= MAX_ROWS else "continue"
