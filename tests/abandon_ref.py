"""numpy model of the tile scan's early-abandon bound (csrc/knn_hi.inc, "EARLY ABANDON"; csrc/knn_plan.h).

Operands are raw f16 values (the accumulators' units).  After the first e0 = 64 c elements of a dot product the kernel holds the fp32
partial sum acc_c (bias start included) and abandons when, for every pair of the tile,

    acc_c + RQ RY (1 + 2^-10) + slack  <  threshold,       RQ = |qh[e0:]|, RY = |yh[e0:]| (fp32 sums of squares, each inflated by 2^-10),
                                                           slack = 2 dim 2^-23 (|qh| |yh| + |c0|)

which is sound iff the fp32-accumulated FULL score -- whatever order the accumulation takes -- never exceeds the left-hand side.
Everything here is computed in float32 the way the device does it (products of two f16 values are exact in fp32)."""
import numpy as np

F = np.float32
INFL = F(1.0) + F(2.0 ** -10)


def checkpoint(dim):
    """knn_abandon_checkpoint: K stages of 64 elements multiplied before the test (0: never)"""
    if dim < 128 or dim % 64:
        return 0
    return max(1, dim // 64 // 8)


def norm_f32(xh):
    """|xh| per row as hi_rows_body forms it: fp32 fma chain over the squares, square root, inflated"""
    x = xh.astype(F)
    s = np.zeros(x.shape[0], F)
    for j in range(x.shape[1]):
        s = (x[:, j].astype(np.float64) * x[:, j] + s).astype(F)          # fmaf: one rounding
    return np.sqrt(s).astype(F) * INFL


def slack(dim, qh, yh, c0):
    return (F(2.0) * F(dim) * F(2.0 ** -23) * (norm_f32(qh) * norm_f32(yh) + np.abs(c0).astype(F)) * INFL).astype(F)


def bound(acc_c, qh, yh, c0, e0):
    """the left-hand side of the kernel's test, in its arithmetic: acc_c + fmaf(RQ, RY (1 + 2^-10), slack)"""
    dim = qh.shape[1]
    rq, ry = norm_f32(qh[:, e0:]), (norm_f32(yh[:, e0:]) * INFL).astype(F)
    t = (rq.astype(np.float64) * ry + slack(dim, qh, yh, c0)).astype(F)
    return (acc_c + t).astype(F)


def _prod(qh, yh):
    return qh.astype(F) * yh.astype(F)          # exact: 11-bit x 11-bit significands


def acc_sequential(qh, yh, c0, lo, hi):
    p, s = _prod(qh, yh), c0.astype(F).copy()
    for j in range(lo, hi):
        s = (s + p[:, j]).astype(F)
    return s


def _pair(p):
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), F)], axis=1)
        p = (p[:, 0::2] + p[:, 1::2]).astype(F)
    return p[:, 0]


def acc_pairwise(qh, yh, c0, lo, hi):
    return (c0.astype(F) + _pair(_prod(qh, yh)[:, lo:hi])).astype(F)


def _blocks(qh, yh, lo, hi):
    p = _prod(qh, yh)[:, lo:hi]
    return [_pair(p[:, b:b + 32]) for b in range(0, hi - lo, 32)]


def acc_blocks_forward(qh, yh, c0, lo, hi):
    s = c0.astype(F).copy()
    for b in _blocks(qh, yh, lo, hi):
        s = (s + b).astype(F)
    return s


def acc_blocks_reverse(qh, yh, c0, lo, hi):
    s = c0.astype(F).copy()
    for b in reversed(_blocks(qh, yh, lo, hi)):
        s = (s + b).astype(F)
    return s


ORDERS = {"sequential": acc_sequential, "pairwise": acc_pairwise, "blocks_forward": acc_blocks_forward, "blocks_reverse": acc_blocks_reverse}
