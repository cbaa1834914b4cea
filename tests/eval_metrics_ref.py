"""float64 numpy model of csrc/eval_metrics.inc, written from the formulas in include/radad_hip.h: sort the scores, count the
positives and negatives in front of each distinct score, evaluate a formula at each distinct score, reduce.

Candidates of a score set, in order: -inf, each distinct score ascending, +inf.  At candidate t
    fnr = #{positives with score < t} / P        fpr = #{negatives with score >= t} / N
-0.0 and +0.0 are one score.  tests/test_eval_metrics_model.py pins this model to the reference's own outputs
(tests/golden/eval_metrics.npz); tests/test_gpu_eval_metrics.py bounds the kernels against it.
"""
import math

import numpy as np

ASV_KEYS = ("P_miss_asv", "P_fa_asv", "P_fa_spoof_asv", "C_miss_asv", "C_fa_asv", "C_miss_cm", "C_fa_cm", "pi_tar", "pi_non",
            "pi_spoof")
ASV_2019 = dict(P_miss_asv=0.0476, P_fa_asv=0.0248, P_fa_spoof_asv=0.3012, C_miss_asv=1.0, C_fa_asv=10.0, C_miss_cm=1.0,
                C_fa_cm=10.0, pi_tar=0.9405, pi_non=0.0095, pi_spoof=0.05)


def _f64(scores):
    return np.asarray(scores, dtype=np.float64) + 0.0          # -0.0 + 0.0 is +0.0


def counts(scores, labels):
    """(u, pos_below, neg_below, P, N): the distinct scores ascending and, per distinct score, how many positives / negatives lie
    strictly below it."""
    s, y = _f64(scores), np.asarray(labels).astype(np.int64)
    u, inv = np.unique(s, return_inverse=True)
    pos_at = np.bincount(inv, weights=(y == 1), minlength=len(u)).astype(np.int64)
    neg_at = np.bincount(inv, weights=(y != 1), minlength=len(u)).astype(np.int64)
    pos_below = np.cumsum(pos_at) - pos_at
    neg_below = np.cumsum(neg_at) - neg_at
    return u, pos_below, neg_below, int(pos_at.sum()), int(neg_at.sum())


def rates(scores, labels, c=None):
    """(thresholds, fnr, fpr) over all candidates, or None with one class only.  c: counts(scores, labels) where the caller has them."""
    u, pb, nb, P, N = c or counts(scores, labels)
    if P == 0 or N == 0:
        return None
    thr = np.concatenate([[-np.inf], u, [np.inf]])
    miss = np.concatenate([[0], pb, [P]])
    below = np.concatenate([[0], nb, [N]])
    return thr, miss / P, (N - below) / N


def eer(scores, labels, c=None):
    """(EER in percent, threshold): the first candidate with the least |fnr - fpr|; (nan, nan) with one class only."""
    r = rates(scores, labels, c)
    if r is None:
        return float("nan"), float("nan")
    thr, fnr, fpr = r
    k = int(np.argmin(np.abs(fnr - fpr)))
    return float((fnr[k] + fpr[k]) / 2.0 * 100.0), float(thr[k])


def group_eers(scores, labels, groups):
    """{group id: EER} over the groups that hold both classes, ascending id."""
    s, y, g = np.asarray(scores), np.asarray(labels), np.asarray(groups)
    order = np.argsort(g, kind="stable")
    s, y, g = s[order], y[order], g[order]
    cuts = np.flatnonzero(np.diff(g)) + 1
    out = {}
    for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(g)]])):
        pos = int((y[lo:hi] == 1).sum())
        if 0 < pos < hi - lo:
            out[g[lo].item()] = eer(s[lo:hi], y[lo:hi])[0]
    return out


def macro_eer(scores, labels, groups):
    """(mean of the groups' EERs, number of groups that contributed); (nan, 0) if none did."""
    e = group_eers(scores, labels, groups)
    if not e:
        return float("nan"), 0
    return math.fsum(e.values()) / len(e), len(e)


def tdcf_consts(asv):
    """(c0, c1, c2, P_fa_spoof_asv, C_def) as Python floats in left-to-right order, or None (no parameters, C_def <= 0)."""
    if asv is None:
        return None
    a = {k: float(asv[k]) for k in ASV_KEYS}
    c_def = min(a["C_miss_asv"] * a["pi_tar"], a["C_fa_asv"] * a["pi_non"])
    if not c_def > 0:
        return None
    return (a["C_miss_asv"] * a["pi_tar"] * a["P_miss_asv"] + a["C_fa_asv"] * a["pi_non"] * a["P_fa_asv"],
            a["C_fa_cm"] * a["pi_spoof"], a["C_miss_cm"] * a["pi_tar"], a["P_fa_spoof_asv"], c_def)


def tdcf_curve(scores, labels, asv, c=None):
    """(thresholds, tdcf) over all candidates, or None."""
    k = tdcf_consts(asv)
    r = rates(scores, labels, c)
    if k is None or r is None:
        return None
    c0, c1, c2, pfa, c_def = k
    thr, pmiss, _ = r
    return thr, (c0 + c1 * (1.0 - pmiss) * pfa + c2 * pmiss) / c_def


def min_tdcf(scores, labels, asv, c=None):
    t = tdcf_curve(scores, labels, asv, c)
    if t is None:
        return float("nan"), float("nan")
    k = int(np.argmin(t[1]))
    return float(t[1][k]), float(t[0][k])


def auc_parts(scores, labels, c=None):
    """(numerator, 2 P N) as Python ints: sum over distinct scores descending of (fp_i - fp_{i-1}) (tp_i + tp_{i-1}), counts taken
    at the end of each run of equal scores."""
    u, pb, nb, P, N = c or counts(scores, labels)
    tp = np.concatenate([[0], (P - pb)[::-1]])            # positives with score >= u, descending u, behind the origin
    fp = np.concatenate([[0], (N - nb)[::-1]])
    num = sum(int(a) * int(b) for a, b in zip(np.diff(fp), tp[1:] + tp[:-1]))
    return num, 2 * P * N


def auc(scores, labels, c=None):
    num, den = auc_parts(scores, labels, c)
    return 0.5 if den == 0 else num / den


def auc_brute(scores, labels):
    """(#{pos > neg} + #{pos == neg} / 2) / (P N), pair by pair."""
    s, y = _f64(scores), np.asarray(labels)
    pos, neg = s[y == 1], s[y != 1]
    if len(pos) == 0 or len(neg) == 0:
        return 0.5
    gt = int((pos[:, None] > neg[None, :]).sum())
    eq = int((pos[:, None] == neg[None, :]).sum())
    return (2 * gt + eq) / (2 * len(pos) * len(neg))


def roc(scores, labels, c=None):
    """(fpr, tpr, thresholds): (0, 0, max + 1e-6), one point per distinct score descending with the counts at the end of its run,
    (1, 1, min - 1e-6); the two fixed points with one class only."""
    u, pb, nb, P, N = c or counts(scores, labels)
    if P == 0 or N == 0:
        return np.array([0.0, 1.0]), np.array([0.0, 1.0]), np.array([np.inf, -np.inf])
    d = u[::-1]
    tpr = np.concatenate([[0.0], (P - pb)[::-1] / P, [1.0]])
    fpr = np.concatenate([[0.0], (N - nb)[::-1] / N, [1.0]])
    return fpr, tpr, np.concatenate([[d[0] + 1e-6], d, [d[-1] - 1e-6]])


def bce_terms(x, y, pos_weight):
    """Per-sample BCEWithLogitsLoss(pos_weight) terms in float64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = 1.0 + (float(pos_weight) - 1.0) * y
    return (1.0 - y) * x + w * (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0))


def loss_acc(x, y, pos_weight):
    """(mean loss, correct count): the loss summed exactly (math.fsum) over float64 terms."""
    x32, y = np.asarray(x, dtype=np.float32), np.asarray(y)
    return math.fsum(bce_terms(x32, y, pos_weight)) / len(x32), int(((x32 > 0) == (y == 1)).sum())


def everything(scores, labels, groups=None, asv=None, pos_weight=1.0):
    """What HipEvalMetrics.compute() returns, from the model."""
    e, et = eer(scores, labels)
    if groups is None:
        groups = np.zeros(len(scores), dtype=np.int32)
    me, G = macro_eer(scores, labels, groups)
    td, tt = min_tdcf(scores, labels, asv)
    loss, correct = loss_acc(scores, labels, pos_weight)
    return {"loss": loss, "correct": correct, "n": len(scores), "auc": auc(scores, labels), "eer_percent": e, "eer_threshold": et,
            "macro_eer_percent": me, "groups_scored": G, "min_tDCF": td, "min_tDCF_threshold": tt}
