"""Generate tests/golden/eval_metrics.npz by RUNNING the reference's own metric code: DeepfakeDetectionPipeline._compute_eer,
_compute_macro_eer_by_group, _compute_min_tDCF, _roc_curve and _auc (pipeline.py:152-234, 277-326), imported the way
make_golden.py imports the reference.  Only DATA is written: the inputs (float32 scores, labels, group ids) and the outputs.

    python tests/golden/make_golden_eval.py

Cases (n <= 600): tie-free, heavily tied, signed zeros, nearly separable, separable, one class only (both ways), one sample
per group, a giant group beside many small ones; each with the ASVspoof-2019-like parameters of tests/eval_metrics_ref.py, plus
the two parameter sets for which the reference returns NaN.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))


def cases():
    rng = np.random.default_rng(20261)
    c = {}

    def put(name, s, y, g=None):
        s = np.asarray(s, dtype=np.float32)
        y = np.asarray(y, dtype=np.int32)
        g = np.zeros(len(s), dtype=np.int32) if g is None else np.asarray(g, dtype=np.int32)
        c[name] = (s, y, g)

    y = (rng.random(600) < 0.4).astype(np.int32)
    s = (rng.standard_normal(600) + 1.2 * y).astype(np.float32)
    assert len(np.unique(s)) == 600
    put("tie_free", s, y, rng.integers(0, 20, 600))
    y = (rng.random(500) < 0.5).astype(np.int32)
    put("tied", np.clip(np.rint(rng.standard_normal(500) * 1.5 + y), -3, 3), y, rng.integers(0, 7, 500))
    y = (rng.random(200) < 0.5).astype(np.int32)
    put("signed_zero", rng.choice(np.array([-1.0, -0.0, 0.0, 0.5, 1.0], dtype=np.float32), 200), y, rng.integers(0, 3, 200))
    y = (rng.random(300) < 0.3).astype(np.int32)
    s = np.where(y == 1, 2.0 + rng.random(300), -2.0 - rng.random(300))
    put("separable", s, y)
    y2 = y.copy()
    y2[[5, 77, 201]] ^= 1
    put("nearly_separable", s, y2, rng.integers(0, 4, 300))
    put("all_positive", rng.standard_normal(50), np.ones(50))
    put("all_negative", rng.standard_normal(50), np.zeros(50))
    put("one_per_group", rng.standard_normal(60), rng.random(60) < 0.5, np.arange(60))
    n = 600
    g = np.zeros(n, dtype=np.int32)
    g[300:] = 1 + np.arange(300) // 2 + (rng.random(300) < 0.3)          # groups of 1-3 beside one of 300
    y = (rng.random(n) < 0.5).astype(np.int32)
    put("giant_and_small", rng.standard_normal(n) + y, y, g)
    put("one_sample", [0.25], [1])
    return c


def main():
    from make_golden import import_reference
    import_reference()
    import pipeline as ref_pipeline
    import eval_metrics_ref as M
    P = ref_pipeline.DeepfakeDetectionPipeline
    out = {"names": np.array(sorted(cases()))}
    for name, (s32, y, g) in cases().items():
        s = s32.astype(np.float64)                           # evaluate_with_scores returns float64 of the float32 logits
        out[f"{name}/scores"], out[f"{name}/labels"], out[f"{name}/groups"] = s32, y, g
        out[f"{name}/eer"] = np.array(P._compute_eer(s, y))
        names = [f"spk{v:05d}" for v in g]                   # zero-padded: name order is id order
        out[f"{name}/macro_eer"] = np.array(P._compute_macro_eer_by_group(s, y, names))
        ids, eers = [], []
        for v in np.unique(g):
            m = g == v
            if (y[m] == 1).any() and (y[m] == 0).any():
                ids.append(v)
                eers.append(P._compute_eer(s[m], y[m])[0])
        out[f"{name}/group_ids"], out[f"{name}/group_eers"] = np.array(ids, dtype=np.int32), np.array(eers, dtype=np.float64)
        out[f"{name}/tdcf"] = np.array(P._compute_min_tDCF(s, y, dict(M.ASV_2019)))
        out[f"{name}/tdcf_none"] = np.array(P._compute_min_tDCF(s, y, None))
        out[f"{name}/tdcf_cdef0"] = np.array(P._compute_min_tDCF(s, y, dict(M.ASV_2019, pi_non=0.0)))
        fpr, tpr, thr = P._roc_curve(s, y)
        out[f"{name}/roc_fpr"], out[f"{name}/roc_tpr"], out[f"{name}/roc_thr"] = (np.asarray(fpr, dtype=np.float64),
                                                                                   np.asarray(tpr, dtype=np.float64),
                                                                                   np.asarray(thr, dtype=np.float64))
        out[f"{name}/auc"] = np.array(P._auc(np.asarray(fpr, dtype=np.float64), np.asarray(tpr, dtype=np.float64)))
    np.savez_compressed(os.path.join(OUT, "eval_metrics.npz"), **out)
    print("wrote eval_metrics.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
