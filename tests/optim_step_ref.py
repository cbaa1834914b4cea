"""float64 restatement of the training step behind the backward (pipeline.py:815-836), the reference of
tests/test_optim_step_model.py (which pins it to torch's own objects in float64) and tests/test_gpu_optim_step.py.

bce():        BCEWithLogitsLoss(pos_weight), mean reduction, the gradient of scale * loss for the logits, the accuracy count.
optim_step(): per group GradScaler.unscale_, clip_grad_norm_, GradScaler.step over torch.optim.Adam (weight decay added to the
              gradient), then GradScaler.update.  A group is a list of tensor indices; a tensor whose gradient is None takes no
              part; a group none of whose tensors has a gradient does nothing (norm 0, step count unchanged).
Everything is numpy float64 and nothing is modified in place.
"""
import numpy as np


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce(x, y, pos_weight=1.0, scale=1.0):
    """-> (mean loss, d (scale * loss) / dx, correct count)."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    w = 1.0 + (float(pos_weight) - 1.0) * y
    l = (1.0 - y) * x + w * (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0))
    d = (float(scale) / x.size) * ((1.0 - y) - w * sigmoid(-x))
    return float(l.sum() / x.size), d, int(((x > 0) == (y == 1)).sum())


def scale_update(scale, tracker, found_any, growth=2.0, backoff=0.5, interval=2000):
    """GradScaler.update -> (scale, growth_tracker)."""
    if found_any:
        return scale * backoff, 0
    if tracker + 1 == interval:
        return scale * growth, 0
    return scale, tracker + 1


def optim_step(p, g, m, v, group_of, steps, hyper, scale=None, tracker=0, growth=2.0, backoff=0.5, interval=2000):
    """p, g, m, v: lists of arrays (g[i] None: no gradient); group_of[i]: the group of tensor i; steps: Adam's t per group;
    hyper: per group a dict lr, beta1, beta2, eps, weight_decay, max_norm (<= 0: no clipping).  scale None: no loss scale and
    no skipping.  Returns a dict: p, g (what is left in .grad; None where a group was skipped), m, v, steps, norms, found,
    coef, skipped, scale, tracker."""
    f64 = lambda a: None if a is None else np.array(a, np.float64)
    p, g, m, v = [f64(a) for a in p], [f64(a) for a in g], [f64(a) for a in m], [f64(a) for a in v]
    steps = list(steps)
    inv = 1.0 if scale is None else 1.0 / float(scale)
    norms, found, coefs, skipped = [], [], [], []
    with np.errstate(all="ignore"):
        for gi, h in enumerate(hyper):
            live = [i for i in range(len(p)) if group_of[i] == gi and g[i] is not None and g[i].size > 0]
            norm = float(np.sqrt(sum(float(((g[i] * inv) ** 2).sum()) for i in live)))
            bad = any(not np.isfinite(g[i]).all() for i in live)
            coef = 1.0
            if h["max_norm"] > 0:
                coef = h["max_norm"] / (norm + 1e-6)
                if coef > 1.0:                       # a NaN stays a NaN, as torch.clamp(max=1) leaves it
                    coef = 1.0
            skip = not live or (scale is not None and bad)
            norms.append(norm), found.append(int(bad)), coefs.append(coef), skipped.append(bool(skip))
            if skip:
                for i in live:
                    g[i] = None
                continue
            steps[gi] += 1
            t = steps[gi]
            b1, b2 = h["beta1"], h["beta2"]
            for i in live:
                g[i] = g[i] * inv * coef
                gd = g[i] + h["weight_decay"] * p[i]
                m[i] = b1 * m[i] + (1.0 - b1) * gd
                v[i] = b2 * v[i] + (1.0 - b2) * gd * gd
                p[i] = p[i] - (h["lr"] / (1.0 - b1 ** t)) * m[i] / (np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t) + h["eps"])
    out = dict(p=p, g=g, m=m, v=v, steps=steps, norms=norms, found=found, coef=coefs, skipped=skipped, scale=scale, tracker=tracker)
    if scale is not None:
        out["scale"], out["tracker"] = scale_update(float(scale), int(tracker), any(found), growth, backoff, interval)
    return out
