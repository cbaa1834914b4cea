"""CPU: the early-abandon bound of the tile scan holds in fp32 (tests/abandon_ref.py): for f16 operand pairs, the fp32-accumulated
full score is <= the partial score at the checkpoint + the bound, whichever order either accumulation takes -- sequential, pairwise,
32-element blocks forward or backward.  Where the remaining elements are parallel (Cauchy-Schwarz tight) the bound must also be
TIGHT: within the inflations and the slack of the true score, or the test would be vacuous."""
import numpy as np
import pytest

import abandon_ref as A

DIMS = (128, 512, 5376)
PAIRS = 24


def _f16(x):
    return np.clip(x, -65504.0, 65504.0).astype(np.float16)


def _cases(dim, rng):
    e0 = 64 * A.checkpoint(dim)
    g = lambda: rng.standard_normal((PAIRS, dim))
    out = {}
    out["random"] = (_f16(g() * 4000.0), _f16(g() * 4000.0))
    q, y = g() * 3000.0, g() * 3000.0
    tail = np.round(rng.standard_normal((PAIRS, dim - e0)) * 200.0)       # small integers: 2 x them is exact in f16
    q[:, e0:], y[:, e0:] = tail, 2.0 * tail
    out["parallel_tail"] = (_f16(q), _f16(y))
    q, y = g() * 4000.0, g() * 4000.0
    q[:, e0:] = 0.0
    out["energy_before"] = (_f16(q), _f16(y))
    q, y = g() * 4000.0, g() * 4000.0
    q[:, :e0], y[:, :e0] = 0.0, 0.0
    out["energy_after"] = (_f16(q), _f16(y))
    out["saturated"] = (_f16(np.full((PAIRS, dim), 65504.0)), _f16(np.where(rng.random((PAIRS, dim)) < 0.5, -65504.0, 65504.0)))
    out["saturated_aligned"] = (_f16(np.full((PAIRS, dim), 65504.0)), _f16(np.full((PAIRS, dim), 65504.0)))
    out["zeros"] = (_f16(np.zeros((PAIRS, dim))), _f16(g() * 4000.0))
    return out, e0


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("bias", [False, True])
def test_full_score_never_exceeds_partial_plus_bound(dim, bias):
    rng = np.random.default_rng(dim + bias)
    cases, e0 = _cases(dim, rng)
    assert 0 < e0 < dim
    for name, (qh, yh) in cases.items():
        # an fp32 bias start of the accumulator's magnitude (RSC 3: |y|^2 / 2 or mu.y in accumulator units), either sign
        c0 = (rng.standard_normal(PAIRS) * 0.5 * A.norm_f32(qh) * A.norm_f32(yh)).astype(np.float32) if bias else np.zeros(PAIRS, np.float32)
        partial = {o: f(qh, yh, c0, 0, e0) for o, f in A.ORDERS.items()}
        full = {o: f(qh, yh, c0, 0, dim) for o, f in A.ORDERS.items()}
        # the kernel's own full score continues ITS partial sum: sequential over the rest on top of each partial
        for o, p in partial.items():
            full["continued_" + o] = A.acc_sequential(qh, yh, p, e0, dim)
        for po, p in partial.items():
            b = A.bound(p, qh, yh, c0, e0)
            assert np.isfinite(b).all(), (name, po)
            for fo, f in full.items():
                assert (f <= b).all(), f"{name}: full ({fo}) exceeds partial ({po}) + bound at dim {dim}: {np.max(f - b)}"


@pytest.mark.parametrize("dim", DIMS)
def test_bound_is_tight_where_cauchy_schwarz_is(dim):
    rng = np.random.default_rng(7 * dim)
    cases, e0 = _cases(dim, rng)
    qh, yh = cases["parallel_tail"]
    c0 = np.zeros(PAIRS, np.float32)
    p = A.acc_sequential(qh, yh, c0, 0, e0)
    b = A.bound(p, qh, yh, c0, e0).astype(np.float64)
    exact = (qh.astype(np.float64) * yh.astype(np.float64)).sum(axis=1)
    scale = A.norm_f32(qh).astype(np.float64) * A.norm_f32(yh)
    # three inflations of 2^-10 on the suffix product, two on the slack's norms, the slack itself and the partial sum's own error
    assert ((b - exact) <= scale * (4 * 2.0 ** -10 + 3 * dim * 2.0 ** -23)).all()
    assert (b >= exact).all()


def test_checkpoints():
    assert [A.checkpoint(d) for d in (64, 124, 128, 192, 512, 1024, 5376, 16320)] == [0, 0, 1, 1, 1, 2, 10, 31]
