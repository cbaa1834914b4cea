"""CPU checks of the host model of a store's contents (oracle.radad_oracle.stored_rows / stored_rows_err): against the reference's
own recorded output, against an fp32 evaluation in the kernels' order of operations, and on hand-made fp16 rounding cases.
tests/test_gpu_store_contents.py compares the device with this model."""
import os

import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth

DIMS = [4, 12, 64, 100, 252, 256, 260, 512, 1024, 5376]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "pipeline.npz"))


def _ratio(got, exact, bound):
    """worst |got - exact| / bound (0 / 0 counts as 0: the regimes with bound 0 must be met exactly)"""
    err = np.abs(np.asarray(got, np.float64) - exact)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))))


def test_model_reproduces_the_reference_rows_within_its_bound(g):
    rows = g["k7_rows"]
    exact, bound = O.stored_rows_err(rows)
    assert O.cosine_sum_depth(rows.shape[1]) == 11
    for name in ("k7_norm_1", "shell_1_added"):                       # the reference's fp32 _maybe_normalize, and what reached index.add
        r = _ratio(g[name], exact, bound)
        assert r <= 1.0, f"{name}: error / bound = {r:.3f}"
    # not vacuous: the bound is a few ulp, and rows off by one part in 1e6 are outside it
    assert np.all(bound <= 9.5 * 2.0 ** -24 * np.abs(exact))
    assert _ratio(g["k7_norm_1"] * np.float32(1 + 1e-6), exact, bound) > 1.0
    # L2 / IP: the input itself
    for metric in ("L2", "IP"):
        assert O.stored_rows(rows, metric).tobytes() == rows.tobytes()
    np.testing.assert_array_equal(g["k7_norm_0"], O.stored_rows(rows, "L2"))
    assert O.stored_rows(rows, "COSINE").dtype == np.float32 and O.stored_rows(rows, "COSINE", f16=True).dtype == np.float16


@pytest.mark.parametrize("dim", DIMS)
def test_kernel_order_in_fp32_stays_inside_the_bound(dim):
    worst = 0.0
    for j, mag in enumerate([1e-6, 1e-3, 1.0, 37.0, 1e5]):
        rows = synth.rows(0, 64, dim, 7100 + j) * np.float32(mag)
        rows[1] = np.abs(rows[1])                                      # all of one sign
        rows[2, 1:] *= np.float32(1e-3)                                # one dominant element
        exact, bound = O.stored_rows_err(rows)
        assert np.all((bound > 0) == (rows != 0))
        worst = max(worst, _ratio(O.rownorm_kernel_order_f32(rows), exact, bound))
    print(f"dim {dim}: worst error / bound {worst:.3f} (d = {O.cosine_sum_depth(dim)})")
    assert worst <= 1.0, f"dim {dim}: fp32 evaluation in kernel order leaves the bound, error / bound = {worst:.3f}"
    assert worst > 0.01, "the bound is orders of magnitude above the error it is meant to bound"


def test_summation_depth():
    assert [O.cosine_sum_depth(d) for d in (4, 256, 260, 512, 1024, 5376)] == [11, 11, 12, 12, 14, 31]


def test_fp16_store_model_rounds_to_nearest_even():
    f = np.float32
    sub_max = f(1023 * 2.0 ** -24)                                     # largest fp16 subnormal
    x = np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65520.0, -65520.0, 65519.996, 65504.0,
                   sub_max, sub_max + 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(1 + 2.0 ** -11)]], np.float32)
    want = np.array([[1.0, 1 + 2.0 ** -9, np.inf, -np.inf, 65504.0, 65504.0,
                      sub_max, 2.0 ** -14, 2.0 ** -24, 0.0, 2.0 ** -23, -1.0]], np.float64)
    for metric in ("L2", "IP"):
        h = O.stored_rows(x, metric, f16=True)
        assert h.dtype == np.float16
        np.testing.assert_array_equal(h.astype(np.float64), want)
    assert O.stored_rows(x, "L2", f16=True)[0, 6].view(np.uint16) == 0x03FF
    # truncation would give another answer on the second and on the subnormal tie cases: the cases tell the two apart
    trunc = (x.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    assert trunc[0, 1] != want[0, 1]


def test_cosine_special_rows():
    dim = 64
    rows = np.zeros((4, dim), np.float32)
    rows[1] = np.float32(2.0 ** 70) * (1 + np.arange(dim) % 3)         # squares overflow float32: norm inf -> zeros
    rows[2] = np.float32(2.0 ** -60)                                   # squares are normal float32 numbers: the 1e-12 dominates
    rows[3] = synth.rows(0, 1, dim, 5)[0]
    exact, bound = O.stored_rows_err(rows)
    assert np.all(exact[0] == 0) and np.all(bound[0] == 0)
    assert np.all(exact[1] == 0) and np.all(bound[1] == 0)
    with np.errstate(over="ignore"):
        ref = rows / (np.linalg.norm(rows, axis=1, keepdims=True) + 1e-12)      # the reference's formula on a float32 array
    assert ref.dtype == np.float32
    np.testing.assert_array_equal(ref[:2], 0)
    want = 2.0 ** -60 / (8 * 2.0 ** -60 + O.COS_EPS32)
    np.testing.assert_allclose(exact[2], want, rtol=1e-15)
    assert 8e-7 < want < 9e-7 and np.all(bound[2] > 0)
    assert _ratio(ref[2:], exact[2:], bound[2:]) <= 1.0
    assert _ratio(O.rownorm_kernel_order_f32(rows), exact, bound) <= 1.0
    # fp16 cosine store: one further rounding of the fp32 value
    h = O.stored_rows(rows, "COSINE", f16=True)
    np.testing.assert_array_equal(h, O.stored_rows(rows, "COSINE").astype(np.float16))
    # scaling a row by a power of two does not change the model beyond the 1e-12
    a = O.stored_rows_err(rows[3:] * np.float32(2.0 ** 40))[0]
    np.testing.assert_allclose(a, exact[3:], rtol=1e-12)
