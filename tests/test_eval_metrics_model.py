"""No GPU: tests/eval_metrics_ref.py against the reference's own outputs (tests/golden/eval_metrics.npz, written by
tests/golden/make_golden_eval.py from DeepfakeDetectionPipeline's five static metric methods), every refusal of the evaluation
ABI (radad_eval_append, radad_eval_metrics, radad_eval_metrics_workspace_bytes) with made-up pointers, every argument error of
HipEvalMetrics, and the host-only plan (csrc/eval_plan.h) through tests/eval_plan_check.cpp.

eval_metrics_ref is what tests/test_gpu_eval_metrics.py bounds the kernels against.  EER, its threshold, the per-group EERs and
the t-DCF pair must equal the golden bit for bit.  On tie-free cases the ROC points are equal and the AUC is within n 2^-52 of
the reference's trapezoid; on tied cases the reference's AUC depends on an unspecified order inside each tie (include/radad_hip.h),
so the model's exact-integer AUC is held against the O(P N) pair count instead.
Every test here fails without the feature: the symbols, the ctypes struct and the modules do not exist.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import eval_metrics_ref as M
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import eval_step as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
NAMES = [str(n) for n in G["names"]]
TIE_FREE = ["tie_free", "separable", "nearly_separable", "one_per_group", "giant_and_small"]
TIED = ["tied", "signed_zero"]


def same(a, b):
    """Equality of float64 arrays element for element, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def case(name):
    return G[f"{name}/scores"], G[f"{name}/labels"], G[f"{name}/groups"]


def test_the_golden_covers_the_cases():
    assert set(TIE_FREE + TIED + ["all_positive", "all_negative", "one_sample"]) == set(NAMES)
    for name in NAMES:
        s, y, g = case(name)
        assert s.dtype == np.float32 and len(s) == len(y) == len(g) <= 600
        distinct = len(np.unique(s.astype(np.float64) + 0.0))
        assert (distinct == len(s)) == (name not in TIED), name
    s, _, _ = case("signed_zero")
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    assert len(np.unique(case("one_per_group")[2])) == 60
    g = case("giant_and_small")[2]
    assert np.bincount(g).max() == 300 and (np.bincount(g) <= 3).sum() > 100


@pytest.mark.parametrize("name", NAMES)
def test_eer_and_tdcf_equal_the_reference_bit_for_bit(name):
    s, y, g = case(name)
    assert same(M.eer(s, y), G[f"{name}/eer"]), (M.eer(s, y), G[f"{name}/eer"])
    assert same(M.min_tdcf(s, y, M.ASV_2019), G[f"{name}/tdcf"]), (M.min_tdcf(s, y, M.ASV_2019), G[f"{name}/tdcf"])
    assert same(M.min_tdcf(s, y, None), G[f"{name}/tdcf_none"]) and np.isnan(G[f"{name}/tdcf_none"]).all()
    assert same(M.min_tdcf(s, y, dict(M.ASV_2019, pi_non=0.0)), G[f"{name}/tdcf_cdef0"]) and np.isnan(G[f"{name}/tdcf_cdef0"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_group_eers_equal_the_reference_and_the_mean_is_close(name):
    s, y, g = case(name)
    mine = M.group_eers(s, y, g)
    assert list(mine) == list(G[f"{name}/group_ids"])
    assert same(list(mine.values()), G[f"{name}/group_eers"])
    mean, count = M.macro_eer(s, y, g)
    want = float(G[f"{name}/macro_eer"])
    if count == 0:
        assert np.isnan(mean) and np.isnan(want)
    else:
        assert abs(mean - want) <= count * 2.0 ** -52 * abs(want)


@pytest.mark.parametrize("name", TIE_FREE)
def test_tie_free_roc_points_equal_and_auc_close(name):
    s, y, _ = case(name)
    fpr, tpr, thr = M.roc(s, y)
    assert same(fpr, G[f"{name}/roc_fpr"]) and same(tpr, G[f"{name}/roc_tpr"]) and same(thr, G[f"{name}/roc_thr"])
    assert abs(M.auc(s, y) - float(G[f"{name}/auc"])) <= len(s) * 2.0 ** -52
    assert M.auc(s, y) == M.auc_brute(s, y)


@pytest.mark.parametrize("name", TIED + ["all_positive", "all_negative", "one_sample"])
def test_tied_and_degenerate_auc_is_the_pair_count(name):
    s, y, _ = case(name)
    assert M.auc(s, y) == M.auc_brute(s, y)
    fpr, tpr, thr = M.roc(s, y)
    assert fpr[0] == tpr[0] == 0.0 and fpr[-1] == tpr[-1] == 1.0 and (np.diff(fpr) >= 0).all() and (np.diff(tpr) >= 0).all()
    assert abs((np.trapezoid if hasattr(np, "trapezoid") else np.trapz)(tpr, fpr) - M.auc(s, y)) <= len(s) * 2.0 ** -52
    if name in TIED:
        assert len(thr) == len(np.unique(s.astype(np.float64) + 0.0)) + 2
    else:                                                    # one class: the reference's two fixed points and its trapezoid
        assert same(fpr, G[f"{name}/roc_fpr"]) and same(thr, G[f"{name}/roc_thr"]) and M.auc(s, y) == 0.5 == float(G[f"{name}/auc"])


def test_signed_zeros_are_one_threshold():
    s = np.array([-0.0, 0.0, -0.0, 0.0, 1.0, -1.0], dtype=np.float32)
    y = np.array([1, 0, 0, 1, 1, 0])
    u, pb, nb, P, N = M.counts(s, y)
    assert list(u) == [-1.0, 0.0, 1.0] and list(pb) == [0, 0, 2] and list(nb) == [0, 1, 3]
    assert M.auc(s, y) == M.auc_brute(s, y) == (2 * (1 + 1 + 3) + 4) / (2 * 9)


def test_bce_model_equals_torch_in_float64():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(200) * 4, [0.0, 100.0, -100.0]]).astype(np.float32)
    y = (rng.random(203) < 0.4).astype(np.float64)
    for pw in (1.0, 3.7):
        loss, correct = M.loss_acc(x, y, pw)
        want = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], dtype=torch.float64))(torch.tensor(x, dtype=torch.float64),
                                                                                               torch.tensor(y))
        assert abs(loss - float(want)) <= 1e-13 * float(want)
        assert correct == int(((torch.tensor(x) > 0).double() == torch.tensor(y)).sum())


# ---- the C ABI's refusals: made-up pointers, refused before any HIP call ---------------------------------------------------
FAKE = 0x1000


def test_eval_workspace_bytes():
    f = _lib.load().radad_eval_metrics_workspace_bytes
    sizes = [f(n, 0) for n in (1, 2047, 2048, 2049, 70001, 1 << 24)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert all(v % 256 == 0 for v in sizes)
    assert f(1 << 24, 1) == 256 + 4 * (1 << 27) + 256 + (1 << 26)
    for bad in (0, -1, (1 << 24) + 1):
        assert f(bad, 0) == -1 and f(bad, 1) == -1


def test_eval_append_argument_errors_without_gpu():
    lib = _lib.load()
    cap = _lib.EVAL_MAX_N

    def call(x=FAKE, y=FAKE, g=None, n=8, pw=1.0, offset=0, keys=FAKE, acc=FAKE):
        return lib.radad_eval_append(x, y, g, n, pw, offset, keys, acc, 0, None)

    for kw, needle in ((dict(n=0), b"at least 1"), (dict(n=-3), b"at least 1"), (dict(offset=-1), b"negative"),
                       (dict(offset=cap - 7), b"above the cap"), (dict(n=cap + 1), b"above the cap"),
                       (dict(offset=cap, n=1), b"above the cap"), (dict(offset=1 << 62, n=1 << 62), b"above the cap"),
                       (dict(pw=0.0), b"pos_weight"), (dict(pw=-2.0), b"pos_weight"), (dict(pw=float("nan")), b"pos_weight"),
                       (dict(x=None), b"NULL buffer"), (dict(y=None), b"NULL buffer"), (dict(keys=None), b"NULL buffer"),
                       (dict(acc=None), b"NULL buffer")):
        assert call(**kw) == _lib.RADAD_EINVAL, kw
        assert needle in lib.radad_last_error(), (kw, lib.radad_last_error())


def test_eval_metrics_argument_errors_without_gpu():
    lib = _lib.load()
    need = lib.radad_eval_metrics_workspace_bytes(5000, 1)

    def call(keys=FAKE, n=5000, groups=1, consts=None, out=FAKE, roc=None, geer=None, ws=FAKE, ws_bytes=1 << 40):
        return lib.radad_eval_metrics(keys, n, groups, consts, out, roc, geer, ws, ws_bytes, 0, None)

    for kw, needle in ((dict(n=0), b"outside 1.."), (dict(n=-1), b"outside 1.."), (dict(n=(1 << 24) + 1), b"outside 1.."),
                       (dict(keys=None), b"NULL buffer"), (dict(out=None), b"NULL buffer"), (dict(ws=None), b"NULL workspace"),
                       (dict(ws=FAKE + 8), b"16-byte"), (dict(ws_bytes=need - 1), b"workspace too small"),
                       (dict(ws_bytes=lib.radad_eval_metrics_workspace_bytes(5000, 0) - 1, groups=0), b"workspace too small")):
        assert call(**kw) == _lib.RADAD_EINVAL, kw
        assert needle in lib.radad_last_error(), (kw, lib.radad_last_error())


# ---- HipEvalMetrics' checks, all in front of the first raw pointer ----------------------------------------------------------
def test_hip_eval_metrics_constructor_errors_without_gpu():
    for pw in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="pos_weight"):
            ES.HipEvalMetrics(pw, "cpu")
    for cap in (0, -4, (1 << 24) + 1):
        with pytest.raises(ValueError, match="capacity"):
            ES.HipEvalMetrics(1.0, "cpu", capacity=cap)
    with pytest.raises(ValueError, match="asv_params lacks"):
        ES.HipEvalMetrics(1.0, "cpu", asv_params={k: 1.0 for k in ES.ASV_KEYS[:-1]})
    with pytest.raises(ValueError, match="no CPU fallback"):
        ES.HipEvalMetrics(1.0, "cpu", asv_params=dict(M.ASV_2019))


def test_tdcf_consts_follow_the_reference():
    assert ES.ASV_KEYS == M.ASV_KEYS
    assert ES.tdcf_consts(None) is None
    assert ES.tdcf_consts(dict(M.ASV_2019, pi_non=0.0)) is None and ES.tdcf_consts(dict(M.ASV_2019, C_miss_asv=-1.0)) is None
    c = ES.tdcf_consts({k: np.float32(v) for k, v in M.ASV_2019.items()})       # float() of whatever the config holds
    want = M.tdcf_consts({k: float(np.float32(v)) for k, v in M.ASV_2019.items()})
    assert (c.c0, c.c1, c.c2, c.p_fa_spoof_asv, c.c_def) == want
    a = M.ASV_2019
    assert want != M.tdcf_consts(a) and M.tdcf_consts(a)[4] == min(a["C_miss_asv"] * a["pi_tar"], a["C_fa_asv"] * a["pi_non"])


def test_add_checks_without_gpu():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    x, y = torch.zeros(4), torch.zeros(4)
    assert ES.check_batch(x, y, None, cpu) == 4
    assert ES.check_batch(x.view(4, 1), y.long(), ["a", "b", "a", "c"], cpu) == 4
    assert ES.check_batch(x, y, torch.arange(4), cpu) == 4
    assert ES.check_batch(x, y, torch.arange(4, dtype=torch.int32).to("meta"), cpu) == 4       # ids may come from anywhere
    with pytest.raises(TypeError, match="float32"):
        ES.check_batch(x.double(), y, None, cpu)
    with pytest.raises(TypeError, match="float32"):
        ES.check_batch([0.0] * 4, y, None, cpu)
    with pytest.raises(TypeError, match="labels"):
        ES.check_batch(x, [0.0] * 4, None, cpu)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ES.check_batch(x, y, None, meta)
    with pytest.raises(ValueError, match="number of"):
        ES.check_batch(x, torch.zeros(5), None, cpu)
    with pytest.raises(ValueError, match="number of"):
        ES.check_batch(torch.zeros(0), torch.zeros(0), None, cpu)
    with pytest.raises(ValueError, match="3 speakers for 4"):
        ES.check_batch(x, y, ["a", "b", "c"], cpu)
    with pytest.raises(ValueError, match="5 speakers for 4"):
        ES.check_batch(x, y, torch.arange(5), cpu)
    with pytest.raises(TypeError, match="int32 or int64"):
        ES.check_batch(x, y, torch.zeros(4), cpu)
    with pytest.raises(TypeError, match="must be str"):
        ES.check_batch(x, y, ["a", 3, "b", "c"], cpu)
    with pytest.raises(TypeError, match="list of str"):
        ES.check_batch(x, y, "abcd", cpu)


def test_the_class_is_exported():
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    assert R.HipEvalMetrics is ES.HipEvalMetrics and "HipEvalMetrics" in R.__all__


# ---- the plan, without a GPU ------------------------------------------------------------------------------------------------
def test_eval_plan_check_program():
    """tests/eval_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where the machine has them."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "eval_plan_check")
        cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
               os.path.join(ROOT, "tests", "eval_plan_check.cpp"), "-o", exe]
        san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
        if san.returncode != 0:
            assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr
            subprocess.run(cmd, check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    tail = "\n".join(l for l in run.stdout.splitlines() if not l.startswith("case "))[-3000:]
    assert run.returncode == 0, tail + run.stderr[-3000:]
    assert run.stdout.rstrip().endswith("eval_plan_check: ok") and "FAILED" not in run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    cases = {l.split()[1]: [int(v) for v in l.split()[2:]] for l in run.stdout.splitlines() if l.startswith("case ")}
    assert cases["n70001_g1"][:5] == [35, 6, 0, 2, 26] and cases["n1_g0"][:5] == [1, 0, 0, 1, 6]
    assert cases["n2049_g0"][:3] == [2, 1, 1] and cases[f"n{1 << 24}_g1"][:2] == [8192, 13]
    lib = _lib.load()
    for name, row in cases.items():           # the library's workspace size is the plan's total
        n, g = name[1:].split("_g")
        assert lib.radad_eval_metrics_workspace_bytes(int(n), int(g)) == row[-1], name
