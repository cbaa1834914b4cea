"""CPU: the case table and the designed stores of the row-width tests (tests/knn_width_ref.py), before anything runs on a GPU.

  * CASES covers what it claims: every (width class x scan kind reachable in that class x list class) with L2 and with COSINE, every
    width with every kind it can reach, the fp16 generic kernel at a width of classes a, d and e; the coverage is printed;
  * every tail_store is a store on which a correct scan has nothing to reject (band_count <= k + 6 for every centre, k and metric)
    and on which the designated column group decides: with that group zeroed in rows and query the float64 top-k is another one;
  * expected_kind is what the host planner plans (tests/knn_width_plan_check.cpp, a stand-alone program built with AddressSanitizer +
    UBSan like tests/knn_plan_check.cpp), and the width x k limit has the corner values include/radad_hip.h states."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import knn_width_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC_ID = {"L2": 0, "IP": 1, "COSINE": 2}


def test_widths_and_classes():
    assert W.WIDTHS == (4, 8, 12, 16, 20, 28, 32, 36, 48, 80, 1040, 60, 68, 124, 132, 64, 192, 1024, 1088, 7168, 16380)
    assert all(w % 4 == 0 for w in W.WIDTHS)
    assert all(w % 32 == 16 for w in W.CLASSES["d"]) and all(w % 64 == 0 for w in W.CLASSES["f"])
    # the rotation: first and last group always; the first group of every partial 16-, 32-, 64-column step; an interior group from 12 on
    for w in W.WIDTHS:
        g = W.column_groups(w)
        assert g[0] == 0 and (w // 4 - 1) in g and len(set(g)) == len(g)
        for step in (16, 32, 64):
            if w % step:
                assert (w - w % step) // 4 in g
        if w >= 12:
            assert any(0 < x < w // 4 - 1 for x in g)
    assert W.column_groups(16380) == [0, 4094, 4092, 4088, 4080, 2047] and W.column_groups(48) == [0, 11, 8, 6]
    # every store's rots give every group a centre; no store is beyond 600 MB
    for (w, n, f16, m) in W.STORES:
        p = W.centres_per_store(w, n, W.K_MAX)
        assert p >= 1 and p * len(W.store_rots(w, n)) >= len(W.column_groups(w))
        assert n * w * 4 <= 600e6
    assert W.DECOYS == 1100 and W.DECOYS > 1024


def test_cases_cover_classes_kinds_and_lists():
    cases = W.CASES
    assert len(set(cases)) == len(cases)
    seen = {}
    for case in cases:
        w, n, f16, metric, nq, k = case
        pl = W.plan(w, n, f16, nq, k)
        seen.setdefault((W.CLASS_OF[w], pl["kernel"], W.list_class(k)), set()).add(metric)
    # what a class can reach at all: every width x store size x store type x batch x k of the grid, whether or not it is a case
    reachable, per_width = set(), {}
    for w in W.WIDTHS:
        for n in (W.N_SMALL, W.N_LARGE, W.N_PLANE_WIDE):
            if n * w * 4 > 600e6 or (w > 1088 and n == W.N_LARGE) or (n == W.N_PLANE_WIDE and w != 7168):
                continue
            for f16 in (False, True):
                if f16 and W.CLASS_OF[w] not in W.F16_CLASSES:
                    continue
                for nq, k in W.SEARCHES:
                    pl = W.plan(w, n, f16, nq, k)
                    reachable.add((W.CLASS_OF[w], pl["kernel"], W.list_class(k)))
                    per_width.setdefault(w, set()).add(pl["kernel"])
    missing = {key for key in reachable if key not in seen or not {"L2", "COSINE"} <= seen[key]}
    assert not missing, sorted(missing)
    got_width = {}
    for (w, n, f16, metric, nq, k) in cases:
        got_width.setdefault(w, set()).add(W.plan(w, n, f16, nq, k)["kernel"])
    for w in W.WIDTHS:
        assert per_width[w] <= got_width[w], (w, per_width[w] - got_width[w])
    for cls in "ade":
        assert any(c == cls and kern == "k_knn_f32<f16>" for (c, kern, _) in seen), cls
    assert {"IP"} <= set().union(*seen.values())
    for cls in W.CLASSES:
        assert any("IP" in v for (c, _, _), v in seen.items() if c == cls), cls
    kinds = {W.expected_kind(c) for c in cases}
    assert kinds == set(W.KINDS), kinds
    assert any(W.plan(w, n, f16, nq, k)["ksplit"] for (w, n, f16, m, nq, k) in cases)
    print(f"{len(cases)} cases on {len(W.STORES)} stores ({len(W.store_params())} with the rotation); class x kernel x list class:")
    for key in sorted(seen):
        print("   ", *key, sorted(seen[key]))


def _unique_tail_stores():
    out = []
    for (w, n, f16, m, rot) in W.store_params():
        if (w, n, rot) not in out:
            out.append((w, n, rot))
    return out


@pytest.mark.parametrize("width,n,rot", _unique_tail_stores(), ids=lambda v: str(v))
def test_tail_stores_have_nothing_to_reject_and_the_group_decides(width, n, rot):
    rows, q, info = W.tail_store(width, n, 17, W.K_MAX, W.STORE_SEED, rot)
    C = info["centre_rows"]
    P = info["centres"]
    assert rows.shape == (n, width) and q.shape == (17, width) and np.isfinite(rows).all()
    assert np.array_equal(q, C[np.arange(17) % P]) and len(info["groups"]) == P
    assert info["groups"] == [W.column_groups(width)[(rot + i) % len(W.column_groups(width))] for i in range(P)]
    assert np.abs(rows).max() < 60000 and all(len(d) == W.DECOYS for d in info["decoys"])       # an fp16 store holds them
    for a, g in enumerate(info["groups"]):
        d = rows[info["decoys"][a]]
        other = np.ones(width, bool); other[4 * g:4 * g + 4] = False
        assert np.array_equal(d[:, other], np.broadcast_to(C[a][other], d[:, other].shape)), "a decoy differs from its query outside its group"
    for metric in ("L2", "IP", "COSINE"):
        s, _ = W.scores64(rows, C, metric)
        counts = W.band_counts(rows, C, W.K_LIST, metric)
        for k in W.K_LIST:
            assert (counts[k] <= k + 6).all(), (metric, k, counts[k])
        top = W.topk64(s, W.K_MAX + 8)
        for a, g in enumerate(info["groups"]):
            assert set(top[a]) == set(info["neighbours"][a]), (metric, a)
            assert top[a].min() >= W.LEAD
            s0, _ = W.scores64(W.zero_group(rows, g), W.zero_group(C[a:a + 1], g), metric)
            for k in W.K_LIST:
                t0 = W.topk64(s0, k)[0]
                assert not np.array_equal(t0, top[a, :k]), (metric, a, k)
                if width > 4:          # (one group in all: everything ties at 0 and the lowest ids win)
                    assert set(t0) <= set(info["decoys"][a]), (metric, a, k)


def test_dup_store_has_its_copies():
    rows, q, info = W.dup_store(48, 1500, 17, 27, W.STORE_SEED)
    assert info["centres"] == 4 and rows.shape == (1500, 48)
    for a in range(info["centres"]):
        cp = info["copies"][a]
        assert len(cp) == 100 and np.array_equal(cp, np.arange(cp[0], cp[0] + 100))
        assert (rows[cp] == rows[info["neighbours"][a][3]]).all()
        s, _ = W.scores64(rows, info["centre_rows"][a:a + 1], "L2")
        top = W.topk64(s, 104)[0]
        assert list(top[3:103]) == list(cp) and top[103] == info["neighbours"][a][3]      # ties: the lower ids first


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("knn_width_plan") / "knn_width_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_width_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr
        print("knn_width_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    text = "".join(f"{w} {n} {int(f16)} {METRIC_ID[m]} {nq} {k}\n" for (w, n, f16, m, nq, k) in W.CASES)
    text += "16380 1500 0 0 17 1024\n16384 1500 0 0 17 1024\n16384 1500 0 0 17 10\n"
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run


def test_expected_kind_is_the_planners(planner):
    out = planner.stdout
    assert out.rstrip().endswith("knn_width_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in planner.stderr and "Sanitizer" not in planner.stderr, planner.stderr[-3000:]
    lines = [l.split() for l in out.splitlines() if l.startswith("plan ")]
    assert len(lines) == len(W.CASES) + 3
    wrong = []
    for case, f in zip(W.CASES, lines):
        w, n, f16, m, nq, k = case
        assert [int(v) for v in f[1:7]] == [w, n, int(f16), METRIC_ID[m], nq, k]
        pl = W.plan(w, n, f16, nq, k)
        if (f[7], int(f[8])) != (pl["kind"], int(pl["ksplit"])) or int(f[11]) != 1:
            wrong.append((case, f[7:], pl))
    assert not wrong, wrong[:8]
    # the limit: 16380 x 1024 fits exactly, 16384 x 1024 does not, 16384 x 10 does
    tail = lines[-3:]
    assert [int(t[10]) for t in tail[:2]] == [163840, 163856] and [int(t[11]) for t in tail] == [1, 0, 1] and [int(t[9]) for t in tail] == [1, 1, 1]
