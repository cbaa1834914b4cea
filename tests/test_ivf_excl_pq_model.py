"""No GPU: the conditions that make every designed case of tests/ivf_excl_pq_ref.py the case it claims to be, the model against a
brute force written another way, and that the library offers the search (fails on a build without radad_ivf_search_excl_pq)."""
import os

import numpy as np
import pytest

from oracle import radad_oracle as O
from test_gpu_ivf_adversarial import KS
from ivf_excl_pq_ref import KMAX, case, expected_pq, list_major, live_tags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(db, assign, cent, q, k, nprobe, tags, qtags, counts):
    """the same answer from the definition: distances to every row, probed lists and admission as masks"""
    d = ((db.astype(np.float64)[None, :, :] - q.astype(np.float64)[:, None, :]) ** 2).sum(-1)
    _, probes = O.knn(cent, q, nprobe, "L2")
    out = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        ok = np.isin(assign, probes[j]) & ~np.isin(tags, live_tags(qtags, counts, j))
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, d[j, cand]))][:k]
        out[j, :len(order)] = order
    return out


@pytest.mark.parametrize("dim", [128, 96])
def test_twins(dim):
    c = case("twins", dim)
    oi = c["oi"][:, :KMAX]
    A, B = set(c["planted_a"].tolist()), set(c["planted_b"].tolist())
    assert set(oi[1, :20].tolist()) == A                                   # the copy that excludes nothing: its 20 near-copies first
    assert not A & set(oi[0].tolist()) and (oi[0] >= 0).all()
    rest = [i for i in oi[1] if i not in A]
    assert list(oi[0][:len(rest)]) == rest                                 # copy 0 = copy 1 without the planted rows, in order
    assert list(oi[2]) == list(oi[1])                                      # another query's planted rows: not among this query's hits
    assert (c["tags"][c["planted_b"]] == 1_000_001).all() and (c["tags"][c["planted_a"]] == 1_000_000).all() and c["counts"][1] == 0
    for cp in range(3, len(oi)):                                           # the single far row a copy excludes is not among its hits
        assert list(oi[cp]) == list(oi[1])
    assert len({tuple(np.unique(live_tags(c["qtags"], c["counts"], j)).tolist()) for j in range(len(oi))}) == len(oi)      # every copy another set
    assert (c["q"] == c["q"][0]).all()
    sub = slice(0, 6)
    np.testing.assert_array_equal(_brute(c["db"], c["assign"], c["cent"], c["q"][sub], KMAX, 3, c["tags"], c["qtags"][sub], c["counts"][sub]), oi[sub])


@pytest.mark.parametrize("dim", [128, 96])
def test_crowded_leave_one_out(dim):
    c = case("loo", dim)
    db, cent, q, tags, assign = c["db"], c["cent"], c["q"], c["tags"], c["assign"]
    union = np.unique(c["qtags"])
    for k in KS:       # the reference's loop (search K + 10, drop the batch's union, pad) is defeated for every planted query ...
        _, pi = O.ivf_search(db, assign, cent, q[c["planted"]], k + 10, 3)
        left = ((pi >= 0) & ~np.isin(tags[np.clip(pi, 0, None)], union)).sum(1)
        assert np.all(left < k), (dim, k, left)
        assert np.all(c["oi"][c["planted"], :k] >= 0), (dim, k)            # ... although k admissible neighbours exist
    for j, rows in zip(c["planted"], c["at"]):
        assert not np.isin(c["oi"][j], rows).any()
    # query 11 next to query 3: query 3's planted rows are admissible for it and are its 20 nearest
    assert set(c["oi"][11, :20].tolist()) == set(c["at"][0].tolist())
    others = np.setdiff1d(np.arange(len(q)), np.concatenate([c["planted"], [11]]))
    np.testing.assert_array_equal(c["oi"][others], c["plain"][1][others])      # a query whose tag no row carries: the plain search
    sub = np.array([3, 4, 11, 12])
    np.testing.assert_array_equal(_brute(db, assign, cent, q[sub], KMAX, 3, tags, c["qtags"][sub], None), c["oi"][sub, :KMAX])


@pytest.mark.parametrize("dim", [128, 96])
def test_position_coverage(dim):
    c = case("positions", dim)
    assign, rows, home, P = c["assign"], c["rows"], c["home"], c["P"]
    off, pos = list_major(assign, len(c["cent"]))
    assert (assign[rows] == home).all()                                    # planting kept the rows in the list, so positions are as designed
    p = pos[rows]
    assert list(p) == list(range(P - 20, P + 20)) and P % 256 == 0 and P % 64 == 0      # one run across a multiple of 64 and of 256
    assert off[home] <= p[0] and p[-1] < off[home + 1]
    assert set(((p - off[home]) % 16).tolist()) == set(range(16))          # every residue of a 16-row step
    oi = c["oi"][:, :KMAX]
    assert set(oi[1, :26].tolist()) <= set(rows.tolist())                  # nothing excluded: the run's rows fill the answer
    assert not np.isin(oi[0], rows).any() and (oi[0] >= 0).all()
    full = _brute(c["db"], assign, c["cent"], c["q"][:1], 41, 3, c["tags"], np.zeros((1, 0), np.int64), None)[0]
    for i in range(40):                                                    # copy 2 + i misses row i of the run and nothing else
        assert list(oi[2 + i]) == [r for r in full if r != rows[i]][:KMAX], i
    # the whole home list excluded: nothing at nprobe 1, a full answer at nprobe 3; the twin excludes a list it never probes
    (d1, i1), (d3, i3) = c["list1"], c["list3"]
    assert (i1[0] == -1).all() and (i3[0, :15] >= 0).all() and not np.isin(assign[i3[0, :15]], [home]).any()
    assert set(i1[1, :15].tolist()) <= set(rows.tolist()) and list(i3[1]) == list(i1[1])
    assert c["other"] not in O.knn(c["cent"], c["q"][:1], 3, "L2")[1][0]


@pytest.mark.parametrize("dim", [128, 96])
def test_long_lists(dim):
    c = case("long", dim)
    assert np.bincount(c["assign"]).min() > 256                            # every list is longer than a chunk: the split shares start anywhere
    _, top = O.ivf_search(c["db"], c["assign"], c["cent"], c["q"], 40 + KMAX, 3)
    np.testing.assert_array_equal(c["oi"][:, :KMAX], top[:, 40:])          # the answer starts at rank 41


@pytest.mark.parametrize("dim", [128, 96])
def test_set_shapes(dim):
    c = case("shapes", dim)
    top, oi, plain = c["top"], c["oi"][:, :KMAX], c["plain"][1][:, :KMAX]
    deep = O.ivf_search(c["db"], c["assign"], c["cent"], c["q"], KMAX + 12, 3)[1]
    for j in range(len(oi)):
        kind = j % 4
        if kind in (0, 1):        # count 0 or negative: nothing excluded although the row is full of the query's top hits
            assert list(oi[j]) == list(plain[j]) and np.isin(top[j, :12], c["qtags"][j]).sum() >= 12
        elif kind == 2:           # count above m: all 64 entries live
            assert list(oi[j]) == [r for r in deep[j] if r not in top[j, :5]][:KMAX]
        else:                     # 9 live entries: the top 3 twice, any order; the ranks 4 .. 12 behind the count are ignored
            assert list(oi[j, :9]) == list(top[j, 3:12])
            live = live_tags(c["qtags"], c["counts"], j)
            assert len(live) == 9 and len(np.unique(live)) < 9
    assert not np.array_equal(c["oi_null"], c["oi"])                      # NULL counts: the entries behind the counts are live
    j = 3
    assert not np.isin(top[j, :12], c["oi_null"][j]).any()
    np.testing.assert_array_equal(c["oi_one"][:, :KMAX - 1], plain[:, 1:])  # m = 1: the nearest row gone


def test_the_library_offers_the_search():
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    assert "radad_ivf_search_excl_pq" in _lib.SIGNATURES and _lib.IVF_OPT_PQ_FILTER == 1
    assert hasattr(R.HipIVFFlatIndex, "search_probed_excluding_per_query") and hasattr(R.VectorDatabase, "search_probed_excluding_per_query")
    hdr = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert "int radad_ivf_search_excl_pq(" in hdr and "#define RADAD_IVF_OPT_PQ_FILTER 1" in hdr
    assert "the IVF index (its admission bitmap is per call" not in hdr
    lib = _lib.load()
    assert hasattr(lib, "radad_ivf_search_excl_pq")
