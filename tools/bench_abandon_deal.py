#!/usr/bin/env python3
"""The abandoning tile scan with its row tiles dealt by ticket (RADAD_KNN_OPT_ABANDON_DEAL) against static chunks, at the benchmark
scale: 1 M x 512, cosine, 1024 queries, k = 10.  Two stores, each on a handle of its own:
  spread    a near-duplicate of a query planted in every third row tile, all over the store (the benchmark's kind of skip pattern)
  cluster   the planted rows inside ONE contiguous eighth of the store (a store filled cluster by cluster): the tiles that cannot be
            skipped are neighbours, i.e. a few static chunks hold all of them
  rows      unstructured unit-variance noise
  queries   four groups (query j: group j % 4) around four unrelated centres, noise of relative norm 0.05; the i-th planted tile holds one
            row of group i % 4, so every query tile vetoes every planted tile and a query sees a quarter of the planted rows (they
            fit the re-rank's 512 candidates)
Legs per store, timed in ALTERNATION on the same handle in one process (round r: deal on, deal off; wall clock around a synchronised
loop of REPS searches after WARM warm-up searches each; the median of ROUNDS rounds and every round are reported), plus from one
profiled search per leg the milliseconds of the scan's launches.  Results of the two legs are asserted equal.
Prints one JSON line.  tools/bench_abandon_deal.py [rows] [queries] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OUT = sys.argv[3] if len(sys.argv) > 3 else None
D, K, GROUPS, WARM, REPS, ROUNDS = 512, 10, 4, 5, 50, 3


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def store(kind):
    """(rows [N, D], queries [NQ, D], planted tiles) on the device"""
    g = torch.Generator(device=dev).manual_seed(3000 + len(kind))
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = torch.randn((GROUPS, D), device=dev, generator=g)
    q = ctr[torch.arange(NQ, device=dev) % GROUPS] + 0.05 * torch.randn((NQ, D), device=dev, generator=g)
    tiles = N // 256
    planted = torch.arange(0, tiles, 3, device=dev) if kind == "spread" else torch.arange(tiles // 8, tiles // 4, device=dev)
    where = planted * 256 + 19
    i = torch.arange(len(planted), device=dev)
    src = q[(GROUPS * i + i % GROUPS) % NQ]              # the i-th planted tile holds a row of group i % GROUPS
    rows[where] = src + 0.03 * torch.randn((len(planted), D), device=dev, generator=g)
    return rows, q, len(planted)


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "queries": NQ, "k": K, "groups": GROUPS, "warmup": WARM, "reps": REPS, "rounds": ROUNDS,
                  "alternation": "deal on, deal off per round"}}
for kind in ("spread", "cluster"):
    rows, q, n_planted = store(kind)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    search = lambda: idx.search_device(q, K, return_f64=True)                                   # noqa: E731
    t = {1: [], 0: []}
    res, info = {}, {}
    for deal in (1, 0):
        idx.set_abandon_deal(deal)
        for _ in range(WARM):
            search()
    for _ in range(ROUNDS):
        for deal in (1, 0):
            idx.set_abandon_deal(deal)
            ms, res[deal] = window(search, REPS)
            t[deal].append(round(ms, 4))
    for deal in (1, 0):
        idx.set_abandon_deal(deal)
        idx.profile(True)
        search()
        torch.cuda.synchronize()
        prof = idx.profile_read()
        idx.profile(False)
        launch = idx.last_launch()
        info[deal] = {"search_ms": round(statistics.median(t[deal]), 4), "rounds": t[deal], "scan_launch_ms": [round(p, 4) for p in prof],
                      "scan_ms": round(sum(prof), 4), "abandon": launch["early_abandon"], "deal": launch["abandon_deal"],
                      "rechecked": launch["rechecked_queries"]}
    idx.set_abandon_deal(1)
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)
    assert info[1]["abandon"] == info[0]["abandon"] and info[0]["deal"]["launches"] == 0, info
    out[kind] = {"planted_tiles": n_planted, "dealt": info[1], "static": info[0],
                 "dealt_over_static_scan": round(info[1]["scan_ms"] / info[0]["scan_ms"], 3)}
    del idx, q
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
