#!/usr/bin/env python3
"""Exclusion inside the certified tile scan (radad_knn_search_excl_scan) at the benchmark scale: 1 M x 512, cosine, k = 10, 1024 queries.
Legs, each the median of ROUNDS rounds of REPS calls after WARM warm-up calls (wall clock around a synchronised loop), plus the
scan-launch times (HIP events around each scan launch, radad_knn_profile: the median over 9 profiled searches):
  plain            HipFlatIndex.search_device
  in_scan 0 %      search_excluding_in_scan with a one-tag set no row carries (the pre-pass and the biased instantiation run)
  in_scan 50 / 90 %   ... with that share of the rows excluded (tags = row ids)
  over_fetch 90 %  radad_knn_search_excl at k_fetch = 20 with 90 % excluded, on 64 QUERIES ONLY: every query takes its exact pass, the
                   slow case.  "scaled_to_1024_ms" is 16 x the 64-query time -- an extrapolation (the exact pass streams the store
                   once per group of <= 8 queries, so it is linear in the batch), not a measurement.
Prints one JSON line.  tools/bench_excl_scan.py [rows] [queries]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
lib = _lib.load()
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
D, K, WARM, REPS, ROUNDS = 512, 10, 5, 200, 3          # (200 calls: windows of 0.2 s and more)
rows = torch.empty((N, D), device=dev)
_lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, N, D, 4321, 0, _lib.stream_ptr(dev)))
q = torch.empty((NQ, D), device=dev)
_lib.check(lib.radad_synth_rows(q.data_ptr(), 0, NQ, D, 977, 0, _lib.stream_ptr(dev)))
idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
idx.add_device(rows)
tags = torch.arange(N, device=dev, dtype=torch.int64)
perm = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
EXCL = {"0pct": torch.tensor([N + 7], device=dev, dtype=torch.int64), "50pct": torch.sort(perm[:N // 2]).values,
        "90pct": torch.sort(perm[:N * 9 // 10]).values}


def timed(fn):
    for _ in range(WARM):
        r = fn()
    rounds = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(REPS):
            r = fn()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / REPS)
    return round(statistics.median(rounds), 4), [round(x, 4) for x in rounds], r


def scan_launches(fn):
    """HIP-event time of each scan launch of a search: the median over 9 profiled searches"""
    idx.profile(True)
    for _ in range(9):
        fn()
    ms = idx.profile_read()
    idx.profile(False)
    per = len(ms) // 9
    return [round(statistics.median(ms[i::per]), 4) for i in range(per)] if per else []


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "k": K, "queries": NQ, "warmup": WARM, "reps": REPS, "rounds": ROUNDS}}
ms, rounds, (D0, I0) = timed(lambda: idx.search_device(q, K))
plane = idx.plane_info()
rsc_plain = (3 if plane["one_scale"] else 2) if plane["centred"] else (0 if plane["one_scale"] else 1)
out["plain"] = {"search_ms": ms, "rounds": rounds, "scan_kind": idx.last_launch()["scan_kind"], "rsc": rsc_plain, "plane": plane,
                "scan_launch_ms": scan_launches(lambda: idx.search_device(q, K))}
plain_scan = sum(out["plain"]["scan_launch_ms"])
for name, ex in EXCL.items():
    ms_x, rounds, (Dx, Ix) = timed(lambda: idx.search_excluding_in_scan(q, K, tags, ex))
    info = idx.last_excl_scan()
    assert not torch.isin(Ix[Ix >= 0], ex).any() and (Ix >= 0).all()
    if name == "0pct":
        assert torch.equal(Ix, I0)
    launches = scan_launches(lambda: idx.search_excluding_in_scan(q, K, tags, ex))
    out["in_scan_" + name] = {"search_ms": ms_x, "rounds": rounds, "over_plain": round(ms_x / ms, 3), **info, "rsc": 3 if plane["one_scale"] else 2,
                              "scan_launch_ms": launches, "scan_over_plain": round(sum(launches) / plain_scan, 3) if plain_scan else None}
q64 = q[:64].contiguous()
ms_o, rounds, (Do, Io) = timed(lambda: idx.search_excluding(q64, K, tags, EXCL["90pct"], k_fetch=20))
info = idx.last_excl()
ms_i, _, (Di, Ii) = timed(lambda: idx.search_excluding_in_scan(q64, K, tags, EXCL["90pct"]))
assert torch.equal(Io, Ii)
out["over_fetch_90pct_64_queries"] = {"search_ms": ms_o, "rounds": rounds, **info, "per_listed_query_ms": round(ms_o / max(info["exact"], 1), 4),
                                      "scaled_to_1024_ms": round(ms_o * 16, 2), "scaled": "16 x the 64-query time: extrapolated, not measured",
                                      "in_scan_64_queries_ms": ms_i}
print(json.dumps(out))
