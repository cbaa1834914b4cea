#!/usr/bin/env python3
"""Certified range search (radad_knn_range_search) at the benchmark scale: 1 M x 512, cosine, 1024 queries, threshold 0.9,
max_per_query 128.  One case per number of planted hits h in {0, 10, 1000}, each on a handle of its own:
  rows      unstructured unit-variance noise (cosines of ~0.044 standard deviation with anything: nothing random comes near 0.9)
  queries   64 groups of 16: query j = centre of group j % 64 + noise of norm 0.05 (1024 x 1000 planted rows of its own per query do
            not fit a 1 M-row store; the 16 queries of a group share theirs)
  planted   h rows per group at cosines 0.93 .. 0.99 with the group's centre, spread over the store: every query has h rows above
            the threshold (the exact counts are reported, and asserted to be h)
Legs per case, timed in ALTERNATION on the same handle in one process (round r: range, plain; wall clock around a synchronised loop
of REPS calls after WARM warm-up calls each; the median of ROUNDS rounds and every round are reported):
  range     HipFlatIndex.range_search_device; its route and n_exact (last_range), the rows the scan emitted per query, and from one
            profiled call the milliseconds of its one scan launch and of its re-rank (k_range_refine)
  plain     HipFlatIndex.search_device at k = 10 (radad_knn_search_ex): unchanged code, the yardstick
Prints one JSON line.  tools/bench_range.py [rows] [queries] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OUT = sys.argv[3] if len(sys.argv) > 3 else None
D, K, M, THRESH, GROUPS, WARM, REPS, ROUNDS = 512, 10, 128, 0.9, 64, 5, 100, 3


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def store(h):
    """(rows [N, D], queries [NQ, D]) on the device"""
    g = torch.Generator(device=dev).manual_seed(2000 + h)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = unit(torch.randn((GROUPS, D), device=dev, generator=g))
    q = ctr[torch.arange(NQ, device=dev) % GROUPS] + 0.05 * unit(torch.randn((NQ, D), device=dev, generator=g))
    if h:
        where = torch.randperm(N, device=dev, generator=g)[:GROUPS * h].reshape(GROUPS, h)
        for s in range(GROUPS):
            u = torch.randn((h, D), device=dev, generator=g)
            u = unit(u - (u @ ctr[s]).unsqueeze(1) * ctr[s])
            c = torch.linspace(0.93, 0.99, h, device=dev).unsqueeze(1)
            rows[where[s]] = c * ctr[s] + torch.sqrt(1 - c * c) * u
    return rows, q


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "queries": NQ, "threshold": THRESH, "max_per_query": M, "plain_k": K,
                  "groups": GROUPS, "warmup": WARM, "reps": REPS, "rounds": ROUNDS, "alternation": "range, plain per round"}}
for h in (0, 10, 1000):
    rows, q = store(h)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    plain = lambda: idx.search_device(q, K)                                                     # noqa: E731
    rng = lambda: idx.range_search_device(q, THRESH, M)                                         # noqa: E731
    for _ in range(WARM):
        rng(); plain()
    t_rng, t_plain = [], []
    for _ in range(ROUNDS):
        ms, (counts, Dr, Ir) = window(rng, REPS)
        t_rng.append(round(ms, 4))
        ms, (D0, I0) = window(plain, REPS)
        t_plain.append(round(ms, 4))
    launch = idx.last_launch()
    rng()
    info = idx.last_range()
    emitted, floors = idx.last_emitted(NQ)
    ab = idx.last_abandon()
    idx.profile(True)
    rng()
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    assert int(counts.min()) == h and int(counts.max()) == h, (h, int(counts.min()), int(counts.max()))
    assert info["route"] == "tile" and len(prof) == 2, (info, prof)
    n = min(h, K)
    assert torch.equal(Ir[:, :n], I0[:, :n])                                                    # the nearest hits are the plain search's nearest
    out[f"hits_{h}"] = {
        "range": {"search_ms": round(statistics.median(t_rng), 4), "rounds": t_rng, **info, "scan_ms": round(prof[0], 4),
                  "rerank_ms": round(prof[1], 4), "emitted_mean": round(float(emitted.mean()), 1), "emitted_max": int(emitted.max()),
                  "eps_max": float(THRESH - floors.min()), "abandon": ab,
                  "over_plain": round(statistics.median(t_rng) / statistics.median(t_plain), 3)},
        "plain": {"search_ms": round(statistics.median(t_plain), 4), "rounds": t_plain, "scan_kind": launch["scan_kind"],
                  "scan_phases": launch["scan_phases"], "rechecked": launch["rechecked_queries"]}}
    del idx, q
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
