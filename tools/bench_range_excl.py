#!/usr/bin/env python3
"""Certified range search among the rows a query does not exclude (radad_knn_range_search_excl / _excl_pq) at the benchmark scale:
1 M x 512, cosine, 1024 queries, threshold 0.9, max_per_query 128.  Stores as tools/bench_range.py's: unstructured noise rows, 64
groups of 16 queries around a centre each, planted rows at cosines 0.93 .. 0.99 with the group's centre, spread over the store.
  per_query_c   c in {0, 200, 1500}: every group has HITS = 10 planted rows of other speakers and c planted rows of ITS OWN speaker,
                all above the threshold; query j excludes its own speaker's tag (m = 1).  The exact admissible count is HITS for every
                query (asserted); the plain range search of the same handle counts HITS + c.
  batch_pct     pct in {0, 50, 90}, on the c = 0 store: the rows whose tag (row % 100) is below pct are excluded, one set for the
                batch.  The counts are asserted against the plain range search's lists filtered on the device.
Legs per case, timed in ALTERNATION on the same handle in one process (round r: excluding, plain range; wall clock around a
synchronised loop of REPS calls after WARM warm-up calls each; the median of ROUNDS rounds and every round are reported).  From one
profiled call: the milliseconds of the scan launch and of the re-rank.
Prints one JSON line.  tools/bench_range_excl.py [rows] [queries] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OUT = sys.argv[3] if len(sys.argv) > 3 else None
D, M, THRESH, GROUPS, HITS, WARM, REPS, ROUNDS = 512, 128, 0.9, 64, 10, 5, 100, 3
SPEAKER0 = 1_000_000                     # tag of group s's own speaker: SPEAKER0 + s; every other row: row % 100


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def store(c):
    """(rows [N, D], queries [NQ, D], row tags [N]) on the device: HITS + c planted rows per group, the last c the group's own speaker"""
    g = torch.Generator(device=dev).manual_seed(3000 + c)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    tags = torch.arange(N, device=dev, dtype=torch.int64) % 100
    ctr = unit(torch.randn((GROUPS, D), device=dev, generator=g))
    q = ctr[torch.arange(NQ, device=dev) % GROUPS] + 0.05 * unit(torch.randn((NQ, D), device=dev, generator=g))
    h = HITS + c
    where = torch.randperm(N, device=dev, generator=g)[:GROUPS * h].reshape(GROUPS, h)
    for s in range(GROUPS):
        u = torch.randn((h, D), device=dev, generator=g)
        u = unit(u - (u @ ctr[s]).unsqueeze(1) * ctr[s])
        lv = torch.linspace(0.93, 0.99, h, device=dev)[torch.randperm(h, device=dev, generator=g)].unsqueeze(1)
        rows[where[s]] = lv * ctr[s] + torch.sqrt(1 - lv * lv) * u
        tags[where[s, HITS:]] = SPEAKER0 + s
    return rows, q, tags


def measure(idx, excluding, plain, want_counts):
    for _ in range(WARM):
        excluding(); plain()
    t_x, t_p = [], []
    for _ in range(ROUNDS):
        ms, (counts, Dx, Ix) = window(excluding, REPS)
        t_x.append(round(ms, 4))
        ms, _ = window(plain, REPS)
        t_p.append(round(ms, 4))
    excluding()
    info = idx.last_range()
    emitted, floors = idx.last_emitted(NQ)
    ab = idx.last_abandon()
    idx.profile(True)
    excluding()
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    assert torch.equal(counts.to(torch.int64), want_counts.to(torch.int64)), (counts[:8], want_counts[:8])
    assert info["route"] == "tile" and len(prof) == 2, (info, prof)
    return {"excluding": {"search_ms": round(statistics.median(t_x), 4), "rounds": t_x, **info, "scan_ms": round(prof[0], 4),
                          "rerank_ms": round(prof[1], 4), "emitted_mean": round(float(emitted.mean()), 1), "emitted_max": int(emitted.max()),
                          "eps_max": float(THRESH - floors.min()), "abandon": ab, "count_mean": round(float(counts.float().mean()), 2),
                          "over_plain_range": round(statistics.median(t_x) / statistics.median(t_p), 3)},
            "plain_range": {"search_ms": round(statistics.median(t_p), 4), "rounds": t_p}}


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "queries": NQ, "threshold": THRESH, "max_per_query": M, "groups": GROUPS,
                  "admissible_hits": HITS, "warmup": WARM, "reps": REPS, "rounds": ROUNDS,
                  "alternation": "excluding, plain range per round"}}
for c in (0, 200, 1500):
    rows, q, tags = store(c)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    q_tags = (SPEAKER0 + torch.arange(NQ, device=dev, dtype=torch.int64) % GROUPS).reshape(NQ, 1)
    plain = lambda: idx.range_search_device(q, THRESH, M)                                                       # noqa: E731
    pq = lambda: idx.range_search_excluding_per_query_device(q, THRESH, tags, q_tags, None, M)                  # noqa: E731
    pc = plain()[0]
    assert int(pc.min()) == HITS + c and int(pc.max()) == HITS + c, (int(pc.min()), int(pc.max()))
    out[f"per_query_c{c}"] = measure(idx, pq, plain, torch.full((NQ,), HITS, device=dev))
    out[f"per_query_c{c}"]["plain_range"]["count"] = HITS + c
    if c == 0:
        pcounts, pD, pI = plain()
        for pct in (0, 50, 90):
            excl = torch.arange(pct, device=dev, dtype=torch.int64)
            kept = (pI >= 0) & (tags[pI.clamp(min=0)] >= pct)                                                   # (HITS <= M: the lists are whole)
            batch = lambda: idx.range_search_excluding_device(q, THRESH, tags, excl, M)                         # noqa: E731
            out[f"batch_pct{pct}"] = measure(idx, batch, plain, kept.sum(dim=1))
            out[f"batch_pct{pct}"]["excluded_rows"] = int((tags < pct).sum())
    del idx, q, tags
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
