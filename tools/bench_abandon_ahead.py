#!/usr/bin/env python3
"""The abandon checkpoint's head prefetch (RADAD_KNN_OPT_ABANDON_AHEAD) where it mis-speculates, at the benchmark scale: 1 M x 512, cosine,
1024 queries, k = 10.  Three stores, each on a handle of its own:
  leave     a near-duplicate of a query planted in every third row tile (the benchmark's kind of store): every tile task is skipped or
            deferred, every head fetched ahead is used
  alternate as `leave`, and every odd tile holds 24 rows that are live at the checkpoint and far below the floor in full (their first
            64 elements are 0.9 of a query centre's direction there, the rest noise): odd tiles stay, even tiles leave -- "the last
            tested tile left" is wrong at every tile
  stay      as `leave`, and EVERY tile holds such rows: each workgroup wastes one head, its first
In all three the other rows are unstructured unit-variance noise, and the queries come in four groups (query j: group j % 4) around four
unrelated centres with noise of relative norm 0.05, as in tools/bench_abandon_deal.py.
Legs per store, in ALTERNATION on the same handle in one process: option off, on, off, on; wall clock around a synchronised loop of REPS
searches after WARM warm-up searches, plus from one profiled search per leg the milliseconds of the scan's launches (each followed by
its tail) and the heads used / wasted.  Results of all legs are asserted equal.
Prints one JSON line.  tools/bench_abandon_ahead.py [rows] [queries] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OUT = sys.argv[3] if len(sys.argv) > 3 else None
D, K, GROUPS, WARM, REPS, LIVE = 512, 10, 4, 5, 40, 24


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def store(kind):
    g = torch.Generator(device=dev).manual_seed(4000 + len(kind))
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = torch.randn((GROUPS, D), device=dev, generator=g)
    q = ctr[torch.arange(NQ, device=dev) % GROUPS] + 0.05 * torch.randn((NQ, D), device=dev, generator=g)
    tiles = N // 256
    stay = {"leave": torch.empty(0, dtype=torch.long, device=dev), "alternate": torch.arange(1, tiles, 2, device=dev),
            "stay": torch.arange(0, tiles, device=dev)}[kind]
    if len(stay):
        where = (stay[:, None] * 256 + 1 + 2 * torch.arange(LIVE, device=dev)[None, :]).reshape(-1)
        head = ctr[0, :64] / ctr[0, :64].norm()
        tail = torch.randn((len(where), D - 64), device=dev, generator=g)
        tail *= (1 - 0.81) ** 0.5 / tail.norm(dim=1, keepdim=True)
        rows[where, :64] = D ** 0.5 * 0.9 * head[None, :]
        rows[where, 64:] = D ** 0.5 * tail
    planted = torch.arange(0, tiles, 3, device=dev)
    i = torch.arange(len(planted), device=dev)
    rows[planted * 256 + 18] = q[(GROUPS * i + i % GROUPS) % NQ] + 0.03 * torch.randn((len(planted), D), device=dev, generator=g)
    return rows, q, len(stay)


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "queries": NQ, "k": K, "warmup": WARM, "reps": REPS, "legs": "ahead off, on, off, on"}}
for kind in ("leave", "alternate", "stay"):
    rows, q, n_stay = store(kind)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    search = lambda: idx.search_device(q, K, return_f64=True)                                   # noqa: E731
    for ahead in (0, 1):
        idx.set_abandon_ahead(ahead)
        for _ in range(WARM):
            search()
    legs, first = [], None
    for ahead in (0, 1, 0, 1):
        idx.set_abandon_ahead(ahead)
        ms, res = window(search, REPS)
        first = first or res
        for a, b in zip(res, first):
            assert torch.equal(a, b)
        idx.profile(True)
        search()
        torch.cuda.synchronize()
        prof = idx.profile_read()
        idx.profile(False)
        launch = idx.last_launch()
        legs.append({"ahead": ahead, "search_ms": round(ms, 4), "scan_launch_ms": [round(p, 4) for p in prof], "scan_ms": round(sum(prof), 4),
                     "heads": launch["abandon_ahead"], "abandon": launch["early_abandon"], "deferred": launch["abandon_defer"]["tile_tasks_deferred"],
                     "rechecked": launch["rechecked_queries"]})
    off, on = [l["search_ms"] for l in legs if not l["ahead"]], [l["search_ms"] for l in legs if l["ahead"]]
    out[kind] = {"stay_tiles": n_stay, "legs": legs, "search_ms_off": off, "search_ms_on": on,
                 "on_over_off_scan": round(sum(l["scan_ms"] for l in legs if l["ahead"]) / sum(l["scan_ms"] for l in legs if not l["ahead"]), 3)}
    del idx, q
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
