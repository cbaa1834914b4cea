#!/usr/bin/env python3
"""The tail of a deferring launch on DENSE lists, at the benchmark scale (the family of tools/bench_abandon_ahead.py): 1 M x 512, cosine,
1024 queries (4 query tiles), k = 10, and every 1 / FILL-th tile task defers 16 rows -- FILL 1: every tile task, the lists are full
(62 496 of 62 512 entries a query tile, 30 times the benchmark's).  There every 16-row group of the row tail (k_knn_hi_rowtail) re-reads
its query tile from L2, where a 256-row tile of the tile tail (k_knn_hi_tail) reads it once.

The store: the queries are 0.08 off a common direction b.  The sample's tiles (every 61st) hold 16 rows 0.005 off b -- every floor comes
from them, cos 0.9968 -- and each other planted tile 16 near-duplicates of one query each, 0.02 off it: 0.9998 to their own query (emitted:
~61 per query at FILL 1), 0.9934 to the others -- below every floor, yet alive at the checkpoint (score + 7/8 (1 - cos) = 0.9992): listed
by all four query tiles, scored by the tail, emitted once.  (The 1024 sample rows are candidates of every query: the first warm-up
search overflows a fresh handle's 1024-entry buffers and the handle widens them; the timed searches recheck nothing.)  The other rows
are unit-variance noise.

One process measures ONE library (RADAD_HIP_LIB, or the tree's own): REPS searches per leg after WARM, the legs of two trees are
alternated by running the tool from each in turn.  Prints one JSON line per FILL; --dump keeps ids, distances and float64 keys,
--compare asserts two dumps equal.
  tools/bench_row_tail.py [--fill 1,2,8,32] [--out results.jsonl] [--dump results.npz]
  tools/bench_row_tail.py --compare a.npz b.npz"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--fill", default="1")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=1024)
ap.add_argument("--out", default=None)
ap.add_argument("--dump", default=None)
ap.add_argument("--compare", nargs=2, default=None)
args = ap.parse_args()

if args.compare:
    a, b = np.load(args.compare[0]), np.load(args.compare[1])
    assert sorted(a.files) == sorted(b.files) and a.files, (a.files, b.files)
    for name in a.files:
        assert np.array_equal(a[name], b[name]), f"{name} differs"
    print(f"{len(a.files)} arrays (ids, distances, float64 keys, emitted counts, floors per fill): array_equal")
    sys.exit(0)

import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib

dev = torch.device("cuda:0")
N, NQ, D, K, WARM, REPS, P = args.rows, args.queries, 512, 10, 5, 40, 16


def store(fill):
    g = torch.Generator(device=dev).manual_seed(5000 + fill)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    b = torch.randn(D, device=dev, generator=g)
    q = b[None, :] + 0.08 * torch.randn((NQ, D), device=dev, generator=g)
    tiles = N // 256
    stride = max(1, tiles // 64)                                     # knn_hi_sample_stride in tiles
    t = torch.arange(tiles, device=dev)
    sample = (t % stride == 0) & (t // stride < 64)
    planted = (t % fill == 0) | sample
    where = (t[planted][:, None] * 256 + 3 + 15 * torch.arange(P, device=dev)[None, :]).reshape(-1)
    is_sample = sample[planted][:, None].expand(-1, P).reshape(-1)
    own = q[torch.arange(len(where), device=dev) % NQ] + 0.02 * torch.randn((len(where), D), device=dev, generator=g)
    common = b[None, :] + 0.005 * torch.randn((len(where), D), device=dev, generator=g)
    rows[where] = torch.where(is_sample[:, None], common, own)
    return rows, q, int(planted.sum())


results, dump = [], {}
for fill in [int(x) for x in args.fill.split(",")]:
    rows, q, n_planted = store(fill)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    search = lambda: idx.search_device(q, K, return_f64=True)         # noqa: E731
    for _ in range(WARM):
        res = search()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        res = search()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / REPS
    idx.profile(True)
    for _ in range(5):
        search()
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    launch = idx.last_launch()
    n = launch["scan_launches"]
    per = sorted(sum(prof[i:i + n]) for i in range(0, len(prof) - n + 1, n))
    counts, floors = idx.last_emitted(NQ)
    out = {"fill": fill, "planted_tiles": n_planted, "search_ms": round(ms, 4), "scan_plus_tail_ms_median": round(per[len(per) // 2], 4),
           "scan_launch_ms": [round(p, 4) for p in prof[:n]], "defer": launch["abandon_defer"], "abandon": launch["early_abandon"],
           "rechecked": launch["rechecked_queries"], "emitted_max": int(counts.max()), "lib": _lib.LIB_PATH}
    print(json.dumps(out), flush=True)
    results.append(out)
    D_, I_, K64 = res
    for name, a in (("D", D_.cpu().numpy()), ("I", I_.cpu().numpy()), ("K64", K64.cpu().numpy()), ("counts", counts), ("floors", floors)):
        dump[f"fill{fill}_{name}"] = a
    del idx, q
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "a") as f:
        for o in results:
            f.write(json.dumps(o) + "\n")
if args.dump:
    np.savez(args.dump, **dump)
