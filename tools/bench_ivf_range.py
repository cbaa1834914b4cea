#!/usr/bin/env python3
"""Certified range search over the probed lists (radad_ivf_range_search) at the benchmark scale: 1 M x 512 (squared L2), nlist 4096,
nprobe 32, max_per_query 128.  One store per number of planted members h in {0, 10, 1000}, planted as tools/bench_range.py does:
  rows      unstructured unit-variance noise (squared distances of ~1024 with anything: nothing random comes near the radius)
  queries   64 groups: query j = centre of group j % 64 + noise of norm 0.05 (the queries of a group share their planted rows)
  planted   h rows per group at squared distances 1 .. 20 from the group's centre, spread over the store; radius 50
On the store without planted rows the same legs also run with UNSTRUCTURED queries (noise like the rows, every query probing lists of
its own: the workload of tools/bench_ivf.py), keys hits_0_nq_*_unstructured.
For each store and each batch size nq in {1, 256, 1024}, three legs timed in ALTERNATION in one process (round r: a, b, c; wall clock
around a synchronised loop of REPS calls after WARM warm-up calls each; the median of ROUNDS rounds and every round are reported):
  a  ivf_range   HipIVFFlatIndex.range_search_probed_device; its route, the queries its exact pass answered and the largest number of
                 positions a query emitted (last_range), the exact counts (min / max)
  b  ivf_topk    HipIVFFlatIndex.search_device at k = 10 on the SAME handle: unchanged code, the yardstick
  c  flat_range  HipFlatIndex(L2).range_search_device of the same rows: the exact answer over the whole store, and what the audit
                 costs without an index
Legs a and c must agree where every member's list is probed; the counts of both are reported, not asserted equal (an IVF search sees
the probed lists).  Prints one JSON line and, with an output stem, writes <stem>.json and the table <stem>.md.
tools/bench_ivf_range.py [rows] [out stem]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
D, K, M, RADIUS, GROUPS, NLIST, NPROBE, WARM, REPS, ROUNDS = 512, 10, 128, 50.0, 64, 4096, 32, 5, 50, 3
NQS = (1, 256, 1024)
if N < 200_000:                       # a rehearsal at a toy size keeps ~250 rows per list
    NLIST = max(64, N // 250)


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def store(h):
    """(rows [N, D], queries [1024, D]) on the device"""
    g = torch.Generator(device=dev).manual_seed(3000 + h)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = torch.randn((GROUPS, D), device=dev, generator=g)
    q = ctr[torch.arange(max(NQS), device=dev) % GROUPS] + 0.05 * unit(torch.randn((max(NQS), D), device=dev, generator=g))
    if h:
        where = torch.randperm(N, device=dev, generator=g)[:GROUPS * h].reshape(GROUPS, h)
        for s in range(GROUPS):
            u = unit(torch.randn((h, D), device=dev, generator=g))
            d2 = torch.linspace(1.0, 20.0, h, device=dev).unsqueeze(1)
            rows[where[s]] = ctr[s] + torch.sqrt(d2) * u
    return rows, q


out = {"config": {"rows": N, "dim": D, "metric": "L2", "nlist": NLIST, "nprobe": NPROBE, "radius": RADIUS, "max_per_query": M,
                  "topk_k": K, "groups": GROUPS, "warmup": WARM, "reps": REPS, "rounds": ROUNDS,
                  "alternation": "ivf_range, ivf_topk, flat_range per round"}}
for h in (0, 10, 1000):
    rows, q_all = store(h)
    ivf = R.HipIVFFlatIndex(D, NLIST, 0)
    ivf.train(rows[:50_000])
    ivf.add(rows)
    ivf.nprobe = NPROBE
    flat = R.HipFlatIndex(D, _lib.METRIC_L2, 0)
    flat.add_device(rows)
    del rows
    # the grouped queries, and on the store without planted rows also UNSTRUCTURED ones (noise like the rows: every query probes lists
    # of its own, the workload of tools/bench_ivf.py; no row is within the radius of any of them)
    sets = [("", q_all)]
    if h == 0:
        sets.append(("_unstructured", torch.randn((max(NQS), D), device=dev, generator=torch.Generator(device=dev).manual_seed(77))))
    for tag, nq in [(tag, nq) for tag, _ in sets for nq in NQS]:
        q = dict(sets)[tag][:nq].contiguous()
        legs = {"ivf_range": lambda: ivf.range_search_probed_device(q, RADIUS, M),
                "ivf_topk": lambda: ivf.search_device(q, K),
                "flat_range": lambda: flat.range_search_device(q, RADIUS, M)}
        for _ in range(WARM):
            for fn in legs.values():
                fn()
        t = {name: [] for name in legs}
        last = {}
        for _ in range(ROUNDS):
            for name, fn in legs.items():
                ms, last[name] = window(fn, REPS)
                t[name].append(round(ms, 4))
        legs["ivf_range"]()
        info = ivf.last_range()
        legs["ivf_topk"]()
        topk_info = ivf.last_search_info()
        flat_info = flat.last_range()
        c_ivf, c_flat = last["ivf_range"][0], last["flat_range"][0]
        assert int(c_flat.min()) == h and int(c_flat.max()) == h, (h, int(c_flat.min()), int(c_flat.max()))
        assert bool((c_ivf <= c_flat).all())
        med = {name: statistics.median(v) for name, v in t.items()}
        out[f"hits_{h}_nq_{nq}{tag}"] = {
            "ivf_range": {"search_ms": round(med["ivf_range"], 4), "rounds": t["ivf_range"], **info,
                          "count_min": int(c_ivf.min()), "count_max": int(c_ivf.max()),
                          "over_ivf_topk": round(med["ivf_range"] / med["ivf_topk"], 3)},
            "ivf_topk": {"search_ms": round(med["ivf_topk"], 4), "rounds": t["ivf_topk"], **topk_info},
            "flat_range": {"search_ms": round(med["flat_range"], 4), "rounds": t["flat_range"], **flat_info}}
    del ivf, flat, q_all
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT + ".json", "w") as f:
        f.write(line + "\n")
    with open(OUT + ".md", "w") as f:
        c = out["config"]
        f.write(f"| members | nq | ivf_range ms (rounds) | route | exact | max_emitted | counts | ivf_topk k={K} ms (rounds) | flat_range ms (rounds) | flat route |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        for h, tag in ((0, ""), (10, ""), (1000, ""), (0, "_unstructured")):
            for nq in NQS:
                e = out[f"hits_{h}_nq_{nq}{tag}"]
                a, b, cc = e["ivf_range"], e["ivf_topk"], e["flat_range"]
                f.write(f"| {h}{tag.replace('_', ' ')} | {nq} | {a['search_ms']} ({', '.join(str(x) for x in a['rounds'])}) | {a['route']} | {a['exact']} | {a['max_emitted']} | "
                        f"{a['count_min']}..{a['count_max']} | {b['search_ms']} ({', '.join(str(x) for x in b['rounds'])}) | "
                        f"{cc['search_ms']} ({', '.join(str(x) for x in cc['rounds'])}) | {cc['route']} |\n")
        f.write(f"\n{c['rows']} x {c['dim']} rows, nlist {c['nlist']}, nprobe {c['nprobe']}, radius {c['radius']}, M {c['max_per_query']}; "
                f"{c['reps']} calls per window after {c['warmup']} warm-up calls, {c['rounds']} rounds, legs alternated within a round.\n")
