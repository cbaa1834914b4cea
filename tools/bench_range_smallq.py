#!/usr/bin/env python3
"""Certified range search of a small batch (RADAD_KNN_OPT_RANGE_SMALLQ, route "stream") at the benchmark scale: 1 M x 512, cosine,
threshold 0.9, max_per_query 128, nq = 1, 8 and 16.  One store per number of planted hits h in {0, 10, 1000}:
  rows      unstructured unit-variance noise (cosines of ~0.044 standard deviation with anything: nothing random comes near 0.9)
  queries   16 unit centres + noise of norm 0.05, one centre per query
  planted   h rows per centre at cosines 0.93 .. 0.99 with it, spread over the store: every query has h rows above the threshold
            (the exact counts are reported, and asserted to be h)
Legs per (h, nq), timed in ALTERNATION on the same handle in one process (round r: stream, exact, plain; wall clock around a
synchronised loop of REPS calls -- REPS_EXACT for the exact leg -- after WARM warm-up calls each; the median of ROUNDS rounds and every
round are reported):
  stream    HipFlatIndex.range_search_device with the option on; its route and n_exact (last_range), the rows the scan emitted per
            query, and from one profiled call the milliseconds of its one scan launch (k_range_hi_smallq) and of its re-rank
  exact     the same call with the option off (radad_knn_set_option on the same handle): the float64 exact range kernel for every query
  plain     HipFlatIndex.search_device at k = 10 (k_knn_hi_smallq<16>): unchanged code, the yardstick; its scan launch from one
            profiled call
The three legs must return the same counts (stream, exact) and the same nearest ids.  Prints one JSON line.
tools/bench_range_smallq.py [rows] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
D, K, M, THRESH, CENTRES, WARM, REPS, REPS_EXACT, ROUNDS = 512, 10, 128, 0.9, 16, 5, 500, 30, 3


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def store(h):
    """(rows [N, D], queries [CENTRES, D]) on the device"""
    g = torch.Generator(device=dev).manual_seed(3000 + h)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = unit(torch.randn((CENTRES, D), device=dev, generator=g))
    q = ctr + 0.05 * unit(torch.randn((CENTRES, D), device=dev, generator=g))
    if h:
        where = torch.randperm(N, device=dev, generator=g)[:CENTRES * h].reshape(CENTRES, h)
        for s in range(CENTRES):
            u = torch.randn((h, D), device=dev, generator=g)
            u = unit(u - (u @ ctr[s]).unsqueeze(1) * ctr[s])
            c = torch.linspace(0.93, 0.99, h, device=dev).unsqueeze(1)
            rows[where[s]] = c * ctr[s] + torch.sqrt(1 - c * c) * u
    return rows, q


def profiled(idx, fn):
    idx.profile(True)
    fn()
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    return prof


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "threshold": THRESH, "max_per_query": M, "plain_k": K, "warmup": WARM,
                  "reps": REPS, "reps_exact": REPS_EXACT, "rounds": ROUNDS, "alternation": "stream, exact, plain per round"}}
for h in (0, 10, 1000):
    rows, q_all = store(h)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows

    def option(v):
        _lib.check(idx._lib.radad_knn_set_option(idx._h, _lib.KNN_OPT_RANGE_SMALLQ, v), "radad_knn_set_option")
    for nq in (1, 8, 16):
        q = q_all[:nq].contiguous()

        def stream():
            option(1)
            return idx.range_search_device(q, THRESH, M)

        def exact():
            option(0)
            return idx.range_search_device(q, THRESH, M)
        plain = lambda: idx.search_device(q, K)                                                 # noqa: E731
        for _ in range(WARM):
            stream(); exact(); plain()
        t_s, t_x, t_p = [], [], []
        for _ in range(ROUNDS):
            ms, (counts, Dr, Ir) = window(stream, REPS)
            t_s.append(round(ms, 4))
            ms, (cx, Dx, Ix) = window(exact, REPS_EXACT)
            t_x.append(round(ms, 4))
            ms, (D0, I0) = window(plain, REPS)
            t_p.append(round(ms, 4))
        launch = idx.last_launch()
        exact()
        info_x = idx.last_range()
        stream()
        info = idx.last_range()
        emitted, floors = idx.last_emitted(nq)
        splits = idx.last_launch()["db_splits"]
        prof = profiled(idx, stream)
        prof_plain = profiled(idx, plain)
        assert int(counts.min()) == h and int(counts.max()) == h, (h, int(counts.min()), int(counts.max()))
        assert torch.equal(counts, cx) and torch.equal(Ir, Ix), "stream and exact routes differ"
        assert info["route"] == "stream" and info_x["route"] == "exact" and len(prof) == 2, (info, info_x, prof)
        n = min(h, K)
        assert torch.equal(Ir[:, :n], I0[:, :n])                                                # the nearest hits are the plain search's nearest
        med = statistics.median
        out[f"hits_{h}_nq_{nq}"] = {
            "stream": {"search_ms": round(med(t_s), 4), "rounds": t_s, **info, "scan_ms": round(prof[0], 4), "rerank_ms": round(prof[1], 4),
                       "workgroups": splits, "emitted_mean": round(float(emitted.mean()), 1), "emitted_max": int(emitted.max()),
                       "eps_max": float(THRESH - floors.min()), "over_exact": round(med(t_s) / med(t_x), 3),
                       "over_plain": round(med(t_s) / med(t_p), 3)},
            "exact": {"search_ms": round(med(t_x), 4), "rounds": t_x, **info_x},
            "plain": {"search_ms": round(med(t_p), 4), "rounds": t_p, "scan_kind": launch["scan_kind"],
                      "scan_ms": round(prof_plain[0], 4) if prof_plain else None, "rechecked": launch["rechecked_queries"]}}
    del idx, q_all
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
