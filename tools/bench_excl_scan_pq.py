#!/usr/bin/env python3
"""Per-query exclusion sets on the certified tile scan (radad_knn_search_excl_scan_pq) at the benchmark scale: 1 M x 512, cosine,
k = 10, 1024 queries, leave-one-speaker-out.  One case per crowd size c in {0, 200, 1500}, each on a handle of its own:
  c = 0     the benchmark's unstructured rows and queries; nothing is excluded (m = 0)
  c > 0     every row belongs to a speaker of c rows (rows of a speaker = its centre + 0.3 x noise, spread over the store), query j is
            the centre of speaker j % speakers + 0.01 x noise and excludes that speaker's tag: c excluded rows crowd in front of
            every query's first admissible neighbour
Legs per case, timed in ALTERNATION (round r: plain, in_scan_pq, plain, in_scan_pq, ...; wall clock around a synchronised loop of
REPS calls after WARM warm-up calls each; the median of ROUNDS rounds and every round are reported):
  plain        HipFlatIndex.search_device on the same handle in the same run: unchanged code, the yardstick
  in_scan_pq   search_excluding_per_query_in_scan; its route and n_exact (last_excl_scan), scan phases and the emitted rows per query
  over_fetch   search_excluding_per_query at k_fetch = min(1024, k + c), timed after the alternation with as many calls as fit ~0.5 s
               (at least 2): its n_exact (last_excl); ids must equal in_scan_pq's
Prints one JSON line.  tools/bench_excl_scan_pq.py [rows] [queries] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
lib = _lib.load()
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OUT = sys.argv[3] if len(sys.argv) > 3 else None
D, K, WARM, REPS, ROUNDS = 512, 10, 5, 200, 5


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def store(c):
    """(rows [N, D], queries [NQ, D], row tags or None, query tags [NQ, 1] or None) on the device"""
    if c == 0:
        rows = torch.empty((N, D), device=dev)
        _lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, N, D, 4321, 0, _lib.stream_ptr(dev)))
        q = torch.empty((NQ, D), device=dev)
        _lib.check(lib.radad_synth_rows(q.data_ptr(), 0, NQ, D, 977, 0, _lib.stream_ptr(dev)))
        return rows, q, None, None
    g = torch.Generator(device=dev).manual_seed(1000 + c)
    n_spk = N // c
    spk = (torch.randperm(N, device=dev, generator=g) % n_spk).to(torch.int64)          # speakers of c (or c + 1) rows, spread over the store
    ctr = torch.randn((n_spk, D), device=dev, generator=g)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = ctr[spk[r0:r1]] + 0.3 * torch.randn((r1 - r0, D), device=dev, generator=g)
    qs = torch.arange(NQ, device=dev) % n_spk
    q = ctr[qs] + 0.01 * torch.randn((NQ, D), device=dev, generator=g)
    return rows, q, spk.contiguous(), qs.to(torch.int64).reshape(NQ, 1).contiguous()


out = {"config": {"rows": N, "dim": D, "metric": "cosine", "k": K, "queries": NQ, "warmup": WARM, "reps": REPS, "rounds": ROUNDS,
                  "alternation": "plain, in_scan_pq per round"}}
for c in (0, 200, 1500):
    rows, q, tags, qtags = store(c)
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, 0)
    idx.add_device(rows)
    del rows
    plain = lambda: idx.search_device(q, K)                                                     # noqa: E731
    in_scan = lambda: idx.search_excluding_per_query_in_scan(q, K, tags, qtags)                 # noqa: E731
    for _ in range(WARM):
        plain(); in_scan()
    t_plain, t_new = [], []
    for _ in range(ROUNDS):
        ms, (D0, I0) = window(plain, REPS)
        t_plain.append(round(ms, 4))
        ms, (Dn, In) = window(in_scan, REPS)
        t_new.append(round(ms, 4))
    info = idx.last_excl_scan()
    phases = idx.last_launch()["scan_phases"]
    emitted, _ = idx.last_emitted(NQ)
    plain()
    launch = idx.last_launch()
    case = {"plain": {"search_ms": round(statistics.median(t_plain), 4), "rounds": t_plain, "scan_kind": launch["scan_kind"],
                      "scan_phases": launch["scan_phases"], "rechecked": launch["rechecked_queries"]},
            "in_scan_pq": {"search_ms": round(statistics.median(t_new), 4), "rounds": t_new, **info, "scan_phases": phases,
                           "scrub_launches": (phases + 1) if c else 0, "emitted_mean": round(float(emitted.mean()), 1),
                           "emitted_max": int(emitted.max()),
                           "over_plain": round(statistics.median(t_new) / statistics.median(t_plain), 3)}}
    if c == 0:
        assert torch.equal(In, I0)
    else:
        assert (In >= 0).all() and not (tags[In] == qtags).any()
    kf = min(1024, K + c)
    over = lambda: idx.search_excluding_per_query(q, K, tags, qtags, k_fetch=kf)               # noqa: E731
    t1, (Do, Io) = window(over, 1)                                                              # (also its warm-up)
    reps = int(max(2, min(REPS, 500.0 / max(t1, 1e-3))))
    t_over = []
    for _ in range(3):
        ms, (Do, Io) = window(over, reps)
        t_over.append(round(ms, 4))
    assert torch.equal(Io, In)
    case["over_fetch"] = {"k_fetch": kf, "search_ms": round(statistics.median(t_over), 4), "rounds": t_over, "reps": reps, **idx.last_excl()}
    case["in_scan_pq"]["over_over_fetch"] = round(statistics.median(t_new) / statistics.median(t_over), 4)
    out[f"c_{c}"] = case
    del idx, q, tags, qtags
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
