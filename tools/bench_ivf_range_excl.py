#!/usr/bin/env python3
"""Certified range search among the rows a query does not exclude, over the probed lists (radad_ivf_range_search_excl / _excl_pq), at
the benchmark scale: 1 M x 512 (squared L2), nlist 4096, nprobe 32, max_per_query 128.  Stores as tools/bench_ivf_range.py plants them:
  rows      unstructured unit-variance noise (squared distances of ~1024 with anything: nothing random comes near the radius)
  queries   64 groups: query j = centre of group j % 64 + noise of norm 0.05
  planted   per group 10 rows of OTHER files at squared distances 1 .. 20 from the group's centre, and c rows of the group's own
            SPEAKER (one tag per group) at the same distances, c in {0, 200, 1500}: one store per c; radius 50
Every other row carries a tag of its own.  For each batch size nq in {1, 256, 1024} the legs run in ALTERNATION on one handle (round r:
plain, then the exclusion-aware call; wall clock around a synchronised loop of REPS calls after WARM warm-up calls each; the median of
ROUNDS rounds and every round are reported):
  speaker_c   one set PER QUERY: query j excludes its group's speaker tag (m = 1), on the store with c speaker rows per group
  batch_f     ONE set for the batch on the c = 0 store, the rows re-tagged id % 100 and the set = the tags below f, f in {0, 50, 90}:
              0 / 50 / 90 % of the rows excluded (f = 0 is the empty set: the plain kernels run)
The yardstick of every leg is the plain radad_ivf_range_search of the same queries on the same handle in the same round.  Nothing is
asserted about the times.  An IVF search sees the probed lists, so the counts are reported; asserted is what must hold whatever the
lists are: at most 10 admissible members per query on the speaker legs and no listed row of the own speaker, plain minus admissible
count at most c; on the batch legs exactly the plain search's members whose tag is not excluded.
Prints one JSON line and, with an output stem, writes <stem>.json and the table <stem>.md.
tools/bench_ivf_range_excl.py [rows] [out stem]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
D, M, RADIUS, GROUPS, NLIST, NPROBE, WARM, REPS, ROUNDS, OTHERS = 512, 128, 50.0, 64, 4096, 32, 5, 30, 3, 10
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


def store(c):
    """(rows [N, D], queries [1024, D], speaker tags [N]) on the device: 10 + c planted rows per group, the c under the group's tag"""
    g = torch.Generator(device=dev).manual_seed(4000 + c)
    rows = torch.empty((N, D), device=dev)
    for r0 in range(0, N, 1 << 17):
        r1 = min(N, r0 + (1 << 17))
        rows[r0:r1] = torch.randn((r1 - r0, D), device=dev, generator=g)
    ctr = torch.randn((GROUPS, D), device=dev, generator=g)
    q = ctr[torch.arange(max(NQS), device=dev) % GROUPS] + 0.05 * unit(torch.randn((max(NQS), D), device=dev, generator=g))
    tags = 10_000 + torch.arange(N, device=dev, dtype=torch.int64)
    h = OTHERS + c
    where = torch.randperm(N, device=dev, generator=g)[:GROUPS * h].reshape(GROUPS, h)
    for s in range(GROUPS):
        u = unit(torch.randn((h, D), device=dev, generator=g))
        d2 = torch.linspace(1.0, 20.0, h, device=dev)[torch.randperm(h, device=dev, generator=g)].unsqueeze(1)
        rows[where[s]] = ctr[s] + torch.sqrt(d2) * u
        tags[where[s, OTHERS:]] = s
    return rows, q, tags


def measure(ivf, q, excl_fn):
    legs = {"plain": lambda: ivf.range_search_probed_device(q, RADIUS, M), "excl": excl_fn}
    for _ in range(WARM):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    last, info = {}, {}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            ms, last[name] = window(fn, REPS)
            t[name].append(round(ms, 4))
    for name, fn in legs.items():
        fn()
        info[name] = ivf.last_range()
    med = {name: statistics.median(v) for name, v in t.items()}
    entry = {name: {"search_ms": round(med[name], 4), "rounds": t[name], **info[name], "count_min": int(last[name][0].min()),
                    "count_max": int(last[name][0].max())} for name in legs}
    entry["excl"]["over_plain"] = round(med["excl"] / med["plain"], 3)
    return entry, last


out = {"config": {"rows": N, "dim": D, "metric": "L2", "nlist": NLIST, "nprobe": NPROBE, "radius": RADIUS, "max_per_query": M,
                  "groups": GROUPS, "others_per_group": OTHERS, "warmup": WARM, "reps": REPS, "rounds": ROUNDS,
                  "alternation": "plain, excl per round"}}
for c in (0, 200, 1500):
    rows, q_all, spk_tags = store(c)
    ivf = R.HipIVFFlatIndex(D, NLIST, 0)
    ivf.train(rows[:50_000])
    ivf.add(rows)
    ivf.nprobe = NPROBE
    del rows
    q_spk = (torch.arange(max(NQS), device=dev, dtype=torch.int64) % GROUPS).reshape(-1, 1)
    for nq in NQS:
        q = q_all[:nq].contiguous()
        qt = q_spk[:nq].contiguous()
        entry, last = measure(ivf, q, lambda: ivf.range_search_probed_excluding_per_query_device(q, RADIUS, spk_tags, qt, None, M))
        # (an IVF search sees the probed lists: the counts are reported; what must hold whatever the lists are is asserted)
        pc, xc, xi = last["plain"][0], last["excl"][0], last["excl"][2]
        assert bool((xc <= OTHERS).all()) and bool((pc - xc <= c).all()) and bool((pc >= xc).all()), entry
        assert not bool((torch.isin(spk_tags[xi.clamp(min=0)], torch.arange(GROUPS, device=dev)) & (xi >= 0)).any())
        if c == 0:
            assert bool((pc == xc).all()), entry
        out[f"speaker_{c}_nq_{nq}"] = entry
    if c == 0:
        mod_tags = torch.arange(N, device=dev, dtype=torch.int64) % 100
        for f in (0, 50, 90):
            excl = torch.arange(f, device=dev, dtype=torch.int64)
            for nq in NQS:
                q = q_all[:nq].contiguous()
                entry, last = measure(ivf, q, lambda: ivf.range_search_probed_excluding_device(q, RADIUS, mod_tags, excl, M))
                ids = last["plain"][2][:, :OTHERS]
                want = ((mod_tags[ids.clamp(min=0)] >= f) & (ids >= 0)).sum(1).to(torch.int32)
                assert bool((last["excl"][0] == want).all()), entry
                out[f"batch_{f}_nq_{nq}"] = entry
    del ivf, q_all, spk_tags
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT + ".json", "w") as fh:
        fh.write(line + "\n")
    with open(OUT + ".md", "w") as fh:
        cfg = out["config"]
        fh.write("| leg | nq | excl ms (rounds) | plain ms (rounds) | excl / plain | excl route, exact, max_emitted, counts | plain route, exact, max_emitted, counts |\n")
        fh.write("|---|---|---|---|---|---|---|\n")
        for leg in [f"speaker_{c}" for c in (0, 200, 1500)] + [f"batch_{f}" for f in (0, 50, 90)]:
            for nq in NQS:
                e = out[f"{leg}_nq_{nq}"]
                a, b = e["excl"], e["plain"]
                fh.write(f"| {leg} | {nq} | {a['search_ms']} ({', '.join(str(x) for x in a['rounds'])}) | {b['search_ms']} ({', '.join(str(x) for x in b['rounds'])}) | "
                         f"{a['over_plain']} | {a['route']}, {a['exact']}, {a['max_emitted']}, {a['count_min']}..{a['count_max']} | "
                         f"{b['route']}, {b['exact']}, {b['max_emitted']}, {b['count_min']}..{b['count_max']} |\n")
        fh.write(f"\n{cfg['rows']} x {cfg['dim']} rows, nlist {cfg['nlist']}, nprobe {cfg['nprobe']}, radius {cfg['radius']}, M {cfg['max_per_query']}; "
                 f"{cfg['reps']} calls per window after {cfg['warmup']} warm-up calls, {cfg['rounds']} rounds, legs alternated within a round.\n")
