#!/usr/bin/env python3
"""IVF-flat (the reference's optional index type, vector_database.py:65-70,174-181) at the benchmark scale: 1M x 512, nlist 4096,
nprobe 32 (config.py:76), k = 15.  Prints build times and, per batch size, the search time, recall@15 against the exact flat
search, the flat search's own time, and a roofline block: the bytes of the lists the batch touches (f16 plane rows + their scale /
bias, each list once) over the search time against HBM (8 TB/s).  "excl_ms": the exclusion-aware search (radad_ivf_search_excl, tags =
row ids) at the same shape with 0 % (a one-tag set no row carries: the filtered kernels run), 1 % and 95 % of the rows excluded.
"excl_pq_ms": one exclusion set per query (radad_ivf_search_excl_pq) in three cases -- "loo_m1": every query excludes the one stored row
it was drawn from (tags = row ids); "none_m64": 64 tags per query that no row carries; "speaker_m1": tags = row id % 100, every query
excludes the tag of its source row, carried by 1 % of the rows (the per-(row, query) branch runs often) -- each beside "union_ms", the
batch-wide radad_ivf_search_excl with the UNION of the batch's sets: another question, the same rows streamed.
tools/bench_ivf.py [nq,nq,...] [hi_scan 0|1]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
lib = _lib.load()
dev = torch.device("cuda:0")
N, D, K, NLIST, NPROBE = 1_000_000, 512, 15, 4096, 32
NQS = tuple(int(x) for x in sys.argv[1].split(",")) if len(sys.argv) > 1 else (1, 256, 1024)
HI = int(sys.argv[2]) if len(sys.argv) > 2 else None
# clustered store: 2000 gaussian blobs (uniform random data would make any IVF useless)
cent = torch.empty((2000, D), device=dev)
_lib.check(lib.radad_synth_rows(cent.data_ptr(), 0, 2000, D, 11, 0, _lib.stream_ptr(dev)))
rows = torch.empty((N, D), device=dev)
_lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, N, D, 4321, 0, _lib.stream_ptr(dev)))
rows += 3.0 * cent[(torch.arange(N, device=dev) * 7919) % 2000]
out = {"config": {"rows": N, "dim": D, "k": K, "nlist": NLIST, "nprobe": NPROBE}}
idx = R.HipIVFFlatIndex(D, NLIST, 0, hi_scan=HI)
t0 = time.perf_counter(); idx.train(rows[:50000]); torch.cuda.synchronize(); out["train_s"] = round(time.perf_counter() - t0, 3)
t0 = time.perf_counter(); idx.add(rows); torch.cuda.synchronize(); out["add_s"] = round(time.perf_counter() - t0, 3)
flat = R.HipFlatIndex(D, _lib.METRIC_L2, 0); flat.add_device(rows)
idx.nprobe = NPROBE
assign = torch.from_numpy(idx.assignments()).to(dev)
list_rows = torch.bincount(assign.long(), minlength=NLIST)
centroids = torch.from_numpy(idx.centroids()).to(dev)
tags = torch.arange(N, device=dev, dtype=torch.int64)
perm = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
EXCL = {"0pct": torch.tensor([N + 7], device=dev, dtype=torch.int64), "1pct": torch.sort(perm[:N // 100]).values,
        "95pct": torch.sort(perm[:N * 95 // 100]).values}


def timed(fn, reps=20):
    for _ in range(3):
        r = fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


for nq in NQS:
    q = rows[(torch.arange(nq, device=dev) * 977 + 5) % N] + 0.5 * torch.randn((nq, D), device=dev)
    ms, (Di, Ii) = timed(lambda: idx.search_device(q, K))
    info = idx.last_search_info()
    ms_flat, (De, Ie) = timed(lambda: flat.search_device(q, K))
    excl_ms = {}
    for name, ex in EXCL.items():
        ms_x, (Dx, Ix) = timed(lambda: idx.search_probed_excluding(q, K, tags, ex))
        xi = idx.last_search_info()
        assert not torch.isin(Ix[Ix >= 0], ex).any()
        if name == "0pct":
            assert torch.equal(Ix, Ii)
        excl_ms[name] = {"search_ms": round(ms_x, 4), "over_plain": round(ms_x / ms, 3), "rejected": xi["rejected"], "filled": round(float((Ix >= 0).float().mean()), 4)}
    src = (torch.arange(nq, device=dev) * 977 + 5) % N           # the row every query was drawn from
    spk = tags % 100
    PQ = {"loo_m1": (tags, src.reshape(-1, 1)), "none_m64": (tags, N + 1 + torch.arange(nq * 64, device=dev).reshape(nq, 64)),
          "speaker_m1": (spk, spk[src].reshape(-1, 1))}
    excl_pq_ms = {}
    for name, (rt, qt) in PQ.items():
        ms_p, (Dp, Ip) = timed(lambda: idx.search_probed_excluding_per_query(q, K, rt, qt))
        pi = idx.last_search_info()
        union = torch.unique(qt)
        ms_u, _ = timed(lambda: idx.search_probed_excluding(q, K, rt, union))
        hit = (rt[Ip.clamp(min=0)].unsqueeze(2) == qt.unsqueeze(1)).any(2) & (Ip >= 0)
        assert not hit.any()
        if name == "none_m64":
            assert torch.equal(Ip, Ii)
        excl_pq_ms[name] = {"search_ms": round(ms_p, 4), "union_ms": round(ms_u, 4), "over_union": round(ms_p / ms_u, 3), "over_plain": round(ms_p / ms, 3),
                            "rejected": pi["rejected"], "filled": round(float((Ip >= 0).float().mean()), 4)}
    rec = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(Ii.cpu().tolist(), Ie.cpu().tolist())]))
    # the lists this batch probes (float64 centroid distances, as the oracle's ivf_search): each is streamed once per task of <= 16 queries
    d2 = torch.cdist(q.double(), centroids.double())
    probes = d2.topk(NPROBE, largest=False).indices
    touched = torch.unique(probes)
    per_list_q = torch.bincount(probes.flatten(), minlength=NLIST)
    tasks = int(((per_list_q + 15) // 16).sum().item())
    row_bytes = (2 if info["scan"] == "hi_lists" else 4) * D + 8
    alg = int(list_rows[touched].sum().item()) * row_bytes
    streamed = int((list_rows * ((per_list_q + 15) // 16)).sum().item()) * row_bytes
    out[f"nq{nq}"] = {"search_ms": round(ms, 4), "flat_search_ms": round(ms_flat, 4), "recall_at_15_vs_flat": round(rec, 4), **info, "excl_ms": excl_ms, "excl_pq_ms": excl_pq_ms,
                      "lists_touched": int(touched.numel()), "tasks": tasks,
                      "roofline": {"bound": "hbm", "algorithmic_bytes": alg, "streamed_bytes": streamed, "achieved": round(alg / (ms * 1e-3) / 1e9, 1),
                                   "peak": 8000.0, "unit": "GB/s", "frac": round(alg / (ms * 1e-3) / 1e9 / 8000.0, 4),
                                   "note": "whole search (coarse + grouping + list scan + re-rank) over the bytes of the touched lists"}}
print(json.dumps(out))
