#!/usr/bin/env python3
"""Removing rows from a flat store in place (HipFlatIndex.remove_ids) against the only alternative there was: a new handle plus
radad_knn_add of the kept rows from device memory.  1 M x 512 fp32 cosine store; 0.1 % / 10 % / 50 % of the rows go, scattered over
the store or as one run in its middle.  Each point is measured --rounds times, the two ways alternating on one box, every time on a
freshly filled and warmed store.  For both ways the first search afterwards (256 queries, k = 10) is measured too: that is where the
f16 plane is brought up to date (in place: from the first removed row on; a new handle: decided and built from scratch), and a second
search for the steady state.

    python tools/bench_remove.py [--rows 1000000] [--dim 512] [--rounds 3] [--json out.json] [--md out.md]

Times are wall-clock milliseconds around synchronised calls.  moved_GB is what the plan's launches read + write (a staged row twice);
GBps = moved_GB / the in-place time, which also holds the mark, the scan and two read-backs."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
ap.add_argument("--md", default=None)
args = ap.parse_args()
N, D = args.rows, args.dim
dev = torch.device("cuda:0")
lib = _lib.load()
rows = torch.empty((N, D), device=dev)
_lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, N, D, 4321, 0, _lib.stream_ptr(dev)))
q = torch.empty((256, D), device=dev)
_lib.check(lib.radad_synth_rows(q.data_ptr(), 0, 256, D, 977, 0, _lib.stream_ptr(dev)))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def full_store():
    idx = R.HipFlatIndex(D, _lib.METRIC_COSINE, device=0)
    idx.add_device(rows)
    idx.search_device(q, 10)          # builds the plane
    idx.search_device(q, 10)
    return idx


def ids_of(fraction, layout):
    m = max(1, int(round(N * fraction)))
    if layout == "run":
        return torch.arange(N // 2 - m // 2, N // 2 - m // 2 + m, device=dev)
    g = torch.Generator(device="cpu").manual_seed(int(fraction * 1e6) + 5)
    return torch.randperm(N, generator=g)[:m].to(dev)


points = []
for fraction in (0.001, 0.1, 0.5):
    for layout in ("scattered", "run"):
        ids = ids_of(fraction, layout)
        keep = torch.ones(N, dtype=torch.bool, device=dev)
        keep[ids] = False
        keep_ids = torch.nonzero(keep).reshape(-1)
        rec = {"fraction": fraction, "layout": layout, "removed": int(ids.numel()), "rounds": []}
        for rnd in range(args.rounds):
            r = {}
            # in place
            a = full_store()
            r["inplace_ms"], removed = timed(lambda: a.remove_ids(ids))
            assert removed == ids.numel() and a.ntotal == N - removed
            last = a.last_remove()
            r["launches"], r["moved_GB"] = last["launches"], last["bytes_moved"] / 1e9
            r["inplace_first_search_ms"], (da, ia) = timed(lambda: a.search_device(q, 10))
            r["inplace_second_search_ms"], _ = timed(lambda: a.search_device(q, 10))
            r["inplace_plane_rebuilds"] = a.plane_info()["rebuilds"]
            # a new handle + add of the kept rows
            old = full_store()            # (the store the audit ran on stays alive while the new one is filled)
            r["gather_ms"], kept_rows = timed(lambda: old.reconstruct_batch(keep_ids))

            def rebuild():
                b = R.HipFlatIndex(D, _lib.METRIC_COSINE, device=0)
                b.reserve(N - removed)
                b.add_device(kept_rows)
                return b
            r["rebuild_add_ms"], b = timed(rebuild)
            r["rebuild_first_search_ms"], (db, ib) = timed(lambda: b.search_device(q, 10))
            r["rebuild_second_search_ms"], _ = timed(lambda: b.search_device(q, 10))
            # the two stores hold the same rows (the new handle normalises the already normalised rows again: a few ulp), so the
            # two searches may order a near-tie differently; what must hold bit for bit is the in-place store against the gathered rows
            r["rows_equal"] = bool(torch.equal(a.reconstruct_batch(torch.arange(a.ntotal, device=dev)), kept_rows))
            r["same_ids"] = bool(torch.equal(ia, ib))
            r["queries_differing"] = int((ia != ib).any(dim=1).sum())
            r["max_score_difference"] = float((da - db).abs().max())
            del a, b, old, kept_rows
            rec["rounds"].append(r)
            print(json.dumps({"fraction": fraction, "layout": layout, "round": rnd, **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}}), flush=True)
        points.append(rec)

keys = ("inplace_ms", "inplace_first_search_ms", "inplace_second_search_ms", "gather_ms", "rebuild_add_ms", "rebuild_first_search_ms",
        "rebuild_second_search_ms")
lines = ["| removed | layout | launches | moved GB | in place ms | GB/s | + first search | second search | gather ms | new handle + add ms | + first search | second search | rows equal | queries ordered differently |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
for rec in points:
    med = {k: sorted(r[k] for r in rec["rounds"])[len(rec["rounds"]) // 2] for k in keys}
    r0 = rec["rounds"][0]
    rec["median"] = med
    lines.append(f"| {rec['fraction'] * 100:g} % | {rec['layout']} | {r0['launches']} | {r0['moved_GB']:.3f} | {med['inplace_ms']:.2f} | "
                 f"{r0['moved_GB'] / (med['inplace_ms'] / 1e3):.0f} | {med['inplace_first_search_ms']:.2f} | {med['inplace_second_search_ms']:.2f} | "
                 f"{med['gather_ms']:.2f} | {med['rebuild_add_ms']:.2f} | {med['rebuild_first_search_ms']:.2f} | {med['rebuild_second_search_ms']:.2f} | "
                 f"{all(r['rows_equal'] for r in rec['rounds'])} | {max(r['queries_differing'] for r in rec['rounds'])} |")
table = "\n".join(lines)
print(table)
if args.json:
    with open(args.json, "w") as f:
        json.dump({"rows": N, "dim": D, "rounds": args.rounds, "points": points}, f, indent=1)
if args.md:
    with open(args.md, "w") as f:
        f.write(table + "\n")
