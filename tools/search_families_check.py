#!/usr/bin/env python3
"""One call of each of the nine flat-store searches on every route a 20 480 x 64 store and 24 queries reach, for comparing two builds
of the library (RADAD_HIP_LIB selects the build, as tools/ab_lib.sh does): the plain search, the two two-pass exclusion searches, the
two in-scan exclusion searches and the three range searches, on the tile route (20 480 rows) and the exact route (2 048 rows), L2 and
inner product; and the three range searches of 16 queries on the stream route (RADAD_KNN_OPT_RANGE_SMALLQ on).

  search_families_check.py run [--out DIR]     the calls; with --out every call's outputs (distances, ids, float64 keys, counts) as raw
                                               bytes and its last_* read-backs as JSON
  search_families_check.py launches DIR        the ordered (kernel, grid, workgroup) list of a `rocprofv3 --kernel-trace
                                               --output-format csv -d DIR -- python3 tools/search_families_check.py run`
  search_families_check.py same A B            exit 0 when the files of directories A and B (or the files A and B) are equal byte for
                                               byte, else name the first that differs"""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NQ, DIM, N_TILE, N_EXACT = 24, 64, 20480, 2048


def _data(n, seed):
    """rows, queries and tags: queries 0 .. 5 have 30 near-copies each at the first 180 rows; four rows share a tag"""
    import numpy as np
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, DIM)).astype(np.float32)
    q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    for j in range(6):
        db[30 * j:30 * j + 30] = q[j] + np.float32(1e-3) * rng.standard_normal((30, DIM)).astype(np.float32)
    tags = (np.arange(n, dtype=np.int64) // 4) * 7 + 11
    excl = np.unique(tags[:180])
    qtags = np.stack([tags[rng.choice(n, 8, replace=False)] for _ in range(NQ)])
    for j in range(6):
        qtags[j] = np.unique(tags[30 * j:30 * j + 30])[:8]
    qcnt = (np.arange(NQ) % 9).astype(np.int32)
    qcnt[:6] = 8
    return db, q, tags, excl, qtags, qcnt


def run(out_dir):
    import numpy as np
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    gpu = torch.device("cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    log = {}

    def keep(name, idx, out):
        """the read-backs that describe this call: the last scan's, and its own family's"""
        torch.cuda.synchronize()
        own = idx.last_range if "range" in name else idx.last_excl_scan if "excl_scan" in name else idx.last_excl if "excl" in name else dict
        log[name] = dict(launch=idx.last_launch(), family=own())
        print(name, log[name]["family"], log[name]["launch"].get("scan_kind"))
        if out_dir:
            for i, t in enumerate(out):
                with open(os.path.join(out_dir, f"{name}.{i}.bin"), "wb") as f:
                    f.write(t.cpu().numpy().tobytes())

    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    for metric, radius in (("L2", 75.0), ("IP", 20.0)):
        m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP}[metric]
        for route, n, kw, nq in (("tile", N_TILE, {}, NQ), ("exact", N_EXACT, {}, NQ), ("stream", N_TILE, {"range_smallq": 1}, 16)):
            db, q, tags, excl, qtags, qcnt = (dev(a) for a in _data(n, 100 + n))
            q, qtags, qcnt = q[:nq].contiguous(), qtags[:nq].contiguous(), qcnt[:nq].contiguous()
            idx = HipFlatIndex(DIM, m, 0, 0, **kw)
            idx.add_device(db)
            tag = f"{metric}_{route}_"
            if route != "stream":
                keep(tag + "plain", idx, idx.search_device(q, 10, return_f64=True))
                keep(tag + "excl", idx, idx.search_excluding(q, 10, tags, excl, k_fetch=20, return_f64=True))
                keep(tag + "excl_pq", idx, idx.search_excluding_per_query(q, 10, tags, qtags, qcnt, k_fetch=20, return_f64=True))
                keep(tag + "excl_scan", idx, idx.search_excluding_in_scan(q, 10, tags, excl, return_f64=True))
                keep(tag + "excl_scan_pq", idx, idx.search_excluding_per_query_in_scan(q, 10, tags, qtags, qcnt, return_f64=True))
            keep(tag + "range", idx, idx.range_search_device(q, radius, 64, return_f64=True))
            keep(tag + "range_excl", idx, idx.range_search_excluding_device(q, radius, tags, excl, 64, return_f64=True))
            keep(tag + "range_excl_pq", idx, idx.range_search_excluding_per_query_device(q, radius, tags, qtags, qcnt, 64, return_f64=True))
            for name in ("range", "range_excl", "range_excl_pq") + (("excl_scan", "excl_scan_pq") if route != "stream" else ()):
                assert log[tag + name]["family"]["route"] == route, (tag + name, log[tag + name]["family"])
    if out_dir:
        with open(os.path.join(out_dir, "readbacks.json"), "w") as f:
            json.dump(log, f, indent=1, sort_keys=True, default=str)
    print("library", _lib.LIB_PATH)


def launches(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0) or 0)))
    for r in rows:
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        block = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        print(f'{r["Kernel_Name"]}\tgrid {grid}\tworkgroup {block}')


def same(a, b):
    pairs = [(a, b)] if os.path.isfile(a) else [(os.path.join(a, n), os.path.join(b, n)) for n in sorted(os.listdir(a))]
    if not os.path.isfile(a) and sorted(os.listdir(a)) != sorted(os.listdir(b)):
        print("different file lists")
        return 1
    bad = [x for x, y in pairs if open(x, "rb").read() != open(y, "rb").read()]
    for x in bad:
        print("DIFFERENT:", x)
    if not bad:
        print(f"equal byte for byte: {len(pairs)} file(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--out" else None)
    elif sys.argv[1] == "launches":
        launches(sys.argv[2])
    else:
        sys.exit(same(sys.argv[2], sys.argv[3]))
