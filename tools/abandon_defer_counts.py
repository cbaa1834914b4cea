"""The deferral of a vetoed tile's few live rows (RADAD_KNN_OPT_ABANDON_DEFER) on a bench-shaped search -- the 1 M x 512 store and the
1024 embedded queries exactly as bench.py builds them: with the option off and on, the abandon's and the deferral's counters of one
search (how many of the vetoed tile tasks had 1 ... KNN_DEFER_MAX_ROWS live rows and left, how many rows they listed) and the scan's
event-timed launches of ten searches.  Asserts that both settings return the same ids, distances, counts and floors.

usage: python tools/abandon_defer_counts.py [out.txt]     (default: stdout only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib

B, CLIP, N, DIM, K = 1024, 64000, 1_000_000, 512, 10
dev = torch.device("cuda", 0)
lib = _lib.load()
sp = _lib.stream_ptr(dev)

cfg = R.Config()
cfg.update(device=dev, tpp_levels=[1], tpp_pooling_type="max", feature_dim=DIM, vector_db_index_type="IP")
fe = R.MelProjectionFeatureExtractor(cfg)
wave = torch.empty(B * CLIP, device=dev)
_lib.check(lib.radad_synth_audio(wave.data_ptr(), 0, B, CLIP, 1234, 0, sp))
emb = fe.embed_clips(wave, np.arange(B + 1, dtype=np.int64) * CLIP).float()
rows = torch.empty((N, DIM), device=dev)
_lib.check(lib.radad_synth_rows(rows.data_ptr(), 0, N, DIM, 4321, 0, sp))
noise = torch.empty((2 * B, DIM), device=dev)
_lib.check(lib.radad_synth_rows(noise.data_ptr(), 0, 2 * B, DIM, 99, 0, sp))
jj = torch.arange(B, device=dev)
scale = emb.norm(dim=1, keepdim=True) / (DIM ** 0.5)
for c, e in ((0, 0.05), (1, 0.10)):
    rows[(jj * 977 + c * 350003 + 17) % N] = emb + e * scale * noise[c * B:(c + 1) * B]
vdb = R.VectorDatabase(cfg)
vdb.create_index(DIM)
vdb.index.reserve(N)
vdb.index.add_device(rows)
del noise, rows
idx = vdb.index

out, seen = [], {}
for defer in (0, 1, 0, 1):
    idx.set_abandon_defer(defer)
    for _ in range(3):
        D, I = idx.search_device(emb, K)
    launch = idx.last_launch()
    counts, floors = idx.last_emitted(B)
    seen.setdefault(defer, (D.cpu().numpy(), I.cpu().numpy(), counts, floors))
    idx.profile(True)
    for _ in range(10):
        idx.search_device(emb, K)
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    n = launch["scan_launches"]
    per_search = sorted(sum(prof[i:i + n]) for i in range(0, len(prof) - n + 1, n))
    ab, df = launch["early_abandon"], launch["abandon_defer"]
    vetoed = ab["checked"] - ab["skipped"]
    out.append({"defer": defer, "scan_launches": n, "scan_ms_min": round(per_search[0], 4), "scan_ms_median": round(per_search[len(per_search) // 2], 4),
                "early_abandon": ab, "abandon_defer": df, "vetoed": vetoed,
                "deferred_of_vetoed": round(df["tile_tasks_deferred"] / max(1, vetoed), 4),
                "rows_per_deferred_task": round(df["rows_listed"] / max(1, df["tile_tasks_deferred"]), 3)})
    print(json.dumps(out[-1]), flush=True)
for a, b in zip(seen[0], seen[1]):
    assert np.array_equal(a, b), "the option changed a result"
print("ids, distances, emitted counts and floors: array_equal with the option off and on")
# unstructured queries never open the gate: what the (empty) tail launches cost them
rnd = torch.empty((B, DIM), device=dev)
_lib.check(lib.radad_synth_rows(rnd.data_ptr(), 0, B, DIM, 777, 0, sp))
for defer in (0, 1, 0, 1):
    idx.set_abandon_defer(defer)
    for _ in range(3):
        idx.search_device(rnd, K)
    launch = idx.last_launch()
    idx.profile(True)
    for _ in range(10):
        idx.search_device(rnd, K)
    torch.cuda.synchronize()
    prof = idx.profile_read()
    idx.profile(False)
    n = launch["scan_launches"]
    per_search = sorted(sum(prof[i:i + n]) for i in range(0, len(prof) - n + 1, n))
    out.append({"unstructured": True, "defer": defer, "scan_ms_min": round(per_search[0], 4), "scan_ms_median": round(per_search[len(per_search) // 2], 4),
                "early_abandon": launch["early_abandon"], "abandon_defer": launch["abandon_defer"]})
    print(json.dumps(out[-1]), flush=True)
idx.set_abandon_defer(1)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        for o in out:
            f.write(json.dumps(o) + "\n")
