"""Dry run of the tile scan's early abandon: on a bench-shaped search -- the 1 M x 512 store and the 1024 embedded
queries exactly as bench.py builds them -- read the admission floors the scan ran with (radad_knn_last_emitted) and count, on the
host side of the API (torch on the device, from the recomputed f16 operands), the (query tile, row tile) tasks the abandon test
would skip after c = 1, 2, 3 K-stages of 64 elements.  Nothing here runs the abandoning kernel: it is the estimate that is
compared with the kernel's own counters afterwards.

usage: python tools/abandon_dryrun.py [out.txt]     (default profiles/abandon_dryrun.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib

B, CLIP, N, DIM, K = 1024, 64000, 1_000_000, 512, 10
KW = 256
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
planted = torch.zeros(N, dtype=torch.bool, device=dev)
for c, e in ((0, 0.05), (1, 0.10)):
    g = (jj * 977 + c * 350003 + 17) % N
    rows[g] = emb + e * scale * noise[c * B:(c + 1) * B]
    planted[g] = True
vdb = R.VectorDatabase(cfg)
vdb.create_index(DIM)
vdb.index.reserve(N)
vdb.index.add_device(rows)
del noise, rows
for _ in range(2):
    D, I = vdb.index.search_device(emb, K)
launch = vdb.index.last_launch()
counts, floors = vdb.index.last_emitted(B)
floors_t = torch.from_numpy(floors).to(dev)

# the operands as the scan multiplies them: rows as stored (unit norm) x 2^14 -> f16; queries normalised, x 2^eq with the row
# maximum in [2^13, 2^14) -> f16.  Accumulator units: a = qh . yh = q.y 2^(14 + eq), so the floor is thr = floor 2^(14 + eq).
qn = torch.empty_like(emb)
_lib.check(lib.radad_rownorm(emb.contiguous().data_ptr(), qn.data_ptr(), B, DIM, 0, sp))
eq = 14 - torch.frexp(qn.abs().amax(dim=1))[1]
qh = (qn * torch.ldexp(torch.ones_like(qn[:, :1]), eq[:, None])).half().float()
thr_final = floors_t * torch.ldexp(torch.ones(B, device=dev), eq + 14)
n_tiles = (N + KW - 1) // KW
infl = 1.0 + 2.0 ** -10
qnorm = qh.norm(dim=1)

# the first phase runs with the sample's floor: the (k + 6)-th best score over the sample's tiles (every (tiles / 64)-th), lowered by
# 2 eps.  Estimated here from the same rows (eps ~ 2e-3 at this shape, taken as 4e-3 in all: the estimate errs low).
stride = max(1, (N // KW) // 64) * KW
samp = torch.cat([torch.arange(t * stride, t * stride + KW, device=dev) for t in range(64)])
ys = vdb.index.reconstruct_batch(samp)
floor_sample = (qn @ ys.T).topk(K + 6, dim=1).values[:, -1] - 4e-3
thr_sample = floor_sample * torch.ldexp(torch.ones(B, device=dev), eq + 14)

res = {}
ymax = 0.0
pad =torch.zeros(n_tiles * KW, dtype=torch.bool, device=dev)
pad[:N] = planted
tile_has_planted = pad.view(n_tiles, KW).any(dim=1)
CH = 128                                  # row tiles per pass
margins = {c: [] for c in (1, 2, 3)}
skip = {(c, w): 0 for c in (1, 2, 3) for w in ("final", "sample")}
for t0 in range(0, n_tiles, CH):
    r0, r1 = t0 * KW, min(N, (t0 + CH) * KW)
    y = vdb.index.reconstruct_batch(torch.arange(r0, r1, device=dev))
    yh = (y * 16384.0).half().float()
    if r1 - r0 < CH * KW:
        yh = torch.cat([yh, torch.zeros((CH * KW - (r1 - r0), DIM), device=dev)])
    nt = (r1 - r0 + KW - 1) // KW
    ymax = max(ymax, float(yh.norm(dim=1).max()))
    for c in (1, 2, 3):
        e0 = 64 * c
        acc = yh[:, :e0] @ qh[:, :e0].T                                            # [rows, B]
        amax = acc.view(CH, KW, B).amax(dim=1)[:nt]                                # [tiles, B]
        ry = yh[:, e0:].norm(dim=1).view(CH, KW).amax(dim=1)[:nt] * infl
        rq = qh[:, e0:].norm(dim=1) * infl
        slack = 2.0 * DIM * 2.0 ** -23 * qnorm * (16384.0 * infl)                  # |yh| <= 2^14 (unit rows), no bias start
        bound = amax + ry[:, None] * rq[None, :] * infl + slack[None, :]
        for w, thr in (("final", thr_final), ("sample", thr_sample)):
            ok = (bound < thr[None, :]).view(nt, B // KW, KW).all(dim=2)           # [tiles, query tiles]
            skip[(c, w)] += int(ok.sum())
        m = ((thr_final[None, :] - bound) / thr_final[None, :])[~tile_has_planted[t0:t0 + nt]]
        if m.numel():
            margins[c].append(float(m.min()))
tasks = n_tiles * (B // KW)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "abandon_dryrun.txt")
lines = [
    "early abandon, dry run on the parent's scan (tools/abandon_dryrun.py): bench.py's store and queries, cosine top-10",
    "scan: %s, %d launches; certificate %s" % (launch["scan_kind"], launch["scan_launches"], launch["certificate"]),
    "floors of the last phase (radad_knn_last_emitted), true scale: min %.5f median %.5f max %.5f" % (floors.min(), np.median(floors), floors.max()),
    "floors of the first phase (host estimate: (k+6)-th best over the sample's 64 tiles - 4e-3): min %.5f median %.5f" % (float(floor_sample.min()), float(floor_sample.median())),
    "candidates emitted per query: mean %.1f max %d" % (counts.mean(), counts.max()),
    "row tiles %d, of which %d hold a planted row; query tiles %d; tile tasks %d" % (n_tiles, int(tile_has_planted.sum()), B // KW, tasks),
]
for c in (1, 2, 3):
    lines.append("c = %d: skippable fraction %.4f with the last phase's floors, %.4f with the first phase's; smallest relative margin over "
                 "tiles without a planted row %.4f" % (c, skip[(c, "final")] / tasks, skip[(c, "sample")] / tasks, min(margins[c]) if margins[c] else float("nan")))
text = "\n".join(lines) + "\n"
print(text, flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
