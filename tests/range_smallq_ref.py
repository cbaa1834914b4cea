"""The designed stores of tests/test_gpu_knn_range_smallq.py -- the certified range search of a batch of 16 or fewer queries
(RADAD_RANGE_STREAM, k_range_hi_smallq) -- built from range_ref.graded and checked on the CPU by tests/test_range_smallq_model.py.
The reference is range_ref.expected_range (one set: range_excl_ref.expected_range_excl); nothing new is computed here.

The "knife" stores plant rows 1e-5 (cosine) / 2e-5 (squared distance) inside and outside the threshold: far inside the scan's eps, so
the scan emits both and only the float64 re-rank tells them apart -- every one inside must come back, none outside.

Every store has range_ref.N_ROWS = 16 677 rows: 131 waves' slices of 128 rows (waves change at multiples of 128, workgroups at
multiples of 512), the last workgroup's fourth wave starts beyond the store, and the last 16-row step holds 5 rows."""
import numpy as np

import range_ref as R

KNIFE_IN = (0.99, 0.9001, 0.90001, 0.95)
KNIFE_OUT = (0.89999, 0.8999)
ROWS_PER_WAVE = 128                      # the stream's slice at these stores (knn_sq_stream_geometry: 128 KB of f16 rows, at most 128 rows)


def case(name):
    """-> range_ref.case's dict: metric, db, q, radius, M, kind, info, overflow (queries meant to overflow their buffer), and
    counts: the rows planted within the radius of each query"""
    c = dict(name=name, M=64, route="stream", overflow=np.zeros(0, np.int64), kind="uncentred")
    if name in ("knife_cos16", "knife_f16", "knife_bf16"):
        db, q, info = R.graded("COSINE", nq=16, dim=64, seed=8100, in_levels=KNIFE_IN, out_levels=KNIFE_OUT)
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, counts=[R.COUNTS[j % 4] for j in range(16)],
                 kind="f16" if name == "knife_f16" else "uncentred")
    elif name == "knife_l2":
        db, q, info = R.graded("L2", nq=3, dim=576, seed=8110, counts=(5, 40, 1), in_levels=KNIFE_IN, out_levels=KNIFE_OUT)
        c.update(metric="L2", db=db, q=q, radius=0.2, info=info, counts=[5, 40, 1])       # squared distance 2 - 2 cos: 0.2 <-> 0.9
    elif name == "ip1":
        db, q, info = R.graded("IP", nq=1, dim=128, seed=8120, counts=(40,))
        c.update(metric="IP", db=db, q=q, radius=0.9, info=info, counts=[40])
    elif name == "centred16":
        db, q, info = R.graded("COSINE", nq=16, seed=8130, common=0.3, in_levels=(0.999, 0.995, 0.99, 0.985), out_levels=(0.975, 0.97))
        c.update(metric="COSINE", db=db, q=q, radius=0.98, info=info, kind="centred", counts=[R.COUNTS[j % 4] for j in range(16)])
    elif name == "many9":
        db, q, info = R.graded("COSINE", nq=9, seed=8150, many=(0, 300))
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, counts=[300] + [R.COUNTS[j % 4] for j in range(1, 9)])
    elif name == "crowd5":
        db, q, info = R.graded("COSINE", nq=5, seed=8140, counts=(0, 1, 5, 12), crowds=(0,))
        c.update(metric="COSINE", db=db, q=q, radius=0.9, info=info, counts=[5000, 1, 5, 12, 0], overflow=np.array([0]))
    else:
        raise KeyError(name)
    if name == "knife_bf16":
        import torch
        c["q"] = torch.from_numpy(c["q"]).to(torch.bfloat16).float().numpy()          # what a bfloat16 tensor of these queries holds
    return c


MODEL_CASES = ("knife_cos16", "knife_l2", "ip1", "centred16", "many9", "crowd5")
CASES = MODEL_CASES + ("knife_f16", "knife_bf16")

BOUNDARY_ROWS = (0, 15, 16, 127, 128, 511, 512, R.N_ROWS - 6, R.N_ROWS - 1)


def with_boundary_copies(c, query=3):
    """a copy of the case whose rows BOUNDARY_ROWS hold copies of one planted in-row of `query`: the first and last row of a 16-row
    step, of a wave's slice, of a workgroup's, the last row of the last full step and the last row of the last, 5-row step -> (case, the copied row)"""
    src = int(c["info"]["planted_in"][query][0])
    assert src not in BOUNDARY_ROWS
    d = dict(c)
    d["db"] = c["db"].copy()
    d["db"][list(BOUNDARY_ROWS)] = c["db"][src]
    return d, src


def tags_by_query(c):
    """row tags for the per-query sets: 1_000_000 + row, except that every second planted in-row of query j carries 10 + j"""
    row_tags = 1_000_000 + np.arange(len(c["db"]), dtype=np.int64)
    for j, rows in c["info"]["planted_in"].items():
        row_tags[np.asarray(rows, np.int64)[0::2]] = 10 + j
    return row_tags


ABSENT = 5_000_000_000                   # tags no row carries
CLASS_OF_QUERY_3 = 777


def tags_by_class(c):
    """row tags for one set for the batch: ten classes, row % 10, and every planted in-row of query 3 in a class of its own"""
    row_tags = np.arange(len(c["db"]), dtype=np.int64) % 10
    row_tags[np.asarray(c["info"]["planted_in"][3], np.int64)] = CLASS_OF_QUERY_3
    return row_tags


def class_set(n_classes):
    """an ascending set: the first n_classes of the ten classes (a tenth of the rows each) and query 3's"""
    return np.array(list(range(n_classes)) + [CLASS_OF_QUERY_3], np.int64)


def query_tags(nq, m):
    """[nq, m]: query j lists 10 + j in slot j % m and tags no row carries in the others"""
    q_tags = ABSENT + np.arange(nq * m, dtype=np.int64).reshape(nq, m)
    for j in range(nq):
        q_tags[j, j % m] = 10 + j
    return q_tags
