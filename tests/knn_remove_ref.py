"""numpy model of radad_knn_remove_ids: what a removal leaves (keep mask, old -> new id map) and the plan of its moves
(csrc/knn_plan.h, knn_remove_plan), written from the description, not from the C++ text:

  - the store is walked in slabs of S rows from the slab that holds the first removed row r0;
  - a slab with at least S removed rows in front of it is DIRECT (its kept rows land wholly below its own first row); consecutive
    direct slabs share a launch while the launch's span stays within the rows removed in front of its first row;
  - any other slab is STAGED: gathered into a buffer of S rows, then copied to its destination by the next launch.  The first slab's
    rows in front of r0 do not move.
"""
import numpy as np

MIN_STAGE_ROWS = 64
STAGE_BYTES = 64 << 20
SCAN_ROWS = 2048
GATHER, SCATTER, DIRECT = 0, 1, 2
PATTERNS = ("none", "first", "last", "mid_slab", "boundary", "every_other", "run", "all_but_one", "all", "random30")


def stage_rows(row_bytes: int, opt: int = 0) -> int:
    return max(MIN_STAGE_ROWS, opt if opt and opt > 0 else STAGE_BYTES // max(row_bytes, 1))


def pattern_flags(pat: str, n: int, S: int) -> np.ndarray:
    """the drop flags of tests/knn_remove_plan_check.cpp's patterns (random30: the same 64-bit LCG)"""
    f = np.zeros(n, bool)

    def put(i):
        if 0 <= i < n:
            f[i] = True
    if pat == "first":
        put(0)
    elif pat == "last":
        put(n - 1)
    elif pat == "mid_slab":
        put(S + S // 2)
    elif pat == "boundary":
        put(S)
    elif pat == "every_other":
        f[0::2] = True
    elif pat == "run":
        f[S // 2:S // 2 + 2 * S + 3] = True
    elif pat == "all_but_one":
        f[:] = True
        f[n // 2] = False
    elif pat == "all":
        f[:] = True
    elif pat == "random30":
        m = (1 << 64) - 1
        s = (0x9e3779b97f4a7c15 ^ ((n * 1315423911 + S) & m)) & m
        for i in range(n):
            s = (s * 6364136223846793005 + 1442695040888963407) & m
            if (s >> 33) % 100 < 30:
                f[i] = True
    elif pat != "none":
        raise ValueError(pat)
    return f


def removal(n: int, ids, id_base: int = 0):
    """-> (keep bool [n], old_to_new int64 [n], n_removed): what remove_ids(ids) does to a store of n rows"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    pos = ids - id_base
    pos = pos[(ids >= id_base) & (pos < n)]
    keep = np.ones(n, bool)
    keep[pos] = False
    omap = np.where(keep, id_base + np.cumsum(keep) - 1, -1).astype(np.int64)
    return keep, omap, int(n - keep.sum())


def plan(n: int, row_bytes: int, flags: np.ndarray, opt: int = 0, l2: bool = True):
    """-> dict(S, r0, removed, slabs [(row0, rows, removed_before, kept, direct)], launches [(kind, row0, rows, dst0)], rows_moved,
    bytes_moved)"""
    S = stage_rows(row_bytes, opt)
    flags = np.asarray(flags, bool)
    excl = np.concatenate([[0], np.cumsum(flags)]).astype(np.int64)      # excl[i] = removed in front of row i; excl[n] = removed
    removed = int(excl[n])
    out = dict(S=S, r0=n, removed=removed, slabs=[], launches=[], rows_moved=0, bytes_moved=0)
    if removed == 0:
        return out
    r0 = int(np.flatnonzero(flags)[0])
    out["r0"] = r0
    per_row = row_bytes + (4 if l2 else 0)
    for a in range(r0 // S * S, n, S):
        b = min(a + S, n)
        out["slabs"].append((a, b - a, int(excl[a]), int((b - a) - (excl[b] - excl[a])), bool(excl[a] >= S)))
    j = 0
    while j < len(out["slabs"]):
        a, rows, before, kept, direct = out["slabs"][j]
        if direct:
            span = rows
            while j + 1 < len(out["slabs"]) and span + out["slabs"][j + 1][1] <= before:
                j += 1
                span += out["slabs"][j][1]
                kept += out["slabs"][j][3]
            if kept:
                out["launches"].append((DIRECT, a, span, a - before))
                out["rows_moved"] += kept
                out["bytes_moved"] += 2 * kept * per_row
        else:
            start = r0 if j == 0 else a
            kept -= start - a
            if kept > 0:
                out["launches"].append((GATHER, start, a + rows - start, start - before))
                out["launches"].append((SCATTER, 0, kept, start - before))
                out["rows_moved"] += kept
                out["bytes_moved"] += 4 * kept * per_row
        j += 1
    return out


def checksum(launches) -> int:
    s = 0
    for kind, row0, rows, dst0 in launches:
        s = (s * 1000003 + (kind + 1) * (row0 * 31 + rows * 17 + dst0 * 13 + 7)) % 2147483647
    return s


def execute(p, flags: np.ndarray, a: np.ndarray) -> np.ndarray:
    """run the plan's launches on a copy of `a` (one value per row); every launch reads ALL its sources before it writes -- the
    order-free semantics a racing launch would not have -- and asserts that what it writes in the store it did not read"""
    a = np.array(a)
    flags = np.asarray(flags, bool)
    n = len(a)
    excl = np.concatenate([[0], np.cumsum(flags)])[:n]
    stage = np.full(p["S"], -1, a.dtype)
    for kind, row0, rows, dst0 in p["launches"]:
        if kind == SCATTER:
            assert rows <= p["S"] and dst0 + rows <= n
            a[dst0:dst0 + rows] = stage[:rows]
            continue
        src = np.arange(row0, row0 + rows)
        assert src[-1] < n
        src = src[~flags[src]]
        dst = src - excl[src]
        if kind == GATHER:
            assert dst.min() - dst0 >= 0 and dst.max() - dst0 < p["S"]
            stage[dst - dst0] = a[src]
        else:
            assert dst.max() < row0, "a direct launch writes at or above its own first row"
            a[dst] = a[src]
    return a[:n - p["removed"]]
