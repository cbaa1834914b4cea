"""Designed stores and the case table of the row-width tests (tests/test_knn_width_cases.py on the CPU, tests/test_gpu_knn_widths.py
on the GPU).  Host only: numpy and oracle.synth.

Which kernel answers a flat search is decided by the residues of the row width (csrc/knn_plan.h), and every result is "exact by
certificate": a scan that mishandles the last partial K step of a width does not return wrong ids on random rows -- the float64
re-rank repairs it, or the certificate rejects the query and the exact kernel answers.  These stores make such a scan visible.

tail_store: per designed query ("centre") c, |c| = R, with 60 % of |c|^2 in ONE vec4 column group g (w = 4: all of it):
  neighbours  t = 0 .. k_max + 7:  r_t c + a_t R p_t + e_t -- p_t a unit vector orthogonal to every centre and zero in group g, e_t noise of
              1e-4 R in ALL columns -- with r_t, a_t stepped so that inner product, squared distance and cosine all fall by more than
              2^-9 |q| max|y| per rank: a correct scan has nothing near the k-th score to reject (band_count);
  decoys      DECOYS = 1100 rows equal to c EXCEPT in group g, which holds -(1 + z) c_g, z in [0, 0.5): far by every metric -- and the
              best rows of the store for a scan that drops, zero-fills wrongly or misplaces group g.  1100 is more than any candidate
              capacity a scan has (lists of k + 6 <= 32, dense k + 32, the emit buffer's 1024);
  background  oracle.synth rows with the centres' span projected out and a negative component along every centre: far by every metric.
The group g rotates over the centres: first group, last group, the first group of the last partial 16-, 32- and 64-column step where
the width has one, one interior group (column_groups).  A centre costs 1100 + k_max + 8 rows, so a store of n rows holds
min(groups, (n - 200) // (1108 + k_max)) centres; `rot` says which group the first one takes, and a store of 1500 rows -- one centre --
is built once per group (store_rots).  A batch of nq queries repeats the centres: query j is centre j % P, so every query slot of a
tile sees a designed query and the float64 reference is computed once per centre.

What differs from the plan this file was written to: the scan kinds are the SIX that radad_knn_last_launch reports -- the K-split
form of the small-batch stream is a flag of `hi_smallq` (ScanPlan::sq_ksplit), reported here by plan()["ksplit"]; and a batch of <= 16
queries whose k + 6 exceeds 32 takes `hi_tile` on the plane widths, not `hi_smallq` (knn_tile_eligibility: the small-batch kernels'
lists hold 32).  csrc/knn_plan.h is the authority: tests/knn_width_plan_check.cpp runs every case through it."""
import numpy as np

from oracle import synth

CLASSES = {"a": (4, 8, 12), "b": (16, 20, 28), "c": (32, 36), "d": (48, 80, 1040), "e": (60, 68, 124, 132),
           "f": (64, 192, 1024, 1088), "g": (7168, 16380)}
WIDTHS = tuple(w for ws in CLASSES.values() for w in ws)
CLASS_OF = {w: c for c, ws in CLASSES.items() for w in ws}
DECOYS = 1100
K_LIST = (1, 10, 26, 27, 150)
NQ_LIST = (1, 16, 17, 300)
K_MAX = max(K_LIST)
N_SMALL, N_LARGE, N_PLANE_WIDE = 1500, 20000, 16384
LEAD = 200                  # rows at the start of a store that are background: the "all ties" answer (ids 0, 1, ...) is never the true one
R = 4.0
HEAVY = 0.6                 # share of |c|^2 in the designated group


# ---- column groups ------------------------------------------------------------------------------------------------------------------
def column_groups(width):
    """the vec4 groups the designated group rotates over, in order, without repeats"""
    ng = width // 4
    out = [0, ng - 1]
    for step in (16, 32, 64):
        if width % step:
            out.append((width - width % step) // 4)
    out.append(ng // 2)
    seen = []
    for g in out:
        if g not in seen:
            seen.append(g)
    return seen


def centres_per_store(width, n, k_max):
    return max(0, min(len(column_groups(width)), (n - LEAD) // (DECOYS + k_max + 8)))


def store_rots(width, n, k_max=K_MAX):
    """the `rot` values whose stores together give every column group a centre"""
    p = centres_per_store(width, n, k_max)
    assert p >= 1, (width, n, k_max)
    return list(range(0, len(column_groups(width)), p))


# ---- the stores -----------------------------------------------------------------------------------------------------------------------
def _null_project(x, N):
    """x [m, c] minus its component in the row space of N [r, c]"""
    if len(N) == 0:
        return x
    coef = np.linalg.lstsq(N.T, x.T, rcond=None)[0]
    return x - (N.T @ coef).T


def _centres(width, groups, rng):
    """[P, width] float64, |c| = R: HEAVY of |c|^2 in the centre's group; the rest ("light") off that group, orthogonal to the other
    light parts, with a component along the heavy part of every other centre (so that a decoy of centre B scores BELOW B itself for
    query A, by an amount that varies with the decoy)"""
    P = len(groups)
    if width == 4:
        h = rng.uniform(0.5, 1.0, 4) * rng.choice([-1.0, 1.0], 4)
        return (h / np.linalg.norm(h) * R)[None, :]
    heavy = []
    for g in groups:
        h = rng.uniform(0.5, 1.0, 4) * rng.choice([-1.0, 1.0], 4)
        heavy.append(h / np.linalg.norm(h) * np.sqrt(HEAVY) * R)
    lights = []
    for a, g in enumerate(groups):
        off = np.setdiff1d(np.arange(width), np.arange(4 * g, 4 * g + 4))
        pos = {c: i for i, c in enumerate(off)}
        N = []
        for b, gb in enumerate(groups):
            if b != a:
                row = np.zeros(len(off))
                row[[pos[c] for c in range(4 * gb, 4 * gb + 4)]] = heavy[b]
                N.append(row)
        N += [l[off] for l in lights]
        N = np.array(N).reshape(-1, len(off))
        l = _null_project(rng.standard_normal((1, len(off))), N)[0]
        assert np.linalg.norm(l) > 1e-6, (width, groups)
        # the component along the other centres' heavy parts: 0.1 R^2 of inner product each
        along = np.zeros(len(off))
        for b, gb in enumerate(groups):
            if b != a:
                along[[pos[c] for c in range(4 * gb, 4 * gb + 4)]] = heavy[b] * (0.1 * R * R / (HEAVY * R * R))
        rest = (1 - HEAVY) * R * R - along @ along
        assert rest > 0, (width, groups)
        l = l / np.linalg.norm(l) * np.sqrt(rest) + along
        full = np.zeros(width)
        full[off] = l
        lights.append(full)
    C = np.array(lights)
    for a, g in enumerate(groups):
        C[a, 4 * g:4 * g + 4] = heavy[a]
    return C


def _ladder(T):
    """(r_t, a_t): inner product r R^2, squared distance ((1 - r)^2 + a^2) R^2 and cosine r / sqrt(r^2 + a^2) of neighbour t all
    move by >= 0.003 (0.0015 for the cosine) per rank -- band_count's band is ~0.005 R^2 (1 / 256 for the cosine)"""
    t = np.arange(1, T + 1, dtype=np.float64)
    return 1.0 - 0.003 * t, np.sqrt(0.003 * t)


def _background(width, n_rows, C, seed, rng, chunk=2048):
    """synth rows (a block of <= 512 columns tiled and rolled along wide rows) with the centres' span projected out, a negative
    component of varying size along every centre, norm 0.9 R; float32 [n_rows, width], made 2048 rows at a time"""
    out = np.empty((n_rows, width), np.float32)
    wc = min(width, 512)
    Ch = C / np.linalg.norm(C, axis=1, keepdims=True)
    wv = np.linalg.lstsq(Ch, np.ones(len(Ch)), rcond=None)[0]           # wv . c^_A = 1 for every centre
    for r0 in range(0, n_rows, chunk):
        m = min(chunk, n_rows - r0)
        blk = synth.rows(r0, m, wc, seed).astype(np.float64)
        s = np.concatenate([np.roll(blk, 7 * i, axis=1) * (1.0 if i % 2 == 0 else -1.0) for i in range(-(-width // wc))], axis=1)[:, :width]
        u = _null_project(s, Ch)
        u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-30)
        b = u - rng.uniform(0.1, 0.5, (m, 1)) * wv[None, :]
        out[r0:r0 + m] = b / np.linalg.norm(b, axis=1, keepdims=True) * (0.9 * R)
    return out


def _neighbours(width, C, a, g, T, rng):
    off = np.arange(width) if width == 4 else np.setdiff1d(np.arange(width), np.arange(4 * g, 4 * g + 4))
    N = C[:, off] if width > 4 else C
    p = _null_project(rng.standard_normal((T, len(off))), N)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    r, al = _ladder(T)
    y = r[:, None] * C[a][None, :]
    y[:, off] += (al * R)[:, None] * p
    return y + rng.standard_normal((T, width)) * (1e-4 * R / np.sqrt(width))


def _planted(width, n, nq, k_max, seed, rot, decoys, copies):
    groups_all = column_groups(width)
    per = decoys + k_max + 8 + copies
    P = max(0, min(len(groups_all), (n - LEAD) // per))
    assert P >= 1, f"a store of {n} rows holds no centre of {per} rows"
    groups = [groups_all[(rot + i) % len(groups_all)] for i in range(P)]
    rng = np.random.default_rng([seed, width, n, rot])
    C = _centres(width, groups, rng)
    T = k_max + 8
    rows = np.empty((n, width), np.float32)
    free = LEAD + rng.permutation(n - LEAD)
    info = {"groups": groups, "centres": P, "centre_of": np.arange(nq) % P, "neighbours": [], "decoys": [], "copies": []}
    planted = np.zeros(n, bool)
    at = 0
    if copies:                                           # adjacent blocks right behind the leading background rows
        for a in range(P):
            lo = LEAD + a * copies
            info["copies"].append(np.arange(lo, lo + copies))
            planted[lo:lo + copies] = True
        free = free[~planted[free]]
    for a, g in enumerate(groups):
        ids = np.sort(free[at:at + T]); at += T
        y = _neighbours(width, C, a, g, T, rng)
        rows[ids] = y[rng.permutation(T)] if not copies else y          # (rank and id are unrelated)
        planted[ids] = True
        info["neighbours"].append(ids)
        if copies:
            rows[info["copies"][a]] = rows[ids[3]]
        ids = np.sort(free[at:at + decoys]); at += decoys
        if decoys:
            d = np.repeat(C[a][None, :], decoys, axis=0)
            z = (np.arange(decoys) / (2.0 * decoys))[rng.permutation(decoys)]
            d[:, 4 * g:4 * g + 4] = -(1.0 + z)[:, None] * C[a, 4 * g:4 * g + 4][None, :]
            rows[ids] = d
            planted[ids] = True
        info["decoys"].append(ids)
    bg = np.flatnonzero(~planted)
    rows[bg] = _background(width, len(bg), C, 77000 + seed, rng)
    queries = C.astype(np.float32)[info["centre_of"]]
    info["centre_rows"] = C.astype(np.float32)
    return rows, queries, info


def tail_store(width, n, nq, k_max, seed, rot=0):
    """(rows float32 [n, width], queries float32 [nq, width], info): see the module docstring.  info: "groups" (the designated group
    of each centre), "centre_of" [nq], "centre_rows" [P, width] (the distinct queries), "neighbours" / "decoys" (row ids per centre)"""
    return _planted(width, n, nq, k_max, seed, rot, DECOYS, 0)


def dup_store(width, n, nq, k_max, seed, rot=0):
    """the same background and neighbours without decoys, plus 100 exact copies of ONE neighbour per centre (the one stored at the
    centre's 4th neighbour id), adjacent in the store (info["copies"]): ties go to the lower id, and a scan whose lists or candidate
    capacity the copies use up has to hand the query to the exact kernel"""
    return _planted(width, n, nq, k_max, seed, rot, 0, 100)


def zero_group(x, g):
    out = np.array(x, copy=True)
    out[:, 4 * g:4 * g + 4] = 0
    return out


# ---- float64 scores, the band check --------------------------------------------------------------------------------------------------
def scores64(rows, queries, metric, chunk=4096):
    """float64 [nq, n], larger is better: q.y (IP), q^.y^ (COSINE: both normalised in float64), -|q - y|^2 (L2, summed directly);
    and the band unit |q| max|y| per query of the operands as the metric sees them"""
    q = np.asarray(queries, np.float64)
    if metric == "COSINE":
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-12)
    out = np.empty((len(q), len(rows)))
    ymax = 0.0
    for r0 in range(0, len(rows), chunk):
        y = np.asarray(rows[r0:r0 + chunk], np.float64)
        if metric == "COSINE":
            y = y / (np.linalg.norm(y, axis=1, keepdims=True) + 1e-12)
        ymax = max(ymax, float(np.sqrt((y * y).sum(1)).max()))
        if metric == "L2":
            for j in range(len(q)):
                out[j, r0:r0 + chunk] = -((y - q[j][None, :]) ** 2).sum(1)
        else:
            out[:, r0:r0 + chunk] = q @ y.T
    return out, np.linalg.norm(q, axis=1) * ymax


def topk64(scores, k):
    """ids [nq, k] by (score descending, id ascending)"""
    ids = np.broadcast_to(np.arange(scores.shape[1]), scores.shape)
    return np.lexsort((ids, -scores), axis=1)[:, :k]


def band_counts(rows, queries, ks, metric):
    """{k: int [nq]}: rows whose float64 score lies within 2^-8 |q| max|y| of the k-th best (8 x the f16 rounding unit: wider than
    any route's 2 eps)"""
    s, unit = scores64(rows, queries, metric)
    srt = -np.sort(-s, axis=1)
    out = {}
    for k in ks:
        kth = srt[:, k - 1][:, None]
        out[k] = (np.abs(s - kth) <= (unit * 2.0 ** -8)[:, None]).sum(1)
    return out


def band_count(rows, queries, k, metric):
    return band_counts(rows, queries, (k,), metric)[k]


# ---- the planner's rules, restated (csrc/knn_plan.h; tests/knn_width_plan_check.cpp compares) ----------------------------------------
SQ_NQ, SQ_LDS_BUDGET, SQ_SLOT_BYTES = 16, 160 * 1024, max(8 * 4 * 16 * 16, 8 * 3 * 16 * 32) + 4 * 4 * 16
KNN_MARGIN, KNN_F16_MAX_K, RF_STAGE_MAX, RF_STAGE_MAX_SMALLQ = 6, 128, 6144, 16384
KINDS = ("f32_tile", "hi_tile", "f32_smallq", "hi_smallq", "f16_tile", "f32_dense")


def plan(width, n, f16, nq, k):
    """{"kind", "ksplit", "kernel"}: the scan a fresh handle with default options takes (knn_tile_eligibility, knn_smallq_hi_eligible,
    knn_finish_plan) and, for the coverage table, the kernel behind the kind (knn_scan_tile's choice among the tile kernels)"""
    ksel = k + KNN_MARGIN
    lds_hi = 2 * nq * (width + 8) + SQ_SLOT_BYTES
    lds_f32 = 4 * nq * (width + 4) + SQ_SLOT_BYTES
    sq_fits = nq <= SQ_NQ and ksel <= 32 and ((width % 64 == 0 and lds_hi <= SQ_LDS_BUDGET) or
                                             (not f16 and width % 32 == 0 and lds_f32 <= SQ_LDS_BUDGET))
    use_hi = False
    if k <= KNN_F16_MAX_K and (nq >= SQ_NQ + 1 or not sq_fits) and n > 0 and width % 64 == 0:
        wq = -(-nq // 256)
        tiles = n // 256
        want = (tiles * 3 // 100 + 4) // 8 * 8
        need = ((2 * ksel + 15) // 16 + 7) // 8 * 8
        want = max(want, need, 8)
        want = max(want, min(64, (256 // max(1, min(wq, 256))) // 8 * 8))
        s_splits = min(64, want, tiles // 8 // 8 * 8)
        use_hi = s_splits >= 8 and s_splits * 16 >= 2 * ksel
    geom = (not use_hi) and nq <= SQ_NQ and ksel <= 32 and n > 0
    smallq_hi = geom and k <= KNN_F16_MAX_K and width % 64 == 0 and n >= 16384 and lds_hi <= SQ_LDS_BUDGET
    dense = (not use_hi and not smallq_hi and not f16 and 1 <= n <= (RF_STAGE_MAX_SMALLQ if nq <= SQ_NQ else RF_STAGE_MAX)
             and width % 16 == 0 and nq * ((max(n, 1) + 3) // 4 * 4) <= 1 << 24)
    smallq = geom and not dense and not smallq_hi and not f16 and width % 32 == 0 and lds_f32 <= SQ_LDS_BUDGET
    f16_tile = not use_hi and not smallq_hi and bool(f16) and ksel <= 32 and width % 64 == 0
    kind = ("hi_tile" if use_hi else "f32_dense" if dense else "hi_smallq" if smallq_hi else "f32_smallq" if smallq
            else "f16_tile" if f16_tile else "f32_tile")
    ksplit = bool(smallq_hi and width >= 1024 and -(-n // 16) < 4096)
    if kind == "f32_tile":
        kernel = "k_knn_f32_reg" if (not f16 and ksel <= 32 and width % 32 == 0) else ("k_knn_f32<f16>" if f16 else "k_knn_f32")
    else:
        kernel = {"hi_tile": "hi_tile", "f32_dense": "k_knn_dense", "hi_smallq": "hi_smallq_ksplit" if ksplit else "hi_smallq",
                  "f32_smallq": "k_knn_f32_smallq", "f16_tile": "k_knn_f32_reg<f16>"}[kind]
    return {"kind": kind, "ksplit": ksplit, "kernel": kernel}


def expected_kind(case):
    width, n, f16, metric, nq, k = case
    return plan(width, n, f16, nq, k)["kind"]


def list_class(k):
    return "k>128" if k > 128 else "<=16" if k + 6 <= 16 else "<=32" if k + 6 <= 32 else ">32"


# ---- the stores and cases the tests run ----------------------------------------------------------------------------------------------
F16_CLASSES = "acdef"
LARGE_F16 = (64, 68, 1024)          # fp16 stores of >= 16384 rows: the plane routes read the store itself; the generic kernel on many chunks


def _stores():
    """(width, n, f16, metric), in order: every width at N_SMALL rows (fp32, and fp16 in classes a, c, d, e, f) and, up to 1088, at
    N_LARGE rows; L2 and COSINE everywhere, IP on the first width of each class; one 7168 x 16384 store for the plane routes"""
    out = []
    for cls, ws in CLASSES.items():
        for i, w in enumerate(ws):
            metrics = ("L2", "COSINE", "IP") if i == 0 else ("L2", "COSINE")
            for m in metrics:
                out.append((w, N_SMALL, False, m))
                if cls in F16_CLASSES and m != "IP":
                    out.append((w, N_SMALL, True, m))
                if w <= 1088:
                    out.append((w, N_LARGE, False, m))
                    if w in LARGE_F16 and m != "IP":
                        out.append((w, N_LARGE, True, m))
            if w == 7168:
                out += [(w, N_PLANE_WIDE, False, "L2"), (w, N_PLANE_WIDE, False, "COSINE")]
    return out


STORES = _stores()
SEARCHES = tuple((nq, k) for nq in NQ_LIST for k in K_LIST)
CASES = [(w, n, f16, m, nq, k) for (w, n, f16, m) in STORES for (nq, k) in SEARCHES]
STORE_SEED = 4100


def store_params():
    """(width, n, f16, metric, rot) of every store a GPU test builds: a store per rot (store_rots)"""
    return [(w, n, f16, m, rot) for (w, n, f16, m) in STORES for rot in store_rots(w, n)]
