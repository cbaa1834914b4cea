"""The designed store of the per-query search on the certified tile scan (HipFlatIndex.search_excluding_per_query_in_scan,
radad_knn_search_excl_scan_pq), shared by tests/test_gpu_knn_excl_scan_pq.py and checked on the CPU by
tests/test_excl_scan_pq_model.py.  Expected results are tests/excl_per_query_ref.expected_pq's: the float64 oracle over the rows AS
STORED.

speakers(): leave-one-speaker-out.  The rows of one speaker -- its CROWD, c rows spread over the whole store -- share a tag and sit
around the speaker's centre; every owning query is that centre plus a much smaller noise and excludes the speaker's tag; a few
BYSTANDER queries sit at the same centres and exclude nothing.  Owners and bystanders of one speaker have near-identical vectors,
share a query tile and have different admissible sets.

Nothing about the ranks the tests compare is left to chance.  With ctr the speaker's centre and w a unit vector orthogonal to it
(and to the all-ones vector, so that a store with a common component added keeps the geometry), a planted row is
    y = (1 - a) ctr + t (1 - a) |ctr| w:
it is `a` short of the centre along it and at an angle atan(t) off it, so every metric ranks planted rows of one speaker by their
position on a ladder where a and t grow together -- L2 by a^2 |ctr|^2 + (t (1 - a) |ctr|)^2, IP by (1 - a) |ctr|^2, cosine by
1 / sqrt(1 + t^2):
    crowd rung i < ladder   a = 0.001 i, t = 0.02 sqrt(i + 1)       (cosine steps of 2e-4, IP steps of 0.001 |ctr|^2)
    crowd filler            a in [0.001 ladder, 0.2], t in [0.02 sqrt(ladder + 1), 0.25], random
    NEAR row i < ladder     a = 0.25 + 0.001 i, t = 0.30 + 0.004 i   (unique tags: every query's admissible neighbours)
so all c crowd rows outrank every near row, the near rows outrank the random rest of the store (L2 distances around 2 dim), a
bystander's top k are crowd rungs and an owner's top k are near rows, all with gaps far above the 1e-4 the comparisons need.
ladder = k_max + 4."""
import numpy as np

from oracle import synth

SPEAKER_TAG0 = 1 << 40          # tag of speaker s: SPEAKER_TAG0 + s (the other rows: 7 row + 11)


def _orthonormal_dirs(rng, ctr, count, dim):
    """[count, dim] unit vectors orthogonal to ctr and to the all-ones vector"""
    w = rng.standard_normal((count, dim))
    basis = np.stack([ctr / np.linalg.norm(ctr), np.ones(dim) / np.sqrt(dim)])
    basis[1] -= (basis[1] @ basis[0]) * basis[0]
    basis[1] /= np.linalg.norm(basis[1])
    w -= (w @ basis.T) @ basis
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def speakers(n, dim, n_speakers, c, nq, seed, k_max=10, owners=None, q_noise=1e-3):
    """-> (db [n, dim] f32, q [nq, dim] f32, tags [n], qtags [nq, 1], qcnt [nq] int32, info); info: "crowd" [n_speakers, c] rows
    (ladder order), "near" [n_speakers, ladder] rows, "speaker" [nq] the speaker a query sits at, "owner" [nq] bool (False = bystander),
    "ladder".  Query j sits at speaker j % n_speakers.  Every eighth round of the speakers is a round of bystanders (queries
    7 n_speakers .. 8 n_speakers - 1, 15 n_speakers .., ...), so any prefix of >= 8 n_speakers queries holds both kinds at every
    centre; owners = an int: only the first `owners` queries own, all the others are bystanders."""
    rng = np.random.default_rng(seed)
    ladder = k_max + 4
    assert c >= ladder and n >= n_speakers * (c + ladder) * 2
    db = synth.rows(0, n, dim, seed).astype(np.float32)
    ctrs = synth.rows(0, n_speakers, dim, seed + 1).astype(np.float64)
    tags = np.arange(n, dtype=np.int64) * 7 + 11
    rows = rng.choice(n, n_speakers * (c + ladder), replace=False).reshape(n_speakers, c + ladder)
    crowd, near = rows[:, :c], rows[:, c:]
    for s in range(n_speakers):
        ctr, cn = ctrs[s], np.linalg.norm(ctrs[s])
        w = _orthonormal_dirs(rng, ctr, c + ladder, dim)
        i = np.arange(ladder)
        a_c = np.concatenate([0.001 * i, rng.uniform(0.001 * ladder, 0.2, c - ladder)])
        t_c = np.concatenate([0.02 * np.sqrt(i + 1.0), rng.uniform(0.02 * np.sqrt(ladder + 1.0), 0.25, c - ladder)])
        a = np.concatenate([a_c, 0.25 + 0.001 * i])
        t = np.concatenate([t_c, 0.30 + 0.004 * i])
        db[rows[s]] = ((1 - a)[:, None] * ctr + (t * (1 - a) * cn)[:, None] * w).astype(np.float32)
        tags[crowd[s]] = SPEAKER_TAG0 + s
    spk = np.arange(nq) % n_speakers
    owner = ((np.arange(nq) // n_speakers) % 8 != 7) if owners is None else (np.arange(nq) < owners)
    q = (ctrs[spk] + q_noise * rng.standard_normal((nq, dim))).astype(np.float32)
    qtags = (SPEAKER_TAG0 + spk).astype(np.int64).reshape(nq, 1)
    qcnt = owner.astype(np.int32)
    return db, q, tags, qtags, qcnt, {"crowd": crowd, "near": near, "speaker": spk, "owner": owner, "ladder": ladder}


# the shapes the GPU tests use (tests/test_gpu_knn_excl_scan_pq.py); tests/test_excl_scan_pq_model.py asserts the properties of each
TWO_PHASE_ROWS = 211200          # printed by tests/knn_excl_scan_pq_plan_check.cpp: the smallest dim-64 store scanned in two phases at k = 100
SHAPES = {
    "grid": dict(n=20480, dim=64, n_speakers=4, c=200, nq=300, seed=9100, k_max=10),
    "c1500": dict(n=20480, dim=64, n_speakers=4, c=1500, nq=40, seed=9200, k_max=10),
    "c5000": dict(n=20480, dim=64, n_speakers=2, c=5000, nq=40, seed=9300, k_max=10, owners=8),
    "two_phase": dict(n=TWO_PHASE_ROWS, dim=64, n_speakers=4, c=300, nq=40, seed=9400, k_max=100),
    "shards": dict(n=32768, dim=64, n_speakers=4, c=200, nq=40, seed=9500, k_max=10),
}
KINDS = ("centred", "uncentred", "f16")


def shape(name, kind="uncentred"):
    """speakers(**SHAPES[name]) as a store of `kind` holds it: centred = with a common component, f16 = rounded to fp16"""
    db, q, tags, qtags, qcnt, info = speakers(**SHAPES[name])
    if kind == "centred":
        db, q = with_common_component(db, q)
    if kind == "f16":
        db = db.astype(np.float16).astype(np.float32)
    return db, q, tags, qtags, qcnt, info


def with_common_component(db, q, shift=0.25):
    """the `centred` stores of the GPU tests: every row and query moved by one vector (what centring a plane is for)"""
    return db + np.float32(shift), q + np.float32(shift)


def keys64(db, q, metric):
    """float64 keys [nq, n], LARGER IS BETTER (minus the squared distance under L2; cosine over the normalised rows and queries)"""
    d, x = np.asarray(db, np.float64), np.asarray(q, np.float64)
    if metric == "COSINE":
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    if metric == "L2":
        return -((x * x).sum(axis=1)[:, None] - 2.0 * (x @ d.T) + (d * d).sum(axis=1)[None, :])
    return x @ d.T


def store_properties(db, q, tags, qtags, qcnt, info, k, metric):
    """what the GPU tests rely on, from plain float64 numpy -> dict:
       crowd_outranks   every crowd row of a query's speaker has a better key than the query's k-th ADMISSIBLE neighbour
       min_gap          the smallest gap between adjacent admissible ranks 1 .. k + 1 over all queries
       bystanders_inside  the top k of every bystander are crowd rows of its speaker"""
    key = keys64(db, q, metric)
    nq = len(q)
    crowd_ok, inside, gap = True, True, np.inf
    for j in range(nq):
        s = info["speaker"][j]
        adm = np.ones(len(db), bool)
        if qcnt[j] > 0:
            adm &= ~np.isin(tags, qtags[j, :qcnt[j]])
        kj = np.where(adm, key[j], -np.inf)
        top = np.argpartition(-kj, k + 1)[:k + 2]
        top = top[np.argsort(-kj[top], kind="stable")][:k + 1]
        gap = min(gap, float(np.min(-np.diff(kj[top]))))
        crowd_ok &= bool(np.all(key[j, info["crowd"][s]] > kj[top[k - 1]])) if info["owner"][j] else True
        if not info["owner"][j]:
            inside &= bool(np.all(np.isin(top[:k], info["crowd"][s])))
    return {"crowd_outranks": crowd_ok, "min_gap": gap, "bystanders_inside": inside}
