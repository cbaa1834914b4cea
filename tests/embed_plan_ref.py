"""Host model of the embedding path's segment and chunk plan (numpy / Python ints only: no GPU, no library).

What csrc/embed.hip's k_build_plan must produce, restated as a plain loop over the clips -- no prefix scan, no rounds of 1024
clips, no carries:

  * the segmenter's rule (segmenter.py:25-39): a clip of n samples has max(1, (n - L) // hop + 1) segments (Python floor
    division), segment i starts i * hop samples into the clip and holds clamp(n - i * hop, 0, L) real samples;
  * the repairs of device-resident offsets (the comment above k_build_plan): both ends of every clip are clamped into [0, total]
    (flag 1 when that changed anything), a clip that then ends before it starts becomes empty (flag 2), segments beyond seg_cap are
    dropped (flag 4) -- the clip at the boundary keeps the segments that fit, the clips behind it keep none;
  * the chunk work list of the shared-frame log-mel kernels: per clip, in clip order, count_fn(S) records for the S segments the clip
    kept, each with the clip's first sample, its first segment, S, the chunk's index inside the clip and the samples those S segments
    cover.  count_fn is the library's chunk arithmetic (radad_embed_clip_chunks / radad_embed_fft_clip_chunks, pinned to its coverage
    properties by tests/test_host_logic.py and tests/test_fft_tables.py); everything else here is independent of the library.

tests/test_embed_plan_model.py checks the model against oracle.radad_oracle.segment_plan and the repair properties;
tests/test_gpu_embed_plan.py compares what MelProjectionFeatureExtractor.last_plan() reads back with it, exactly."""
import numpy as np

FLAG_OUTSIDE, FLAG_NEGATIVE, FLAG_CAPPED = 1, 2, 4
PLAN_ARRAYS = ("clip_seg", "seg_start", "seg_valid")
CHUNK_ARRAYS = ("chunk_beg", "chunk_seg0", "chunk_n_seg", "chunk_cidx", "chunk_avail")


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def plan(offsets, L, hop, total=None, seg_cap=None):
    """offsets: n_clips + 1 ints (any values).  total: samples in the wave buffer (None: unknown, nothing is clamped -- the
    host-offset entry, which has validated the offsets).  seg_cap: segments the plan may hold (None: no cap).
    Returns a dict: clip_seg [n_clips + 1] int64, seg_start [n_seg] int64 (absolute), seg_valid [n_seg] int32, n_clips, n_seg, flags,
    and `clips`: per clip (first sample, samples, segments wanted, segments kept) after the repairs."""
    offs = [int(v) for v in offsets]
    L, hop = int(L), int(hop)
    flags, wanted_total = 0, 0
    clip_seg, seg_start, seg_valid, clips = [0], [], [], []
    for b in range(len(offs) - 1):
        beg, end = offs[b], offs[b + 1]
        if total is not None:
            cb, ce = _clamp(beg, 0, int(total)), _clamp(end, 0, int(total))
            if (cb, ce) != (beg, end):
                flags |= FLAG_OUTSIDE
            beg, end = cb, ce
        n = end - beg
        if n < 0:
            n = 0
            flags |= FLAG_NEGATIVE
        wanted = max(1, (n - L) // hop + 1)
        wanted_total += wanted
        kept = wanted if seg_cap is None else _clamp(int(seg_cap) - len(seg_start), 0, wanted)
        for i in range(kept):
            seg_start.append(beg + i * hop)
            seg_valid.append(_clamp(n - i * hop, 0, L))
        clip_seg.append(len(seg_start))
        clips.append((beg, n, wanted, kept))
    if seg_cap is not None and wanted_total > int(seg_cap):
        flags |= FLAG_CAPPED
    return {"clip_seg": np.asarray(clip_seg, np.int64), "seg_start": np.asarray(seg_start, np.int64),
            "seg_valid": np.asarray(seg_valid, np.int32), "n_clips": len(offs) - 1, "n_seg": len(seg_start), "flags": flags,
            "clips": clips}


def chunk_records(p, L, hop, count_fn):
    """the chunk work list of plan `p`: dict of chunk_beg int64 and chunk_seg0 / chunk_n_seg / chunk_cidx / chunk_avail int32 arrays
    plus n_chunks.  count_fn(S) -> chunks of a clip that kept S segments (0 for S == 0)."""
    rec = []
    for b, (beg, n, _, S) in enumerate(p["clips"]):
        count = int(count_fn(S))
        assert count >= 0 and (count == 0) == (S == 0), (S, count)
        avail = (S - 1) * hop + _clamp(n - (S - 1) * hop, 0, L)
        for cidx in range(count):
            rec.append((beg, int(p["clip_seg"][b]), S, cidx, avail))
    cols = list(zip(*rec)) if rec else [[]] * 5
    out = {name: np.asarray(col, np.int64 if name == "chunk_beg" else np.int32) for name, col in zip(CHUNK_ARRAYS, cols)}
    out["n_chunks"] = len(rec)
    return out


def check_repaired(p, n_clips, total, seg_cap, flags):
    """the properties a repaired plan must have whatever the offsets held"""
    assert p["n_clips"] == n_clips and len(p["clip_seg"]) == n_clips + 1
    assert p["n_seg"] == len(p["seg_start"]) == len(p["seg_valid"]) <= seg_cap
    start, valid = p["seg_start"].astype(object), p["seg_valid"].astype(object)       # Python ints: no wrap-around in the check itself
    assert all(0 <= s and 0 <= v and s + v <= total for s, v in zip(start, valid)), "a segment leaves [0, total]"
    cs = p["clip_seg"]
    assert cs[0] == 0 and cs[-1] == p["n_seg"] and bool((np.diff(cs) >= 0).all())
    assert p["flags"] == flags, (p["flags"], flags)


def assert_plan_equal(got, want, chunks=None):
    """got: MelProjectionFeatureExtractor.last_plan(); want: plan(...); chunks: chunk_records(...) or None (no chunk plan).
    Every count and every array, exactly (dtype included)."""
    for key in ("n_clips", "n_seg", "flags"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in PLAN_ARRAYS:
        a, b = np.asarray(got[key]), want[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{key} differs first at {i}: plan {a[i]}, model {b[i]} ({int((a != b).sum())} entries differ)")
    if chunks is None:
        assert got["n_chunks"] == 0 and all(len(got[key]) == 0 for key in CHUNK_ARRAYS), got["n_chunks"]
        return
    assert got["n_chunks"] == chunks["n_chunks"], (got["n_chunks"], chunks["n_chunks"])
    for key in CHUNK_ARRAYS:
        a, b = np.asarray(got[key]), chunks[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{key} differs first at chunk {i}: plan {a[i]}, model {b[i]}")


# ---- what the tests share: the tiny-segment configuration, the ragged batches, the designed repair vectors ----------------------
L_SMALL, HOP_SMALL, T_SMALL, H_SMALL = 1600, 800, 10, 5        # segment_length 0.1 s, overlap 0.5: 10 frames per segment, hop 5 frames


def length_menu(L, hop):
    return [0, 1, L - 1, L, L + 1, L + hop - 1, L + hop, L + hop + 1, 3 * L + 17, L + 40 * hop + 5]


def ragged_lengths(B, L, hop, seed=20260101):
    """B clip lengths: seeded draws from length_menu; the clips around the plan kernel's round boundaries (indices 1022..1026 and
    2046..2050) are forced to multi-segment lengths with mutually different segment counts (2, 5, 41, 3, 6), so that a carry that is
    wrong across a round cannot cancel against its neighbours."""
    rng = np.random.default_rng(seed + B)
    menu = length_menu(L, hop)
    lens = [menu[i] for i in rng.integers(0, len(menu), B)]
    forced = [L + hop, 3 * L + 17, L + 40 * hop + 5, L + 2 * hop + 3, L + 5 * hop]
    for base in (1022, 2046):
        for j, n in enumerate(forced):
            if base + j < B:
                lens[base + j] = n
    return lens


def repair_cases(L, hop):
    """(name, offsets, designed flags) over a wave buffer of total = 10 L samples (device offsets only)"""
    u, total = L, 10 * L
    return total, [
        ("end_past_total", [0, 2 * u, 5 * u, 40 * u], 1),
        ("end_2pow40", [0, 2 * u, 5 * u, 2 ** 40], 1),
        ("negative_start", [-5 * u, 2 * u, 5 * u, 10 * u], 1),
        ("not_monotone", [0, 4 * u, 2 * u, 6 * u, 10 * u], 2),
        ("outside_and_not_monotone", [0, 4 * u, 2 * u, 6 * u, 40 * u], 1 | 2),
        ("not_monotone_over_cap", [0, total, 0, total, 0, total], 2 | 4),
        ("all_three", [0, total, 0, 2 ** 40, -3, total], 1 | 2 | 4),
    ]


def dev_caps(total, n_clips, L, hop, T, H, geometry):
    """(seg_cap, chunk_cap) by the expressions of radad_embed_forward_dev; geometry "fft_64" | "gemm_104" | "none" """
    seg_cap = total // hop + n_clips
    if geometry == "none":
        return seg_cap, 0
    per, edge = (64, 26) if geometry == "fft_64" else (104, 32)
    return seg_cap, (seg_cap * H + n_clips * T) // per + (3 * seg_cap) // edge + 2 * n_clips + 1
