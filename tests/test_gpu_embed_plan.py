"""The embedding path's segment and chunk plan (k_build_plan, csrc/embed.hip), read back through
MelProjectionFeatureExtractor.last_plan() and held to the host model tests/embed_plan_ref.py -- exactly; the embeddings across the
plan kernel's round boundary and of zero-length clips against the float64 oracle (the suite's 1e-4 bar); the repairs of bad
device-resident offsets, the segment-cap truncation included; the handle's plan state across a scripted sequence of calls; and
which batch a repair report is attributed to.

Tiny segments (0.1 s, overlap 0.5: L = 1600 samples, hop 800, 10 frames per segment, hop 5 frames -- eligible for the shared-frame
kernels, two owners per frame) keep a 3001-clip ragged batch near 10 M samples; the benchmark's (2.0 s, 0.5) runs once."""
import ctypes as C

import numpy as np
import pytest

from oracle import radad_oracle as O

import embed_plan_ref as M

pytestmark = pytest.mark.gpu

KERNELS = ["fft", "gemm", "per_segment"]
GEOMETRY = {"fft": "fft_64", "gemm": "gemm_104", "per_segment": "none"}
KIND = {"fft": "clip_frames_fft", "gemm": "clip_frames", "per_segment": "per_segment"}
LEVELS = [1, 2]


def _extractor(gpu, kernel, seg_s=0.1, overlap=0.5, feature_dim=32):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, melproj_share_frames=kernel != "per_segment", melproj_logmel_fft=kernel != "gemm", feature_dim=feature_dim,
               tpp_levels=LEVELS, tpp_pooling_type="max", segment_length=seg_s, segment_overlap=overlap, melproj_seed=7)
    return R.MelProjectionFeatureExtractor(cfg)


def _count_fn(kernel, T, H):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    fn = lib.radad_embed_fft_clip_chunks if kernel == "fft" else lib.radad_embed_clip_chunks
    out, memo = (C.c_int32 * 5)(), {}

    def count(S):
        if S not in memo:
            _lib.check(fn(S, T, H, out))
            memo[S] = int(out[4])
        return memo[S]
    return count


def _audio(gpu, n, seed):
    """n samples of oracle.synth.audio (its device twin, the same bits: tests/test_gpu_reference_fixtures.py) as one long clip"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    wave = torch.empty(max(n, 1), device=gpu, dtype=torch.float32)
    _lib.check(_lib.load().radad_synth_audio(wave.data_ptr(), 0, 1, wave.numel(), seed, gpu.index or 0, _lib.stream_ptr(gpu)))
    return wave


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _model(fe, kernel, offs, total=None, seg_cap=None):
    L, hop = fe.segment_length, fe.hop_length
    want = M.plan(offs, L, hop, total=total, seg_cap=seg_cap)
    chunks = None if kernel == "per_segment" else M.chunk_records(want, L, hop, _count_fn(kernel, fe.num_frames, hop // 160))
    return want, chunks


def _check_host_plan(fe, kernel, offs):
    got = fe.last_plan()
    want, chunks = _model(fe, kernel, offs)
    assert (got["kind"], got["geometry"]) == ("host_offsets", GEOMETRY[kernel])
    M.assert_plan_equal(got, want, chunks)
    assert got["n_seg"] == got["seg_cap"] and got["n_chunks"] == got["chunk_cap"]          # sized on the host: the exact counts
    return got


def _check_dev_plan(fe, kernel, offs, total):
    got = fe.last_plan()
    n_clips = len(offs) - 1
    seg_cap, chunk_cap = M.dev_caps(total, n_clips, fe.segment_length, fe.hop_length, fe.num_frames, fe.hop_length // 160, GEOMETRY[kernel])
    assert (got["kind"], got["geometry"]) == ("device_offsets", GEOMETRY[kernel])
    assert (got["seg_cap"], got["chunk_cap"]) == (seg_cap, chunk_cap)
    want, chunks = _model(fe, kernel, offs, total=total, seg_cap=seg_cap)
    M.assert_plan_equal(got, want, chunks)
    assert got["n_seg"] <= seg_cap and got["n_chunks"] <= chunk_cap
    return got


# ---- a. the plan equals the model, exactly ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 7, 1023, 1024, 1025, 2049, 3001])
@pytest.mark.parametrize("kernel", KERNELS)
def test_plan_equals_the_model(gpu, kernel, B):
    """host and device offsets, every log-mel kernel's chunk geometry, batches on both sides of the plan kernel's rounds of 1024 clips
    (one round, exactly one, one clip into the second, one into the third, three rounds) with ragged clips at the boundaries"""
    import torch
    fe = _extractor(gpu, kernel)
    L, hop = fe.segment_length, fe.hop_length
    assert (L, hop, fe.num_frames) == (M.L_SMALL, M.HOP_SMALL, M.T_SMALL)
    offs = _offsets(M.ragged_lengths(B, L, hop))
    wave = _audio(gpu, int(offs[-1]), 100 + B)
    fe.embed_clips(wave, offs)
    assert fe.last_logmel_kind() == KIND[kernel]
    got = _check_host_plan(fe, kernel, offs)
    assert got["flags"] == 0 and got["n_clips"] == B
    fe.embed_clips(wave, torch.from_numpy(offs).to(gpu))
    assert fe.last_logmel_kind() == KIND[kernel]
    got = _check_dev_plan(fe, kernel, offs, wave.numel())
    assert got["flags"] == 0 and got["n_clips"] == B
    fe.check_device_plan()


def test_plan_equals_the_model_at_the_benchmarks_segments(gpu):
    """(2.0 s, 0.5): L = 32000, hop 16000, 200 frames per segment -- full chunks, tail chunks and edge-only chunks all occur"""
    import torch
    for kernel in ("fft", "gemm"):
        fe = _extractor(gpu, kernel, seg_s=2.0, overlap=0.5)
        L, hop = fe.segment_length, fe.hop_length
        lens = M.length_menu(L, hop) + [L + 12 * hop, 64000, 7]
        offs = _offsets(lens)
        wave = _audio(gpu, int(offs[-1]), 9)
        fe.embed_clips(wave, offs)
        _check_host_plan(fe, kernel, offs)
        fe.embed_clips(wave, torch.from_numpy(offs).to(gpu))
        _check_dev_plan(fe, kernel, offs, wave.numel())
        fe.check_device_plan()


def test_last_plan_checks_the_callers_capacities(gpu):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    fe = _extractor(gpu, "fft")
    lib, info, st = fe._lib, (C.c_int64 * 8)(), _lib.stream_ptr(gpu)
    assert lib.radad_embed_last_plan(fe._h, info, None, 0, None, None, 0, None, None, 0, st) == _lib.RADAD_ESTATE     # no plan yet
    with pytest.raises(ValueError, match="no plan yet"):
        fe.last_plan()
    L = fe.segment_length
    offs = _offsets([3 * L, L])
    fe.embed_clips(_audio(gpu, 4 * L, 3), offs)
    assert lib.radad_embed_last_plan(fe._h, info, None, 0, None, None, 0, None, None, 0, st) == 0                      # info only
    n_clips, n_seg, n_chunks = int(info[0]), int(info[1]), int(info[2])
    assert (n_clips, n_seg) == (2, 6) and n_chunks > 0
    cs, ss, sv = np.full(n_clips + 1, -7, np.int64), np.full(n_seg, -7, np.int64), np.full(n_seg, -7, np.int32)
    cb, cf = np.full(n_chunks, -7, np.int64), np.full((n_chunks, 4), -7, np.int32)
    p64, p32 = (lambda a: a.ctypes.data_as(_lib.c_i64p)), (lambda a: a.ctypes.data_as(_lib.c_i32p))
    for args, what in (((p64(cs), n_clips, p64(ss), p32(sv), n_seg, p64(cb), p32(cf), n_chunks), "clip_seg needs room for 3"),
                       ((p64(cs), n_clips + 1, p64(ss), p32(sv), n_seg - 1, p64(cb), p32(cf), n_chunks), "segment arrays need room for 6"),
                       ((p64(cs), n_clips + 1, p64(ss), p32(sv), n_seg, p64(cb), p32(cf), n_chunks - 1), "chunk arrays need room"),
                       ((p64(cs), n_clips + 1, p64(ss), None, n_seg, p64(cb), p32(cf), n_chunks), "come in pairs"),
                       ((p64(cs), n_clips + 1, p64(ss), p32(sv), n_seg, None, p32(cf), n_chunks), "come in pairs"),
                       ((p64(cs), -1, None, None, 0, None, None, 0), "negative capacity")):
        assert lib.radad_embed_last_plan(fe._h, info, *args, st) == _lib.RADAD_EINVAL
        assert what.encode() in lib.radad_last_error(), lib.radad_last_error()
        assert all(int(a.min()) == -7 == int(a.max()) for a in (cs, ss, sv, cb, cf))       # a refused call copies nothing
    assert lib.radad_embed_last_plan(fe._h, info, p64(cs), n_clips + 1, None, None, 0, None, None, 0, st) == 0          # one array alone
    assert cs.tolist() == [0, 5, 6] and int(ss.max()) == -7
    _check_host_plan(fe, "fft", offs)                                                        # reading changed nothing


# ---- b. embeddings across the round boundary, zero-length clips ----------------------------------------------------------------

_BOUNDARY = {}


def _boundary_case(gpu, fe):
    """the 2049-clip ragged batch, its audio, the clips whose embeddings are compared with the oracle and the oracle's answer
    (float64, computed once for the three kernels: they share the projection weights)"""
    if not _BOUNDARY:
        L, hop = fe.segment_length, fe.hop_length
        lens = M.ragged_lengths(2049, L, hop)
        offs = _offsets(lens)
        wave = _audio(gpu, int(offs[-1]), 2049)
        host = wave.cpu().numpy()
        pick = sorted(set([0, 1022, 1023, 1024, 1025, 1026, 2046, 2047, 2048] + [b for b, n in enumerate(lens) if n <= 1]))
        ref = O.embed_clips([host[offs[b]:offs[b + 1]] for b in pick], L, hop, fe.proj_w, fe.proj_b, tuple(LEVELS), "max")
        _BOUNDARY.update(offs=offs, wave=wave, pick=pick, ref=ref, lens=lens, w=fe.proj_w.copy())
    assert np.array_equal(_BOUNDARY["w"], fe.proj_w)
    return _BOUNDARY


@pytest.mark.parametrize("kernel", KERNELS)
def test_embeddings_across_the_round_boundary(gpu, kernel):
    import torch
    fe = _extractor(gpu, kernel)
    c = _boundary_case(gpu, fe)
    assert sum(n == 0 for n in c["lens"]) > 50 and sum(n == 1 for n in c["lens"]) > 50
    emb = fe.embed_clips(c["wave"], c["offs"])
    emb_dev = fe.embed_clips(c["wave"], torch.from_numpy(c["offs"]).to(gpu))
    fe.check_device_plan()
    assert fe.last_logmel_kind() == KIND[kernel]
    assert torch.equal(emb, emb_dev)
    assert bool(torch.isfinite(emb).all())
    err = np.abs(emb[c["pick"]].cpu().numpy().astype(np.float64) - c["ref"]).max(axis=1)
    print(f"{kernel}: max |embedding - oracle| over {len(c['pick'])} clips = {err.max():.3e}")
    np.testing.assert_allclose(emb[c["pick"]].cpu().numpy(), c["ref"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_length_clips(gpu, kernel):
    """a batch made only of zero-length clips, and a zero-length clip between two long ones: one segment with no real samples each
    (seg_valid 0, chunk records covering 0 samples), embedded as the oracle embeds an all-zero segment"""
    import torch
    fe = _extractor(gpu, kernel)
    L, hop = fe.segment_length, fe.hop_length
    wave = _audio(gpu, 6 * L + 45, 31)
    host = wave.cpu().numpy()
    for offs in (np.full(6, 5, np.int64), np.asarray([0, 0, 0], np.int64), np.asarray([3, 3 * L + 20, 3 * L + 20, 6 * L + 45], np.int64)):
        ref = O.embed_clips([host[a:b] for a, b in zip(offs[:-1], offs[1:])], L, hop, fe.proj_w, fe.proj_b, tuple(LEVELS), "max")
        emb = fe.embed_clips(wave, offs)
        got = _check_host_plan(fe, kernel, offs)
        emb_dev = fe.embed_clips(wave, torch.from_numpy(offs).to(gpu))
        _check_dev_plan(fe, kernel, offs, wave.numel())
        fe.check_device_plan()
        empty = [b for b in range(len(offs) - 1) if offs[b] == offs[b + 1]]
        assert empty and all(got["seg_valid"][got["clip_seg"][b]] == 0 and got["clip_seg"][b + 1] - got["clip_seg"][b] == 1 for b in empty)
        assert torch.equal(emb, emb_dev)
        np.testing.assert_allclose(emb.cpu().numpy(), ref, rtol=0, atol=1e-4)


# ---- c. repairs of device-resident offsets ---------------------------------------------------------------------------------------

REASONS = {1: "offsets outside the wave buffer", 2: "offsets not non-decreasing", 4: "more segments than the wave buffer can hold"}
_TOTAL, _CASES = M.repair_cases(M.L_SMALL, M.HOP_SMALL)


@pytest.mark.parametrize("name,offs,flags", _CASES, ids=[c[0] for c in _CASES])
@pytest.mark.parametrize("kernel", KERNELS)
def test_repaired_device_offsets(gpu, kernel, name, offs, flags):
    """every store of k_build_plan under its caps: the plan of bad offsets is the model's repaired plan exactly (the clip cut at the
    segment cap, the empty clips behind it), nothing faults, the report names every reason once, intact clips embed as in a clean
    batch, and the next clean batch is clean.  (What the rows of the repaired clips hold is unspecified: not asserted.)"""
    import torch
    fe = _extractor(gpu, kernel)
    L, hop = fe.segment_length, fe.hop_length
    total = _TOTAL
    wave = _audio(gpu, total, 77)
    assert wave.numel() == total
    good = torch.tensor([0, 3 * L, 3 * L + 1, 10 * L], device=gpu, dtype=torch.int64)
    ref = fe.embed_clips(wave, good)
    fe.check_device_plan()
    n_clips = len(offs) - 1
    out = fe.embed_clips(wave, torch.tensor(offs, device=gpu, dtype=torch.int64))
    torch.cuda.synchronize()                                             # a fault would surface here
    got = _check_dev_plan(fe, kernel, offs, total)                       # (asserts seg_cap == total // hop + n_clips, n_chunks <= chunk_cap)
    assert got["flags"] == flags and got["seg_cap"] == total // hop + n_clips
    M.check_repaired(got, n_clips, total, got["seg_cap"], flags)
    assert fe.last_plan()["flags"] == flags                              # reading the plan does not consume the report ...
    with pytest.raises(ValueError) as ei:
        fe.check_device_plan()                                           # ... which names every flagged reason
    for bit, why in REASONS.items():
        assert (why in str(ei.value)) == bool(flags & bit), (str(ei.value), flags)
    assert "a device-offset batch" in str(ei.value)
    fe.check_device_plan()                                               # reported once
    # clips whose own offsets were valid and whose segments all made it into the plan: bit for bit as in a clean batch
    want = M.plan(offs, L, hop, total=total, seg_cap=got["seg_cap"])
    intact = [b for b in range(n_clips) if 0 <= offs[b] <= offs[b + 1] <= total and want["clips"][b][2] == want["clips"][b][3]]
    assert intact, name
    for b in intact:
        alone = fe.embed_clips(wave, torch.tensor([offs[b], offs[b + 1]], device=gpu, dtype=torch.int64))
        assert torch.equal(out[b], alone[0]), (name, b)
    fe.check_device_plan()
    again = fe.embed_clips(wave, good)
    fe.check_device_plan()
    assert torch.equal(again, ref)


# ---- d. the handle's plan state --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_plan_state_across_a_sequence_of_calls(gpu, kernel):
    """plan cache (plan_key), device / host / explicit-segment plans replacing each other, the chunk plan switched off by the stage
    entry points, the two pinned staging slots reused by back-to-back batches: every result equals what a FRESH extractor returns for
    that single call, and last_plan() shows that call's plan"""
    import torch
    fe = _extractor(gpu, kernel)
    L, hop = fe.segment_length, fe.hop_length
    wave = _audio(gpu, 60 * L, 5)
    pcm = torch.round(wave * 32767.0).clamp(-32768, 32767).to(torch.int16)
    A = _offsets([0, 3 * L + 17, 1, L + hop, L - 1, L + 7 * hop + 3])
    Bo = 13 + _offsets([L + hop + 1, 0, 2 * L, L])
    tail = [_offsets([L + i * hop + i, i, 3 * L - i]) + 100 * i for i in range(1, 5)]
    segs = [wave[i * 1000:i * 1000 + n].cpu().numpy() for i, n in enumerate([L, L - 3, 1, 0, L // 2])]
    dev = lambda o: torch.from_numpy(o).to(gpu)

    def fresh(call):
        return call(_extractor(gpu, kernel))

    def host_plan(o):
        return lambda: _check_host_plan(fe, kernel, o)

    def dev_plan(o):
        return lambda: _check_dev_plan(fe, kernel, o, wave.numel())

    def seg_plan():
        got = fe.last_plan()
        want = {"n_clips": len(segs), "n_seg": len(segs), "flags": 0, "clip_seg": np.arange(len(segs) + 1, dtype=np.int64),
                "seg_start": np.arange(len(segs), dtype=np.int64) * L, "seg_valid": np.asarray([len(s) for s in segs], np.int32)}
        assert (got["kind"], got["geometry"], got["seg_cap"], got["chunk_cap"]) == ("segments", "none", len(segs), 0)
        M.assert_plan_equal(got, want, None)

    stage = {"fft": lambda f: f.log_mel(segs), "gemm": lambda f: f.normalize_segments(segs),
             "per_segment": lambda f: torch.stack(f.extract_features(segs))}[kernel]
    script = [
        ("host A", lambda f: f.embed_clips(wave, A), host_plan(A)),
        ("device A", lambda f: f.embed_clips(wave, dev(A)), dev_plan(A)),
        ("stage", stage, seg_plan),
        ("host A again", lambda f: f.embed_clips(wave, A), host_plan(A)),
        ("host A from the cache", lambda f: f.embed_clips(wave, A), host_plan(A)),
        ("host B", lambda f: f.embed_clips(wave, Bo), host_plan(Bo)),
        ("device B bf16", lambda f: f.embed_clips(wave, dev(Bo), out_dtype=torch.bfloat16), dev_plan(Bo)),
        ("host A int16", lambda f: f.embed_clips(pcm, A), host_plan(A)),
    ]
    for what, call, check in script:
        got = call(fe)
        check()
        want = fresh(call)
        assert got.dtype == want.dtype and torch.equal(got, want), what
        assert bool(torch.isfinite(got.float()).all()), what
    assert fe.embed_clips(wave, dev(Bo), out_dtype=torch.bfloat16).dtype == torch.bfloat16
    # four different host-offset batches back to back, nothing synchronises in between: the staging slots are reused every second call
    outs = [fe.embed_clips(wave, o) for o in tail]
    _check_host_plan(fe, kernel, tail[-1])
    for o, got in zip(tail, outs):
        assert torch.equal(got, fresh(lambda f: f.embed_clips(wave, o)))
    fe.check_device_plan()


# ---- e. which batch a repair is attributed to -------------------------------------------------------------------------------------

def test_a_bad_batch_is_never_reported_as_an_earlier_one(gpu, monkeypatch):
    """embed_clips polls the reports of EARLIER device-offset batches without waiting.  Here every non-waiting poll is preceded by a
    device synchronisation, i.e. the batch just enqueued has always completed by the time of the poll -- the case that used to make
    a bad batch name itself "an earlier batch" and hand its own clamped output back as a valid .result."""
    import torch
    fe = _extractor(gpu, "fft")
    L = fe.segment_length
    wave = _audio(gpu, 10 * L, 77)
    good = torch.tensor([0, 3 * L, 3 * L + 1, 10 * L], device=gpu, dtype=torch.int64)
    bad = torch.tensor([0, 3 * L, 3 * L + 1, 40 * L], device=gpu, dtype=torch.int64)
    ref = fe.embed_clips(wave, good)
    fe.check_device_plan()
    poll = fe.check_device_plan

    def completed_then_poll(what="a device-offset batch", wait=True):
        if not wait:
            torch.cuda.synchronize()
        return poll(what=what, wait=wait)

    monkeypatch.setattr(fe, "check_device_plan", completed_then_poll)
    out = fe.embed_clips(wave, bad)                                       # must RETURN: the report is this batch's own
    assert torch.equal(out[:2], ref[:2])
    with pytest.raises(ValueError, match="of a device-offset batch were invalid .offsets outside the wave buffer."):
        fe.check_device_plan()
    fe.check_device_plan()
    fe.embed_clips(wave, bad)
    with pytest.raises(ValueError, match="an earlier device-offset batch") as ei:
        fe.embed_clips(wave, good)
    assert torch.equal(ei.value.result, ref)                              # the raising call's own batch was valid and is not lost
    fe.check_device_plan()                                                # the bad batch was reported once; the good one is clean
    assert torch.equal(fe.embed_clips(wave, good), ref)
    fe.check_device_plan()
