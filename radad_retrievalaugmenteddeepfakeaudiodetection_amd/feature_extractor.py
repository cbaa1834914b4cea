"""Feature extractors behind the reference's protocol (`.feature_dim`, `.extract_features(segments)`),
feature_extractor.py:6-170, selected by `build_feature_extractor` (pipeline.py:54-65).

The reference's three extractors are a HuggingFace front-end plus a PRETRAINED transformer fetched by
model name (feature_extractor.py:14-15, :70-71, :131-132).  Those weights are not part of the repository, so
this build's native extractor keeps the front-ends the reference calls -- per-segment zero-mean /
unit-variance (HF Wav2Vec2FeatureExtractor) and the HF Whisper log-mel spectrogram -- and puts a dense
frame projection [T,80] x [80,F] where the encoder forward sits.  Everything runs in csrc/embed.hip;
`embed_clips` is the batched entry that replaces the nested loops of process_audio_batch.
Any object with the same two members can still be plugged into the pipeline shell.
"""
import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib

N_FFT, FFT_HOP, N_MELS, N_BINS = 400, 160, 80, 201


def mel_filter_bank_slaney(n_bins: int = N_BINS, n_mels: int = N_MELS, fmin: float = 0.0, fmax: float = 8000.0,
                           sr: int = 16000) -> np.ndarray:
    """Slaney-scale, slaney-normalised triangular filters [n_bins, n_mels] -- the bank the HF Whisper
    front-end builds (feature_extraction_whisper.py:94-103), float64."""
    def hz2mel(f):
        f = np.asarray(f, np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)

    def mel2hz(m):
        m = np.asarray(m, np.float64)
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)

    edges = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), n_mels + 2))
    bins = np.linspace(0, sr // 2, n_bins)
    width = np.diff(edges)
    rel = edges[None, :] - bins[:, None]
    tri = np.maximum(0.0, np.minimum(-rel[:, :-2] / width[:-1], rel[:, 2:] / width[1:]))
    return tri * (2.0 / (edges[2:] - edges[:-2]))[None, :]


def synthetic_projection(feat_dim: int, seed: int):
    """Seeded stand-in for trained projection weights: W ~ N(0, 1/80), b ~ N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N_MELS, feat_dim)) / np.sqrt(N_MELS)).astype(np.float32)
    b = (0.1 * rng.standard_normal(feat_dim)).astype(np.float32)
    return w, b


class MelProjectionFeatureExtractor:
    """normalise -> log-mel -> frame projection, on the GPU.

    extract_features(segments) follows the reference protocol (list of 1-D arrays -> list of [T, F] tensors
    on config.device, as Wav2Vec2FeatureExtractor.extract_features returns them, feature_extractor.py:21-52).
    """

    def __init__(self, config, levels=None, pool_mode=None, weights=None):
        import torch
        self.config = config
        self.device = torch.device(config.device)
        if self.device.type != "cuda":
            raise RuntimeError("MelProjectionFeatureExtractor needs a ROCm device: the HIP path has no CPU fallback")
        self.feature_dim = int(getattr(config, "feature_dim", 512))
        self.segment_length = int(config.segment_length * config.sample_rate)
        self.hop_length = int(self.segment_length * (1 - config.segment_overlap))
        self.levels = list(levels if levels is not None else config.tpp_levels)
        mode = pool_mode if pool_mode is not None else config.tpp_pooling_type
        if mode not in ("max", "avg"):
            raise ValueError(f"Unsupported pooling type: {mode}")           # pooling.py:81
        self.pool_mode = mode
        if weights is None:
            path = getattr(config, "melproj_weights_path", None)
            if path:
                z = np.load(path)
                weights = (z["w"], z["b"])
            else:
                weights = synthetic_projection(self.feature_dim, int(getattr(config, "melproj_seed", 20251003)))
        w, b = (np.ascontiguousarray(weights[0], np.float32), np.ascontiguousarray(weights[1], np.float32))
        if w.shape != (N_MELS, self.feature_dim) or b.shape != (self.feature_dim,):
            raise ValueError(f"projection weights must be [{N_MELS},{self.feature_dim}] and [{self.feature_dim}]")
        self.proj_w, self.proj_b = w, b
        self.mel_filters = np.ascontiguousarray(mel_filter_bank_slaney(), np.float32)

        lib = _lib.load()
        cfg = _lib.EmbedCfg()
        cfg.segment_length, cfg.hop_length = self.segment_length, self.hop_length
        cfg.normalize = 1 if getattr(config, "melproj_normalize", True) else 0
        cfg.n_fft, cfg.fft_hop, cfg.n_mels = N_FFT, FFT_HOP, N_MELS
        cfg.padded_samples = int(getattr(config, "melproj_padded_samples", 0) or 0)
        cfg.feat_dim = self.feature_dim
        cfg.n_levels = len(self.levels)
        if not 1 <= len(self.levels) <= _lib.MAX_LEVELS:
            raise ValueError(f"1..{_lib.MAX_LEVELS} pyramid levels supported")
        for i, l in enumerate(self.levels):
            cfg.levels[i] = int(l)
        cfg.pool_mode = _lib.POOL_MAX if mode == "max" else _lib.POOL_AVG
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        # which log-mel kernel (all within the parity bar; A/B measurements and the parity tests choose through these knobs, read the
        # way the reference reads its optional ones): melproj_share_frames (default True), melproj_logmel_f32 (False),
        # melproj_logmel_fft (True: the radix FFT on the vector ALU; False: the DFT-as-GEMM on the matrix pipe)
        flags = 0
        if not getattr(config, "melproj_share_frames", True):
            flags |= _lib.EMBED_NO_SHARED_FRAMES
        if getattr(config, "melproj_logmel_f32", False):
            flags |= _lib.EMBED_LOGMEL_F32
        if not getattr(config, "melproj_logmel_fft", True):
            flags |= _lib.EMBED_LOGMEL_DFT_GEMM
        h = C.c_void_p()
        _lib.check(lib.radad_embed_create_ex(C.byref(cfg), flags, self.mel_filters.ctypes.data, w.ctypes.data, b.ctypes.data,
                                             self._dev_index, C.byref(h)), "radad_embed_create")
        self._h = h
        self._lib = lib
        d, t = C.c_int(), C.c_int()
        _lib.check(lib.radad_embed_output_dim(h, C.byref(d)))
        _lib.check(lib.radad_embed_num_frames(h, C.byref(t)))
        self.output_dim, self.num_frames = d.value, t.value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.radad_embed_destroy(h)
            except Exception:
                pass

    # ---- batched device path --------------------------------------------------------------------------
    def embed_clips(self, wave, clip_offsets, out_dtype=None):
        """wave: 1-D float32 CUDA tensor holding the clips back to back (or int16 PCM: converted on the device as librosa.load would,
        sample / 32768); clip_offsets: B+1 ints, either on the host
        (sequence / numpy) or an int64 CUDA tensor -- then the segment plan (segmenter.py:25-39) is built on the device and
        nothing synchronises with the host.  out_dtype: torch.float32 (default) or torch.bfloat16 (BASELINE config 5).
        Returns the clip embeddings [B, sum(levels)*F] (segment -> embed of pipeline.py:392-414)."""
        import torch
        _lib.require_cuda(wave, "wave")
        if wave.dtype == torch.int16:
            # 16-bit PCM as the audio files hold it: sample / 32768 on the device (what librosa.load returns), into a buffer this
            # extractor keeps -- an upload of the PCM moves half the bytes of the float samples over PCIe.  (ONE buffer per extractor:
            # int16 batches of one extractor must be issued on one stream at a time, like everything else of a handle.)
            pcm = wave.contiguous()
            if getattr(self, "_pcm_f32", None) is None or self._pcm_f32.numel() < pcm.numel() or self._pcm_f32.device != pcm.device:
                self._pcm_f32 = torch.empty(pcm.numel(), device=pcm.device, dtype=torch.float32)
            wave = self._pcm_f32[:pcm.numel()]
            with torch.cuda.device(pcm.device):
                _lib.check(self._lib.radad_pcm16_to_f32(pcm.data_ptr(), wave.data_ptr(), pcm.numel(), pcm.device.index or 0,
                                                        _lib.stream_ptr(pcm.device)), "radad_pcm16_to_f32")
        elif wave.dtype != torch.float32 or not wave.is_contiguous():
            wave = wave.contiguous().float()
        out_dtype = out_dtype or torch.float32
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be torch.float32 or torch.bfloat16")
        code = _lib.OUT_BF16 if out_dtype == torch.bfloat16 else _lib.OUT_F32
        if isinstance(clip_offsets, torch.Tensor) and clip_offsets.is_cuda:
            offs = clip_offsets.contiguous().to(torch.int64)
            n_clips = offs.numel() - 1
            if n_clips < 0:
                raise ValueError("clip_offsets must hold at least one entry")
            # device offsets cannot be checked here without a synchronisation: the plan kernel clamps them (no out-of-bounds
            # read whatever the tensor holds) and flags what it repaired.  Earlier batches that have COMPLETED are collected without
            # waiting (a caller may queue batches back to back) BEFORE this one is enqueued -- polled afterwards, a small batch of
            # this call could finish first and be reported as an earlier one, its clamped output handed back as a valid `.result`.
            # THIS batch is enqueued whatever the poll found; then the exception names the earlier ones and carries this call's
            # output (`.result`), so a valid batch is never lost to another batch's offsets;
            # check_device_plan() after the last batch waits for the rest, this one included
            self._dev_batches = getattr(self, "_dev_batches", 0) + 1
            earlier = None
            try:
                self.check_device_plan(what=f"an earlier device-offset batch (before batch #{self._dev_batches} of this extractor, which HAS "
                                            "been enqueued: its output is this exception's .result)", wait=False)
            except ValueError as e:
                earlier = e
            out = torch.empty((n_clips, self.output_dim), device=wave.device, dtype=out_dtype)
            try:
                with torch.cuda.device(wave.device):
                    _lib.check(self._lib.radad_embed_forward_dev(self._h, wave.data_ptr(), offs.data_ptr(), n_clips, wave.numel(),
                                                                 out.data_ptr(), code, _lib.stream_ptr(wave.device)),
                               "radad_embed_forward_dev")
            except Exception as e:
                if earlier is not None:                                    # (the report was consumed: it travels with this failure)
                    raise e from earlier
                raise
            if earlier is not None:
                earlier.result = out
                raise earlier
            return out
        offs = np.ascontiguousarray(np.asarray(clip_offsets, np.int64))
        n_clips = len(offs) - 1
        if n_clips < 0 or (n_clips >= 0 and (offs[0] < 0 or offs[-1] > wave.numel())):
            raise ValueError("clip_offsets outside the wave buffer")
        out = torch.empty((n_clips, self.output_dim), device=wave.device, dtype=out_dtype)
        with torch.cuda.device(wave.device):
            _lib.check(self._lib.radad_embed_forward_ex(self._h, wave.data_ptr(), offs.ctypes.data_as(_lib.c_i64p),
                                                        n_clips, out.data_ptr(), code, _lib.stream_ptr(wave.device)),
                       "radad_embed_forward")
        return out

    def check_device_plan(self, what="a device-offset batch", wait=True):
        """ValueError if the segment-plan kernel had to repair the device-resident clip offsets of an embed_clips(wave, <CUDA
        offsets>) call since the last report (the host-offset path raises up front, as segmenter.py:18-19 does for bad input).
        wait=True (the default: call it after the LAST batch) waits for every batch in flight; wait=False reports only batches
        that have completed and never blocks -- embed_clips does that before each launch."""
        f, pend = C.c_int(), C.c_int()
        if wait:
            _lib.check(self._lib.radad_embed_plan_flags(self._h, C.byref(f)), "radad_embed_plan_flags")
        else:
            _lib.check(self._lib.radad_embed_plan_flags_poll(self._h, C.byref(f), C.byref(pend)), "radad_embed_plan_flags_poll")
        if f.value:
            why = [m for b, m in ((1, "offsets outside the wave buffer"), (2, "offsets not non-decreasing"),
                                  (4, "more segments than the wave buffer can hold")) if f.value & b]
            raise ValueError(f"clip_offsets of {what} were invalid ({', '.join(why)}); its embeddings are not those of the intended clips")

    def last_plan(self) -> dict:
        """Diagnostic: the segment and chunk plan the most recent embed_clips / stage call of this extractor built, read back from the
        handle (radad_embed_last_plan; waits for the current stream, changes nothing, does not consume check_device_plan's report).
        Counts and caps as ints, `flags` (the repair bits of that plan), `kind` (_lib.PLAN_KINDS), `geometry` (_lib.PLAN_CHUNKS),
        clip_seg [n_clips + 1], seg_start / seg_valid [n_seg] and the chunk records chunk_beg / chunk_seg0 / chunk_n_seg / chunk_cidx /
        chunk_avail [n_chunks] as numpy arrays."""
        import torch
        info = (C.c_int64 * 8)()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            _lib.check(self._lib.radad_embed_last_plan(self._h, info, None, 0, None, None, 0, None, None, 0, st), "radad_embed_last_plan")
            n_clips, n_seg, n_chunks = int(info[0]), int(info[1]), int(info[2])
            clip_seg, seg_start, seg_valid = np.empty(n_clips + 1, np.int64), np.empty(n_seg, np.int64), np.empty(n_seg, np.int32)
            beg, fields = np.empty(n_chunks, np.int64), np.empty((n_chunks, 4), np.int32)
            _lib.check(self._lib.radad_embed_last_plan(self._h, info, clip_seg.ctypes.data_as(_lib.c_i64p), n_clips + 1,
                                                       seg_start.ctypes.data_as(_lib.c_i64p), seg_valid.ctypes.data_as(_lib.c_i32p), n_seg,
                                                       beg.ctypes.data_as(_lib.c_i64p), fields.ctypes.data_as(_lib.c_i32p), n_chunks, st),
                       "radad_embed_last_plan")
        return {"n_clips": n_clips, "n_seg": n_seg, "n_chunks": n_chunks, "flags": int(info[3]), "seg_cap": int(info[4]),
                "chunk_cap": int(info[5]), "kind": _lib.PLAN_KINDS[int(info[6])], "geometry": _lib.PLAN_CHUNKS[int(info[7])],
                "clip_seg": clip_seg, "seg_start": seg_start, "seg_valid": seg_valid, "chunk_beg": beg,
                "chunk_seg0": fields[:, 0].copy(), "chunk_n_seg": fields[:, 1].copy(), "chunk_cidx": fields[:, 2].copy(),
                "chunk_avail": fields[:, 3].copy()}

    def last_logmel_kind(self) -> str:
        """"per_segment" (k_logmel_h: one transform per segment and frame), "clip_frames" (k_logmel_h_clip: the frames overlapping
        segments share are transformed once, DFT-as-GEMM on the matrix pipe) or "clip_frames_fft" (k_logmel_fft_clip: the same work
        list as a radix FFT on the vector ALU, the default) -- which log-mel kernel the most recent call took"""
        k = C.c_int()
        _lib.check(self._lib.radad_embed_last_logmel_kind(self._h, C.byref(k)), "radad_embed_last_logmel_kind")
        return {0: "per_segment", 1: "clip_frames", 2: "clip_frames_fft"}[k.value]

    def last_logmel(self):
        """Diagnostic: the log-mel rows [S, T, 80] the most recent embed_clips / stage call of this extractor computed, segments in plan
        order, clamped at each segment's max - 8 and scaled (x + 4) / 4 as log_mel() returns them (radad_embed_last_logmel: one small
        kernel on the current stream, nothing of the handle changes)."""
        import torch
        n = C.c_int64()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            _lib.check(self._lib.radad_embed_last_logmel(self._h, None, 0, C.byref(n), st), "radad_embed_last_logmel")
            out = torch.empty((n.value, self.num_frames, N_MELS), device=self.device, dtype=torch.float32)
            _lib.check(self._lib.radad_embed_last_logmel(self._h, out.data_ptr(), n.value, C.byref(n), st), "radad_embed_last_logmel")
        return out

    def profile(self, enable: bool = True):
        _lib.check(self._lib.radad_embed_profile(self._h, 1 if enable else 0), "radad_embed_profile")

    def profile_read(self):
        """(k_logmel ms list, k_proj_pool ms list) of the recorded radad_embed_forward calls"""
        a, b, n = (C.c_float * 64)(), (C.c_float * 64)(), C.c_int()
        _lib.check(self._lib.radad_embed_profile_read(self._h, a, b, 64, C.byref(n)), "radad_embed_profile_read")
        return [float(a[i]) for i in range(n.value)], [float(b[i]) for i in range(n.value)]

    def _stage(self, fn, segments, out_shape_tail):
        """run a per-stage entry point on a list of host segments (each <= segment_length samples)"""
        import torch
        L = self.segment_length
        valid = np.asarray([min(len(s), L) for s in segments], np.int32)
        flat = np.zeros(len(segments) * L, np.float32)
        for i, s in enumerate(segments):
            if np.asarray(s).ndim != 1:
                raise ValueError("Expected 1D audio array")
            flat[i * L:i * L + valid[i]] = np.asarray(s, np.float32)[:valid[i]]
        starts = np.arange(len(segments), dtype=np.int64) * L
        wave = torch.from_numpy(flat).to(self.device)
        out = torch.empty((len(segments),) + tuple(out_shape_tail), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, wave.data_ptr(), starts.ctypes.data_as(_lib.c_i64p), valid.ctypes.data_as(_lib.c_i32p),
                          len(segments), out.data_ptr(), _lib.stream_ptr(self.device)))
        return out

    # ---- reference protocol ---------------------------------------------------------------------------
    def extract_features(self, audio_segments: List[np.ndarray], move_to_cpu: bool = False):
        """feature_extractor.py:21-52: list of S segments -> list of S tensors [T, F]."""
        if len(audio_segments) == 0:
            return []
        feats = self._stage(self._lib.radad_embed_frame_features, audio_segments, (self.num_frames, self.feature_dim))
        return [f.cpu() if move_to_cpu else f for f in feats]

    def normalize_segments(self, audio_segments):
        """HF Wav2Vec2FeatureExtractor zero-mean/unit-variance (feature_extraction_wav2vec2.py:95) -> [S, L]."""
        return self._stage(self._lib.radad_embed_normalize, audio_segments, (self.segment_length,))

    def log_mel(self, audio_segments):
        """HF Whisper log-mel (feature_extraction_whisper.py:135-168) -> [S, T, 80] (HF: [S, 80, T])."""
        return self._stage(self._lib.radad_embed_logmel, audio_segments, (self.num_frames, N_MELS))


# ---- the reference's three named extractors: HIP front-end + a locally stored HuggingFace encoder ---------------------------------
# The reference fetches processor and model by NAME from the hub (feature_extractor.py:14-15, :70-71, :131-132).  Here the configured
# name is a LOCAL directory (save_pretrained layout; `local_files_only=True`: nothing is ever fetched): the front-end the HF processor
# would run on the CPU -- zero-mean / unit-variance (K1) or the 30 s-padded Whisper log-mel (K2) -- runs in csrc/embed.hip, the encoder
# forward is the HuggingFace module itself on the ROCm device (third-party arithmetic with third-party weights: not reproduced).

def _local_model_dir(name, what):
    import os
    if not isinstance(name, str) or not os.path.isdir(name) or not os.path.isfile(os.path.join(name, "config.json")):
        raise FileNotFoundError(
            f"{what}: {name!r} is not a local model directory (expected config.json + weights as written by save_pretrained).  This "
            "build never downloads: point the config's model name at a local copy of the encoder the reference fetches from the hub "
            "(feature_extractor.py:14-15,70-71,131-132), or use feature_extractor_type='melproj'.")
    return name


def _preprocessor_flag(model_dir, key, default):
    """one key of the directory's preprocessor_config.json (what the HF processor's from_pretrained would read)"""
    import json
    import os
    path = os.path.join(model_dir, "preprocessor_config.json")
    if os.path.isfile(path):
        with open(path) as f:
            return json.load(f).get(key, default)
    return default


class _FrontEnd(MelProjectionFeatureExtractor):
    """the HIP front-end kernels alone (the projection weights of the handle are never used)"""

    def __init__(self, config, padded_samples=0, normalize=False):
        import copy
        cfg = copy.copy(config)
        cfg.feature_dim, cfg.tpp_levels, cfg.tpp_pooling_type = 64, [1], "max"
        # normalize: K1 (zero-mean / unit-variance per segment) for the wav2vec2 / WavLM front-end; the Whisper processor does not normalise
        cfg.melproj_padded_samples, cfg.melproj_normalize, cfg.melproj_weights_path = padded_samples, bool(normalize), None
        super().__init__(cfg, weights=(np.zeros((N_MELS, 64), np.float32), np.zeros(64, np.float32)))


class Wav2Vec2FeatureExtractor:
    """feature_extractor.py:6-52.  K1 on the GPU (radad_embed_normalize == the processor's zero_mean_unit_var_norm,
    feature_extraction_wav2vec2.py:78-97, `padding=True` over equal-length segments), then Wav2Vec2Model with all hidden states,
    mean of config.wav2vec2_layers_to_use (:35-39)."""

    def __init__(self, config):
        import torch
        from transformers import Wav2Vec2Model
        self.config = config
        self.device = torch.device(config.device)
        d = _local_model_dir(config.wav2vec2_model_name, "Wav2Vec2FeatureExtractor")
        self.do_normalize = bool(_preprocessor_flag(d, "do_normalize", True))
        self.model = Wav2Vec2Model.from_pretrained(d, local_files_only=True).to(self.device)
        self.model.eval()
        self.feature_dim = self.model.config.hidden_size
        self._front = _FrontEnd(config, normalize=True)

    def _inputs(self, audio_segments):
        import torch
        if self.do_normalize:
            return self._front.normalize_segments(audio_segments)                          # [S, L] on the device
        L = self._front.segment_length
        return torch.stack([torch.from_numpy(np.pad(np.asarray(s, np.float32), (0, L - len(s)))) for s in audio_segments]).to(self.device)

    def extract_features(self, audio_segments: List[np.ndarray], move_to_cpu: bool = False):
        import torch
        if len(audio_segments) == 0:
            return []
        inputs = self._inputs(audio_segments)
        with torch.no_grad():
            hidden_states = self.model(inputs, output_hidden_states=True).hidden_states
            layers = getattr(self.config, "wav2vec2_layers_to_use", None)
            if layers:
                features = torch.mean(torch.stack([hidden_states[i] for i in layers]), dim=0)     # :36-39
            else:
                features = hidden_states[-1]
        return [f.cpu() if move_to_cpu else f for f in features]


class WhisperFeatureExtractor:
    """feature_extractor.py:54-115.  K2 on the GPU: every segment zero-padded to 30 s -> log-mel [80, 3000]
    (feature_extraction_whisper.py:135-168; radad_embed_logmel with padded_samples = 480 000), all segments of a call in one launch
    (the reference loops, :92), then WhisperModel.encoder -> last_hidden_state [1500, d_model] per segment, on the CPU (:112)."""

    def __init__(self, config):
        import torch
        from transformers import WhisperModel
        self.config = config
        self.device = torch.device(config.device)
        d = _local_model_dir(getattr(config, "whisper_model_name", "openai/whisper-small"), "WhisperFeatureExtractor")
        self.model = WhisperModel.from_pretrained(d, local_files_only=True).to(self.device)
        self.model.eval()
        self.feature_dim = int(getattr(self.model.config, "d_model", 768))
        n_mels = int(_preprocessor_flag(d, "feature_size", N_MELS))
        if n_mels != N_MELS or int(_preprocessor_flag(d, "n_fft", N_FFT)) != N_FFT or int(_preprocessor_flag(d, "hop_length", FFT_HOP)) != FFT_HOP:
            raise ValueError("the HIP log-mel front-end is built for n_fft 400 / hop 160 / 80 mel bands (whisper-tiny ... -medium)")
        self._use_amp = bool(getattr(config, "use_mixed_precision", False)) and self.device.type == "cuda"
        self._front = _FrontEnd(config, padded_samples=int(_preprocessor_flag(d, "n_samples", 480000)))

    def extract_features(self, segments):
        import torch
        if len(segments) == 0:
            return []
        mel = self._front.log_mel(segments).transpose(1, 2).contiguous()                    # [S, 80, 3000] on the device
        feats = []
        with torch.no_grad(), torch.autocast("cuda", enabled=self._use_amp):
            for s in range(mel.shape[0]):                                                   # one encoder call per segment, as :92-112
                hs = self.model.encoder(mel[s:s + 1]).last_hidden_state
                feats.append(hs.squeeze(0).detach().float().cpu())
        return feats


class WavLMFeatureExtractor:
    """feature_extractor.py:117-170.  The processor of a WavLM checkpoint is a Wav2Vec2FeatureExtractor whose preprocessor_config
    says whether it normalises (K1 on the GPU when it does); then WavLMModel -> last_hidden_state per segment, on the CPU (:168)."""

    def __init__(self, config):
        import torch
        from transformers import WavLMModel
        self.config = config
        self.device = torch.device(config.device)
        d = _local_model_dir(getattr(config, "wavlm_model_name", "microsoft/wavlm-base-plus"), "WavLMFeatureExtractor")
        self.do_normalize = bool(_preprocessor_flag(d, "do_normalize", True))
        self.return_attention_mask = bool(_preprocessor_flag(d, "return_attention_mask", False))
        self.model = WavLMModel.from_pretrained(d, local_files_only=True).to(self.device)
        self.model.eval()
        self.feature_dim = int(getattr(self.model.config, "hidden_size", 768))
        self._use_amp = bool(getattr(config, "use_mixed_precision", False)) and self.device.type == "cuda"
        self._front = _FrontEnd(config, normalize=True)

    _inputs = Wav2Vec2FeatureExtractor._inputs

    def extract_features(self, segments):
        import torch
        if len(segments) == 0:
            return []
        inputs = self._inputs(segments)
        feats = []
        with torch.no_grad(), torch.autocast("cuda", enabled=self._use_amp):
            for s in range(inputs.shape[0]):                                                # per segment, as :148-168
                mask = torch.ones_like(inputs[s:s + 1], dtype=torch.long) if self.return_attention_mask else None
                out = self.model(inputs[s:s + 1], attention_mask=mask)
                feats.append(out.last_hidden_state.squeeze(0).detach().float().cpu())
        return feats


def build_feature_extractor(config):
    """pipeline.py:54-65, plus 'melproj' (this build's native extractor: front-end + dense frame projection, one fused device
    path; the default here because the reference's three kinds need a pretrained encoder on the local disk)."""
    kind = getattr(config, "feature_extractor_type", "melproj").lower()
    if kind == "melproj":
        return MelProjectionFeatureExtractor(config)
    if kind == "whisper":
        return WhisperFeatureExtractor(config)
    if kind == "wavlm":
        return WavLMFeatureExtractor(config)
    if kind == "wav2vec2":
        return Wav2Vec2FeatureExtractor(config)
    raise ValueError(f"Unsupported feature_extractor_type={kind!r} (use 'melproj' | 'wav2vec2' | 'whisper' | 'wavlm').")
