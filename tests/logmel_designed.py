"""Designed audio for the log-mel kernels, its float64 oracle, a plain float32 reference and the error bound that follows from it.
No GPU here: tests/test_logmel_designed_inputs.py checks the inputs and the references on the CPU, tests/test_gpu_logmel_designed.py
compares the four kernels' rows with `oracle` under `bound`.

The suite's usual audio (oracle/synth.py: white noise plus a strong triangle wave) keeps every mel band of every frame within about
three decades of the segment maximum, far from the `max - 8` clamp, and gives every segment of a clip the same mean and level.  The
inputs here are the opposite: tones and a chirp (most cells at or under the clamp, leakage 6 to 8 decades down), band-limited noise
over a floor, a gated clip (a segment of exact zeros inside a live clip), level steps and DC steps (overlapping segments whose scale
and mean differ by orders of magnitude: what the shared-frame kernels' per-owner correction has to undo) and a slow wander.

The bound of a kernel's error against `oracle`, per input and per region (bands 0-1, where the shared-frame mean correction acts,
and bands 2-79): max(1e-4, 4 x the error of `reference32` there).  1e-4 is the project's bar; `reference32` is the HF front-end
restated in float32 with numpy alone (no code and no trick shared with the kernels), and 4 is the factor the training tests allow
over a float32 reference.  Nothing is bounded against a kernel's own output."""
import numpy as np

from oracle import radad_oracle as O

FS = 16000
N = 64000                     # three 2 s segments at hop 1 s
N_FFT, FFT_HOP, N_MELS = 400, 160, 80
BAR = 1e-4
FACTOR = 4.0

NAMES = ("tone_on_bin", "tone_off_bin", "tone_floor60", "lowpass_floor70", "chirp", "gated", "level_step60", "dc_step",
         "dc_step_tonal", "dc_offset_quiet", "wander", "short_tone")


def make(name, n=N, seed=20260):
    """the input `name`, float32 at 16 kHz"""
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    nz, nz2 = rng.standard_normal(n), rng.standard_normal(n)
    step = np.where(t < 30000, 1.0, -1.0)
    tone_on = 0.5 * np.sin(2 * np.pi * 1000.0 * t / FS)
    tone_off = 0.5 * np.sin(2 * np.pi * 440.3 * t / FS)
    if name == "tone_on_bin":
        x = tone_on
    elif name == "tone_off_bin":
        x = tone_off
    elif name == "tone_floor60":
        x = tone_on + 5e-4 * nz
    elif name == "lowpass_floor70":
        spec = np.fft.rfft(nz)
        spec[np.fft.rfftfreq(n, 1.0 / FS) >= 2000.0] = 0.0
        lp = np.fft.irfft(spec, n)
        x = lp + 3e-4 * lp.std() * nz2
    elif name == "chirp":
        x = np.sin(2 * np.pi * (100.0 * t / FS + (7800.0 / (2 * n)) * t * t / FS))
    elif name == "gated":
        x = np.where(t < 8000, nz, 0.0)
    elif name == "level_step60":
        x = nz * np.where(t < 20000, 1.0, 1e-3)
    elif name == "dc_step":
        x = 0.3 * nz + 0.25 * step
    elif name == "dc_step_tonal":
        x = 0.3 * np.sin(2 * np.pi * 2000.0 * t / FS) + 1e-3 * nz + 0.025 * step
    elif name == "dc_offset_quiet":
        x = 0.3 + 0.05 * nz
    elif name == "wander":
        x = 0.2 * nz * np.abs(np.sin(2 * np.pi * 1.3 * t / FS)) ** 4 + 2e-3 * np.sin(2 * np.pi * 0.4 * t / FS)
    elif name == "short_tone":
        x = (tone_off + 0.1)[:20000]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, np.float32)


def segments(clip, seg=32000, hop=16000):
    """the clip's planned segments (segmenter.py:15-39), zero padded, float32 [S, seg]"""
    return np.stack([np.asarray(s, np.float32) for s in O.segment_audio(np.asarray(clip, np.float32), seg, hop)])


def oracle(clip, seg=32000, hop=16000):
    """float64 [S, T, 80]: O.log_mel(O.zero_mean_unit_var(segment)) of every planned segment"""
    return np.stack([O.log_mel(O.zero_mean_unit_var(s)) for s in segments(clip, seg, hop)])


def oracle_log10(clip, seg=32000, hop=16000, normalize=True):
    """float64 [S, T, 80]: log10(max(mel, 1e-10)) before the clamp (decades; for the properties the inputs are named for)"""
    out = []
    for s in segments(clip, seg, hop):
        x = O.zero_mean_unit_var(s) if normalize else np.asarray(s, np.float64)
        xp = np.pad(x, (N_FFT // 2, N_FFT // 2), mode="reflect")
        idx = np.arange(len(x) // FFT_HOP)[:, None] * FFT_HOP + np.arange(N_FFT)[None, :]
        spec = np.fft.rfft(xp[idx] * O.hann_periodic(N_FFT)[None, :], axis=1)
        out.append(np.log10(np.maximum((spec.real ** 2 + spec.imag ** 2) @ O.mel_filter_bank(), 1e-10)))
    return np.stack(out)


_F32 = np.float32
_HANN32 = O.hann_periodic(N_FFT).astype(np.float32)
_FB32 = O.mel_filter_bank().astype(np.float32)


def _frames32(x):
    """float32 [T, 400]: the reflect-padded segment cut into frames (the last frame dropped, feature_extraction_whisper.py:151)"""
    xp = np.pad(np.asarray(x, np.float32), (N_FFT // 2, N_FFT // 2), mode="reflect")
    idx = np.arange(len(x) // FFT_HOP)[:, None] * FFT_HOP + np.arange(N_FFT)[None, :]
    return xp[idx]


def _rfft32(frames):
    spec = np.fft.rfft(frames, axis=1)
    return spec if spec.dtype == np.complex64 else spec.astype(np.complex64)      # (complex64 as it comes under numpy >= 2)


def _finish32(logs):
    logs = np.maximum(logs, logs.max() - _F32(8.0))
    return ((logs + _F32(4.0)) / _F32(4.0)).astype(np.float32)


def reference32(clip, seg=32000, hop=16000):
    """float32 [S, T, 80]: the HF front-end in float32 -- numpy's mean and variance of the float32 segment, reflect padding, a float32
    periodic hann window, np.fft.rfft, power spectrum, mel product, log10 / clamp / scale, every step in float32"""
    out = []
    for s in segments(clip, seg, hop):
        x = (s - s.mean(dtype=np.float32)) / np.sqrt(s.var(dtype=np.float32) + _F32(1e-7))
        spec = _rfft32(_frames32(x) * _HANN32[None, :])
        power = spec.real * spec.real + spec.imag * spec.imag
        out.append(_finish32(np.log10(np.maximum(power @ _FB32, _F32(1e-10)))))
    return np.stack(out)


def shared_identity32(clip, seg=32000, hop=16000, form="factored"):
    """float32 statement of the shared-frame kernels' identity (csrc/logmel_h.inc): frames of x - c are transformed once, an owner s
    gets mel_s = (mel' + bin 1's share) / sd_s^2 with X_s[1] = (X'[1] + d) / sd_s, d = -100 (c - m_s).  Returns {pivot: [S, T, 80]}
    for the pivots "own" (c = m_s), "prev" and "next" (c = the mean of the neighbouring segment; the segment's own at the clip's ends).
      form "factored" (what the kernels ship): bin 1 stays out of mel' and every owner adds fb[1][b] ((Re X'[1] + d)^2 + Im X'[1]^2);
      form "expanded" (what they shipped before): mel' holds fb[1][b] |X'[1]|^2 and fb[1][b] (2 d Re X'[1] + d^2) is added -- three
      large terms that cancel when d is large against what the frame holds in bin 1."""
    segs = segments(clip, seg, hop)
    mean = np.array([s.mean(dtype=np.float32) for s in segs], np.float32)
    inv = np.array([_F32(1.0) / np.sqrt(s.var(dtype=np.float32) + _F32(1e-7)) for s in segs], np.float32)
    S = len(segs)
    fb1 = _FB32[1, :2]
    fb_rest = _FB32.copy()
    fb_rest[1, :] = 0.0
    out = {}
    for pivot, shift in (("own", 0), ("prev", -1), ("next", 1)):
        rows = []
        for s in range(S):
            c = mean[min(max(s + shift, 0), S - 1)]
            spec = _rfft32((_frames32(segs[s]) - c) * _HANN32[None, :])
            power = spec.real * spec.real + spec.imag * spec.imag
            d = _F32(-100.0) * (c - mean[s])
            g2 = inv[s] * inv[s]
            re1, im1 = spec.real[:, 1], spec.imag[:, 1]
            if form == "factored":
                z = power @ fb_rest
                low = z[:, :2] + fb1[None, :] * ((re1 + d) * (re1 + d) + im1 * im1)[:, None]
            else:
                z = power @ _FB32
                low = z[:, :2] + fb1[None, :] * (_F32(2.0) * d * re1 + d * d)[:, None]
            with np.errstate(divide="ignore"):
                logs = np.maximum(np.log10(z) + _F32(2.0) * np.log10(inv[s]), _F32(-10.0)).astype(np.float32)
            logs[:, :2] = np.log10(np.maximum(low * g2, _F32(1e-10)))
            rows.append(_finish32(logs))
        out[pivot] = np.stack(rows)
    return out


def errors(got, want):
    """worst |got - want| over bands 0-1 and over bands 2-79 ([S, T, 80] each), and a histogram of the worst error by decades under
    the segment maximum (want's cells at 0-1, 1-2, ... 7-8 decades down, the clamped ones last), for the printed line"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.shape[-1] == N_MELS, (got.shape, want.shape)
    err = np.abs(got - want)
    down = 4.0 * (want.max(axis=(1, 2), keepdims=True) - want)                  # decades under the segment's maximum (<= 8)
    hist = []
    for lo in range(9):
        sel = (down >= lo) & (down < lo + 1) if lo < 8 else down >= 8.0 - 1e-12
        hist.append(float(err[sel].max()) if sel.any() else 0.0)
    finite = bool(np.isfinite(got).all())
    return {"low": float(np.nanmax(err[..., :2])) if finite else float("inf"),
            "rest": float(np.nanmax(err[..., 2:])) if finite else float("inf"), "hist": hist}


_BOUNDS = {}


def bounds(name, seg=32000, hop=16000, n=None):
    """{"low", "rest"}: max(1e-4, 4 x reference32's error against the oracle) for the input `name` (cut to n samples when given) under
    this segmentation, with the reference's own errors as "ref_low", "ref_rest"; computed once"""
    key = (name, seg, hop, n)
    if key not in _BOUNDS:
        clip = make(name) if n is None else clipped(name, n)
        e = errors(reference32(clip, seg, hop), oracle(clip, seg, hop))
        _BOUNDS[key] = {"low": max(BAR, FACTOR * e["low"]), "rest": max(BAR, FACTOR * e["rest"]), "ref_low": e["low"], "ref_rest": e["rest"]}
    return _BOUNDS[key]


def clipped(name, n):
    """the input cut to its first n samples, or continued to n samples (the same formulas over a longer time axis)"""
    return make(name)[:n] if n <= len(make(name)) else make(name, n=n)


def line(label, e, b):
    """one printed line of the table: measured pair, the float32 reference's pair, the bound, worst error by decade"""
    return (f"{label:<52s} low {e['low']:.2e} rest {e['rest']:.2e} | ref32 {b['ref_low']:.2e} {b['ref_rest']:.2e} | bound "
            f"{b['low']:.2e} {b['rest']:.2e} | by decade " + " ".join(f"{h:.0e}" for h in e["hist"]))
