"""The four log-mel kernels on designed audio (tests/logmel_designed.py), row by row against the float64 oracle.

Every other GPU test of these kernels feeds them oracle/synth.py's noise-plus-triangle audio, and sees the two shared-frame kernels
(k_logmel_fft_clip, the default, and k_logmel_h_clip) only behind a dense projection and pooling.  Here the rows a forward produced
are read back (MelProjectionFeatureExtractor.last_logmel) and compared per frame and per band: tones and a chirp (cells on the
clamp and in the two decades above it), a gated clip, level and DC steps inside a clip (the per-owner mean correction in bands 0-1),
ragged copies that move chunks and pivots.  The bound per input and region is max(1e-4, 4 x the float32 reference's own error);
every measured pair is printed before anything is asserted (run with -s)."""
import numpy as np
import pytest

import logmel_designed as D
from oracle import radad_oracle as O

pytestmark = pytest.mark.gpu

# the knobs tests/test_gpu_embed.py::test_log_mel_kernels_agree selects the kernels with, and what last_logmel_kind() must say
KERNELS = {
    "fft_clip": (dict(), "clip_frames_fft"),                              # k_logmel_fft_clip (the default)
    "h_clip": (dict(melproj_logmel_fft=False), "clip_frames"),            # k_logmel_h_clip
    "h": (dict(melproj_share_frames=False), "per_segment"),               # k_logmel_h
    "f32": (dict(melproj_logmel_f32=True), "per_segment"),                # k_logmel
}
RAGGED = [("dc_step_tonal", 48000), ("tone_off_bin", 48000), ("dc_step_tonal", 80000), ("tone_off_bin", 80000)]
SECOND = dict(seg=16000, hop=4000, n=40000)      # 1.0 s segments, 0.75 overlap: T = 100, H = 25, four owners


def _fe(gpu, kernel, **kw):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    kw = dict(dict(feature_dim=32, tpp_levels=[1]), **kw)
    cfg.update(device=gpu, **KERNELS[kernel][0], **kw)
    return R.MelProjectionFeatureExtractor(cfg)


# Two (kernel, input) pairs of the f16-matrix-pipe kernels miss the bound in bands 2-79, in cells 7 to 8 decades under the segment
# maximum (25 steps of three split-f16 products into one fp32 accumulator carry the tone's rounding noise into every bin; their load
# queue is counted by hand in inline assembly, so the float64 meeting of short sums that cured k_logmel is no small change there):
# kept as strict expected failures with the measured error, include/radad_hip.h says what was measured.  Bands 0-1, the gated clip
# and the two other kernels are never marked.
XFAIL = {
    ("h", "tone_floor60"): "k_logmel_h on tone_floor60: bands 2-79 off by 1.59e-4 (bound 1.0e-4; float32 reference 2.1e-5), cells 7-8 decades down",
    ("h_clip", "tone_floor60"): "k_logmel_h_clip on tone_floor60: bands 2-79 off by 1.18e-4 (bound 1.0e-4; float32 reference 2.1e-5), cells 7-8 decades down",
}


def _pairs(kernels, labels, *extra):
    return [pytest.param(k, *extra, l, marks=[pytest.mark.xfail(strict=True, reason=XFAIL[(k, l)])] if (k, l) in XFAIL else [])
            for k in kernels for l in labels]


class Batch:
    """clips back to back, their oracle rows and bounds (computed once per module, never changed), and the rows every (kernel, offsets)
    forward produced (one forward each, shared by the cases of its clips)"""

    def __init__(self, items, seg=32000, hop=16000, **cfg):
        self.seg, self.hop, self.cfg = seg, hop, cfg
        self.labels = [name if n is None else f"{name}[{n}]" for name, n in items]
        self.clips = [D.make(name) if n is None else D.clipped(name, n) for name, n in items]
        self.offs = np.concatenate([[0], np.cumsum([len(c) for c in self.clips])]).astype(np.int64)
        self.want = [D.oracle(c, seg, hop) for c in self.clips]
        self.bounds = [D.bounds(name, seg, hop, n) for name, n in items]
        self.seg_offs = np.concatenate([[0], np.cumsum([len(w) for w in self.want])])
        self.rows = {}

    def forward(self, gpu, kernel, offsets):
        import torch
        if (kernel, offsets) not in self.rows:
            fe = _fe(gpu, kernel, **self.cfg)
            assert (fe.segment_length, fe.hop_length, fe.num_frames) == (self.seg, self.hop, self.seg // 160)
            wave = torch.from_numpy(np.concatenate(self.clips)).to(gpu)
            fe.embed_clips(wave, torch.from_numpy(self.offs).to(gpu) if offsets == "device" else self.offs)
            assert fe.last_logmel_kind() == KERNELS[kernel][1]
            rows = fe.last_logmel().cpu().numpy()
            if offsets == "device":
                fe.check_device_plan()
            assert rows.shape == (self.seg_offs[-1], self.seg // 160, 80), rows.shape
            self.rows[(kernel, offsets)] = rows
        return self.rows[(kernel, offsets)]

    def check(self, gpu, kernel, offsets, label, what):
        """print the clip's measured pair, then assert it"""
        i = self.labels.index(label)
        got = self.forward(gpu, kernel, offsets)[self.seg_offs[i]:self.seg_offs[i + 1]]
        e, b = D.errors(got, self.want[i]), self.bounds[i]
        print("\n" + D.line(f"{what} {label}", e, b))
        assert bool(np.isfinite(got).all())
        assert e["low"] <= b["low"] and e["rest"] <= b["rest"], (label, e["low"], b["low"], e["rest"], b["rest"])


ITEMS = [(n, None) for n in D.NAMES] + RAGGED
LABELS = [name if n is None else f"{name}[{n}]" for name, n in ITEMS]
SECOND_LABELS = [f"{n}[{SECOND['n']}]" for n in ("level_step60", "dc_step", "dc_step_tonal")]
STAGE_NAMES = ("tone_off_bin", "tone_floor60", "chirp", "level_step60")


@pytest.fixture(scope="module")
def batch():
    return Batch(ITEMS)


@pytest.fixture(scope="module")
def batch_second():
    return Batch([(n, SECOND["n"]) for n in ("level_step60", "dc_step", "dc_step_tonal")], SECOND["seg"], SECOND["hop"],
                 segment_length=1.0, segment_overlap=0.75)


@pytest.mark.parametrize("kernel,offsets,label", _pairs(KERNELS, LABELS, "host") + _pairs(["fft_clip"], LABELS, "device"))
def test_rows_of_a_forward_match_the_oracle(gpu, batch, kernel, offsets, label):
    """(k_logmel, the fp32 kernel, missed the bound in bands 2-79 on the off-bin tone, 1.28e-4, and on tone_floor60, 2.96e-4, while
    its 200-tap sums ran through one fp32 accumulator; it adds four taps at a time on the matrix pipe now and the short sums meet in
    float64: 2.4e-5 and 3.7e-5.)"""
    batch.check(gpu, kernel, offsets, label, f"{kernel}/{offsets}")


@pytest.mark.parametrize("kernel,label", sorted(XFAIL))
def test_marked_pairs_hold_in_bands_0_1(gpu, batch, kernel, label):
    """an expected failure in bands 2-79 may not hide bands 0-1 or a non-finite row"""
    i = batch.labels.index(label)
    got = batch.forward(gpu, kernel, "host")[batch.seg_offs[i]:batch.seg_offs[i + 1]]
    e = D.errors(got, batch.want[i])
    assert bool(np.isfinite(got).all()) and e["low"] <= batch.bounds[i]["low"], e


@pytest.mark.parametrize("kernel,label", _pairs(KERNELS, SECOND_LABELS))
def test_rows_with_four_owners_per_frame(gpu, batch_second, kernel, label):
    batch_second.check(gpu, kernel, "host", label, f"{kernel}/T100H25")


@pytest.mark.parametrize("kernel,name", _pairs(["h", "f32"], STAGE_NAMES))
def test_stage_api_rows_match_the_oracle(gpu, kernel, name):
    """fe.log_mel(segments): explicit segments take the per-segment kernels"""
    fe = _fe(gpu, kernel)
    clip = D.make(name)
    rows = fe.log_mel(list(D.segments(clip))).cpu().numpy()
    assert fe.last_logmel_kind() == "per_segment"
    e, b = D.errors(rows, D.oracle(clip)), D.bounds(name)
    print("\n" + D.line(f"{kernel}/stage {name}", e, b))
    np.testing.assert_array_equal(fe.last_logmel().cpu().numpy(), rows)              # the read-back is the stage API's own finalisation
    assert e["low"] <= b["low"] and e["rest"] <= b["rest"], (name, e["low"], b["low"], e["rest"], b["rest"])


def test_gated_clip(gpu):
    """a segment of exact zeros inside a live clip: its rows are exactly -1.5 ((log10(1e-10) + 4) / 4) from every kernel, everything
    is finite, and the shared-frame kernels agree with the per-segment kernel within the bound"""
    import torch
    clip = D.make("gated")
    want, b = D.oracle(clip), D.bounds("gated")
    wave, offs = torch.from_numpy(clip).to(gpu), np.array([0, len(clip)], np.int64)
    rows, bad = {}, []
    print()
    for kernel in KERNELS:
        fe = _fe(gpu, kernel)
        fe.embed_clips(wave, offs)
        assert fe.last_logmel_kind() == KERNELS[kernel][1]
        rows[kernel] = fe.last_logmel().cpu().numpy()
        e = D.errors(rows[kernel], want)
        zero_dev = float(np.abs(rows[kernel][1:] + 1.5).max())
        print(D.line(f"{kernel}/gated", e, b) + f" | all-zero segments: max |row + 1.5| = {zero_dev:.2e}")
        if not (np.isfinite(rows[kernel]).all() and zero_dev == 0.0 and e["low"] <= b["low"] and e["rest"] <= b["rest"]):
            bad.append((kernel, zero_dev, e["low"], e["rest"]))
    for kernel in ("fft_clip", "h_clip"):
        e = D.errors(rows[kernel], rows["h"])
        print(f"{kernel} vs h: low {e['low']:.2e} rest {e['rest']:.2e}")
        if not (e["low"] <= b["low"] and e["rest"] <= b["rest"]):
            bad.append((kernel + " vs h", e["low"], e["rest"]))
    assert not bad, bad


def test_read_back_errors(gpu):
    """RADAD_ESTATE before any forward, RADAD_EINVAL for a buffer that is too small (the count is reported all the same), the count
    alone for a NULL buffer"""
    import ctypes as C
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    fe = _fe(gpu, "fft_clip")
    lib, n = fe._lib, C.c_int64(-1)
    st = _lib.stream_ptr(gpu)
    assert lib.radad_embed_last_logmel(fe._h, None, 0, C.byref(n), st) == _lib.RADAD_ESTATE
    with pytest.raises(ValueError):
        fe.last_logmel()
    assert lib.radad_embed_last_logmel(None, None, 0, C.byref(n), st) == _lib.RADAD_EINVAL
    assert lib.radad_embed_last_logmel(fe._h, None, 0, None, st) == _lib.RADAD_EINVAL
    clip = D.make("tone_on_bin")
    fe.embed_clips(torch.from_numpy(clip).to(gpu), [0, len(clip)])
    assert lib.radad_embed_last_logmel(fe._h, None, 0, C.byref(n), st) == 0 and n.value == 3
    out = torch.full((3, 200, 80), 7.0, device=gpu)
    n.value = -1
    assert lib.radad_embed_last_logmel(fe._h, out.data_ptr(), 2, C.byref(n), st) == _lib.RADAD_EINVAL and n.value == 3
    assert lib.radad_embed_last_logmel(fe._h, out.data_ptr(), -1, C.byref(n), st) == _lib.RADAD_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                  # nothing was written
    assert lib.radad_embed_last_logmel(fe._h, out.data_ptr(), 3, C.byref(n), st) == 0
    assert torch.equal(out, fe.last_logmel())


@pytest.mark.parametrize("kernel", ["fft_clip", "h_clip"])
def test_chain_selects_the_owners_clamp(gpu, tmp_path, kernel):
    """dc_step_tonal and gated through embed_clips with a selector projection (F = 96, W[:, :80] = I, b = 0) and 16 time bins, avg and
    max: feature m < 80 of a frame IS its log-mel band m as k_proj_pool2 clamped it -- with the maximum of the segment that owns the
    row, not of the chunk or a neighbour.  Against the oracle's pooling of its own rows; columns 80-95 are exactly 0.
    Tolerance: the input's bound for the column's region (pooling cannot raise a row error) + 2e-6 for the projection itself (three
    split-f16 products of |v| <= 2.5 with 1.0, each product's error below 2^-21 |v|)."""
    import torch
    F = 96
    w = np.zeros((80, F), np.float32)
    w[np.arange(80), np.arange(80)] = 1.0
    path = str(tmp_path / "selector.npz")
    np.savez(path, w=w, b=np.zeros(F, np.float32))
    names = ("dc_step_tonal", "gated")
    clips = [D.make(n) for n in names]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    wave = torch.from_numpy(np.concatenate(clips)).to(gpu)
    print()
    bad = []
    for mode in ("avg", "max"):
        fe = _fe(gpu, kernel, feature_dim=F, tpp_levels=[16], tpp_pooling_type=mode, melproj_weights_path=path)
        emb = fe.embed_clips(wave, offs).cpu().numpy().reshape(len(names), 16, F)
        assert fe.last_logmel_kind() == KERNELS[kernel][1]
        for i, name in enumerate(names):
            rows = D.oracle(clips[i])
            ref = O.segment_mean([O.tpp(r, (16,), mode) for r in rows]).reshape(16, 80)
            b = D.bounds(name)
            err = np.abs(emb[i, :, :80] - ref)
            lo, rest = float(err[:, :2].max()), float(err[:, 2:].max())
            print(f"{kernel}/chain/{mode} {name:<14s} low {lo:.2e} rest {rest:.2e} | bound {b['low'] + 2e-6:.2e} {b['rest'] + 2e-6:.2e}")
            if not (lo <= b["low"] + 2e-6 and rest <= b["rest"] + 2e-6):
                bad.append((mode, name, lo, rest))
            assert bool(np.all(emb[i, :, 80:] == 0.0))
    assert not bad, bad
