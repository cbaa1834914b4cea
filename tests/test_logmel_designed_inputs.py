"""The designed log-mel inputs (tests/logmel_designed.py) on the CPU: every input has the property it is named for, the float32
reference is a fair yardstick (inside the 1e-4 bar itself, so no bound exceeds 4e-4), and the float32 statement of the shared-frame
identity in the form the kernels ship -- bin 1 kept out of the shared mel sums, fb[1][b] ((Re X'[1] + d)^2 + Im X'[1]^2) added per
owner -- stays within the bound for every input and every pivot.  The expanded form the kernels shipped before
(mel' + fb[1][b] (2 d Re X'[1] + d^2)) is measured beside it: it is what a level step or a DC step inside a clip breaks."""
import numpy as np
import pytest

import logmel_designed as D

SECOND = dict(seg=16000, hop=4000, n=40000)          # 1.0 s segments, 0.75 overlap: T = 100, H = 25, four owners
SECOND_NAMES = ("level_step60", "dc_step", "dc_step_tonal")


@pytest.fixture(scope="module")
def decades():
    """decades under the segment maximum of every (frame, band) cell, before the clamp, per input"""
    out = {}
    for name in D.NAMES:
        raw = D.oracle_log10(D.make(name))
        out[name] = raw.max(axis=(1, 2), keepdims=True) - raw
    return out


@pytest.mark.parametrize("name", ["tone_on_bin", "tone_off_bin", "short_tone", "chirp"])
def test_tones_and_chirp_sit_on_the_clamp(decades, name):
    down = decades[name]
    assert (down >= 8.0).mean() >= 0.5, (down >= 8.0).mean()
    assert int(((down >= 6.0) & (down < 8.0)).sum()) >= 100


@pytest.mark.parametrize("name", ["tone_floor60", "lowpass_floor70"])
def test_floors_fill_the_two_decades_above_the_clamp(decades, name):
    """a tone (band-limited noise) over a noise floor 60 (70) dB down: the floor's cells lie 6 to 8 decades under the maximum, where
    a split-precision product loses them first.  (The floor lifts two thirds of tone_floor60's cells off the clamp: 0.33 of them
    stay clamped, so the pure tones' `half the cells` does not apply to it.)"""
    down = decades[name]
    assert int(((down >= 6.0) & (down < 8.0)).sum()) >= 1000
    assert (down >= 8.0).mean() >= 0.25


def test_gated_clip_holds_an_all_zero_segment():
    segs = D.segments(D.make("gated"))
    assert segs.shape[0] == 3 and bool(np.any(segs[0] != 0.0)) and bool(np.all(segs[1] == 0.0))
    rows = D.oracle(D.make("gated"))
    assert bool(np.all(rows[1] == -1.5))             # log10(1e-10) everywhere: (-10 + 4) / 4


def test_level_step_separates_overlapping_segments_by_five_decades():
    """the maxima of the segments' log-mel BEFORE normalisation -- the rows overlapping segments share -- differ by >= 5 in log10"""
    raw = D.oracle_log10(D.make("level_step60"), normalize=False).max(axis=(1, 2))
    assert float(np.abs(np.diff(raw)).max()) >= 5.0, raw


def _low_rms(x):
    """rms of the content of x below 80 Hz (the main lobe of bin 1 under the hann window), its mean removed"""
    x = np.asarray(x, np.float64)
    spec = np.fft.rfft(x - x.mean())
    spec[np.fft.rfftfreq(len(x), 1.0 / D.FS) >= 80.0] = 0.0
    return float(np.fft.irfft(spec, len(x)).std())


@pytest.mark.parametrize("name,ratio", [("dc_step_tonal", 10.0), ("dc_step", 5.0)])
def test_dc_steps_move_the_mean_far_beyond_the_low_band(name, ratio):
    """neighbouring segments' means differ by `ratio` x the rms of what the side after the step holds below 80 Hz.  dc_step_tonal: 10 x
    (it has 200 x).  dc_step cannot have 10 x with its formula: its 0.3 nz holds 0.3 sqrt(80 / 8000) = 0.03 below 80 Hz and the
    means of segments 1 and 2 differ by 0.25 (1 - 4000 / 32000) = 0.219, a ratio of 7.3; asserted at 5 x, still far above the 1 x
    from which the expanded correction starts to cancel."""
    clip = D.make(name)
    mean = D.segments(clip).mean(axis=1, dtype=np.float64)
    quiet = _low_rms(clip[34000:])
    assert float(np.abs(np.diff(mean)).min()) >= ratio * quiet, (mean, quiet)


def test_reference32_is_inside_the_bar_on_every_input(capsys):
    lines, worst = [], 0.0
    for name in D.NAMES:
        b = D.bounds(name)
        lines.append(f"{name:<18s} reference32 vs oracle: bands 0-1 {b['ref_low']:.2e}  bands 2-79 {b['ref_rest']:.2e}  bound "
                     f"{b['low']:.2e} {b['rest']:.2e}")
        worst = max(worst, b["ref_low"], b["ref_rest"])
        assert b["ref_low"] <= D.BAR and b["ref_rest"] <= D.BAR, lines[-1]
        assert b["low"] <= 4e-4 and b["rest"] <= 4e-4
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert worst < 1e-4


def _identity_cases():
    return [(n, {}) for n in D.NAMES] + [(n, SECOND) for n in SECOND_NAMES]


@pytest.mark.parametrize("name,cfg", _identity_cases(), ids=lambda v: v if isinstance(v, str) else ("second" if v else "default"))
def test_factored_identity_is_within_the_bound(capsys, name, cfg):
    """the form the kernels ship, every pivot (the segment's own mean, each neighbour's); the expanded form printed beside it"""
    seg, hop, n = cfg.get("seg", 32000), cfg.get("hop", 16000), cfg.get("n")
    clip = D.make(name) if n is None else D.clipped(name, n)
    want = D.oracle(clip, seg, hop)
    b = D.bounds(name, seg, hop, n)
    fac, exp = D.shared_identity32(clip, seg, hop, "factored"), D.shared_identity32(clip, seg, hop, "expanded")
    lines = []
    for pivot in ("own", "prev", "next"):
        e, x = D.errors(fac[pivot], want), D.errors(exp[pivot], want)
        lines.append(D.line(f"{name} T={seg // 160} pivot={pivot} factored", e, b) + f" | expanded low {x['low']:.2e} rest {x['rest']:.2e}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for pivot in ("own", "prev", "next"):
        e = D.errors(fac[pivot], want)
        assert e["low"] <= b["low"] and e["rest"] <= b["rest"], (pivot, e, b)


def test_expanded_identity_breaks_on_steps():
    """why the kernels changed: with a neighbour's mean as the pivot the expanded correction leaves bands 0-1 of level_step60 and
    dc_step_tonal outside the bound (3.9e-4 and 1.0e-2 in this model), bands 2-79 untouched"""
    for name in ("level_step60", "dc_step_tonal"):
        clip = D.make(name)
        e = D.errors(D.shared_identity32(clip, form="expanded")["prev"], D.oracle(clip))
        b = D.bounds(name)
        assert e["low"] > b["low"] and e["rest"] <= b["rest"], (name, e, b)
