"""CPU tests of the loudness entries (include/rocoder_hip.h: rc_engine_stretch_frames_loud and its host helpers): the
coefficients against the f64 formulas and the table of BS.1770-4, the numpy definition of tests/loudnessutil.py against the
answers of EBU Tech 3341, rc_loudness_integrated against the numpy gate, and the proof that the gates of the GPU tests
(0.01 LU on the loudness, 2.3e-3 relative on a sub-block energy, bit for bit on the true peak) catch the mistakes a kernel
or a host loop can make: every mutant below moves a result by more than its gate on an input the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import loudnessutil as U

rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402

_fp = C.POINTER(C.c_float)


def _c_integrated(e, rate, stride=None):
    e = np.ascontiguousarray(np.atleast_2d(e), np.float32)
    ch, nb = e.shape
    stride = nb if stride is None else stride
    buf = np.full(ch * stride + 1, np.nan, np.float32)
    for c in range(ch):
        buf[c * stride:c * stride + nb] = e[c]
    out = C.c_float(123.0)
    rc = _lib.lib().rc_loudness_integrated(buf.ctypes.data_as(_fp), ch, nb, stride, rate, C.byref(out))
    assert rc == _lib.RC_OK
    return np.float32(out.value)


@pytest.mark.parametrize("rate", [8000, 44100, 48000, 96000, 192000])
def test_coefficients_are_the_f64_formulas_rounded_once(rate):
    got = np.zeros(10, np.float32)
    assert _lib.lib().rc_loudness_coeffs(rate, got.ctypes.data_as(_fp)) == _lib.RC_OK
    assert U.coeffs_f64(rate).astype(np.float32).view(np.uint32).tolist() == got.view(np.uint32).tolist()


def test_f64_formulas_meet_the_table_of_bs1770_at_48k():
    c = U.coeffs_f64(48000)
    err = np.abs(c - np.array(U.BS1770_48K))
    print("coefficient errors against BS.1770-4:", err)
    assert err.max() <= 1e-12


def test_helpers_reject_what_the_header_says():
    L = _lib.lib()
    got = np.full(10, 7.0, np.float32)
    for rate in (0, 7999, 768001):
        assert L.rc_loudness_coeffs(rate, got.ctypes.data_as(_fp)) == _lib.RC_EINVAL
        assert L.rc_loudness_sub_blocks(10 ** 6, rate) == 0
    assert L.rc_loudness_coeffs(48000, None) == _lib.RC_EINVAL
    assert (got == 7.0).all()
    out = C.c_float(5.0)
    e = np.ones(8, np.float32)
    assert L.rc_loudness_integrated(e.ctypes.data_as(_fp), 0, 8, 8, 48000, C.byref(out)) == _lib.RC_EINVAL
    assert L.rc_loudness_integrated(e.ctypes.data_as(_fp), 1, 8, 7, 48000, C.byref(out)) == _lib.RC_EINVAL
    assert L.rc_loudness_integrated(e.ctypes.data_as(_fp), 1, 8, 8, 100, C.byref(out)) == _lib.RC_EINVAL
    assert L.rc_loudness_integrated(None, 1, 8, 8, 48000, C.byref(out)) == _lib.RC_EINVAL
    assert L.rc_loudness_integrated(e.ctypes.data_as(_fp), 1, 8, 8, 48000, None) == _lib.RC_EINVAL
    assert out.value == 5.0
    # rates that 10 does not divide: sub = (R + 5) / 10
    for rate, sub in ((8000, 800), (11025, 1103), (22050, 2205), (44100, 4410), (8004, 800), (8005, 801), (768000, 76800)):
        assert U.sub_frames(rate) == sub
        for n in (0, sub - 1, sub, 4 * sub - 1, 4 * sub, 10 ** 7 + 3):
            assert L.rc_loudness_sub_blocks(n, rate) == n // sub, (rate, n)


def _tone(dbfs, secs, rate=48000):
    t = np.arange(int(round(secs * rate)), dtype=np.float64)
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t / rate)


TECH3341 = [  # (segments of (dBFS, seconds), the answer of EBU Tech 3341, what the f64 definition gave)
    ([(-23, 20)], -23.0, -22.993),
    ([(-33, 20)], -33.0, -32.993),
    ([(-36, 10), (-23, 60), (-36, 10)], -23.0, -23.014),
    ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0, -23.014),
    ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0, -22.979),
]


@pytest.fixture(scope="module")
def tech3341_energies():
    out = []
    for segs, _, _ in TECH3341:
        x = np.concatenate([_tone(db, s) for db, s in segs])
        out.append(U.sub_energies(np.stack([x, x]), 48000))
    return out


def test_numpy_definition_gives_the_answers_of_ebu_tech_3341(tech3341_energies):
    for (segs, want, measured), e in zip(TECH3341, tech3341_energies):
        got = U.integrated(e, 4800)
        print(segs, "->", round(got, 4), "LUFS")
        assert abs(got - want) <= 0.1, (segs, got)
        assert abs(got - measured) <= 2e-3, (segs, got, measured)  # (the figures are quoted to three places)
    e = tech3341_energies[0]
    assert abs((U.integrated(e, 4800) - U.integrated(e[:1], 4800)) - 10.0 * np.log10(2.0)) < 1e-9  # mono: 3.01 LU below


def test_library_gate_equals_the_numpy_gate(tech3341_energies):
    """within 1e-4 LU: the f32 of the returned value (both sides sum in f64, over the f32 energy words)"""
    rng = np.random.default_rng(7)
    cases = [(e.astype(np.float32), 48000) for e in tech3341_energies]
    for ch, nb, rate in ((1, 4, 8000), (2, 37, 44100), (3, 200, 8000), (6, 64, 96000)):
        # random levels over 90 dB: blocks on both sides of both gates
        e = (U.sub_frames(rate) * 10.0 ** rng.uniform(-9.0, 0.0, (ch, nb))).astype(np.float32)
        cases.append((e, rate))
    for e, rate in cases:
        want = U.integrated(e.astype(np.float64), U.sub_frames(rate))
        got = _c_integrated(e, rate)
        assert np.isfinite(want) and abs(float(got) - want) <= 1e-4, (e.shape, rate, got, want)
        assert _c_integrated(e, rate, stride=e.shape[1] + 5) == got
    sub = 800
    assert _c_integrated(np.ones((2, 3), np.float32), 8000) == -np.inf           # nb < 4
    assert _c_integrated(np.zeros((2, 0), np.float32), 8000) == -np.inf          # no sub-block at all
    assert _c_integrated(np.zeros((2, 40), np.float32), 8000) == -np.inf         # silence
    quiet = np.full((1, 40), 0.5 * U.ABS_GATE_ENERGY * sub, np.float32)          # every block 3 LU below -70
    assert _c_integrated(quiet, 8000) == -np.inf
    assert np.isfinite(_c_integrated(4.0 * quiet, 8000))


# ---- the mutants ----------------------------------------------------------------------------------------------------------------
RATE = 8000


def test_energy_gate_catches_the_filter_mutants():
    """2.3e-3 relative on a sub-block energy. Which input catches which mutant: no high-pass - the 30 Hz tone and the DC row
    (both live below the corner); no shelf - white noise (the shelf lifts its upper half); a state reset at every sub-block -
    the DC row and the tone (the step the reset makes rings through the high-pass)."""
    n = 80037
    caught = {}
    for kind in ("white", "tone", "dc", "burst"):
        x = U.test_input(kind, 1, n)
        want = U.sub_energies(x, RATE)
        for name, kw in (("no_highpass", dict(highpass=False)), ("no_shelf", dict(shelf=False)), ("reset", dict(reset=True))):
            rel, quiet = U.energy_errors(U.sub_energies(x, RATE, **kw), want, 800)
            caught.setdefault(name, {})[kind] = max(rel, quiet)
    print(caught)
    assert caught["no_highpass"]["tone"] > U.GATE_REL and caught["no_highpass"]["dc"] > U.GATE_REL
    assert caught["no_shelf"]["white"] > U.GATE_REL
    assert caught["reset"]["dc"] > U.GATE_REL and caught["reset"]["tone"] > U.GATE_REL
    # and the warm-up the kernel takes instead of the whole past stays far inside the gate: two sub-blocks
    for kind in ("white", "tone", "dc"):
        x = U.test_input(kind, 1, 8000).astype(np.float64)
        full = U.sub_energies(x, RATE)[0]
        for j in (3, 6, 9):
            cut = U.sub_energies(x[:, (j - 2) * 800:(j + 1) * 800], RATE)[0, 2]
            assert abs(cut - full[j]) <= 1e-9 * full[j], (kind, j, cut, full[j])


def test_loudness_gate_catches_the_gate_mutants():
    """0.01 LU on the loudness, on the sectioned programme the engine tests stretch (loudnessutil.programme: near-silence, a
    passage 14 LU down, a loud passage, a louder partial tail). No relative gate and no absolute gate - the passage 14 LU down
    counts, or the near-silence drags the relative threshold below it; blocks without overlap and the partial tail counted -
    the section edges and the loud tail; -0.691 dropped - every input."""
    x = U.programme(2, RATE)
    want = U.loudness(x, RATE)
    assert np.isfinite(want) and U.gate_margin(x, RATE) >= 0.1
    moved = {}
    for name, kw in (("no_rel_gate", dict(rel_gate=False)), ("no_abs_gate", dict(abs_gate=False)), ("no_overlap", dict(overlap=False)),
                     ("tail", dict(tail=True)), ("no_offset", dict(offset=False)), ("no_highpass", dict(highpass=False)),
                     ("no_shelf", dict(shelf=False))):
        moved[name] = abs(U.loudness(x, RATE, **kw) - want)
    # (a state reset at every sub-block moves this noise by 0.002 LU only: the energy gate on the DC row and the tone catches it)
    print(want, moved)
    for name, d in moved.items():
        assert d > 0.01, (name, d)


def test_true_peak_gate_catches_its_mutants_and_the_definition_is_the_resampler_s():
    """bit for bit. No sample peak - a click (the table's centre tap is 0.9: every oversampled point lies below the sample);
    y not zero-extended - the DC row (cut off at its ends it overshoots, held it does not) and a click at frame 0."""
    import resampleutil as R

    t = U.table_1_4()
    click = np.zeros((1, 300), np.float32)
    click[0, 120] = 1.0
    assert U.true_peak(click, t) == np.float32(1.0) and U.true_peak(click, t, sample_peak=False) < np.float32(1.0)
    dc = U.test_input("dc", 1, 801)
    assert U.true_peak(dc, t) > np.float32(1.05) and U.true_peak(dc, t, zero_extend=False) < np.float32(1.02)
    first = np.zeros((1, 300), np.float32)
    first[0, 0] = -0.5
    assert U.true_peak(first, t, sample_peak=False) != U.true_peak(first, t, zero_extend=False, sample_peak=False)
    # the chain is the resampler's: against its f64 definition inside its own bound, and next to the sequential f32 sum
    x = U.test_input("white", 2, 500)
    u = U.oversampled(x, t)
    y, bound = R.resample_f64(x, t, 1, 4)
    assert u.shape == y.shape and (np.abs(u - y) <= bound).all()
    assert np.abs(u - R.resample_f32(x, t, 1, 4)).max() <= 2.0 * bound.max()
    # fma_f32 rounds once: against exact rational arithmetic
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(300).astype(np.float32), rng.standard_normal(300).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.choice([0.0, 2.0 ** -24, 2.0 ** -25, 1e-3], 300))).astype(np.float32)
    got = U.fma_f32(a, b, c)
    for i in range(300):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # (float(Fraction) rounds once to f64: only used to find the two f32 neighbours)
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: abs(Fraction(v) - exact))
        ties = [v for v in cands if abs(Fraction(v) - exact) == abs(Fraction(best) - exact)]
        assert float(got[i]) in ties, (i, a[i], b[i], c[i], got[i], best)
    # the tone at R / 4 with phase 45 degrees under a 512-frame raised-cosine fade: the crest between the samples
    n = 4096
    k = np.arange(n, dtype=np.float64)
    env = np.ones(n)
    env[:512] = 0.5 - 0.5 * np.cos(np.pi * k[:512] / 512)
    env[-512:] = env[:512][::-1]
    tone = (env * np.sin(2.0 * np.pi * k / 4.0 + np.pi / 4.0)).astype(np.float32)[None, :]
    print("R/4 tone: sample peak", U.finite_peak(tone), "true peak", U.true_peak(tone, t))
    assert U.finite_peak(tone) == np.float32(0.70710677) and abs(float(U.true_peak(tone, t)) - 1.0000061) < 2e-6
    # the worst case at R / 8: a crest half way between two of the four points
    k = np.arange(2048, dtype=np.float64)
    worst = min(float(np.abs(U.oversampled(np.sin(2.0 * np.pi * (k / 8.0) + ph)[None, :].astype(np.float32), t)[:, 800:-800]).max())
                for ph in np.pi / 4 * np.arange(0, 1, 1 / 16))  # (away from the ends: a row cut off there overshoots)
    print("R/8 tone: the lowest true peak over the phases", worst, 20 * np.log10(worst), "dB")
    assert -0.05 < 20 * np.log10(worst) < 0.0


def test_gain_formula():
    assert U.gain_of(-np.inf, 0.5, -23.0, 0.0) == np.float32(1.0)
    assert U.gain_of(-np.inf, 0.5, -23.0, 0.25) == np.float32(0.5)
    assert U.gain_of(-20.0, 0.5, -23.0, 0.0) == np.float32(10.0 ** (-3.0 / 20.0))
    assert U.gain_of(-20.0, 0.5, -14.0, 0.5) == np.float32(1.0)                  # the ceiling binds: 0.5 / 0.5
    assert U.gain_of(-20.0, 0.0, -14.0, 0.5) == np.float32(10.0 ** (6.0 / 20.0))  # no peak: no ceiling
    assert U.gain_of(-20.0, 1e-30, 3.0e38, 0.0) == np.float32(1.0)               # an overflowing gain: 1
