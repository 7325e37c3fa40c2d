"""GPU tests of rc_engine_stretch_frames_loud through the C-ABI, at window 256, factor 2, R = 8000. The yardstick is the numpy
statement of the definition (tests/loudnessutil.py) on what rc_engine_stretch_frames gives under the same engine state:
*true_peak bit for bit; *lufs within 0.01 LU (a tenth of EBU Tech 3341's meter tolerance); *gain within one f32 ulp of the
header's formula on the REPORTED lufs and true_peak (libm's pow and numpy's may differ in the last place); the bytes and
*clipped bit for bit from the numpy pack definition applied with the reported gain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rocoder_amd  # noqa: E402
from ditherutil import dithered_bytes  # noqa: E402
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import pinned_empty  # noqa: E402
from test_frames_pcm_host import count_clipped, pcm_bytes, quantise  # noqa: E402

import loudnessutil as U  # noqa: E402

pytestmark = pytest.mark.gpu
RATE = 8000
_engines, _inputs, _refs = {}, {}, {}


def engine(channels):
    if channels not in _engines:
        _engines[channels] = rocoder_amd.Engine(window_len=256, factor=2.0, channels=channels, seed=9, sample_rate=RATE)
    return _engines[channels]


def teardown_module(module):
    for e in _engines.values():
        e.close()


def frames_in(channels, fmt):
    """about 3 s of loudnessutil.programme at half its level, as [n, channels] frames of int16 or float32"""
    key = (channels, fmt)
    if key not in _inputs:
        x = 0.5 * U.programme(channels, RATE, scale=0.5, tail=False).T
        a = np.clip(np.rint(x * 32767.0), -32768, 32767).astype("<i2") if fmt == "i16" else np.ascontiguousarray(x, np.float32)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


STATES = {
    "plain": dict(),
    "dither": dict(dither=("tpdf", 41)),
    "limiter": dict(limiter=(1.0, 0.2, 64)),
    "step": dict(step=(160, 147)),
    "all": dict(dither=("tpdf-hp", 5), limiter=(1.0, 0.2, 64), step=(160, 147)),
}


def set_state(eng, dither=None, limiter=None, step=None):
    eng.set_output_dither(*(dither or ("none", 0)))
    eng.set_output_limiter(*(limiter or (1.0, 0.0, 0)))
    eng.set_output_resample(*(step or (0, 0)))


def reference(channels, fmt, state, table):
    """(the f32 result of rc_engine_stretch_frames [n, channels], I in f64, tp as float32) under the state; computed once"""
    key = (channels, fmt, state)
    if key not in _refs:
        eng = engine(channels)
        set_state(eng, **STATES[state])
        try:
            ref = eng.stretch_frames(frames_in(channels, fmt))
        finally:
            set_state(eng)
        ref.setflags(write=False)
        rows = np.ascontiguousarray(ref.T)
        _refs[key] = (ref, U.loudness(rows, RATE), U.true_peak(rows, table), U.gate_margin(rows, RATE))
    return _refs[key]


@pytest.fixture(scope="module")
def table():
    return U.table_1_4()


def one_ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return got == want or got == np.nextafter(want, np.float32(np.inf)) or got == np.nextafter(want, np.float32(-np.inf))


def expected_bytes(ref, gain, out_fmt, dither):
    z = (ref * np.float32(gain)).astype(np.float32)
    if out_fmt == "f32":
        return z.tobytes(), count_clipped(z)
    if dither and out_fmt in ("u8", "i16", "i24"):
        return dithered_bytes(z, out_fmt, dither[0], dither[1]).tobytes(), count_clipped(z)
    return pcm_bytes(quantise(z, out_fmt), out_fmt), count_clipped(z)


def run(channels, fmt, state, out_fmt, table, target=-23.0, ceiling=0.0, **kw):
    ref, lufs, tp, margin = reference(channels, fmt, state, table)
    eng = engine(channels)
    set_state(eng, **STATES[state])
    try:
        got = eng.stretch_frames_loud(frames_in(channels, fmt), target, ceiling, out_fmt=out_fmt, sample_rate=RATE, **kw)
    finally:
        set_state(eng)
    print(f"{channels} ch {fmt} {state} -> {out_fmt}: I {eng.last_lufs} (f64 {lufs:.6f}, gate margin {margin:.3f} LU), "
          f"tp {eng.last_true_peak}, gain {eng.last_gain}, clipped {eng.last_clipped}")
    assert margin >= 0.1, "a block of the reference within 0.1 LU of a gate threshold: pick another seed"
    assert np.float32(eng.last_true_peak).view(np.uint32) == np.float32(tp).view(np.uint32), (eng.last_true_peak, tp)
    assert np.isfinite(lufs) and abs(float(eng.last_lufs) - lufs) <= 0.01, (eng.last_lufs, lufs)
    want_gain = U.gain_of(eng.last_lufs, eng.last_true_peak, target, ceiling)
    assert one_ulp(eng.last_gain, want_gain), (eng.last_gain, want_gain)
    want, clipped = expected_bytes(ref, eng.last_gain, out_fmt, STATES[state].get("dither"))
    assert got.tobytes() == want and eng.last_clipped == clipped
    return eng, ref, tp


CASES = [(1, "i16", s) for s in STATES] + [(2, "f32", s) for s in STATES] + [(2, "i16", "plain"), (2, "i16", "all")]


@pytest.mark.parametrize("out_fmt", ["i16", "u8", "f32"])
@pytest.mark.parametrize("channels,fmt,state", CASES)
def test_loudness_true_peak_gain_and_bytes(channels, fmt, state, out_fmt, table):
    run(channels, fmt, state, out_fmt, table)


def test_the_ceiling_binds(table):
    ref, lufs, tp, _ = reference(2, "i16", "plain", table)
    target = float(np.float32(lufs + 12.0))  # gl = 4: the ceiling of half the measured peak asks for 0.5
    eng, ref, tp = run(2, "i16", "plain", "i16", table, target=target, ceiling=float(np.float32(0.5) * tp))
    assert eng.last_gain == np.float32(np.float32(np.float32(0.5) * tp) / tp) and eng.last_gain < 1
    eng, ref, tp = run(2, "i16", "plain", "i16", table, target=target, ceiling=float(np.float32(100.0) * tp))
    assert one_ulp(eng.last_gain, U.gain_of(eng.last_lufs, tp, target, 100.0 * tp)) and eng.last_gain > 3.9


def test_short_jobs(table):
    eng = engine(2)
    a = frames_in(2, "i16")[13000:14000]  # 1000 frames in, 2000 out: 0.25 s, fewer than four sub-blocks
    ref = eng.stretch_frames(a)
    tp = U.true_peak(np.ascontiguousarray(ref.T), table)
    assert RATE * 0.1 < ref.shape[0] < RATE * 0.4
    for ceiling in (0.0, float(np.float32(0.25) * tp), 2.0):
        got = eng.stretch_frames_loud(a, -23.0, ceiling, out_fmt="i16", sample_rate=RATE)
        assert eng.last_lufs == -np.inf and np.float32(eng.last_true_peak).view(np.uint32) == tp.view(np.uint32)
        want = min(np.float32(1.0), np.float32(np.float32(ceiling) / tp)) if ceiling else np.float32(1.0)
        assert eng.last_gain == want
        assert got.tobytes() == pcm_bytes(quantise((ref * want).astype(np.float32), "i16"), "i16")
    got = eng.stretch_frames_loud(np.zeros((0, 2), "<i2"), -23.0, 0.5, out_fmt="i16", sample_rate=RATE)
    # (no input frame still gives rc_offline_output_len(0) frames of silence)
    assert got.shape == (eng.output_len(0), 2) and not got.any()
    assert eng.last_lufs == -np.inf and eng.last_true_peak == 0 and eng.last_gain == 1 and eng.last_clipped == 0


def test_invalid_arguments_leave_the_out_pointers_untouched():
    eng = engine(2)
    a = frames_in(2, "i16")
    n_out = eng.output_len(a.shape[0])
    out = np.full(n_out * 2 * 2, 0x5A, np.uint8)
    nan, inf = float("nan"), float("inf")
    cases = [dict(target=nan), dict(target=inf), dict(target=-inf), dict(ceiling=nan), dict(ceiling=-0.5), dict(rate=7999), dict(rate=768001),
             dict(fmt=9), dict(out_fmt=0), dict(cap=n_out - 1, rc=_lib.RC_ECAPACITY)]
    for kw in cases:
        got, clipped = C.c_size_t(99), C.c_uint64(98)
        lufs, tp, gain = C.c_float(97.0), C.c_float(96.0), C.c_float(95.0)
        rc = eng._L.rc_engine_stretch_frames_loud(
            eng._h, a.ctypes.data, a.shape[0], kw.get("fmt", _lib.RC_PCM_I16), out.ctypes.data, kw.get("cap", n_out), kw.get("out_fmt", _lib.RC_PCM_I16),
            kw.get("rate", RATE), C.c_float(kw.get("target", -23.0)), C.c_float(kw.get("ceiling", 0.0)), C.byref(got), C.byref(lufs), C.byref(tp),
            C.byref(gain), C.byref(clipped))
        assert rc == kw.get("rc", _lib.RC_EINVAL), kw
        assert (got.value, clipped.value, lufs.value, tp.value, gain.value) == (99, 98, 97.0, 96.0, 95.0) and (out == 0x5A).all(), kw
    # sample_rate 0 is the engine's rate
    assert eng.stretch_frames_loud(a, -23.0, out_fmt="i16").tobytes() == eng.stretch_frames_loud(a, -23.0, out_fmt="i16", sample_rate=RATE).tobytes()


def test_the_entries_around_it_write_what_they_wrote_and_memory_kinds_agree(table):
    eng = engine(2)
    a = frames_in(2, "i16")
    before = eng.stretch_frames(a, out_fmt="i16").tobytes()
    norm_before = eng.stretch_frames(a, out_fmt="i16", normalize=0.9).tobytes()
    want = eng.stretch_frames_loud(a, -20.0, 0.9, out_fmt="i16", sample_rate=RATE)
    words = (eng.last_lufs, eng.last_true_peak, eng.last_gain, eng.last_clipped)
    assert eng.stretch_frames(a, out_fmt="i16").tobytes() == before
    assert eng.stretch_frames(a, out_fmt="i16", normalize=0.9).tobytes() == norm_before
    src = pinned_empty(a.shape, a.dtype)
    src[:] = a
    out = pinned_empty((want.nbytes,), np.uint8)
    got = eng.stretch_frames_loud(src, -20.0, 0.9, out=out, out_fmt="i16", sample_rate=RATE)
    assert got.tobytes() == want.tobytes() and words == (eng.last_lufs, eng.last_true_peak, eng.last_gain, eng.last_clipped)
