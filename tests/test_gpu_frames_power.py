"""GPU tests of rc_engine_frames_power / Engine.frames_power / rc_autocrop_points / --autocrop: the peak of every bin of a
raw block of PCM frames, measured on the GPU, and the reference's crop from it. Everything is bit for bit against numpy:
the expected bins are the block decoded with the header's formulas in float32 (tests/autocroputil.py), `abs`, a maximum
per bin. There is no tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import autocroputil as au
import rocoder_amd
from conftest import ROOT
from rocoder_amd import _lib, autocrop_points
from rocoder_amd.stretcher import compile_device_kernel, pinned_empty
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
FORMATS = ("u8", "i16", "i24", "i32", "f32")


def at_phase(raw, phase, pinned=False):
    """the bytes `raw` copied to an address that is `phase` bytes behind a multiple of 4"""
    raw = np.frombuffer(raw, np.uint8)
    big = pinned_empty(raw.size + 8, np.uint8) if pinned else np.empty(raw.size + 8, np.uint8)
    off = (phase - big.ctypes.data) % 4
    view = big[off:off + raw.size]
    view[:] = raw
    assert (big.ctypes.data + off) % 4 == phase  # (numpy gives an empty view an address of its own: ask the block)
    return view


def random_block(fmt, n_frames, channels, seed):
    """seeded random bytes: every sample over the full range of its format (f32: any bits, NaN and inf among them)"""
    return np.random.default_rng(seed).integers(0, 256, n_frames * channels * au.PCM_BYTES[fmt], dtype=np.uint8)


def same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} bins differ, the first {bad[:6].tolist()}: "
                             f"{got[bad[:6]].tolist()} for {want[bad[:6]].tolist()}")


def check(eng, raw, fmt, channels, bin_frames, what):
    want = au.bin_peaks(au.decode(bytes(raw), fmt, channels), bin_frames)
    same_bits(eng.frames_power(raw, fmt=fmt, bin_frames=bin_frames), want, what)


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(channels):
        if channels not in made:
            made[channels] = rocoder_amd.Engine(window_len=1024, factor=2.0, channels=channels, seed=5)
        return made[channels]

    yield get
    for e in made.values():
        e.close()


# ---- small shapes: every format with every channel count, byte phase and bin length ------------------------------------
N_SMALL = 50001
CHANNELS, BINS = (1, 2, 3, 9), (1, 7, 4410, 50000, N_SMALL + 1)
SMALL = [(fmt, CHANNELS[(i + k) % 4], (i + 3 * k + 1) % 4, BINS[i]) for k, fmt in enumerate(FORMATS) for i in range(5)]


def test_the_small_cases_cover_every_axis_with_every_format():
    for fmt in FORMATS:
        mine = [c for c in SMALL if c[0] == fmt]
        assert {c[1] for c in mine} == set(CHANNELS) and {c[2] for c in mine} == {0, 1, 2, 3} and {c[3] for c in mine} == set(BINS)


@pytest.mark.parametrize("fmt,channels,phase,bin_frames", SMALL)
def test_small_shapes(engines, fmt, channels, phase, bin_frames):
    raw = at_phase(random_block(fmt, N_SMALL, channels, 100 + channels), phase)
    check(engines(channels), raw, fmt, channels, bin_frames, f"{fmt} x{channels} phase {phase} bins of {bin_frames}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_lengths(engines, fmt):
    for channels, bin_frames in ((2, 7), (3, 4410)):
        for n in (0, 1, bin_frames - 1, bin_frames, bin_frames + 1):
            raw = at_phase(random_block(fmt, n, channels, n + 1), 1)
            got = engines(channels).frames_power(raw, fmt=fmt, bin_frames=bin_frames)
            assert got.size == -(-n // bin_frames)
            same_bits(got, au.bin_peaks(au.decode(bytes(raw), fmt, channels), bin_frames), f"{fmt} {n} frames in bins of {bin_frames}")


# ---- corner values ---------------------------------------------------------------------------------------------------
def test_corner_values(engines):
    f = np.float32
    eng = engines(1)
    got = eng.frames_power(np.array([0, 255, 128, 127, 129], np.uint8).reshape(-1, 1), bin_frames=1)
    same_bits(got, np.array([f(128) / f(127), f(1), f(0), f(1) / f(127), f(1) / f(127)], np.float32), "u8")
    assert got[0] > 1
    v = [-2 ** 31, 2 ** 31 - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, -(2 ** 24 + 1), -(2 ** 24 + 3),
         2 ** 31 - 128, 2 ** 31 - 129, 2 ** 31 - 127, 2 ** 31 - 65, 2 ** 31 - 64, -(2 ** 31 - 128), -(2 ** 31 - 64), 0, -1, 1]
    a = np.array(v, "<i4").reshape(-1, 1)
    want = np.abs(np.array(v, np.int32).astype(np.float32) / f(2147483647))
    same_bits(eng.frames_power(a, bin_frames=1), want, "i32")
    same_bits(eng.frames_power(a, bin_frames=2), au.bin_peaks(want.reshape(-1, 1), 2), "i32 in pairs")
    i24 = bytes([0, 0, 0x80, 0xff, 0xff, 0x7f, 0xff, 0xff, 0xff, 0, 0, 0])  # -8388608, 8388607, -1, 0
    same_bits(eng.frames_power(i24, fmt="i24", bin_frames=1), np.array([1, f(8388607) / f(8388608), f(1) / f(8388608), 0], np.float32), "i24")
    i16 = np.array([-32768, 32767, -32767, 0], "<i2").reshape(-1, 1)
    same_bits(eng.frames_power(i16, bin_frames=1), np.array([f(32768) / f(32767), 1, 1, 0], np.float32), "i16")
    # f32: NaN alone, NaN beside finite values, +-inf, -0.0, denormals, a bin whose largest value is negative
    den = np.array([1, 0x007fffff], np.uint32).view(np.float32)
    x = np.array([np.nan, np.nan, -np.nan, np.nan,       # a bin of nothing but NaN: +0.0
                  np.nan, 0.25, -0.5, np.nan,            # NaN skipped
                  -0.0, 0.0, -0.0, -0.0,                 # zeros of both signs: +0.0
                  1.0, -np.inf, 2.0, np.nan,             # -inf counts
                  np.inf, 3.0, np.nan, -1.0,
                  den[0], -den[1], 0.0, -0.0,            # denormals are kept
                  -3.0, 2.0, -1.0, 0.5,                  # the largest magnitude is negative
                  -den[0], 0.0, np.nan, -0.0], np.float32).reshape(-1, 1)
    want = np.array([0, 0.5, 0, np.inf, np.inf, den[1], 3.0, den[0]], np.float32)
    got = eng.frames_power(x, bin_frames=4)
    same_bits(got, want, "f32")
    assert got.view(np.uint32)[0] == 0 and got.view(np.uint32)[2] == 0
    same_bits(eng.frames_power(x, bin_frames=1), au.bin_peaks(x, 1), "f32 by sample")
    # the same values as two channels: a bin is both channels of its frames
    same_bits(engines(2).frames_power(x.reshape(-1, 2), bin_frames=2), want, "f32 stereo")


# ---- chunk and launch edges ------------------------------------------------------------------------------------------------
def big_case(eng, fmt, channels, n_frames, bin_frames, seed):
    body = random_block(fmt, n_frames, channels, seed)
    want = au.bin_peaks(au.decode(body, fmt, channels), bin_frames)
    same_bits(eng.frames_power(body, fmt=fmt, bin_frames=bin_frames), want, f"{fmt} {n_frames} frames, pageable")
    pinned = at_phase(body, 1, pinned=True)
    del body
    same_bits(eng.frames_power(pinned, fmt=fmt, bin_frames=bin_frames), want, f"{fmt} {n_frames} frames, page-locked at phase 1")


def test_u8_mono_beyond_one_launch_and_several_uploads(engines):
    """2^27 + 4099 frames: more than a launch takes, eight staging slots and a ragged one; every bin is compared, so a range
    missed, doubled or shifted at any upload or launch edge shows in some bin's maximum"""
    big_case(engines(1), "u8", 1, 2 ** 27 + 4099, 4096, 1)


def test_i16_stereo_several_uploads(engines):
    big_case(engines(2), "i16", 2, 3 * 2 ** 22 + 5, 4096, 2)


# ---- buffers and status ------------------------------------------------------------------------------------------------
def test_buffers_and_status(engines):
    eng = engines(2)
    L = _lib.lib()
    a = np.random.default_rng(3).integers(-32768, 32768, (1000, 2)).astype("<i2")
    guarded = np.full(12, 7.5, np.float32)
    peak = guarded[1:].ctypes.data_as(C.POINTER(C.c_float))
    n = C.c_size_t(99)
    src = C.c_void_p(a.ctypes.data)
    assert L.rc_engine_frames_power(eng._h, src, 1000, _lib.RC_PCM_I16, 100, peak, 9, C.byref(n)) == _lib.RC_ECAPACITY
    assert n.value == 10 and (guarded == 7.5).all()
    for fmt in (0, 6):
        n.value = 99
        assert L.rc_engine_frames_power(eng._h, src, 1000, fmt, 100, peak, 10, C.byref(n)) == _lib.RC_EINVAL
        assert n.value == 99 and (guarded == 7.5).all()
    assert L.rc_engine_frames_power(eng._h, src, 1000, _lib.RC_PCM_I16, 0, peak, 10, C.byref(n)) == _lib.RC_EINVAL
    assert L.rc_engine_frames_power(eng._h, None, 1000, _lib.RC_PCM_I16, 100, peak, 10, C.byref(n)) == _lib.RC_EINVAL
    assert L.rc_engine_frames_power(eng._h, src, 1000, _lib.RC_PCM_I16, 100, None, 10, C.byref(n)) == _lib.RC_EINVAL
    assert L.rc_engine_frames_power(eng._h, src, 1000, _lib.RC_PCM_I16, 100, peak, 10, None) == _lib.RC_EINVAL
    assert n.value == 99 and (guarded == 7.5).all()
    assert L.rc_engine_frames_power(eng._h, None, 0, _lib.RC_PCM_I16, 100, peak, 0, C.byref(n)) == _lib.RC_OK and n.value == 0
    assert (guarded == 7.5).all()
    # the exact capacity: the words around the bins stay
    assert L.rc_engine_frames_power(eng._h, src, 1000, _lib.RC_PCM_I16, 100, peak, 10, C.byref(n)) == _lib.RC_OK and n.value == 10
    assert guarded[0] == 7.5 and guarded[11] == 7.5
    same_bits(guarded[1:11].copy(), au.bin_peaks(au.decode(a.tobytes(), "i16", 2), 100), "through the C-ABI")
    with pytest.raises(ValueError):
        eng.frames_power(a, bin_frames=0)


# ---- the engine is left alone ----------------------------------------------------------------------------------------------
def kernel_times(eng):
    ms = (C.c_float * 256)()
    n = C.c_size_t(0)
    assert _lib.lib().rc_engine_kernel_times(eng._h, ms, 256, C.byref(n)) == _lib.RC_OK
    return n.value


def test_the_engine_is_left_as_it_was():
    a = np.random.default_rng(8).integers(-20000, 20000, (30000, 2)).astype("<i2")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=9) as eng:
        eng.load_device_kernel(compile_device_kernel(open(os.path.join(ROOT, "examples", "kernels", "blur.hip")).read(), "blur.hip"))
        eng.set_device_kernel_params([0.5, 0.25, 0.125, 0.125])
        n_out = eng.output_len(a.shape[0])
        eng.set_output_fade(500, n_out - 700, 700)
        count0 = kernel_times(eng)
        before = eng.stretch_frames(a, out_fmt="i16").tobytes()
        count = kernel_times(eng)
        same_bits(eng.frames_power(a, bin_frames=4410), au.bin_peaks(au.decode(a.tobytes(), "i16", 2), 4410), "between two stretch calls")
        assert kernel_times(eng) == count
        after = eng.stretch_frames(a, out_fmt="i16").tobytes()
        assert after == before
        assert kernel_times(eng) == count + (count - count0)  # (what the first stretch call added, once more)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def take(rate=44100):
    """i16 stereo: 0.7 s of noise at +-3 LSB, 1.5 s of a sine at 0.5, 0.9 s of noise at +-3 LSB: the levels 70 dB apart"""
    rng = np.random.default_rng(44)
    n0, n1, n2 = round(0.7 * rate), round(1.5 * rate), round(0.9 * rate)  # 30 870, 66 150, 39 690: whole bins of 4 410
    sine = np.rint(0.5 * 32767 * np.sin(2 * np.pi * 440 * np.arange(n1) / rate))
    x = np.concatenate([rng.integers(-3, 4, n0), sine, rng.integers(-3, 4, n2)])
    y = np.concatenate([rng.integers(-3, 4, n0), sine[::-1], rng.integers(-3, 4, n2)])
    return np.stack([x, y], axis=1).astype("<i2")


def test_end_to_end_crop_then_stretch():
    a = take()
    n = a.shape[0]
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=5) as eng:
        peaks = eng.frames_power(a, bin_frames=4410)
        want_peaks = au.bin_peaks(au.decode(a.tobytes(), "i16", 2), 4410)
        same_bits(peaks, want_peaks, "the take")
        # the separation condition of the restatement: the bins are a few LSB or the sine's level, 70 dB apart
        quiet, loud = want_peaks[want_peaks < 1e-3], want_peaks[want_peaks >= 1e-3]
        assert quiet.max() <= 3 / 32767 + 1e-9 and loud.min() > 0.3 and quiet.size > 0.3 * want_peaks.size
        assert len(set(quiet.tolist())) == 1  # every quiet bin holds a 3: bit-equal, so the percentile falls among equals
        got = autocrop_points(peaks, 4410, n, 30)
        assert got == au.autocrop_points(want_peaks, 4410, 30) and got is not None
        start, end = got
        assert (start, end) == (7 * 4410, 22 * 4410) and end < n  # (the sine fills bins 7 ... 21 of 31)
        raw = a.reshape(-1).view(np.uint8)
        cut = eng.stretch_frames(raw[start * 4:end * 4], fmt="i16", out_fmt="i16").tobytes()
        copy = eng.stretch_frames(np.ascontiguousarray(a[start:end]), out_fmt="i16").tobytes()
        assert cut == copy and len(cut) == eng.output_len(end - start) * 4


def wav_body(b):
    at = b.index(b"data")
    return b[at + 8:]


def test_cli_autocrop(tmp_path):
    a = take()
    n = a.shape[0]
    start, end = au.autocrop_points(au.bin_peaks(au.decode(a.tobytes(), "i16", 2), 4410), 4410, 30)
    whole, cropped = str(tmp_path / "whole.wav"), str(tmp_path / "cropped.wav")
    write_wav(whole, a.T / 32767.0, 44100, "i16")
    write_wav(cropped, a[start:end].T / 32767.0, 44100, "i16")
    assert wav_body(open(whole, "rb").read()) == a.tobytes()
    o1, o2 = str(tmp_path / "o1.wav"), str(tmp_path / "o2.wav")
    base = ["--seed", "5", "-w", "1024", "-f", "2", "--frames-on-gpu", "--output-format", "i16"]
    r1 = subprocess.run([CLI, "-i", whole, "-o", o1, "--autocrop"] + base, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run([CLI, "-i", cropped, "-o", o2] + base, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert open(o1, "rb").read() == open(o2, "rb").read()
    line = [s for s in r1.stderr.splitlines() if s.startswith("autocropping audio to start ")]
    assert len(line) == 1 and f"start {start} frames" in line[0] and f"end {n - end} frames" in line[0] and "later" in line[0] \
        and "earlier" in line[0], r1.stderr
    assert "autocropping" not in r2.stderr
    # -s / -d inside what remains
    r3 = subprocess.run([CLI, "-i", whole, "-o", o1, "--autocrop", "-s", "0.25", "-d", "0.5"] + base, capture_output=True, text=True, timeout=300)
    r4 = subprocess.run([CLI, "-i", cropped, "-o", o2, "-s", "0.25", "-d", "0.5"] + base, capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0 and r4.returncode == 0, (r3.stderr, r4.stderr)
    assert open(o1, "rb").read() == open(o2, "rb").read()
    # silence: nothing above the threshold, nothing cropped, and the CLI says so
    silent = str(tmp_path / "silent.wav")
    write_wav(silent, np.zeros((2, 20000)), 44100, "i16")
    r5 = subprocess.run([CLI, "-i", silent, "-o", o1, "--autocrop"] + base, capture_output=True, text=True, timeout=300)
    r6 = subprocess.run([CLI, "-i", silent, "-o", o2] + base, capture_output=True, text=True, timeout=300)
    assert r5.returncode == 0 and r6.returncode == 0 and "nothing cropped" in r5.stderr, r5.stderr
    assert open(o1, "rb").read() == open(o2, "rb").read()
