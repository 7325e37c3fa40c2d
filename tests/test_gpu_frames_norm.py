"""GPU tests of rc_engine_stretch_frames_norm / Engine.stretch_frames(normalize=...) / --normalize: the peak of the whole job
measured on the GPU, one gain applied there in front of the quantiser. The yardstick is never the code under test: it is
ref = eng.stretch_frames(raw), the f32 entry (tied to stretch_host and to the oracle by tests/test_gpu_frames.py), put
through test_frames_norm_host.normalise - the definition of include/rocoder_hip.h in numpy - and then through the
quantiser of test_frames_pcm_host. Every comparison is of bytes, peak and gain are compared as bits, clipped as an
integer: there is no tolerance anywhere but in `check_levels`, whose bound is derived there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rocoder_amd
from conftest import ROOT
from rocoder_amd import _lib
from rocoder_amd.stretcher import pinned_empty
from test_frames_norm_host import normalise
from test_frames_pcm_host import PCM, check_header, count_clipped, pcm_bytes, quantise
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
KERNELS = os.path.join(ROOT, "examples", "kernels")
OUT_FORMATS = ["u8", "i16", "i24", "i32", "f32"]
SHAPES = {"u8": (np.dtype(np.uint8), ()), "i16": (np.dtype("<i2"), ()), "i24": (np.dtype(np.uint8), (3,)),
          "i32": (np.dtype("<i4"), ()), "f32": (np.dtype("<f4"), ())}
GUARD = 0xA5


def noise_i16(n, ch, seed, scale=32768):
    """16-bit noise of +-scale, [n, ch]"""
    return np.random.default_rng(seed).integers(-scale, scale, (n, ch), dtype=np.int64).astype("<i2")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def expected(ref, target, fmt):
    """(bytes, peak, gain, clipped) the definition gives for the f32 result `ref`"""
    z, peak, gain = normalise(ref, target)
    return (z.tobytes() if fmt == "f32" else pcm_bytes(quantise(z, fmt), fmt)), peak, gain, count_clipped(z)


def decode_ints(got, fmt):
    """the integers of a result of an integer format"""
    g = got.astype(np.int64)
    if fmt == "u8":
        return g - 128
    if fmt == "i24":
        v = g[..., 0] | (g[..., 1] << 8) | (g[..., 2] << 16)
        return v - ((v & 0x800000) << 1)
    return g


def check_result(got, want, fmt, n_out, ch):
    dt, tail = SHAPES[fmt]
    assert got.dtype == dt and got.shape == (n_out, ch) + tail, (got.dtype, got.shape)
    g = got.tobytes()
    if g != want:
        a, b = np.frombuffer(g, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{fmt} x {ch}: {bad.size} of {a.size} bytes differ, the first at {bad[:8].tolist()}")


def check_words(eng, peak, gain, clipped):
    assert (bits(eng.last_peak), bits(eng.last_gain), eng.last_clipped) == (bits(peak), bits(gain), clipped), \
        (eng.last_peak, eng.last_gain, eng.last_clipped, peak, gain, clipped)


def check_levels(peak, gain, target):
    """peak * gain is the target to two roundings: the division's (relative error at most 2^-24) and the
    multiplication's (the same) - together below 2^-23 of the target."""
    level = float(np.float32(peak) * np.float32(gain))
    assert abs(level - target) <= target * 2.0 ** -23, (peak, gain, level, target)


def call(eng, arg, fmt, target, want, n_out, ch, in_fmt=None):
    want_bytes, peak, gain, clipped = want
    check_result(eng.stretch_frames(arg, fmt=in_fmt, out_fmt=fmt, normalize=target), want_bytes, fmt, n_out, ch)
    check_words(eng, peak, gain, clipped)


def into_guarded(eng, arg, fmt, target, want, n_out, ch, offset, in_fmt=None, pinned=False):
    """The call with its target `offset` bytes off a 16-byte boundary inside a larger buffer filled with the guard byte:
    the result is right and no byte in front of or behind it was written."""
    want_bytes, peak, gain, clipped = want
    big = pinned_empty(len(want_bytes) + 64, np.uint8) if pinned else np.empty(len(want_bytes) + 64, np.uint8)
    big[:] = GUARD
    lo = 16 + offset
    assert (big.ctypes.data + lo) % 4 == offset % 4
    got = eng.stretch_frames(arg, fmt=in_fmt, out=big[lo:lo + len(want_bytes)], out_fmt=fmt, normalize=target)
    assert np.shares_memory(got, big)
    check_result(got, want_bytes, fmt, n_out, ch)
    assert (big[:lo] == GUARD).all() and (big[lo + len(want_bytes):] == GUARD).all(), (fmt, ch, offset, "guard bytes were written")
    check_words(eng, peak, gain, clipped)


@pytest.mark.parametrize("target", [1.0, 0.5])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", OUT_FORMATS)
def test_a_loud_job_comes_out_at_the_target(fmt, ch, target):
    """N = 1024, f = 2, 30001 frames of full-scale noise at amplitude 2: the f32 result overshoots full scale (asserted:
    peak > 1, at least 0.1 % of the samples beyond it), so the gain is below 1 and an integer file that would have
    clipped them no longer does."""
    a = noise_i16(30001, ch, 40 + ch)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=ch, seed=3, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        n_out = eng.output_len(30001)
        share = count_clipped(ref) / ref.size
        print(f"{ch} channels: peak {np.abs(ref).max():.4f}, {share:.4f} of the yardstick beyond full scale")
        assert np.abs(ref).max() > 1 and share >= 0.001
        want = expected(ref, target, fmt)
        _, peak, gain, clipped = want
        assert gain < 1
        check_levels(peak, gain, target)
        assert clipped < count_clipped(ref) and clipped <= (1 if target == 1.0 else 0) * np.count_nonzero(np.abs(ref) == peak)
        call(eng, a, fmt, target, want, n_out, ch)
        if fmt != "f32":  # the level of what was written, decoded: half a quantisation step, the two roundings of
            # check_levels and the one step by which the clamp is asymmetric, from the target
            got = eng.stretch_frames(a, out_fmt=fmt, normalize=target)
            q = decode_ints(got, fmt)
            s = PCM[fmt][0]
            assert abs(np.abs(q).max() / s - target) <= 1.0 / s + target * 2.0 ** -23, (np.abs(q).max(), s, target)
        for offset in (0, 1, 2, 3):
            into_guarded(eng, a, fmt, target, want, n_out, ch, offset)


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_a_quiet_job_is_raised(fmt):
    a = noise_i16(30001, 2, 12)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=0.01) as eng:
        ref = eng.stretch_frames(a)
        assert 0 < np.abs(ref).max() < 1
        want = expected(ref, 1.0, fmt)
        assert want[2] > 1
        check_levels(want[1], want[2], 1.0)
        call(eng, a, fmt, 1.0, want, ref.shape[0], 2)
        into_guarded(eng, a, fmt, 1.0, want, ref.shape[0], 2, 3)


@pytest.mark.parametrize("fmt", ["i16", "i24"])
def test_more_channels_than_a_wave(fmt):
    """67 channels: the wide pack kernel with a gain (its samples in front of a row segment included), and a peak
    launch of 67 rows"""
    a = noise_i16(3000, 67, 5)
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=67, seed=5, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        assert np.abs(ref).max() > 1
        n_out = eng.output_len(3000)
        want = expected(ref, 1.0, fmt)
        for offset in (0, 1, 2, 3):
            into_guarded(eng, a, fmt, 1.0, want, n_out, 67, offset)


SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel


@pytest.fixture(scope="module", params=["start", "end"])
def chunked(request):
    """The shape of tests/test_gpu_frames_pcm.py's `chunked`: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks. Quarter-scale noise with one full-scale burst of 4096 frames near the start or near the end of the
    input: the peak is found in one chunk (asserted on the yardstick: in the first / the last third of the output) and
    has to reach the pack of every other. The yardstick and its bytes are computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4, scale=8192)
    at = 20_000 if request.param == "start" else 1_200_000 - 30_000
    a[at:at + 4096] = noise_i16(4096, 3, 5)
    ref = eng.stretch_frames(a)
    n_out = ref.shape[0]
    assert n_out > 2 * SLOT_FLOATS
    where = int(np.argmax(np.abs(ref).max(axis=1)))
    assert where < n_out // 3 if request.param == "start" else where > 2 * n_out // 3, (where, n_out)
    want = {fmt: expected(ref, 0.9, fmt) for fmt in ("i24", "u8")}
    del ref
    yield eng, a, want, n_out
    eng.close()


@pytest.mark.parametrize("fmt,kind,offset", [("i24", "pageable", 0), ("u8", "pageable", 0), ("i24", "pinned", 0), ("u8", "pinned", 0),
                                             ("i24", "pageable", 1)])
def test_a_peak_in_one_chunk_reaches_every_other(chunked, fmt, kind, offset):
    """(offset 1: the target 1 byte off a dword, so that every chunk edge lies inside one)"""
    eng, a, want, n_out = chunked
    src = a
    if kind == "pinned":
        src = pinned_empty(a.shape, a.dtype)
        src[:] = a
    into_guarded(eng, src, fmt, 0.9, want[fmt], n_out, 3, offset, pinned=kind == "pinned")


def test_negative_pitch_multiple_chunk_edges_inside_a_dword():
    """The shape of test_gpu_frames_pcm.test_chunk_edges_inside_a_dword: neither a window nor a chunk of windows is a
    whole number of dwords of 9-byte frames."""
    with rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21, pitch_multiple=-19) as eng:
        wout = int(eng.params.window_out_len)
        assert (wout * 3 * 3) % 4 != 0 and ((SLOT_FLOATS // wout) * wout * 3 * 3) % 4 != 0
        a = np.random.default_rng(6).integers(0, 256, (11_000_000, 3), dtype=np.uint8)
        ref = eng.stretch_frames(a)
        n_out = ref.shape[0]
        assert n_out > 2 * SLOT_FLOATS
        want = expected(ref, 1.0, "i24")
        del ref
        into_guarded(eng, a, "i24", 1.0, want, n_out, 3, 2)


def test_non_finite_samples_are_skipped_by_the_peak():
    """f32 frames with one NaN and one +inf mid-file: the windows that read them come out as NaN, the rest is finite. The
    peak is the finite maximum, NaN is written as 0 and counted as clipped."""
    a = np.random.default_rng(8).uniform(-1, 1, (30001, 2)).astype(np.float32)
    a[15000, 0] = np.nan
    a[15100, 1] = np.inf
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        nan = np.isnan(ref)
        fin = np.isfinite(ref)
        assert nan.any() and (fin & (ref != 0)).any()
        peak = np.abs(ref[fin]).max()
        for fmt in ("i16", "u8"):
            want = expected(ref, 1.0, fmt)
            assert bits(want[1]) == bits(peak) and want[3] >= np.count_nonzero(nan)
            got = eng.stretch_frames(a, out_fmt=fmt, normalize=1.0)
            check_result(got, want[0], fmt, ref.shape[0], 2)
            check_words(eng, peak, want[2], want[3])
            assert (got[nan] == (128 if fmt == "u8" else 0)).all()


@pytest.mark.parametrize("n", [0, 1, 1023, 5000])
def test_degenerate_inputs(n):
    """No frames, fewer frames than a window, and (5000) silence: peak 0, gain 1, the bytes of zeros"""
    a = noise_i16(n, 3, 16) if n != 5000 else np.zeros((n, 3), "<i2")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=3, seed=3) as eng:
        ref = eng.stretch_frames(a)
        for fmt in ("u8", "i24", "f32"):
            want = expected(ref, 0.5, fmt)
            if n in (0, 5000):
                assert not ref.any() and (bits(want[1]), bits(want[2]), want[3]) == (0, bits(1.0), 0)
            into_guarded(eng, a, fmt, 0.5, want, ref.shape[0], 3, 3)


def test_with_a_user_device_kernel():
    from rocoder_amd.stretcher import compile_device_kernel

    code = compile_device_kernel(open(os.path.join(KERNELS, "blur.hip")).read(), "blur.hip")
    a = noise_i16(30001, 2, 13)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        eng.load_device_kernel(code)
        ref = eng.stretch_frames(a)
        call(eng, a, "i16", 1.0, expected(ref, 1.0, "i16"), ref.shape[0], 2)


def test_with_a_curated_device_kernel():
    a = noise_i16(30001, 2, 14)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, device_kernel=("gain", 0.5)) as eng:
        ref = eng.stretch_frames(a)
        call(eng, a, "i16", 1.0, expected(ref, 1.0, "i16"), ref.shape[0], 2)


def test_with_a_host_frequency_kernel():
    """whole input up, the job, the peak kernel, one pack, one download - into a target at an odd address"""
    a = noise_i16(30001, 2, 15)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x,
                            kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a)
        want = expected(ref, 1.0, "i16")
        call(eng, a, "i16", 1.0, want, ref.shape[0], 2)
        into_guarded(eng, a, "i16", 1.0, want, ref.shape[0], 2, 1)


def test_raw_entry_status_codes_and_null_out_pointers():
    L = _lib.lib()
    a = noise_i16(5000, 2, 18)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        n_out = ref.shape[0]
        want = expected(ref, 1.0, "i16")
        out = np.zeros((n_out, 2), "<i2")
        assert L.rc_engine_stretch_frames_norm(eng._h, a.ctypes.data, 5000, _lib.RC_PCM_I16, out.ctypes.data, n_out, _lib.RC_PCM_I16,
                                               1.0, None, None, None, None) == _lib.RC_OK
        assert out.tobytes() == want[0]
        out[:] = 0
        n, clipped, peak, gain = C.c_size_t(7), C.c_uint64(9), C.c_float(3), C.c_float(4)
        tail = (C.byref(n), C.byref(peak), C.byref(gain), C.byref(clipped))
        f = lambda src, fmt, dst, cap, ofmt, t: L.rc_engine_stretch_frames_norm(eng._h, src, 5000, fmt, dst, cap, ofmt, t, *tail)
        for bad in (0, 6, 255):
            assert f(a.ctypes.data, 2, out.ctypes.data, n_out, bad, 1.0) == _lib.RC_EINVAL
            assert f(a.ctypes.data, bad, out.ctypes.data, n_out, 2, 1.0) == _lib.RC_EINVAL
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            assert f(a.ctypes.data, 2, out.ctypes.data, n_out, 2, bad) == _lib.RC_EINVAL
        assert f(None, 2, out.ctypes.data, n_out, 2, 1.0) == _lib.RC_EINVAL
        assert f(a.ctypes.data, 2, None, n_out, 2, 1.0) == _lib.RC_EINVAL
        assert f(a.ctypes.data, 2, out.ctypes.data, n_out - 1, 2, 1.0) == _lib.RC_ECAPACITY
        assert (n.value, clipped.value, peak.value, gain.value) == (7, 9, 3.0, 4.0) and not out.any()
        assert f(a.ctypes.data, 2, out.ctypes.data, n_out, 2, 1.0) == _lib.RC_OK
        assert (n.value, bits(peak.value), bits(gain.value), clipped.value) == (n_out, bits(want[1]), bits(want[2]), want[3])
        for bad in (0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                eng.stretch_frames(a, out_fmt="i16", normalize=bad)
        got = eng.stretch_frames(a, normalize=0.5)  # out_fmt=None: f32
        assert got.dtype == np.float32 and got.tobytes() == expected(ref, 0.5, "f32")[0]


def test_the_plain_pcm_entry_is_what_it_was_around_a_normalised_call():
    """The new phase leaves no state behind: out_fmt without normalize gives the same bytes - the f32 yardstick
    quantised as it is - before and after a normalised call on the same engine, and so does the f32 entry."""
    a = noise_i16(30001, 2, 19)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        plain = pcm_bytes(quantise(ref, "i16"), "i16")
        before = eng.stretch_frames(a, out_fmt="i16").tobytes()
        n_before = eng.last_clipped
        call(eng, a, "i16", 0.5, expected(ref, 0.5, "i16"), ref.shape[0], 2)
        after = eng.stretch_frames(a, out_fmt="i16").tobytes()
        assert before == plain and after == plain
        assert n_before == eng.last_clipped == count_clipped(ref)
        assert eng.stretch_frames(a).tobytes() == ref.tobytes()


def test_cli_normalize(tmp_path):
    """A 2-channel i16 file at -a 6: --normalize 0.9 --output-format i16 --frames-on-gpu writes the yardstick's bytes
    behind a 16-bit header, and the stderr line carries numpy's peak and gain."""
    x = np.random.default_rng(17).uniform(-1, 1, (2, 5000))
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    body = np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]
    with rocoder_amd.Engine(window_len=1024, factor=4.0, channels=2, seed=5, amplitude=6.0) as eng:
        ref = eng.stretch_frames(body, fmt="i16")
    assert np.abs(ref).max() > 1
    want, peak, gain, clipped = expected(ref, 0.9, "i16")
    out = str(tmp_path / "o.wav")
    r = subprocess.run([CLI, "-i", wav, "--seed", "5", "-w", "1024", "-f", "4", "-a", "6", "-o", out, "--normalize", "0.9",
                        "--output-format", "i16", "--frames-on-gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, 44100) == want
    lines = [re.fullmatch(r"peak (\S+), gain (\S+)", l) for l in r.stderr.splitlines() if l.startswith("peak ")]
    assert len(lines) == 1 and lines[0], r.stderr
    assert (bits(float(lines[0].group(1))), bits(float(lines[0].group(2)))) == (bits(peak), bits(gain)), r.stderr
    assert [l for l in r.stderr.splitlines() if "clipped" in l] == ([f"{clipped} of {ref.size} samples clipped"] if clipped else [])
