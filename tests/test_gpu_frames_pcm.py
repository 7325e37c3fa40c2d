"""GPU tests of rc_engine_stretch_frames_pcm / Engine.stretch_frames(out_fmt=...) / --output-format: PCM frames out of the
GPU, quantised, packed and counted there. The yardstick is never the code under test: it is ref = eng.stretch_frames(raw),
the f32 entry (itself tied to stretch_host and to the oracle by tests/test_gpu_frames.py), quantised in numpy by the
definition of include/rocoder_hip.h (test_frames_pcm_host.quantise). Every comparison is of bytes, with no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rocoder_amd
from conftest import ROOT
from rocoder_amd import _lib
from rocoder_amd.stretcher import pinned_empty
from test_frames_pcm_host import PCM, check_header, count_clipped, pcm_bytes, quantise
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
KERNELS = os.path.join(ROOT, "examples", "kernels")
OUT_FORMATS = ["u8", "i16", "i24", "i32", "f32"]
SHAPES = {"u8": (np.dtype(np.uint8), ()), "i16": (np.dtype("<i2"), ()), "i24": (np.dtype(np.uint8), (3,)),
          "i32": (np.dtype("<i4"), ()), "f32": (np.dtype("<f4"), ())}
GUARD = 0xA5


def noise_i16(n, ch, seed):
    """full-scale 16-bit noise, [n, ch]"""
    return np.random.default_rng(seed).integers(-32768, 32768, (n, ch), dtype=np.int64).astype("<i2")


def expected_bytes(ref, fmt):
    return ref.tobytes() if fmt == "f32" else pcm_bytes(quantise(ref, fmt), fmt)


def check_result(got, want, fmt, n_out, ch):
    dt, tail = SHAPES[fmt]
    assert got.dtype == dt and got.shape == (n_out, ch) + tail, (got.dtype, got.shape)
    g = got.tobytes()
    if g != want:
        a, b = np.frombuffer(g, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{fmt} x {ch}: {bad.size} of {a.size} bytes differ, the first at {bad[:8].tolist()}")


def into_guarded(eng, arg, fmt, want, n_out, ch, offset, in_fmt=None):
    """The call with its target `offset` bytes off a 16-byte boundary inside a larger buffer filled with the guard byte:
    the result is right and no byte in front of or behind it was written."""
    big = np.full(len(want) + 64, GUARD, np.uint8)
    lo = 16 + offset
    assert (big.ctypes.data + lo) % 4 == offset % 4
    got = eng.stretch_frames(arg, fmt=in_fmt, out=big[lo:lo + len(want)], out_fmt=fmt)
    assert np.shares_memory(got, big)
    check_result(got, want, fmt, n_out, ch)
    assert (big[:lo] == GUARD).all() and (big[lo + len(want):] == GUARD).all(), (fmt, ch, offset, "guard bytes were written")


@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("fmt", OUT_FORMATS)
def test_every_output_format_and_channel_count(fmt, ch):
    """N = 1024, f = 2, 30001 frames: the odd length and the 3-, 9- and 15-byte frames put tile edges on every byte
    phase. A fresh result, and the target at each of the four byte phases between guard bytes."""
    a = noise_i16(30001, ch, 40 + ch)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=ch, seed=3) as eng:
        ref = eng.stretch_frames(a)
        n_out = eng.output_len(30001)
        want = expected_bytes(ref, fmt)
        check_result(eng.stretch_frames(a, out_fmt=fmt), want, fmt, n_out, ch)
        assert eng.last_clipped == count_clipped(ref)
        for offset in (0, 1, 2, 3):
            into_guarded(eng, a, fmt, want, n_out, ch, offset)
            assert eng.last_clipped == count_clipped(ref)


def test_f32_out_equals_the_f32_entry_bit_for_bit():
    a = noise_i16(30001, 2, 9)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        ref = eng.stretch_frames(a)
        got = eng.stretch_frames(a, out_fmt="f32")
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("fmt", ["i16", "i24"])
def test_more_channels_than_a_wave(fmt):
    """67 channels: a second channel tile of three channels, whose 6- and 9-byte segments start on every phase"""
    a = noise_i16(3000, 67, 5)
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=67, seed=5) as eng:
        ref = eng.stretch_frames(a)
        n_out = eng.output_len(3000)
        want = expected_bytes(ref, fmt)
        for offset in (0, 1, 2, 3):
            into_guarded(eng, a, fmt, want, n_out, 67, offset)
        assert eng.last_clipped == count_clipped(ref)


SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel


@pytest.fixture(scope="module")
def chunked():
    """The shape of tests/test_gpu_frames.py's `chunked`: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks. The yardstick and its quantised bytes are computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4)
    ref = eng.stretch_frames(a)
    assert ref.shape[0] > 2 * SLOT_FLOATS
    want = {fmt: expected_bytes(ref, fmt) for fmt in ("i24", "u8")}
    clipped = count_clipped(ref)
    yield eng, a, want, ref.shape[0], clipped
    eng.close()


@pytest.mark.parametrize("src_kind,out_kind", [("pageable", "pageable"), ("pinned", "pinned"), ("pageable", "pinned"),
                                               ("pinned", "pageable"), ("pageable", "offset1"), ("pinned", "pinned3")])
@pytest.mark.parametrize("fmt", ["i24", "u8"])
def test_several_pipeline_chunks_with_either_kind_of_memory(chunked, fmt, src_kind, out_kind):
    """(offset1, pinned3: the target 1 and 3 bytes off a dword, so that every chunk edge lies inside one)"""
    eng, a, want, n_out, clipped = chunked
    want = want[fmt]
    src = a
    if src_kind == "pinned":
        src = pinned_empty(a.shape, a.dtype)
        src[:] = a
    if out_kind == "pageable":
        got = eng.stretch_frames(src, out_fmt=fmt)
    else:
        off = {"pinned": 0, "offset1": 1, "pinned3": 3}[out_kind]
        big = pinned_empty(len(want) + 32, np.uint8) if out_kind.startswith("pinned") else np.empty(len(want) + 32, np.uint8)
        big[:] = GUARD
        got = eng.stretch_frames(src, out=big[16 + off:16 + off + len(want)], out_fmt=fmt)
        assert (big[:16 + off] == GUARD).all() and (big[16 + off + len(want):] == GUARD).all(), "guard bytes were written"
    check_result(got, want, fmt, n_out, 3)
    assert eng.last_clipped == clipped


def test_chunk_edges_inside_a_dword():
    """A negative pitch multiple whose window_out_len x channels x bytes is no multiple of 4 - and neither is a whole
    chunk of such windows, so the byte ranges of neighbouring chunks meet inside a dword even in an aligned target."""
    with rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21, pitch_multiple=-19) as eng:
        wout = int(eng.params.window_out_len)
        assert (wout * 3 * 3) % 4 != 0
        assert ((SLOT_FLOATS // wout) * wout * 3 * 3) % 4 != 0
        a = np.random.default_rng(6).integers(0, 256, (11_000_000, 3), dtype=np.uint8)
        ref = eng.stretch_frames(a)
        n_out = ref.shape[0]
        assert n_out > 2 * SLOT_FLOATS
        want = expected_bytes(ref, "i24")
        for offset in (0, 2):
            into_guarded(eng, a, "i24", want, n_out, 3, offset)
        assert eng.last_clipped == count_clipped(ref)


def test_clipped_samples_are_counted():
    """A raised amplitude on full-scale noise: the test first asserts on the f32 yardstick that between 0.1 % and 50 %
    of its samples lie beyond full scale, so it cannot pass with nothing to count. The amplitude: at amplitude 6 the
    yardstick had 60.6 % of its samples beyond full scale (72004 of 118784), too many for the upper bound. The stretched
    noise is close to Gaussian, so P(|x| > 1) = 0.606 puts its standard deviation at 1.94 = 0.32 x amplitude; amplitude 2
    then gives a deviation of 0.65 and an expected share of P(|z| > 1.55) = 12 %, far from both bounds."""
    a = noise_i16(30001, 2, 12)
    L = _lib.lib()
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=2.0) as eng:
        ref = eng.stretch_frames(a)
        n_clip = count_clipped(ref)
        share = n_clip / ref.size
        print(f"share of the yardstick beyond full scale at amplitude 2: {share:.4f} ({n_clip} of {ref.size})")
        assert 0.001 <= share <= 0.5, share
        for fmt in ("i16", "f32"):
            got = eng.stretch_frames(a, out_fmt=fmt)
            check_result(got, expected_bytes(ref, fmt), fmt, ref.shape[0], 2)
            assert eng.last_clipped == n_clip, (fmt, eng.last_clipped, n_clip)
        # clipped = NULL through the raw entry
        out = np.zeros(ref.size, "<i2")
        got_n = C.c_size_t(0)
        assert L.rc_engine_stretch_frames_pcm(eng._h, a.ctypes.data, 30001, _lib.RC_PCM_I16, out.ctypes.data, ref.shape[0],
                                              _lib.RC_PCM_I16, C.byref(got_n), None) == _lib.RC_OK
        assert got_n.value == ref.shape[0] and out.tobytes() == expected_bytes(ref, "i16")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, amplitude=0.01) as eng:
        ref = eng.stretch_frames(a)
        assert count_clipped(ref) == 0
        check_result(eng.stretch_frames(a, out_fmt="i16"), expected_bytes(ref, "i16"), "i16", ref.shape[0], 2)
        assert eng.last_clipped == 0


def test_with_a_user_device_kernel():
    from rocoder_amd.stretcher import compile_device_kernel

    code = compile_device_kernel(open(os.path.join(KERNELS, "blur.hip")).read(), "blur.hip")
    a = noise_i16(30001, 2, 13)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        eng.load_device_kernel(code)
        ref = eng.stretch_frames(a)
        check_result(eng.stretch_frames(a, out_fmt="i16"), expected_bytes(ref, "i16"), "i16", ref.shape[0], 2)
        assert eng.last_clipped == count_clipped(ref)


def test_with_a_curated_device_kernel():
    a = noise_i16(30001, 2, 14)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, device_kernel=("gain", 0.5)) as eng:
        ref = eng.stretch_frames(a)
        check_result(eng.stretch_frames(a, out_fmt="i16"), expected_bytes(ref, "i16"), "i16", ref.shape[0], 2)
        assert eng.last_clipped == count_clipped(ref)


def test_with_a_host_frequency_kernel():
    """whole input up, the job, one pack, one download - into a target at an odd address"""
    a = noise_i16(30001, 2, 15)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x,
                            kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a)
        want = expected_bytes(ref, "i16")
        check_result(eng.stretch_frames(a, out_fmt="i16"), want, "i16", ref.shape[0], 2)
        assert eng.last_clipped == count_clipped(ref)
        into_guarded(eng, a, "i16", want, ref.shape[0], 2, 1)


@pytest.mark.parametrize("n", [0, 1, 1023])
def test_small_lengths(n):
    a = noise_i16(n, 3, 16)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=3, seed=3) as eng:
        ref = eng.stretch_frames(a)
        for fmt in ("u8", "i24"):
            want = expected_bytes(ref, fmt)
            into_guarded(eng, a, fmt, want, ref.shape[0], 3, 3)
            assert eng.last_clipped == count_clipped(ref)


def test_status_codes_and_python_argument_checks():
    L = _lib.lib()
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        a = np.zeros((5000, 2), np.int16)
        n_out = eng.output_len(5000)
        out = np.zeros((n_out, 2), "<i2")
        clipped = C.c_uint64(77)
        call = lambda src, fmt, dst, cap, ofmt: L.rc_engine_stretch_frames_pcm(eng._h, src, 5000, fmt, dst, cap, ofmt, None, C.byref(clipped))
        for bad in (0, 6, 255):
            assert call(a.ctypes.data, 2, out.ctypes.data, n_out, bad) == _lib.RC_EINVAL
            assert call(a.ctypes.data, bad, out.ctypes.data, n_out, 2) == _lib.RC_EINVAL
        assert call(None, 2, out.ctypes.data, n_out, 2) == _lib.RC_EINVAL
        assert call(a.ctypes.data, 2, None, n_out, 2) == _lib.RC_EINVAL
        assert call(a.ctypes.data, 2, out.ctypes.data, n_out - 1, 2) == _lib.RC_ECAPACITY
        assert clipped.value == 77 and not out.any()
        assert call(a.ctypes.data, 2, out.ctypes.data, n_out, 2) == _lib.RC_OK and clipped.value == 0
        with pytest.raises(ValueError):
            eng.stretch_frames(a, out_fmt="i20")
        with pytest.raises(ValueError):
            eng.stretch_frames(a, out=np.empty(n_out * 2 * 2 - 1, np.uint8), out_fmt="i16")
        assert eng.stretch_frames(a).dtype == np.float32  # out_fmt=None: the array of old


def run_cli(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("amp", [None, "6"])
def test_cli_output_format(tmp_path, amp):
    """A 2-channel i16 file: --output-format i16 and input, with and without --frames-on-gpu, write one and the same
    file; its header is a 16-bit PCM header and its data chunk the quantised yardstick; with -a 6 the stderr line names
    numpy's count; without the flag the file is the f32 file of old."""
    x = np.random.default_rng(17).uniform(-1, 1, (2, 5000))
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    body = np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]
    common = ["-i", wav, "--seed", "5", "-w", "1024", "-f", "4"] + (["-a", amp] if amp else [])
    with rocoder_amd.Engine(window_len=1024, factor=4.0, channels=2, seed=5, amplitude=float(amp or 1)) as eng:
        ref = eng.stretch_frames(body, fmt="i16")
    n_clip = count_clipped(ref)
    if amp:  # (at amplitude 1 the stretch overshoots now and then as well: the line is checked against numpy's count either way)
        assert n_clip > 0
    files = []
    for k, extra in enumerate((["--output-format", "i16"], ["--output-format", "input"], ["--output-format", "i16", "--frames-on-gpu"],
                               ["--output-format", "input", "--frames-on-gpu"])):
        out = str(tmp_path / f"o{k}.wav")
        r = run_cli(*common, "-o", out, *extra)
        assert not os.path.exists(out + ".part")
        lines = [l for l in r.stderr.splitlines() if "clipped" in l]
        assert lines == ([f"{n_clip} of {ref.size} samples clipped"] if n_clip else []), r.stderr
        files.append(open(out, "rb").read())
    assert all(f == files[0] for f in files)
    assert check_header(files[0], "i16", 2, 44100) == expected_bytes(ref, "i16")
    if amp:
        return
    old = []
    for k, extra in enumerate(([], ["--output-format", "f32"], ["--output-format", "f32", "--frames-on-gpu"])):
        out = str(tmp_path / f"f{k}.wav")
        r = run_cli(*common, "-o", out, *extra)
        if "--output-format" not in extra:
            assert "clipped" not in r.stderr
        old.append(open(out, "rb").read())
    assert all(f == old[0] for f in old)
    assert check_header(old[0], "f32", 2, 44100) == ref.tobytes()
