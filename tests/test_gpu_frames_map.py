"""GPU tests of rc_engine_set_channel_map / rc_engine_frames_channel_peaks / rc_split_mono_map, their Python mirror and
the CLI's --channel-map / --split-mono. Everything is bit for bit, with no tolerance anywhere.
  - The map's expected result is the unmapped entry on the host-permuted block (`a[:, map]`): the unmapped entry is held
    to the oracle by tests/test_gpu_frames*.py and is not the code under test.
  - Expected channel peaks and split maps are the numpy restatement of tests/splitmonoutil.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import autocroputil as au
import rocoder_amd
import splitmonoutil as sm
from conftest import ROOT
from rocoder_amd import _lib, split_mono_map
from rocoder_amd.stretcher import compile_device_kernel, pinned_empty
from test_gpu_frames import make_frames
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
FORMATS = ("u8", "i16", "i24", "i32", "f32")
F32P, U32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def at_phase(raw, phase, pinned=False):
    """the bytes `raw` copied to an address that is `phase` bytes behind a multiple of 4"""
    raw = np.frombuffer(raw, np.uint8)
    big = pinned_empty(raw.size + 8, np.uint8) if pinned else np.empty(raw.size + 8, np.uint8)
    off = (phase - big.ctypes.data) % 4
    view = big[off:off + raw.size]
    view[:] = raw
    assert (big.ctypes.data + off) % 4 == phase
    return view


def permuted(raw, fmt, channels, cmap):
    """the block whose frame f holds at channel c the sample (f, cmap[c]) of `raw`: a[:, cmap] on the samples' bytes"""
    b = np.frombuffer(raw, np.uint8).reshape(-1, channels, au.PCM_BYTES[fmt])
    return np.ascontiguousarray(b[:, list(cmap), :]).reshape(-1)


def maps_of(channels, seed=0):
    c = channels
    rng = np.random.default_rng(1000 + channels + seed)
    return {"reverse": [c - 1 - k for k in range(c)], "rotate": [(k + c - 1) % c for k in range(c)], "from_one": [c // 2] * c,
            "from_last": [c - 1] * c, "identity": list(range(c)), "random": rng.integers(0, c, c).tolist()}


def mapped_equals_permuted(eng, raw, fmt, channels, cmap, phase, what, **kw):
    """`stretch_frames(**kw)` of `raw` at byte phase `phase` under `cmap` against the same call with no map on the permuted
    block; returns the bytes"""
    eng.set_channel_map(None)
    want = eng.stretch_frames(permuted(raw, fmt, channels, cmap), fmt=fmt, **kw)
    want_words = (eng.last_peak, eng.last_gain, eng.last_clipped)
    eng.set_channel_map(cmap)
    got = eng.stretch_frames(at_phase(raw, phase), fmt=fmt, **kw)
    got_words = (eng.last_peak, eng.last_gain, eng.last_clipped)
    eng.set_channel_map(None)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))[0]
        raise AssertionError(f"{what}: {bad.size} of {got.nbytes} bytes differ, the first at {bad[:6].tolist()}")
    assert repr(got_words) == repr(want_words), (what, got_words, want_words)
    return got.tobytes()


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(channels, window_len=1024, factor=2.0):
        key = (channels, window_len, factor)
        if key not in made:
            made[key] = rocoder_amd.Engine(window_len=window_len, factor=factor, channels=channels, seed=5)
        return made[key]

    yield get
    for e in made.values():
        e.close()


# ---- the narrow tiles: up to 8 channels, 1024 whole frames a tile ----------------------------------------------------------
NARROW = [(fmt, ch, (i + k) % 4) for k, fmt in enumerate(FORMATS) for i, ch in enumerate((1, 2, 3, 8))]


def test_the_narrow_cases_meet_every_byte_phase():
    for fmt in FORMATS:
        assert {c[2] for c in NARROW if c[0] == fmt} == {0, 1, 2, 3}


@pytest.mark.parametrize("fmt,channels,phase", NARROW)
def test_narrow_map(engines, fmt, channels, phase):
    """3001 frames: two full tiles of 1024 frames and a ragged one"""
    eng = engines(channels)
    _arg, raw, _dec = make_frames(fmt, channels, 3001, 11 + channels)
    plain = None
    for name in ("reverse", "rotate", "from_one", "identity"):
        cmap = maps_of(channels)[name]
        what = f"{fmt} x{channels} phase {phase} {name}"
        f32 = mapped_equals_permuted(eng, raw, fmt, channels, cmap, phase, what)
        mapped_equals_permuted(eng, raw, fmt, channels, cmap, phase, what + " -> i16", out_fmt="i16")
        if name == "identity":
            plain = f32
    assert plain == eng.stretch_frames(raw, fmt=fmt).tobytes()  # an identity map is no map


def test_narrow_map_edge_lengths(engines):
    eng = engines(3)
    for n in (0, 1, 1023, 1024, 1025):
        _arg, raw, _dec = make_frames("i24", 3, n, n + 1)
        mapped_equals_permuted(eng, raw, "i24", 3, [2, 0, 1], 1, f"{n} frames")
        mapped_equals_permuted(eng, raw, "i24", 3, [1, 1, 1], 3, f"{n} frames from one", out_fmt="i16")


# ---- the wide tiles: 64 frames x 64 channels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i16", "i24"])
@pytest.mark.parametrize("channels,names", [(9, ("reverse", "random")),      # one partial channel tile
                                            (67, ("reverse", "from_last")),  # sources in the other channel tile; all from 66
                                            (130, ("rotate", "random"))])    # three tiles, the last ragged
def test_wide_map(engines, fmt, channels, names):
    eng = engines(channels, window_len=256)
    _arg, raw, _dec = make_frames(fmt, channels, 3000, 7)
    for k, name in enumerate(names):
        cmap = maps_of(channels)[name]
        if (channels, name) == (67, "reverse"):
            assert all(cmap[c] // 64 != c // 64 for c in (0, 1, 2, 64, 65, 66))  # rows fed from the other channel tile
        mapped_equals_permuted(eng, raw, fmt, channels, cmap, 1 + k, f"{fmt} x{channels} {name}")
    mapped_equals_permuted(eng, raw, fmt, channels, maps_of(channels)[names[0]], 3, f"{fmt} x{channels} -> i16", out_fmt="i16")


# ---- several pipeline chunks: unpack launches with frame0 > 0 ------------------------------------------------------------------
def test_several_pipeline_chunks():
    with rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21) as eng:
        _arg, raw, _dec = make_frames("i24", 3, 600_001, 4)
        ref = eng.stretch_frames(permuted(raw, "i24", 3, [2, 0, 1]), fmt="i24")
        assert ref.shape[0] > (16 << 20) // 4  # more than one staging slot per channel
        big = np.zeros(len(raw) + 64, np.uint8)
        big[1:1 + len(raw)] = np.frombuffer(raw, np.uint8)
        eng.set_channel_map([2, 0, 1])
        got = eng.stretch_frames(big[1:1 + len(raw)], fmt="i24")
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---- the normalised entry, the fade, a host frequency kernel --------------------------------------------------------------------
def test_normalised_entry_and_fade(engines):
    eng = engines(3)
    _arg, raw, _dec = make_frames("i16", 3, 20001, 3)
    for cmap in ([2, 0, 1], [1, 1, 1]):
        mapped_equals_permuted(eng, raw, "i16", 3, cmap, 1, f"normalised {cmap}", out_fmt="i16", normalize=0.9)
        assert eng.last_peak is not None and eng.last_gain is not None
    n_out = eng.output_len(20001)
    eng.set_output_fade(500, n_out - 700, 700)
    try:
        mapped_equals_permuted(eng, raw, "i16", 3, [2, 0, 1], 2, "normalised with a fade", out_fmt="i24", normalize=0.5)
        mapped_equals_permuted(eng, raw, "i16", 3, [0, 0, 2], 2, "f32 with a fade")
    finally:
        eng.set_output_fade()


def test_with_a_host_frequency_kernel():
    """the whole-job branch: the whole input up, one unpack launch, the kernel's own pipeline"""
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x, kernel_time_ms=1) as eng:
        _arg, raw, _dec = make_frames("i16", 2, 5001, 2)
        mapped_equals_permuted(eng, raw, "i16", 2, [1, 0], 1, "host kernel")
        mapped_equals_permuted(eng, raw, "i16", 2, [1, 1], 0, "host kernel, normalised", out_fmt="i16", normalize=0.9)


def test_with_a_user_device_kernel_downstream():
    code = compile_device_kernel(open(os.path.join(ROOT, "examples", "kernels", "mid_side.hip")).read(), "mid_side.hip")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        eng.load_device_kernel(code)
        _arg, raw, _dec = make_frames("i24", 2, 9001, 2)
        mapped_equals_permuted(eng, raw, "i24", 2, [1, 0], 1, "mid_side behind the map")


# ---- state -----------------------------------------------------------------------------------------------------------------
def test_state():
    L = _lib.lib()
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=3, seed=9) as eng:
        a, raw, dec = make_frames("i16", 3, 5001, 6)
        plain = eng.stretch_frames(a).tobytes()
        swapped = eng.stretch_frames(np.ascontiguousarray(a[:, [2, 0, 1]])).tobytes()
        assert plain != swapped
        eng.set_channel_map([2, 0, 1])
        assert eng.stretch_frames(a).tobytes() == swapped
        assert eng.stretch_frames(a).tobytes() == swapped  # it persists
        # an invalid map: RC_EINVAL, and the previous map keeps working
        for bad in ([2, 0], [2, 0, 1, 1], [2, 0, 3], [0, 1, 2 ** 32 - 1]):
            arr = (C.c_uint32 * len(bad))(*bad)
            assert L.rc_engine_set_channel_map(eng._h, arr, len(bad)) == _lib.RC_EINVAL
            with pytest.raises(_lib.RocoderError):
                eng.set_channel_map(bad)
            assert eng.stretch_frames(a).tobytes() == swapped
        # the host form, the bin peaks and the channel peaks read what they read
        host = eng.stretch_host(dec)
        power = eng.frames_power(a, bin_frames=441)
        peaks = eng.frames_channel_peaks(a)
        eng.set_channel_map(None)
        assert np.array_equal(eng.stretch_host(dec).view(np.uint32), host.view(np.uint32))
        assert np.array_equal(host.T.view(np.uint32), np.frombuffer(plain, np.uint32).reshape(-1, 3))
        assert np.array_equal(eng.frames_power(a, bin_frames=441).view(np.uint32), power.view(np.uint32))
        assert np.array_equal(eng.frames_channel_peaks(a).view(np.uint32), peaks.view(np.uint32))
        assert np.array_equal(peaks.view(np.uint32), sm.raw_channel_peaks(raw, "i16", 3).view(np.uint32))
        # clearing restores the unmapped bytes, by None, by an empty list and by an identity map
        assert eng.stretch_frames(a).tobytes() == plain
        eng.set_channel_map([1, 1, 1])
        assert eng.stretch_frames(a).tobytes() == eng.stretch_frames(np.ascontiguousarray(a[:, [1, 1, 1]])).tobytes() != plain
        eng.set_channel_map([])
        assert eng.stretch_frames(a).tobytes() == plain
        eng.set_channel_map([2, 0, 1])
        eng.set_channel_map([0, 1, 2])
        assert eng.stretch_frames(a).tobytes() == plain


# ---- channel peaks -----------------------------------------------------------------------------------------------------------
def same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), (what, [hex(v) for v in g.tolist()][:8], [hex(v) for v in w.tolist()][:8])


N_PEAKS = 50001
PEAK_CHANNELS = (1, 2, 3, 9, 67)
PEAKS = [(fmt, PEAK_CHANNELS[(i + k) % 5], (i + 3 * k + 1) % 4) for k, fmt in enumerate(FORMATS) for i in range(5)]


def test_the_peak_cases_cover_every_axis_with_every_format():
    for fmt in FORMATS:
        mine = [c for c in PEAKS if c[0] == fmt]
        assert {c[1] for c in mine} == set(PEAK_CHANNELS) and {c[2] for c in mine} == {0, 1, 2, 3}


@pytest.mark.parametrize("fmt,channels,phase", PEAKS)
def test_channel_peaks(engines, fmt, channels, phase):
    """seeded random bytes: every sample over the full range of its format (f32: any bits, NaN and inf among them), and the
    same block with its samples scaled down so that no channel saturates"""
    eng = engines(channels)
    rng = np.random.default_rng(200 + channels)
    raw = rng.integers(0, 256, N_PEAKS * channels * au.PCM_BYTES[fmt], dtype=np.uint8)
    same_bits(eng.frames_channel_peaks(at_phase(raw, phase), fmt=fmt), sm.raw_channel_peaks(raw, fmt, channels), "random bytes")
    if fmt == "f32":
        quiet = (rng.standard_normal((N_PEAKS, channels)) * np.logspace(-6, 0, channels)).astype("<f4")
    elif fmt == "u8":
        quiet = (128 + rng.integers(-100, 101, (N_PEAKS, channels)) // (1 + np.arange(channels) % 7)).astype(np.uint8)
    else:
        top = {"i16": 2 ** 15, "i24": 2 ** 23, "i32": 2 ** 31}[fmt]
        q = rng.integers(-top + 1, top, (N_PEAKS, channels)) // (1 + 3 * (np.arange(channels) % 11))
        quiet = q.astype("<i4")
        if fmt == "i16":
            quiet = q.astype("<i2")
        elif fmt == "i24":
            quiet = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
    qraw = np.ascontiguousarray(quiet).reshape(-1).view(np.uint8)
    want = sm.raw_channel_peaks(qraw, fmt, channels)
    same_bits(eng.frames_channel_peaks(at_phase(qraw, phase, pinned=True), fmt=fmt), want, "scaled channels, page-locked")


@pytest.mark.parametrize("fmt", FORMATS)
def test_channel_peaks_edge_lengths(engines, fmt):
    for channels in (2, 9):
        for n in (0, 1):
            raw = np.random.default_rng(n + 5).integers(0, 256, n * channels * au.PCM_BYTES[fmt], dtype=np.uint8)
            got = engines(channels).frames_channel_peaks(at_phase(raw, 1), fmt=fmt)
            same_bits(got, sm.raw_channel_peaks(raw, fmt, channels), f"{fmt} {n} frames x{channels}")
            if n == 0:
                assert got.view(np.uint32).tolist() == [0] * channels


def test_channel_peaks_corner_values(engines):
    """one expectation per channel"""
    n = 5000  # (more than one narrow tile, more than one workgroup's frames of the wide kernel below)
    den = np.array([1], np.uint32).view(np.float32)[0]
    x = np.zeros((n, 8), np.float32)
    x[::2, 0] = -0.0                                  # only +-0.0 -> bits 0
    x[1234, 1] = -den                                 # a lone denormal
    x[:, 2] = 0.5
    x[77, 2] = -np.inf                                # -inf -> +inf
    x[:, 3] = np.linspace(-3, 2, n)
    x[4000, 3] = np.nan                               # NaN beside finite values -> a NaN
    x[n - 1, 4] = -0.25                               # the only non-zero sample is the last frame
    x[0, 5] = 0.125                                   # ... is the first frame
    x[:, 6] = np.linspace(-3, 2, n)                   # the largest magnitude is negative
    x[1500, 7] = np.inf
    x[1501, 7] = np.array([0xFFC00001], np.uint32).view(np.float32)[0]  # a negative NaN with a payload wins over inf
    want = np.array([0, 1, 0x7F800000, 0x7FC00000, 0x3E800000, 0x3E000000, 0x40400000, 0x7FC00001], np.uint32)
    got = engines(8).frames_channel_peaks(x)
    assert got.view(np.uint32).tolist() == want.tolist(), [hex(v) for v in got.view(np.uint32)]
    assert sm.channel_peaks(x).view(np.uint32).tolist() == want.tolist()
    assert split_mono_map(got[:2]) == ([1, 1], True) and split_mono_map(got[[0, 3]]) == ([1, 1], True)
    # the same columns, repeated, through the wide kernel
    wide = np.ascontiguousarray(np.tile(x, (1, 9))[:, :67])
    got = engines(67).frames_channel_peaks(wide)
    assert got.view(np.uint32).tolist() == np.tile(want, 9)[:67].tolist()


def test_channel_peaks_buffers_and_status(engines):
    eng = engines(3)
    L = _lib.lib()
    a = np.random.default_rng(3).integers(-32768, 32768, (1000, 3)).astype("<i2")
    guarded = np.full(6, 7.5, np.float32)
    peak = guarded[1:].ctypes.data_as(F32P)
    src = C.c_void_p(a.ctypes.data)
    assert L.rc_engine_frames_channel_peaks(eng._h, src, 1000, _lib.RC_PCM_I16, peak, 2) == _lib.RC_ECAPACITY
    assert L.rc_engine_frames_channel_peaks(eng._h, src, 1000, _lib.RC_PCM_I16, peak, 0) == _lib.RC_ECAPACITY
    for fmt in (0, 6):
        assert L.rc_engine_frames_channel_peaks(eng._h, src, 1000, fmt, peak, 3) == _lib.RC_EINVAL
    assert L.rc_engine_frames_channel_peaks(eng._h, None, 1000, _lib.RC_PCM_I16, peak, 3) == _lib.RC_EINVAL
    assert L.rc_engine_frames_channel_peaks(eng._h, src, 1000, _lib.RC_PCM_I16, None, 3) == _lib.RC_EINVAL
    assert (guarded == 7.5).all()
    # the exact capacity and a larger one: the words around the channels stay
    for cap in (3, 4):
        guarded[:] = 7.5
        assert L.rc_engine_frames_channel_peaks(eng._h, src, 1000, _lib.RC_PCM_I16, peak, cap) == _lib.RC_OK
        assert guarded[0] == 7.5 and guarded[4] == 7.5 and guarded[5] == 7.5
        same_bits(guarded[1:4].copy(), sm.raw_channel_peaks(a.tobytes(), "i16", 3), "through the C-ABI")
    guarded[:] = 7.5
    assert L.rc_engine_frames_channel_peaks(eng._h, None, 0, _lib.RC_PCM_I16, peak, 3) == _lib.RC_OK
    assert guarded.view(np.uint32)[1:4].tolist() == [0, 0, 0] and guarded[0] == 7.5 and guarded[4] == 7.5


def kernel_times(eng):
    ms = (C.c_float * 256)()
    n = C.c_size_t(0)
    assert _lib.lib().rc_engine_kernel_times(eng._h, ms, 256, C.byref(n)) == _lib.RC_OK
    return n.value


def test_channel_peaks_leave_the_engine_as_it_was():
    a = np.random.default_rng(8).integers(-20000, 20000, (30000, 2)).astype("<i2")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=9) as eng:
        eng.load_device_kernel(compile_device_kernel(open(os.path.join(ROOT, "examples", "kernels", "blur.hip")).read(), "blur.hip"))
        eng.set_device_kernel_params([0.5, 0.25, 0.125, 0.125])
        n_out = eng.output_len(a.shape[0])
        eng.set_output_fade(500, n_out - 700, 700)
        eng.set_channel_map([1, 0])
        count0 = kernel_times(eng)
        before = eng.stretch_frames(a, out_fmt="i16").tobytes()
        count = kernel_times(eng)
        same_bits(eng.frames_channel_peaks(a), sm.raw_channel_peaks(a.tobytes(), "i16", 2), "between two stretch calls")
        assert kernel_times(eng) == count
        after = eng.stretch_frames(a, out_fmt="i16").tobytes()
        assert after == before
        assert kernel_times(eng) == count + (count - count0)  # (what the first stretch call added, once more)
        eng.set_channel_map(None)
        assert eng.stretch_frames(np.ascontiguousarray(a[:, [1, 0]]), out_fmt="i16").tobytes() == before


# ---- end to end ------------------------------------------------------------------------------------------------------------
def mono_take(n=40000, rate=44100):
    """i16 stereo whose left channel is all zero: a mono source on the right input of a stereo device"""
    right = np.rint(0.5 * 32767 * np.sin(2 * np.pi * 440 * np.arange(n) / rate) * np.minimum(1, np.arange(n) / 5000))
    return np.stack([np.zeros(n), right], axis=1).astype("<i2")


def test_end_to_end_split_then_stretch():
    a = mono_take()
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=5) as eng:
        peaks = eng.frames_channel_peaks(a)
        same_bits(peaks, sm.raw_channel_peaks(a.tobytes(), "i16", 2), "the take")
        assert split_mono_map(peaks) == ([1, 1], True) == sm.split_mono_map(peaks)
        copied = a.copy()
        copied[:, 0] = a[:, 1]
        want = eng.stretch_frames(copied, out_fmt="i16").tobytes()
        eng.set_channel_map(split_mono_map(peaks)[0])
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == want


def run_cli(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


MESSAGE = "Detected mono input from non-mono device. Automatically splitting."


def test_cli_split_mono(tmp_path):
    a = mono_take()
    copied = a.copy()
    copied[:, 0] = a[:, 1]
    live = a.copy()
    live[:, 0] = a[::-1, 1]
    paths = {}
    for name, arr in (("take", a), ("copied", copied), ("live", live)):
        paths[name] = str(tmp_path / f"{name}.wav")
        write_wav(paths[name], arr.T / 32767.0, 44100, "i16")
        assert open(paths[name], "rb").read()[44:] == arr.tobytes()
    o1, o2 = str(tmp_path / "o1.wav"), str(tmp_path / "o2.wav")
    base = ["--seed", "5", "-w", "1024", "-f", "2", "--frames-on-gpu", "--output-format", "i16"]
    r1 = run_cli("-i", paths["take"], "-o", o1, "--split-mono", *base)
    r2 = run_cli("-i", paths["copied"], "-o", o2, *base)
    assert open(o1, "rb").read() == open(o2, "rb").read()
    assert r1.stderr.count(MESSAGE) == 1 and MESSAGE not in r2.stderr
    # two live channels: nothing is said and nothing changes
    r3 = run_cli("-i", paths["live"], "-o", o1, "--split-mono", *base)
    run_cli("-i", paths["live"], "-o", o2, *base)
    assert MESSAGE not in r3.stderr and open(o1, "rb").read() == open(o2, "rb").read()
    # the user's map on the split audio: total[c] = split[user[c]] - on this take every row still reads the right channel
    run_cli("-i", paths["take"], "-o", o1, "--split-mono", "--channel-map", "1,0", *base)
    run_cli("-i", paths["copied"], "-o", o2, *base)
    assert open(o1, "rb").read() == open(o2, "rb").read()


def test_cli_channel_map_is_the_host_paths_rotate_channels(tmp_path):
    from oracle import oracle_np as onp

    x = np.stack([onp.synth_input(c, 60000) for c in range(2)])
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    o1, o2 = str(tmp_path / "o1.wav"), str(tmp_path / "o2.wav")
    base = ["-i", wav, "--seed", "5", "-w", "1024", "-f", "4"]
    run_cli(*base, "-o", o1, "--frames-on-gpu", "--channel-map", "1,0")
    run_cli(*base, "-o", o2, "--rotate-channels")
    assert open(o1, "rb").read() == open(o2, "rb").read()
    run_cli(*base, "-o", o2)
    assert open(o1, "rb").read() != open(o2, "rb").read()
    # three channels: rotate_right(1) is map[c] = (c + C - 1) % C
    x3 = np.stack([onp.synth_input(c, 30000) for c in range(3)])
    write_wav(wav, x3, 44100, "i24")
    run_cli(*base, "-o", o1, "--frames-on-gpu", "--channel-map", "2,0,1")
    run_cli(*base, "-o", o2, "--rotate-channels")
    assert open(o1, "rb").read() == open(o2, "rb").read()


def test_cli_split_mono_autocrop_and_clip(tmp_path):
    """--split-mono --autocrop -s .. -d ..: the plain run on the split, cropped, clipped file"""
    rate = 44100
    rng = np.random.default_rng(44)
    n0, n1, n2 = round(0.7 * rate), round(1.5 * rate), round(0.9 * rate)  # whole bins of 4 410
    sine = np.rint(0.5 * 32767 * np.sin(2 * np.pi * 440 * np.arange(n1) / rate))
    right = np.concatenate([rng.integers(-3, 4, n0), sine, rng.integers(-3, 4, n2)])
    a = np.stack([np.zeros(right.size), right], axis=1).astype("<i2")
    split = a[:, [1, 1]]
    start, end = au.autocrop_points(au.bin_peaks(au.decode(split.tobytes(), "i16", 2), 4410), 4410, 30)
    assert (start, end) == au.autocrop_points(au.bin_peaks(au.decode(a.tobytes(), "i16", 2), 4410), 4410, 30)  # a maximum over channels
    s, d = round(0.25 * rate), round(0.5 * rate)
    done = np.ascontiguousarray(split[start:end][s:s + d])
    assert done.shape[0] == d and 0 < start < end < a.shape[0]
    whole, ready = str(tmp_path / "whole.wav"), str(tmp_path / "ready.wav")
    write_wav(whole, a.T / 32767.0, rate, "i16")
    write_wav(ready, done.T / 32767.0, rate, "i16")
    o1, o2 = str(tmp_path / "o1.wav"), str(tmp_path / "o2.wav")
    base = ["--seed", "5", "-w", "1024", "-f", "2", "--frames-on-gpu", "--output-format", "i16"]
    r1 = run_cli("-i", whole, "-o", o1, "--split-mono", "--autocrop", "-s", "0.25", "-d", "0.5", *base)
    run_cli("-i", ready, "-o", o2, *base)
    assert open(o1, "rb").read() == open(o2, "rb").read()
    assert r1.stderr.count(MESSAGE) == 1 and "autocropping audio to start" in r1.stderr
