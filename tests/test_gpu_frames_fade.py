"""GPU tests of rc_engine_set_output_fade / Engine.set_output_fade / --fade-output: the reference's sqrt fade-in and
fade-out applied on the GPU to the result of the four whole-job host-form entries. The yardstick is never the code under
test: it is the same entry on the same engine with the fade cleared, whose f32 output goes through fadeutil.apply_fade -
the definition of include/rocoder_hip.h in numpy float32 - and, where the entry normalises or quantises, through the
definitions of those two steps, restated below from the header. Every comparison is np.array_equal on bytes; peak and
gain are compared as bit patterns, the clipped count as an integer. There is no tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rocoder_amd
from conftest import ROOT
from fadeutil import NONE, apply_fade
from rocoder_amd import _lib
from rocoder_amd.stretcher import pinned_empty
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
KERNELS = os.path.join(ROOT, "examples", "kernels")
GUARD = 0xA5
SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel

# ---- the quantiser and the normaliser of include/rocoder_hip.h, restated ---------------------------------------------
# format -> (S, LO, HI)
PCM = {"u8": (127, -128, 127), "i16": (32767, -32768, 32767), "i24": (8388608, -8388608, 8388607),
       "i32": (2147483647, -2147483648, 2147483647)}


def quantise_bytes(x, fmt):
    """t = x * (float)S in one f32 multiplication, rint (ties to even), NaN -> 0, clamp; little-endian bytes. f32: the bits."""
    x = np.asarray(x, np.float32)
    if fmt == "f32":
        return x.astype("<f4").tobytes()
    s, lo, hi = PCM[fmt]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x * np.float32(s)).astype(np.float32)
        r = np.where(np.isnan(t), 0, np.rint(t))
    q = np.clip(r.astype(np.float64), lo, hi).astype(np.int64).reshape(-1)
    if fmt == "u8":
        return (q + 128).astype(np.uint8).tobytes()
    if fmt == "i16":
        return q.astype("<i2").tobytes()
    if fmt == "i32":
        return q.astype("<i4").tobytes()
    return (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def count_clipped(x):
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(~(np.abs(np.asarray(x, np.float32)) <= 1)))


def normalise(y, target):
    """peak = the largest finite |y| (0 where there is none), gain = target / peak in one f32 division where peak > 0 and
    the quotient is finite, else 1, z = y * gain in one f32 multiplication. (z, peak, gain)"""
    y = np.asarray(y, np.float32)
    mag = np.abs(y)
    with np.errstate(invalid="ignore"):
        finite = mag < np.float32(np.inf)
    peak = np.float32(mag[finite].max()) if finite.any() else np.float32(0)
    gain = np.float32(1)
    if peak > 0:
        with np.errstate(over="ignore"):
            q = np.float32(target) / peak
        if np.isfinite(q):
            gain = np.float32(q)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (y * gain).astype(np.float32)
    return z, peak, gain


# ---- helpers ----------------------------------------------------------------------------------------------------
def noise_i16(n, ch, seed, scale=32768):
    return np.random.default_rng(seed).integers(-scale, scale, (n, ch), dtype=np.int64).astype("<i2")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def same_bytes(got, want, what):
    a, b = np.frombuffer(np.ascontiguousarray(got).tobytes(), np.uint8), np.frombuffer(want, np.uint8)
    assert a.size == b.size, (what, a.size, b.size)
    if not np.array_equal(a, b):
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {bad.size} of {a.size} bytes differ, the first at {bad[:8].tolist()}")


def into_guarded(eng, arg, fmt, want, offset, pinned=False, **kw):
    """The call with its target `offset` bytes off a 16-byte boundary inside a buffer of guard bytes: the result is right
    and no byte in front of or behind it was written."""
    big = pinned_empty(len(want) + 64, np.uint8) if pinned else np.empty(len(want) + 64, np.uint8)
    big[:] = GUARD
    lo = 16 + offset
    got = eng.stretch_frames(arg, out=big[lo:lo + len(want)], out_fmt=fmt, **kw)
    assert np.shares_memory(got, big)
    same_bytes(got, want, f"{fmt} at offset {offset}")
    assert (big[:lo] == GUARD).all() and (big[lo + len(want):] == GUARD).all(), "guard bytes were written"


def rows_of(a):
    """the planar float32 rows the frame entries decode int16 frames to: (float)n / 32767, one division"""
    return np.ascontiguousarray((a.astype(np.float32) / np.float32(32767)).T)


# ---- the small shape ---------------------------------------------------------------------------------------------
def small_fades(T):
    return [(1, NONE, 0), (3, NONE, 0), (1001, NONE, 0), (T, NONE, 0), (0, 5, 0), (0, 7, T - 7), (0, T, 0),
            (1001, T - 1502, 1499), (2000, 1000, 3001)]


@pytest.fixture(scope="module", params=[2, 3])
def small(request):
    """N = 256, f = 2, 5001 int16 frames: the engine, its input and the two yardsticks - frames and planar rows with the
    fade cleared - computed once and never written to."""
    ch = request.param
    eng = rocoder_amd.Engine(window_len=256, factor=2.0, channels=ch, seed=3)
    a = noise_i16(5001, ch, 30 + ch)
    x = rows_of(a)
    ref = eng.stretch_frames(a)
    ref_rows = eng.stretch_host(x).copy()
    assert ref.shape == (eng.output_len(5001), ch) and np.array_equal(ref_rows.T, ref)
    ref.flags.writeable = False
    ref_rows.flags.writeable = False
    yield eng, a, x, ref, ref_rows
    eng.close()


@pytest.mark.parametrize("which", range(9))
def test_every_entry_gives_the_definition(small, which):
    """f32 frames, i16, i24 one byte off a dword, and the planar rows of rc_engine_stretch_host, for fades whose ragged
    ends, p = 0, p = d - 1, hard cut, no-op and overlap are where the kernel can go wrong."""
    eng, a, x, ref, ref_rows = small
    T = ref.shape[0]
    fade = small_fades(T)[which]
    z = apply_fade(ref, *fade)
    if fade == (0, T, 0):
        assert z.tobytes() == ref.tobytes()
    elif fade[1] != NONE and fade[1] + fade[2] < T:
        assert not z[fade[1] + fade[2]:].view(np.uint32).any() and ref[fade[1] + fade[2]:].any()
    try:
        eng.set_output_fade(*(fade[0], None if fade[1] == NONE else fade[1], fade[2]))
        same_bytes(eng.stretch_frames(a), z.tobytes(), f"f32 frames {fade}")
        got = eng.stretch_frames(a, out_fmt="i16")
        same_bytes(got, quantise_bytes(z, "i16"), f"i16 {fade}")
        assert eng.last_clipped == count_clipped(z)
        into_guarded(eng, a, "i24", quantise_bytes(z, "i24"), 1)
        same_bytes(eng.stretch_host(x), apply_fade(ref_rows, *fade, axis=1).tobytes(), f"planar rows {fade}")
    finally:
        eng.set_output_fade()


# ---- several chunks -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    """The shape of the other frame tests' `chunked`: N = 1024, f = 8, three channels, 1 200 000 frames, several pipeline
    chunks. A fade-in of 5 000 001 frames crosses the first chunk edge; the fade-out starts inside the second chunk and
    ends 7 frames before the end. The yardstick's bytes are computed once."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4, scale=8192)
    ref = eng.stretch_frames(a)
    T = ref.shape[0]
    assert T > SLOT_FLOATS, "more than one chunk"
    assert T > 2 * SLOT_FLOATS
    fade = (5_000_001, SLOT_FLOATS + 1_000_003, T - 7 - (SLOT_FLOATS + 1_000_003))
    assert SLOT_FLOATS < fade[0] < fade[1] < 2 * SLOT_FLOATS and fade[1] + fade[2] == T - 7
    want = quantise_bytes(apply_fade(ref, *fade), "i24")
    assert ref[T - 7:].any()
    del ref
    yield eng, a, fade, want
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_fades_across_chunk_edges(chunked, kind):
    eng, a, fade, want = chunked
    src = a
    if kind == "pinned":
        src = pinned_empty(a.shape, a.dtype)
        src[:] = a
    try:
        eng.set_output_fade(*fade)
        into_guarded(eng, src, "i24", want, 1, pinned=kind == "pinned")
    finally:
        eng.set_output_fade()


def test_frame_counts_above_2_to_24():
    """Mono, N = 1024, f = 8, 2 200 000 frames: a fade-out longer than 2^24 frames, whose p and d no longer convert to
    float32 exactly."""
    a = noise_i16(2_200_000, 1, 9, scale=8192)
    with rocoder_amd.Engine(window_len=1024, factor=8.0, channels=1, seed=2) as eng:
        ref = eng.stretch_frames(a)
        T = ref.shape[0]
        fade = (0, 5, 16_777_217 + 3)
        assert T > 2 ** 24 and fade[2] > 2 ** 24 and fade[1] + fade[2] < T
        want = apply_fade(ref, *fade).tobytes()
        del ref
        eng.set_output_fade(*fade)
        same_bytes(eng.stretch_frames(a), want, "f32 frames")


# ---- normalised ------------------------------------------------------------------------------------------------------
def test_the_peak_is_taken_behind_the_fade():
    """Quarter-scale noise with a full-scale burst that lands in the first 2000 output frames, and a fade-in long enough
    to push the burst below the rest: peak, gain and the clipped count are those of the faded result."""
    a = noise_i16(100_001, 2, 50, scale=8192)
    a[:200] = noise_i16(200, 2, 51)
    in_len = 40_000
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
        ref = eng.stretch_frames(a)
        z = apply_fade(ref, in_len)
        at_ref, at_z = int(np.argmax(np.abs(ref).max(axis=1))), int(np.argmax(np.abs(z).max(axis=1)))
        print(f"unfaded peak {np.abs(ref).max():.4f} at frame {at_ref}, faded peak {np.abs(z).max():.4f} at frame {at_z}")
        assert at_ref < 2000 and at_ref < in_len <= at_z, (at_ref, at_z)
        for fmt, target in (("i16", 0.9), ("i16", 1.5), ("f32", 1.0)):
            n, peak, gain = normalise(z, target)
            assert bits(peak) == bits(np.abs(z).max()) and bits(peak) != bits(np.abs(ref).max())
            eng.set_output_fade(in_len)
            got = eng.stretch_frames(a, out_fmt=fmt, normalize=target)
            same_bytes(got, quantise_bytes(n, fmt), f"{fmt} at {target}")
            assert (bits(eng.last_peak), bits(eng.last_gain), eng.last_clipped) == (bits(peak), bits(gain), count_clipped(n))
            if target > 1:
                assert 0 < eng.last_clipped != count_clipped(normalise(ref, target)[0])
            eng.set_output_fade()


# ---- non-finite ------------------------------------------------------------------------------------------------------
def test_nan_stays_nan_inside_the_fade_and_the_tail_is_plus_zero():
    a = np.random.default_rng(8).uniform(-1, 1, (5001, 2)).astype(np.float32)
    a[3500, 0] = np.nan
    a[4600, 1] = np.nan
    fade = (0, 6000, 2000)
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
        ref = eng.stretch_frames(a)
        nan = np.isnan(ref)
        assert nan[6000:8000].any() and nan[8000:].any() and np.isfinite(ref).any()
        z = apply_fade(ref, *fade)
        eng.set_output_fade(*fade)
        got = eng.stretch_frames(a)
        assert np.array_equal(np.isnan(got), np.isnan(z)) and np.isnan(got[6000:8000]).any()
        assert np.array_equal(got.view(np.uint32)[~np.isnan(z)], z.view(np.uint32)[~np.isnan(z)])
        assert not got[8000:].view(np.uint32).any(), "+0.0 bits behind the fade-out, NaN and negative values included"
        n, peak, gain = normalise(z, 1.0)  # the peak skips NaN as before; NaN is written as 0 and counted
        got = eng.stretch_frames(a, out_fmt="i16", normalize=1.0)
        same_bytes(got, quantise_bytes(n, "i16"), "i16 normalised")
        assert (bits(eng.last_peak), bits(eng.last_gain), eng.last_clipped) == (bits(peak), bits(gain), count_clipped(n))
        assert np.isfinite(eng.last_peak) and eng.last_clipped >= np.count_nonzero(np.isnan(z))


# ---- kernel paths ----------------------------------------------------------------------------------------------------
def check_kernel_path(eng):
    a = noise_i16(30001, 2, 13)
    x = rows_of(a)
    ref = eng.stretch_frames(a)
    ref_rows = eng.stretch_host(x).copy()
    T = ref.shape[0]
    fade = (1001, T - 1502, 1499)
    z = apply_fade(ref, *fade)
    eng.set_output_fade(*fade)
    same_bytes(eng.stretch_frames(a, out_fmt="i16"), quantise_bytes(z, "i16"), "i16")
    assert eng.last_clipped == count_clipped(z)
    same_bytes(eng.stretch_frames(a), z.tobytes(), "f32 frames")
    same_bytes(eng.stretch_host(x), apply_fade(ref_rows, *fade, axis=1).tobytes(), "planar rows")
    n, peak, gain = normalise(z, 0.9)
    same_bytes(eng.stretch_frames(a, out_fmt="i24", normalize=0.9), quantise_bytes(n, "i24"), "i24 normalised")
    assert (bits(eng.last_peak), bits(eng.last_gain)) == (bits(peak), bits(gain))


def test_with_a_user_device_kernel():
    from rocoder_amd.stretcher import compile_device_kernel

    code = compile_device_kernel(open(os.path.join(KERNELS, "blur.hip")).read(), "blur.hip")
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        eng.load_device_kernel(code)
        check_kernel_path(eng)


def test_with_a_curated_device_kernel():
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, device_kernel=("gain", 0.5)) as eng:
        check_kernel_path(eng)


def test_with_a_host_frequency_kernel():
    """the simple order: the whole job, the fade, one pack, one download"""
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x,
                            kernel_time_ms=1) as eng:
        check_kernel_path(eng)


# ---- scope -----------------------------------------------------------------------------------------------------------
def test_device_form_and_streaming_seam_ignore_the_fade():
    import torch

    a = noise_i16(5001, 2, 60)
    x = rows_of(a)
    xd = torch.from_numpy(x).cuda()

    def seam(fade):
        with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
            if fade:
                eng.set_output_fade(*fade)
            for c in range(2):
                eng.push_input(c, x[c])
                eng.close_input(c)
            wins = []
            while not eng.is_done(0):  # windows outer, channels inner
                for c in range(2):
                    wins.append(np.array(eng.next_window(c)))
            assert eng.is_done(1) and len(wins) > 2
            return np.concatenate(wins).tobytes()

    outs = []
    for fade in (None, (1001, 4000, 999)):
        with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
            if fade:
                eng.set_output_fade(*fade)
            dev = eng.stretch_tensor(xd)
            torch.cuda.synchronize()
            outs.append((dev.cpu().numpy().tobytes(), seam(fade), eng.stretch_host(x).tobytes()))
    assert outs[0][0] == outs[1][0], "rc_engine_stretch_device"
    assert outs[0][1] == outs[1][1], "rc_engine_next_window"
    assert outs[0][2] != outs[1][2], "(the host form does fade)"


def test_clearing_gives_every_entry_its_old_bytes(small):
    eng, a, x, ref, ref_rows = small
    eng.set_output_fade(1001, 4000, 999)
    assert eng.stretch_frames(a).tobytes() != ref.tobytes()
    eng.set_output_fade()
    same_bytes(eng.stretch_host(x), ref_rows.tobytes(), "rows")
    same_bytes(eng.stretch_frames(a), ref.tobytes(), "f32 frames")
    same_bytes(eng.stretch_frames(a, out_fmt="i16"), quantise_bytes(ref, "i16"), "i16")
    n, peak, gain = normalise(ref, 0.9)
    same_bytes(eng.stretch_frames(a, out_fmt="i16", normalize=0.9), quantise_bytes(n, "i16"), "i16 normalised")
    assert (bits(eng.last_peak), bits(eng.last_gain)) == (bits(peak), bits(gain))


# ---- status codes ----------------------------------------------------------------------------------------------------
def test_a_fade_that_does_not_fit_is_an_error_that_writes_nothing():
    L = _lib.lib()
    a = noise_i16(5001, 2, 61)
    x = rows_of(a)
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
        T = eng.output_len(5001)
        assert L.rc_engine_set_output_fade(eng._h, 0, NONE - 1, 2) == _lib.RC_EINVAL  # wraps
        assert L.rc_engine_set_output_fade(eng._h, 0, NONE, 1) == _lib.RC_EINVAL
        for fade in ((T + 1, NONE, 0), (0, T - 1, 2)):
            assert L.rc_engine_set_output_fade(eng._h, *fade) == _lib.RC_OK
            big = np.full(T * 2 * 4 + 64, GUARD, np.uint8)
            dst = big[16:].ctypes.data
            n, clipped, peak, gain = C.c_size_t(7), C.c_uint64(9), C.c_float(3), C.c_float(4)
            assert L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 5001, _lib.RC_PCM_I16, C.cast(dst, C.POINTER(C.c_float)), T,
                                              C.byref(n)) == _lib.RC_EINVAL
            assert L.rc_engine_stretch_frames_pcm(eng._h, a.ctypes.data, 5001, _lib.RC_PCM_I16, dst, T, _lib.RC_PCM_I16, C.byref(n),
                                                  C.byref(clipped)) == _lib.RC_EINVAL
            assert L.rc_engine_stretch_frames_norm(eng._h, a.ctypes.data, 5001, _lib.RC_PCM_I16, dst, T, _lib.RC_PCM_I16, 0.9,
                                                   C.byref(n), C.byref(peak), C.byref(gain), C.byref(clipped)) == _lib.RC_EINVAL
            rows = (C.POINTER(C.c_float) * 2)(*(C.cast(x[c].ctypes.data, C.POINTER(C.c_float)) for c in range(2)))
            outs = (C.POINTER(C.c_float) * 2)(*(C.cast(dst + c * T * 4, C.POINTER(C.c_float)) for c in range(2)))
            assert L.rc_engine_stretch_host(eng._h, rows, 5001, outs, T, C.byref(n)) == _lib.RC_EINVAL
            assert (n.value, clipped.value, peak.value, gain.value) == (7, 9, 3.0, 4.0)
            assert (big == GUARD).all(), "an entry that failed wrote to its output"
            with pytest.raises(_lib.RocoderError) as ei:
                eng.stretch_frames(a)
            assert ei.value.code == _lib.RC_EINVAL
        eng.set_output_fade(T, T, 0)  # the largest fades that fit
        same_bytes(eng.stretch_frames(a), apply_fade(_cleared(eng, a, (T, T, 0)), T, T, 0).tobytes(), "f32 frames")


def _cleared(eng, a, fade):
    eng.set_output_fade()
    ref = eng.stretch_frames(a)
    eng.set_output_fade(*fade)
    return ref


# ---- the CLI -----------------------------------------------------------------------------------------------------------
def header_body(data):
    """the bytes of the data chunk of a WAV file"""
    at = data.index(b"data")
    size = int.from_bytes(data[at + 4:at + 8], "little")
    return data[at + 8:at + 8 + size]


def test_cli_fade_output(tmp_path):
    """--frames-on-gpu --fade-output -x 0.01 --output-format i16 writes the bytes of the Python entry with the frame
    counts the CLI states: Fi = Fo = (size_t)((float)D * (float)rate), out_start = (size_t)((float)L * factor) - Fo.
    (N = 1024 at f = 1: one of the shapes whose output is at least L * factor frames long, so that the fade-out fits.)"""
    x = np.random.default_rng(17).uniform(-1, 1, (2, 5000))
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    body = np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]
    F = int(np.float32(0.01) * np.float32(44100))
    E = int(np.float32(5000) * np.float32(1.0))
    assert (F, E) == (441, 5000)
    with rocoder_amd.Engine(window_len=1024, factor=1.0, channels=2, seed=5) as eng:
        ref = eng.stretch_frames(body, fmt="i16")
        assert E <= ref.shape[0]
        plain = quantise_bytes(ref, "i16")
        want = quantise_bytes(apply_fade(ref, F, E - F, F), "i16")
        eng.set_output_fade(F, E - F, F)
        same_bytes(eng.stretch_frames(body, fmt="i16", out_fmt="i16"), want, "the Python entry")
    assert want != plain
    out = str(tmp_path / "o.wav")
    base = [CLI, "-i", wav, "--seed", "5", "-w", "1024", "-f", "1", "-o", out, "--output-format", "i16"]
    r = subprocess.run(base + ["--frames-on-gpu", "--fade-output", "-x", "0.01"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert header_body(open(out, "rb").read()) == want
    assert f"fade in {F} frames, out from {E - F} over {F}" in r.stderr.splitlines(), r.stderr
    os.remove(out)
    r = subprocess.run(base + ["--fade-output", "-x", "0.01"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--frames-on-gpu" in r.stderr and not os.path.exists(out)
    # a fade longer than the output: the reference's warnings, and the unfaded file
    r = subprocess.run(base + ["--frames-on-gpu", "--fade-output", "-x", "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Fade in parameters out of bounds, ignoring." in r.stderr and "Fade out parameters out of bounds, ignoring." in r.stderr
    assert not re.search(r"^fade ", r.stderr, re.M)
    assert header_body(open(out, "rb").read()) == plain
    # with --normalize: the peak is the faded one
    r = subprocess.run(base + ["--frames-on-gpu", "--fade-output", "-x", "0.01", "--normalize", "0.9"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    n, peak, gain = normalise(apply_fade(ref, F, E - F, F), 0.9)
    assert header_body(open(out, "rb").read()) == quantise_bytes(n, "i16")
    m = re.search(r"^peak (\S+), gain (\S+)$", r.stderr, re.M)
    assert m and (bits(float(m.group(1))), bits(float(m.group(2)))) == (bits(peak), bits(gain)), r.stderr
