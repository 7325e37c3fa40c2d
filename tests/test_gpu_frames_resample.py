"""GPU tests of rc_engine_set_output_resample through the C-ABI: the four whole-job host-form entries with a step set. The
yardstick is the launcher itself in ONE launch (the test hook, tests/resampleutil.gpu_resample) over the same engine's
unresampled rows - held to the f64 definition by the gate of tests/test_gpu_frames_resample_kernel.py - so every comparison
of the engine's lag bookkeeping is of bits; everything downstream (quantiser, normaliser, fade, dither) is the numpy
statement of its definition applied to the f32 entry's resampled output."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rocoder_amd  # noqa: E402
from ditherutil import dithered_bytes  # noqa: E402
from fadeutil import NONE, apply_fade  # noqa: E402
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import RocoderError, pinned_empty, resample_len, resample_table  # noqa: E402
from test_frames_pcm_host import count_clipped, pcm_bytes, quantise  # noqa: E402

import resampleutil as R  # noqa: E402

pytestmark = pytest.mark.gpu
SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel


def noise_i16(n, ch, seed, scale=32768):
    return np.random.default_rng(seed).integers(-scale, scale, (n, ch), dtype=np.int64).astype("<i2")


def rows_of(a):
    """the planar float32 rows the frame entries decode int16 frames to: (float)n / 32767, one division"""
    return np.ascontiguousarray((a.astype(np.float32) / np.float32(32767)).T)


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} samples differ, the first at {bad[:8].tolist()}")


def one_launch(ref, num, den):
    """the one-launch resample of the unresampled result ref[frames, channels]: float32 [n_rs, channels]"""
    rows = np.ascontiguousarray(ref.T)
    status, y, guards = R.gpu_resample(rows, resample_table(num, den), num, den)
    assert status == 0 and guards
    return np.ascontiguousarray(y.T)


# ---- the small shape ---------------------------------------------------------------------------------------------
SMALL_RATIOS = [(3, 2), (147, 160)]


@pytest.fixture(scope="module")
def small():
    """N = 1024, f = 2, stereo, 20 000 frames: the engine, its input, the unresampled result and, per ratio, the one-launch
    resample of it - computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3)
    a = noise_i16(20000, 2, 11, scale=12000)
    ref = eng.stretch_frames(a)
    want = {r: one_launch(ref, *r) for r in SMALL_RATIOS}
    for w in (ref, *want.values()):
        w.flags.writeable = False
    yield eng, a, ref, want
    eng.close()


@pytest.mark.parametrize("num,den", SMALL_RATIOS)
def test_f32_frames_and_rows_are_the_one_launch_resample_and_meet_the_gate(small, num, den):
    eng, a, ref, want = small
    w = want[(num, den)]
    n_rs = resample_len(ref.shape[0], num, den)
    assert w.shape == (n_rs, 2) and n_rs == R.resample_len(ref.shape[0], num, den)
    eng.set_output_resample(num, den)
    try:
        assert eng.output_len(20000) == ref.shape[0]  # (stays what it is)
        got = eng.stretch_frames(a)
        same_bits(got, w, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), w.T, "rows")
        y, bound = R.resample_f64(ref.T, resample_table(num, den), num, den)
        assert (np.abs(got.T.astype(np.float64) - y) <= bound).all()
        # capacity: one frame short is RC_ECAPACITY with nothing written
        out = np.full((n_rs - 1, 2), 7.0, np.float32)
        got_len = C.c_size_t(99)
        rc = eng._L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 20000, _lib.RC_PCM_I16, out.ctypes.data_as(C.POINTER(C.c_float)),
                                             n_rs - 1, C.byref(got_len))
        assert rc == _lib.RC_ECAPACITY and (out == 7.0).all() and got_len.value == 99
    finally:
        eng.set_output_resample()


@pytest.mark.parametrize("fmt", ["i16", "u8"])
def test_pcm_bytes_and_clipped_count(small, fmt):
    eng, a, ref, want = small
    w = want[(3, 2)]
    eng.set_output_resample(3, 2)
    try:
        got = eng.stretch_frames(a, out_fmt=fmt)
        assert got.tobytes() == pcm_bytes(quantise(w, fmt), fmt)
        assert eng.last_clipped == count_clipped(w)
    finally:
        eng.set_output_resample()


def normalise(y, target):
    mag = np.abs(np.asarray(y, np.float32))
    peak = np.float32(mag[np.isfinite(mag)].max())
    gain = np.float32(target) / peak
    return (y * gain).astype(np.float32), peak, gain


def test_norm_peak_gain_and_bytes(small):
    eng, a, ref, want = small
    w = want[(147, 160)]
    eng.set_output_resample(147, 160)
    try:
        got = eng.stretch_frames(a, out_fmt="i16", normalize=0.9)
        z, peak, gain = normalise(w, 0.9)
        assert (eng.last_peak.view(np.uint32), eng.last_gain.view(np.uint32)) == (peak.view(np.uint32), gain.view(np.uint32))
        assert got.tobytes() == pcm_bytes(quantise(z, "i16"), "i16")
        assert eng.last_clipped == count_clipped(z)
    finally:
        eng.set_output_resample()


def test_fade_positions_are_resampled_frames(small):
    eng, a, ref, want = small
    w = want[(3, 2)]
    n_rs = w.shape[0]
    assert n_rs < ref.shape[0]
    fade = (1001, n_rs - 1500, 1493)
    eng.set_output_resample(3, 2)
    try:
        eng.set_output_fade(*fade)
        same_bits(eng.stretch_frames(a), apply_fade(w, *fade), "faded f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), apply_fade(w, *fade).T, "faded rows")
        # a fade that fits the unresampled job but not the resampled one
        eng.set_output_fade(0, n_rs - 10, 11)
        with pytest.raises(RocoderError) as ei:
            eng.stretch_frames(a)
        assert ei.value.code == _lib.RC_EINVAL
        eng.set_output_fade(n_rs + 1, None, 0)
        with pytest.raises(RocoderError) as ei:
            eng.stretch_host(rows_of(a))
        assert ei.value.code == _lib.RC_EINVAL
    finally:
        eng.set_output_fade()
        eng.set_output_resample()


def test_dither_counts_resampled_frames(small):
    eng, a, ref, want = small
    w = want[(147, 160)]
    eng.set_output_resample(147, 160)
    try:
        eng.set_output_dither("tpdf-hp", 77)
        got = eng.stretch_frames(a, out_fmt="i16")
        assert np.array_equal(np.frombuffer(got.tobytes(), np.uint8), dithered_bytes(w, "i16", "tpdf-hp", 77))
        assert eng.last_clipped == count_clipped(w)
    finally:
        eng.set_output_dither()
        eng.set_output_resample()


def test_set_then_cleared_is_an_engine_that_never_set_it(small):
    eng, a, ref, want = small
    eng.set_output_resample(160, 147)
    assert eng.stretch_frames(a).shape[0] == resample_len(ref.shape[0], 160, 147)
    eng.set_output_resample(5, 5)
    same_bits(eng.stretch_frames(a), ref, "f32 frames")
    same_bits(eng.stretch_host(rows_of(a)), ref.T, "rows")
    assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(ref, "i16"), "i16")
    # a refused step leaves the state: still cleared
    with pytest.raises(RocoderError):
        eng.set_output_resample(9, 1)
    same_bits(eng.stretch_frames(a), ref, "f32 frames behind a refused setter")
    # and a refused step leaves a set state set
    eng.set_output_resample(3, 2)
    try:
        with pytest.raises(RocoderError):
            eng.set_output_resample(0, 1)
        same_bits(eng.stretch_frames(a), want[(3, 2)], "f32 frames, 3/2 behind a refused setter")
    finally:
        eng.set_output_resample()


def test_with_a_host_frequency_kernel():
    """the whole-job order: the whole job, one resample launch, one pack, one download"""
    a = noise_i16(20000, 2, 12, scale=12000)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 0.5 * x, kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a)
        w = one_launch(ref, 160, 147)
        eng.set_output_resample(160, 147)
        same_bits(eng.stretch_frames(a), w, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), w.T, "rows")
        got = eng.stretch_frames(a, out_fmt="i16", normalize=0.5)
        z, peak, gain = normalise(w, 0.5)
        assert got.tobytes() == pcm_bytes(quantise(z, "i16"), "i16")


def test_device_form_and_streaming_seam_ignore_the_step():
    import torch

    a = noise_i16(5001, 2, 60)
    x = rows_of(a)
    xd = torch.from_numpy(x).cuda()
    outs = []
    for step in (None, (3, 2)):
        with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
            if step:
                eng.set_output_resample(*step)
            dev = eng.stretch_tensor(xd)
            torch.cuda.synchronize()
            for c in range(2):
                eng.push_input(c, x[c])
                eng.close_input(c)
            wins = []
            while not eng.is_done(0):
                for c in range(2):
                    wins.append(np.array(eng.next_window(c)))
            outs.append((dev.cpu().numpy().tobytes(), np.concatenate(wins).tobytes(), eng.stretch_host(x).shape))
    assert outs[0][0] == outs[1][0], "rc_engine_stretch_device"
    assert outs[0][1] == outs[1][1], "rc_engine_next_window"
    assert outs[0][2] != outs[1][2], "(the host form does resample)"


# ---- several chunks: the lag bookkeeping -----------------------------------------------------------------------------
CHUNKED_RATIOS = [(160, 147), (2, 3)]


@pytest.fixture(scope="module")
def chunked():
    """The chunked shape of tests/test_gpu_frames_pcm.py: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks. The one-launch resample of the unresampled result, per ratio, is computed once."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4, scale=8192)
    ref = eng.stretch_frames(a)
    assert ref.shape[0] > 2 * SLOT_FLOATS
    want = {r: one_launch(ref, *r) for r in CHUNKED_RATIOS}
    del ref
    yield eng, a, want
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("num,den", CHUNKED_RATIOS)
def test_chunks_give_the_one_launch_resample(chunked, num, den, kind):
    eng, a, want = chunked
    w = want[(num, den)]
    eng.set_output_resample(num, den)
    try:
        if kind == "pinned":
            src = pinned_empty(a.shape, a.dtype)
            src[:] = a
            out = pinned_empty(w.shape, np.float32)
        else:
            src, out = a, np.empty(w.shape, np.float32)
        got = eng.stretch_frames(src, out=out)
        same_bits(got, w, f"{num}/{den} {kind}")
    finally:
        eng.set_output_resample()
