"""GPU tests of rc_engine_set_output_limiter through the C-ABI: the four whole-job host-form entries with a limiter set. The
yardstick is the launcher itself in ONE launch (the test hook, tests/limiterutil.gpu_limit) over the same engine's
unlimited rows - held to the numpy definition bit for bit by tests/test_gpu_frames_limit_kernel.py - so the engine's lag
bookkeeping is compared in bits; everything downstream (quantiser, normaliser, dither) and upstream (fade, resampler) is
the numpy statement of its definition, or its own one-launch yardstick, applied around it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rocoder_amd  # noqa: E402
from ditherutil import dithered_bytes  # noqa: E402
from fadeutil import apply_fade  # noqa: E402
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import RocoderError, pinned_empty, resample_table  # noqa: E402
from test_frames_pcm_host import count_clipped, pcm_bytes, quantise  # noqa: E402

import limiterutil as U  # noqa: E402
import resampleutil as R  # noqa: E402

pytestmark = pytest.mark.gpu
SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel
CEILING = np.float32(0.9)


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


def one_launch(ref, drive, ceiling, L):
    """the one-launch limit of the unlimited result ref[frames, channels]: (float32 [frames, channels], the stats words)"""
    status, y, guards, stats = U.gpu_limit(np.ascontiguousarray(ref.T), drive, ceiling, L)
    assert status == 0 and guards
    return np.ascontiguousarray(y.T), stats


def light_drive(ref):
    """only the top few samples are over"""
    P = np.abs(ref).max()
    return np.float32(CEILING / (np.float32(0.9) * P))


def heavy_drive(ref):
    return np.float32(np.float32(3) * CEILING / np.abs(ref).max())


def stats_bits(eng):
    g, f = eng.last_limiter_stats
    return int(np.float32(g).view(np.uint32)), f


# ---- the small shape ---------------------------------------------------------------------------------------------
L_SMALL = 64


@pytest.fixture(scope="module")
def small():
    """N = 1024, f = 2, stereo, 20 000 frames: the engine, its input, the unlimited result, the drive and the one-launch
    limit of the result - computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3)
    a = noise_i16(20000, 2, 11, scale=12000)
    ref = eng.stretch_frames(a)
    drive = light_drive(ref)
    want, stats = one_launch(ref, drive, CEILING, L_SMALL)
    for w in (ref, want):
        w.flags.writeable = False
    yield eng, a, ref, drive, want, stats
    eng.close()


def test_f32_frames_rows_and_stats(small):
    eng, a, ref, drive, want, stats = small
    n = ref.shape[0]
    y, g, S = U.limit(ref.T, drive, CEILING, L_SMALL)
    assert 0 < U.stats_of(g, S, L_SMALL)[1] < n // 2  # both the pass-through and the limited branch
    same_bits(want.T, y, "the yardstick against numpy")
    assert stats == U.stats_of(g, S, L_SMALL)
    assert eng.last_limiter_stats is None
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        assert eng.output_len(20000) == n
        same_bits(eng.stretch_frames(a), want, "f32 frames")
        assert stats_bits(eng) == stats
        eng.last_limiter_stats = None
        same_bits(eng.stretch_host(rows_of(a)), want.T, "rows")
        assert stats_bits(eng) == stats
        # capacity: one frame short is RC_ECAPACITY with nothing written
        out = np.full((n - 1, 2), 7.0, np.float32)
        got_len = C.c_size_t(99)
        rc = eng._L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 20000, _lib.RC_PCM_I16, out.ctypes.data_as(C.POINTER(C.c_float)),
                                             n - 1, C.byref(got_len))
        assert rc == _lib.RC_ECAPACITY and (out == 7.0).all() and got_len.value == 99
        pcm = np.full(10, 0x5A, np.uint8)
        clipped = C.c_uint64(5)
        rc = eng._L.rc_engine_stretch_frames_pcm(eng._h, a.ctypes.data, 20000, _lib.RC_PCM_I16, pcm.ctypes.data, 2, _lib.RC_PCM_I16,
                                                 C.byref(got_len), C.byref(clipped))
        assert rc == _lib.RC_ECAPACITY and (pcm == 0x5A).all() and got_len.value == 99 and clipped.value == 5
        rc = eng._L.rc_engine_stretch_frames_pcm(eng._h, a.ctypes.data, 20000, 9, pcm.ctypes.data, 2, _lib.RC_PCM_I16,
                                                 C.byref(got_len), C.byref(clipped))
        assert rc == _lib.RC_EINVAL and (pcm == 0x5A).all()
        assert stats_bits(eng) == stats  # (a call that failed leaves the last job's stats)
    finally:
        eng.set_output_limiter()


@pytest.mark.parametrize("fmt", ["i16", "u8"])
def test_pcm_bytes_and_no_clipped_sample(small, fmt):
    eng, a, ref, drive, want, stats = small
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        got = eng.stretch_frames(a, out_fmt=fmt)
        assert got.tobytes() == pcm_bytes(quantise(want, fmt), fmt)
        assert eng.last_clipped == 0 == count_clipped(want)
        assert stats_bits(eng) == stats
    finally:
        eng.set_output_limiter()
    # the same drive without the limiter's ceiling below full scale does clip: the limiter is what keeps the count at 0
    loud = np.float32(1.2) / np.abs(ref).max()
    w2, _s = one_launch(ref, loud, 1.0, L_SMALL)
    assert count_clipped((ref * loud).astype(np.float32)) > 0 and count_clipped(w2) == 0


def normalise(y, target):
    mag = np.abs(np.asarray(y, np.float32))
    peak = np.float32(mag[np.isfinite(mag)].max())
    gain = np.float32(target) / peak
    return (y * gain).astype(np.float32), peak, gain


def test_norm_measures_and_scales_the_limited_rows(small):
    eng, a, ref, drive, want, stats = small
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        got = eng.stretch_frames(a, out_fmt="i16", normalize=0.9)
        z, peak, gain = normalise(want, 0.9)
        assert peak == CEILING  # the limited peak, not the unlimited one
        assert (eng.last_peak.view(np.uint32), eng.last_gain.view(np.uint32)) == (peak.view(np.uint32), gain.view(np.uint32))
        assert got.tobytes() == pcm_bytes(quantise(z, "i16"), "i16")
        assert eng.last_clipped == count_clipped(z)
        assert stats_bits(eng) == stats
    finally:
        eng.set_output_limiter()


def test_the_fade_runs_in_front_of_the_limiter(small):
    eng, a, ref, drive, want, stats = small
    n = ref.shape[0]
    fade = (1001, n - 1500, 1493)
    faded = apply_fade(ref, *fade)
    w, s = one_launch(faded, drive, CEILING, L_SMALL)
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        eng.set_output_fade(*fade)
        same_bits(eng.stretch_frames(a), w, "faded and limited f32 frames")
        assert stats_bits(eng) == s
        same_bits(eng.stretch_host(rows_of(a)), w.T, "faded and limited rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")
    finally:
        eng.set_output_fade()
        eng.set_output_limiter()


def test_both_lags_compose_behind_a_resample_step(small):
    eng, a, ref, drive, want, stats = small
    num, den = 3, 2
    status, rs, guards = R.gpu_resample(np.ascontiguousarray(ref.T), resample_table(num, den), num, den)
    assert status == 0 and guards
    w, s = one_launch(np.ascontiguousarray(rs.T), drive, CEILING, L_SMALL)
    eng.set_output_resample(num, den)
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        same_bits(eng.stretch_frames(a), w, "resampled and limited f32 frames")
        assert stats_bits(eng) == s
        same_bits(eng.stretch_host(rows_of(a)), w.T, "resampled and limited rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")
        assert eng.last_clipped == 0
    finally:
        eng.set_output_limiter()
        eng.set_output_resample()


def test_dither_is_added_to_the_limited_rows(small):
    eng, a, ref, drive, want, stats = small
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        eng.set_output_dither("tpdf", 77)
        got = eng.stretch_frames(a, out_fmt="i16")
        assert np.array_equal(np.frombuffer(got.tobytes(), np.uint8), dithered_bytes(want, "i16", "tpdf", 77))
        assert eng.last_clipped == 0
    finally:
        eng.set_output_dither()
        eng.set_output_limiter()


def test_the_setters_refusals_keep_the_previous_state_and_cleared_is_never_set(small):
    eng, a, ref, drive, want, stats = small
    bad = [(np.nan, 0.5, 1), (0.0, 0.5, 1), (-1.0, 0.5, 1), (np.inf, 0.5, 1), (1.0, np.nan, 1), (1.0, -0.5, 1), (1.0, np.inf, 1),
           (1.0, 0.5, _lib.RC_LIMITER_MAX_LOOKAHEAD + 1)]
    for args in bad:  # refused on a cleared engine: still cleared
        with pytest.raises(RocoderError) as ei:
            eng.set_output_limiter(*args)
        assert ei.value.code == _lib.RC_EINVAL
    same_bits(eng.stretch_frames(a), ref, "f32 frames behind refused setters")
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        for args in bad:  # refused on a set engine: still set as it was
            with pytest.raises(RocoderError):
                eng.set_output_limiter(*args)
        same_bits(eng.stretch_frames(a), want, "limited f32 frames behind refused setters")
        # ceiling 0 clears whatever the other arguments are
        eng.set_output_limiter(np.nan, 0.0, 99999)
        same_bits(eng.stretch_frames(a), ref, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), ref.T, "rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(ref, "i16"), "i16")
        got = eng.stretch_frames(a, out_fmt="i16", normalize=0.9)
        assert got.tobytes() == pcm_bytes(quantise(normalise(ref, 0.9)[0], "i16"), "i16")
        with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as fresh:
            assert fresh.stretch_frames(a, out_fmt="i16").tobytes() == eng.stretch_frames(a, out_fmt="i16").tobytes()
            g, f = C.c_float(0), C.c_uint64(9)
            assert fresh._L.rc_engine_last_limiter_stats(fresh._h, C.byref(g), C.byref(f)) == 0 and (g.value, f.value) == (1.0, 0)
    finally:
        eng.set_output_limiter()


def test_lookahead_zero_and_the_largest(small):
    eng, a, ref, drive, want, stats = small
    for L in (0, _lib.RC_LIMITER_MAX_LOOKAHEAD):
        w, s = one_launch(ref, heavy_drive(ref), CEILING, L)
        eng.set_output_limiter(heavy_drive(ref), CEILING, L)
        try:
            same_bits(eng.stretch_frames(a), w, f"f32 frames, L = {L}")
            assert stats_bits(eng) == s
        finally:
            eng.set_output_limiter()


def test_a_job_of_no_input_frames(small):
    """(the engine's shortest job: whatever it gives for no input, limited; nothing in it is over)"""
    eng, a, ref, drive, want, stats = small
    ref0 = eng.stretch_frames(a[:0])
    eng.set_output_limiter(drive, CEILING, L_SMALL)
    try:
        got = eng.stretch_frames(a[:0])
        assert got.shape == ref0.shape
        if ref0.shape[0]:
            w, s = one_launch(ref0, drive, CEILING, L_SMALL)
            same_bits(got, w, "f32 frames")
            assert stats_bits(eng) == s
        else:
            assert eng.last_limiter_stats == (np.float32(1.0), 0)
    finally:
        eng.set_output_limiter()


def test_with_a_host_frequency_kernel():
    """the whole-job order: the whole job, one limit launch, one pack, one download"""
    a = noise_i16(20000, 2, 12, scale=12000)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 0.5 * x, kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a)
        drive = light_drive(ref)
        w, s = one_launch(ref, drive, CEILING, 200)
        eng.set_output_limiter(drive, CEILING, 200)
        same_bits(eng.stretch_frames(a), w, "f32 frames")
        assert stats_bits(eng) == s
        same_bits(eng.stretch_host(rows_of(a)), w.T, "rows")
        got = eng.stretch_frames(a, out_fmt="i16", normalize=0.5)
        z, peak, gain = normalise(w, 0.5)
        assert got.tobytes() == pcm_bytes(quantise(z, "i16"), "i16")


def test_device_form_and_streaming_seam_ignore_the_limiter():
    import torch

    a = noise_i16(5001, 2, 60)
    x = rows_of(a)
    xd = torch.from_numpy(x).cuda()
    outs = []
    for lim in (None, (2.0, 0.25, 16)):
        with rocoder_amd.Engine(window_len=256, factor=2.0, channels=2, seed=3) as eng:
            if lim:
                eng.set_output_limiter(*lim)
            dev = eng.stretch_tensor(xd)
            torch.cuda.synchronize()
            for c in range(2):
                eng.push_input(c, x[c])
                eng.close_input(c)
            wins = []
            while not eng.is_done(0):
                for c in range(2):
                    wins.append(np.array(eng.next_window(c)))
            outs.append((dev.cpu().numpy().tobytes(), np.concatenate(wins).tobytes(), float(np.abs(eng.stretch_host(x)).max())))
    assert outs[0][0] == outs[1][0], "rc_engine_stretch_device"
    assert outs[0][1] == outs[1][1], "rc_engine_next_window"
    assert outs[0][2] > 0.25 and outs[1][2] <= 0.25, "(the host form does limit)"


# ---- several chunks: the lag bookkeeping -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    """The chunked shape of tests/test_gpu_frames_pcm.py: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks; L = 2048 and a heavy drive, so that the chunk seams lie inside ramps. The one-launch limit of the
    unlimited result is computed once."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4, scale=8192)
    ref = eng.stretch_frames(a)
    assert ref.shape[0] > 2 * SLOT_FLOATS
    drive = heavy_drive(ref)
    want, stats = one_launch(ref, drive, CEILING, 2048)
    assert stats[1] > ref.shape[0] // 2
    del ref
    yield eng, a, drive, want, stats
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_chunks_give_the_one_launch_limit(chunked, kind):
    eng, a, drive, want, stats = chunked
    eng.set_output_limiter(drive, CEILING, 2048)
    try:
        if kind == "pinned":
            src = pinned_empty(a.shape, a.dtype)
            src[:] = a
            out = pinned_empty(want.shape, np.float32)
        else:
            src, out = a, np.empty(want.shape, np.float32)
        got = eng.stretch_frames(src, out=out)
        same_bits(got, want, kind)
        assert stats_bits(eng) == stats
    finally:
        eng.set_output_limiter()
