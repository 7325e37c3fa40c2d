"""GPU tests of rc_engine_set_output_warp through the C-ABI: the whole-job host-form entries with a warp set. The yardstick
is the launcher itself in ONE launch (the test hook, tests/warputil.gpu_warp) over the same engine's unwarped rows - held to
the f64 definition by the gate of tests/test_gpu_frames_warp_kernel.py - so every comparison of the engine's lag
bookkeeping is of bits; everything downstream (fade, limiter, dither, quantiser) is the statement of its own definition
applied to the one-launch warp, as the tests of those stages apply it."""
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
from rocoder_amd.stretcher import RocoderError, pinned_empty, resample_len, time_map_curve, warp_curve, warp_table  # noqa: E402
from test_frames_pcm_host import count_clipped, pcm_bytes, quantise  # noqa: E402

import limiterutil as U  # noqa: E402
import warputil as Wp  # noqa: E402

pytestmark = pytest.mark.gpu
SLOT_FLOATS = (16 << 20) // 4  # the pipeline cuts the job into chunks of about this many output samples per channel
CEILING = np.float32(0.9)
_tables = {}


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


def one_launch(ref, anchors, n_out):
    """the one-launch warp of the unwarped result ref[frames, channels]: float32 [n_out, channels]"""
    tiers = {Wp.tier_of(int(d)) for d in np.unique(np.diff(anchors))}
    for t in tiers:
        if t not in _tables:
            _tables[t] = warp_table(t)
    status, y, guards = Wp.gpu_warp(np.ascontiguousarray(ref.T), {t: _tables[t] for t in tiers}, anchors, n_out)
    assert status == 0 and guards
    return np.ascontiguousarray(y.T)


def limited(w, drive, L):
    status, y, guards, _stats = U.gpu_limit(np.ascontiguousarray(w.T), drive, CEILING, L)
    assert status == 0 and guards
    return np.ascontiguousarray(y.T)


def glide_of(eng, n, in_len, kw, hop_pos=None, lo=0.5, hi=2.0):
    """a glide from `lo` to `hi` over the input, down again to 0.8: tiers 0 ... 4, dropping between blocks on the way down"""
    n_hops = n // eng.params.window_out_len * eng.params.hops_per_window
    at, ratio = [0.0, 0.6 * in_len, float(in_len)], [lo, hi, 0.8]
    return warp_curve(n, at, ratio, hop_pos=hop_pos, n_hops=None if hop_pos is not None else n_hops, **kw)


# ---- the small shape ---------------------------------------------------------------------------------------------
KW = dict(window_len=1024, factor=2.0, channels=2, seed=3)


@pytest.fixture(scope="module")
def small():
    """N = 1024, f = 2, stereo, 20 000 frames: the engine, its input, the unwarped result, a glide's anchors and the
    one-launch warp of the result - computed once and never written to."""
    eng = rocoder_amd.Engine(**KW)
    a = noise_i16(20000, 2, 11, scale=12000)
    ref = eng.stretch_frames(a)
    anchors, n_out = glide_of(eng, ref.shape[0], 20000, KW)
    tiers = [Wp.tier_of(int(d)) for d in np.diff(anchors)]
    assert set(tiers) == set(range(5)) and any(x > y for x, y in zip(tiers, tiers[1:]))
    want = one_launch(ref, anchors, n_out)
    for w in (ref, want, anchors):
        w.flags.writeable = False
    yield eng, a, ref, anchors, n_out, want
    eng.set_output_warp()
    eng.close()


def test_f32_frames_and_rows_are_the_one_launch_warp(small):
    eng, a, ref, anchors, n_out, want = small
    assert want.shape == (n_out, 2) and n_out != ref.shape[0] and np.abs(want).max() > 0.05
    eng.set_output_warp(anchors, n_out)
    try:
        assert eng.output_len(20000) == ref.shape[0]  # (stays what it is)
        same_bits(eng.stretch_frames(a), want, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), want.T, "rows")
        # capacity: one frame short is RC_ECAPACITY with nothing written; the exact capacity reports n_out
        out = np.full((n_out, 2), 7.0, np.float32)
        got_len = C.c_size_t(99)
        fp = out.ctypes.data_as(C.POINTER(C.c_float))
        rc = eng._L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 20000, _lib.RC_PCM_I16, fp, n_out - 1, C.byref(got_len))
        assert rc == _lib.RC_ECAPACITY and (out == 7.0).all() and got_len.value == 99
        rc = eng._L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 20000, _lib.RC_PCM_I16, fp, n_out, C.byref(got_len))
        assert rc == 0 and got_len.value == n_out
        same_bits(out, want, "f32 frames at the exact capacity")
        # fewer frames than the anchors hold: the first n_out - 100 of the same warp
        eng.set_output_warp(anchors, n_out - 100)
        same_bits(eng.stretch_frames(a), want[:n_out - 100], "a shorter n_out")
    finally:
        eng.set_output_warp()


def test_pcm_with_fade_limiter_and_dither_count_warped_frames(small):
    eng, a, ref, anchors, n_out, want = small
    fade = (1001, n_out - 1500, 1493)
    drive = np.float32(CEILING / (np.float32(0.9) * np.abs(want).max()))
    w = limited(apply_fade(want, *fade), drive, 64)
    eng.set_output_warp(anchors, n_out)
    try:
        eng.set_output_fade(*fade)
        eng.set_output_limiter(drive, CEILING, 64)
        same_bits(eng.stretch_frames(a), w, "warped, faded and limited f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), w.T, "warped, faded and limited rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")
        assert eng.last_clipped == count_clipped(w)
        eng.set_output_dither("tpdf-hp", 77)
        got = eng.stretch_frames(a, out_fmt="i16")
        assert np.array_equal(np.frombuffer(got.tobytes(), np.uint8), dithered_bytes(w, "i16", "tpdf-hp", 77))
        # a fade that fits the unwarped job but not the warped one
        eng.set_output_fade(0, n_out - 10, 11)
        with pytest.raises(RocoderError) as ei:
            eng.stretch_frames(a)
        assert ei.value.code == _lib.RC_EINVAL
    finally:
        eng.set_output_dither()
        eng.set_output_limiter()
        eng.set_output_fade()
        eng.set_output_warp()


def test_under_a_time_map(small):
    eng, a, ref, anchors, n_out, want = small
    hop_pos = time_map_curve(20000, [0.0, 20000.0], [1.5, 4.0], **KW)
    eng.set_time_map(hop_pos)
    try:
        mapped = eng.stretch_frames(a)
        assert mapped.shape[0] == eng.output_len(20000) != ref.shape[0]
        anc, no = glide_of(eng, mapped.shape[0], 20000, KW, hop_pos=hop_pos)
        w = one_launch(mapped, anc, no)
        eng.set_output_warp(anc, no)
        same_bits(eng.stretch_frames(a), w, "f32 frames of a map job")
        same_bits(eng.stretch_host(rows_of(a)), w.T, "rows of a map job")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")
    finally:
        eng.set_output_warp()
        eng.set_time_map()


def test_a_constant_three_quarters_is_the_rational_resamplers_bytes(small):
    eng, a, ref, anchors, n_out, want = small
    n_rs = resample_len(ref.shape[0], 3, 4)
    fade = (500, n_rs - 700, 650)
    eng.set_output_fade(*fade)
    eng.set_output_dither("tpdf", 5)
    try:
        eng.set_output_resample(3, 4)
        by_step = eng.stretch_frames(a, out_fmt="i16").tobytes()
        by_step_f32 = eng.stretch_frames(a)
        eng.set_output_resample()
        eng.set_output_warp(Wp.constant_anchors(3, 4, n_rs), n_rs)
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == by_step and len(by_step) == 4 * n_rs
        same_bits(eng.stretch_frames(a), by_step_f32, "f32 frames")
    finally:
        eng.set_output_warp()
        eng.set_output_resample()
        eng.set_output_dither()
        eng.set_output_fade()


def test_the_setters_refuse_each_other_and_bad_tables_and_cleared_is_never_set(small):
    eng, a, ref, anchors, n_out, want = small
    L, i64p = eng._L, C.POINTER(C.c_int64)
    good = np.array(anchors)
    assert L.rc_engine_set_output_warp(None, good.ctypes.data_as(i64p), good.size, n_out) == _lib.RC_EINVAL  # a null engine

    def refused(table, n):
        t = np.ascontiguousarray(table, np.int64)
        return L.rc_engine_set_output_warp(eng._h, t.ctypes.data_as(i64p), t.size, n) == _lib.RC_EINVAL

    def bad_tables():
        yield good[:1], 0                                            # one anchor
        yield good, 64 * (good.size - 1) + 1                          # more frames than the blocks hold
        for v in (-1, 2 ** 62):
            t = good.copy()
            t[0 if v < 0 else -1] = v
            yield t, 10
        for d in (Wp.D_MIN - 1, Wp.D_MAX + 1, 0, -5):
            t = good.copy()
            t[7:] += d - (t[7] - t[6])
            yield t, 10

    try:
        # cleared: every bad table is refused and the job stays the plain one
        for t, n in bad_tables():
            assert refused(t, n)
        same_bits(eng.stretch_frames(a), ref, "f32 frames behind refused setters")
        # set: every bad table is refused and the warp stays
        eng.set_output_warp(anchors, n_out)
        for t, n in bad_tables():
            assert refused(t, n)
        with pytest.raises(RocoderError) as ei:
            eng.set_output_resample(3, 2)
        assert ei.value.code == _lib.RC_EINVAL and "warp" in str(ei.value)
        eng.set_output_resample()  # (clearing what is cleared is no error)
        same_bits(eng.stretch_frames(a), want, "f32 frames, the warp behind refused setters")
        # the other way round
        eng.set_output_warp()
        eng.set_output_resample(3, 2)
        with pytest.raises(RocoderError) as ei:
            eng.set_output_warp(anchors, n_out)
        assert ei.value.code == _lib.RC_EINVAL and "rc_engine_set_output_resample" in str(ei.value)
        assert eng.stretch_frames(a).shape[0] == resample_len(ref.shape[0], 3, 2)
        eng.set_output_resample()
        # set then cleared is an engine that never set it
        eng.set_output_warp(anchors, n_out)
        eng.set_output_warp()
        same_bits(eng.stretch_frames(a), ref, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), ref.T, "rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(ref, "i16"), "i16")
    finally:
        eng.set_output_resample()
        eng.set_output_warp()


def test_with_a_host_frequency_kernel():
    """the whole-job order: the whole job, one warp launch, one pack, one download"""
    a = noise_i16(20000, 2, 12, scale=12000)
    kw = dict(window_len=1024, factor=2.0, channels=2, seed=3)
    with rocoder_amd.Engine(kernel=lambda t, x: 0.5 * x, kernel_time_ms=1, **kw) as eng:
        ref = eng.stretch_frames(a)
        anchors, n_out = glide_of(eng, ref.shape[0], 20000, kw)
        w = one_launch(ref, anchors, n_out)
        eng.set_output_warp(anchors, n_out)
        same_bits(eng.stretch_frames(a), w, "f32 frames")
        same_bits(eng.stretch_host(rows_of(a)), w.T, "rows")
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")


# ---- several chunks: the lag bookkeeping -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    """The chunked shape of tests/test_gpu_frames_resample.py: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks. The one-launch warp of the unwarped result is computed once."""
    kw = dict(window_len=1024, factor=8.0, channels=3, seed=21)
    eng = rocoder_amd.Engine(**kw)
    a = noise_i16(1_200_000, 3, 4, scale=8192)
    ref = eng.stretch_frames(a)
    assert ref.shape[0] > 2 * SLOT_FLOATS
    anchors, n_out = glide_of(eng, ref.shape[0], 1_200_000, kw)
    assert n_out > SLOT_FLOATS  # (the chunks are cut by the unwarped rows; the downloads cross a staging slot as well)
    want = one_launch(ref, anchors, n_out)
    del ref
    want.flags.writeable = False
    yield eng, a, anchors, n_out, want
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_chunks_give_the_one_launch_warp(chunked, kind):
    eng, a, anchors, n_out, want = chunked
    eng.set_output_warp(anchors, n_out)
    try:
        if kind == "pinned":
            src = pinned_empty(a.shape, a.dtype)
            src[:] = a
            out = pinned_empty(want.shape, np.float32)
        else:
            src, out = a, np.empty(want.shape, np.float32)
        same_bits(eng.stretch_frames(src, out=out), want, f"f32 frames, {kind}")
    finally:
        eng.set_output_warp()


def test_chunks_of_rows_and_of_limited_pcm(chunked):
    eng, a, anchors, n_out, want = chunked
    fade = (30001, n_out - 50000, 49999)
    drive = np.float32(CEILING / (np.float32(0.9) * np.abs(want).max()))
    eng.set_output_warp(anchors, n_out)
    try:
        same_bits(eng.stretch_host(rows_of(a)), want.T, "rows")
        w = limited(apply_fade(want, *fade), drive, 64)
        eng.set_output_fade(*fade)
        eng.set_output_limiter(drive, CEILING, 64)
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == pcm_bytes(quantise(w, "i16"), "i16")
    finally:
        eng.set_output_limiter()
        eng.set_output_fade()
        eng.set_output_warp()
