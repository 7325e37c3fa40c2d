"""The mix bus through the C-ABI (include/rocoder_hip_mix.h): rc_engine_mix_frames and rc_engine_bus_frames against the
engine's own frames entries and against the numpy definition of tests/mixutil.py, bit for bit. Window 1024, factor 8 and a
few thousand frames of full-scale 16-bit noise unless a test says otherwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import Bus, RocoderError  # noqa: E402

import mixutil as M  # noqa: E402

pytestmark = pytest.mark.gpu


def noise_i16(n, ch, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, ch), dtype=np.int64).astype("<i2")


def engine(**kw):
    cfg = dict(window_len=1024, factor=8.0, channels=2, seed=3)
    cfg.update(kw)
    return rocoder_amd.Engine(**cfg)


def bus_rows(eng, bus):
    """the bus as float32 [CB, N], read back through the master with nothing set (f32: the bits as they are)"""
    out, _ = eng.bus_frames(bus, "f32")
    return np.ascontiguousarray(out.T)


@pytest.fixture(scope="module")
def layer():
    a = noise_i16(3000, 2, 4)
    with engine() as eng:
        ref = eng.stretch_frames(a).copy()
    ref.flags.writeable = False
    return a, ref


@pytest.mark.parametrize("fmt", ["u8", "i16", "i24", "i32", "f32"])
def test_one_layer_through_the_master_is_the_frames_entry(layer, fmt):
    a, ref = layer
    n = ref.shape[0]
    with engine() as eng, Bus(2, n) as bus:
        assert bus.layers == 0 and eng.mix_frames(a, bus) == n and bus.layers == 1
        got, stats = eng.bus_frames(bus, fmt)
        want = eng.stretch_frames(a, out_fmt=fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        if fmt == "f32":  # values: 0 + (-0) is +0
            assert np.array_equal(got, want) and np.array_equal(got, ref)
        else:
            assert got.tobytes() == want.tobytes()
        assert stats["clipped"] == eng.last_clipped and stats["gain"] == 1.0
        assert stats["peak"] == np.abs(ref).max()
        # at any byte alignment, and nothing else of the target is written
        big = np.full(got.nbytes + 64, 0xA5, np.uint8)
        for lo in (17, 18, 19):
            big[:] = 0xA5
            again, _ = eng.bus_frames(bus, fmt, out=big[lo:lo + got.nbytes])
            assert again.tobytes() == got.tobytes() and (big[:lo] == 0xA5).all() and (big[lo + got.nbytes:] == 0xA5).all()


@pytest.mark.parametrize("fmt", ["u8", "i16", "i24"])
def test_dither_and_limiter_on_both_sides(layer, fmt):
    """a limiter at drive 1 is the identity on what it has limited (every |x| <= ceiling: rq = 2^24, g = 1.0f exactly), so the
    layer's limiter followed by the master's gives the frames entry's bytes; the dither is the master's"""
    a, _ = layer
    with engine(amplitude=1.5) as eng:
        eng.set_output_limiter(1.0, 0.5, 64)
        eng.set_output_dither("tpdf-hp", 77)
        want = eng.stretch_frames(a, out_fmt=fmt)
        stats_want = (eng.last_limiter_stats, eng.last_clipped)
        assert stats_want[0][1] > 0  # the limiter worked
        with Bus(2, want.shape[0]) as bus:
            eng.mix_frames(a, bus)
            assert eng.last_limiter_stats == stats_want[0]
            got, stats = eng.bus_frames(bus, fmt)
            assert got.tobytes() == want.tobytes() and stats["clipped"] == stats_want[1]
            assert eng.last_limiter_stats == (np.float32(1.0), 0)


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_target_peak_is_the_norm_entry(layer, fmt):
    a, ref = layer
    with engine() as eng, Bus(2, ref.shape[0]) as bus:
        eng.mix_frames(a, bus)
        want = eng.stretch_frames(a, out_fmt=fmt, normalize=0.7)
        wstats = (eng.last_peak, eng.last_gain, eng.last_clipped)
        got, stats = eng.bus_frames(bus, fmt, target_peak=0.7)
        assert got.tobytes() == want.tobytes() if fmt != "f32" else np.array_equal(got, want)
        assert (stats["peak"], stats["gain"], stats["clipped"]) == wstats and stats["gain"] != 1.0


def test_fade_keys_are_the_output_fade(layer):
    a, ref = layer
    n = ref.shape[0]
    F, S, G = 1000, n - 3010, 3000
    with engine() as eng, Bus(2, n) as bus:
        eng.set_output_fade(F, S, G)
        want = eng.stretch_frames(a).copy()
        eng.set_output_fade()
        eng.mix_frames(a, bus, keys=[(0, 0.0), (F, 1.0), (S, 1.0), (S + G, 0.0)])
        got, _ = eng.bus_frames(bus, "f32")
        assert np.isfinite(want).all() and np.array_equal(got, want) and not np.array_equal(got, ref)
        assert not got[S + G:].any() and got[F:S].any()
        # the master's fade on the bus is the same fade again: it counts bus frames
        bus.clear()
        eng.mix_frames(a, bus)
        eng.set_output_fade(F, S, G)
        faded, _ = eng.bus_frames(bus, "f32")
        eng.set_output_fade()
        plain, _ = eng.bus_frames(bus, "f32")
        assert np.array_equal(faded, want) and np.array_equal(plain, ref)


def test_three_layers_from_three_engines():
    a4, a8, am = noise_i16(5000, 2, 5), noise_i16(2500, 2, 6), noise_i16(2000, 1, 7)
    send = np.array([[0.75], [-0.5]], np.float32)
    N = 21000
    with engine(factor=4.0, seed=11) as e4, engine(seed=12) as e8, engine(channels=1, seed=13) as em, Bus(2, N) as bus:
        e8.set_output_resample(3, 2)
        layers = [(e4, a4, 700, [(0, 0.0), (4000, 1.0), (15000, 0.15)], None),
                  (e8, a8, 0, [(500, 0.9), (9000, 0.3)], None),
                  (em, am, -1001, [(2000, 0.15), (12000, 0.95)], send)]
        want = np.zeros((2, N), np.float32)
        for eng, a, off, keys, sd in layers:
            x = np.ascontiguousarray(eng.stretch_frames(a).T)
            want, landed = M.mix(want, x, off, keys, sd)
            assert eng.mix_frames(a, bus, offset=off, keys=keys, send=sd) == landed > 0
        assert bus.layers == 3
        got = bus_rows(e4, bus)
        assert M.same(got, want) and np.abs(got).max() > 0.1
        # another call order is another sum (f32 addition does not associate): the order is the call order
        other = np.zeros((2, N), np.float32)
        for eng, a, off, keys, sd in reversed(layers):
            other, _ = M.mix(other, np.ascontiguousarray(eng.stretch_frames(a).T), off, keys, sd)
        assert not M.same(other, want)


def test_several_pipeline_chunks_with_keys_across_the_seams():
    """the chunked shape of tests/test_gpu_frames_pcm.py - three channels, 1 200 000 frames in, 9 600 000 out - with a limiter
    on the layer and a key every 98 304 + 7 frames, so that every chunk seam lies inside a segment"""
    a = noise_i16(1_200_000, 3, 4)
    with engine(channels=3, seed=21) as eng:
        eng.set_output_limiter(1.0, 0.6, 32)
        x = np.ascontiguousarray(eng.stretch_frames(a).T)
        n = x.shape[1]
        rng = np.random.default_rng(8)
        keys = [(int(f), float(v)) for f, v in zip(np.arange(0, n, 98304 + 7), rng.uniform(0.1, 1.0, n // (98304 + 7) + 1).astype(np.float32))]
        with Bus(3, n + 5) as bus:
            assert eng.mix_frames(a, bus, offset=3, keys=keys) == n
            want, _ = M.mix(np.zeros((3, n + 5), np.float32), x, 3, keys)
            eng.set_output_limiter()
            assert M.same(bus_rows(eng, bus), want)


def test_bus_state_and_refusals(layer):
    a, ref = layer
    n = ref.shape[0]
    with engine() as eng, engine(channels=1) as mono, Bus(2, n) as bus, Bus(3, 16) as bus3, Bus(2, 0) as empty:
        assert eng.mix_frames(a, bus, offset=-100) == n - 100 and eng.mix_frames(a, bus, offset=n - 7) == 7
        assert eng.mix_frames(a, bus, offset=n) == 0 and eng.mix_frames(a, bus, offset=-n) == 0 and bus.layers == 4
        n0 = eng.stretch_frames(a[:0]).shape[0]  # no input frames: valid, and a layer (of what the frames entry gives for none)
        assert eng.mix_frames(a[:0], bus) == n0 and bus.layers == 5
        first, _ = eng.bus_frames(bus, "i24")
        second, _ = eng.bus_frames(bus, "i24")
        assert first.tobytes() == second.tobytes() and first.any()
        before = bus_rows(eng, bus)
        L, h, bh = eng._L, eng._h, bus._h
        src = C.c_void_p(a.ctypes.data)
        kf, ka = (C.c_uint64 * 2)(1, 5), (C.c_float * 2)(0.5, 1.0)
        mixed = C.c_uint64(99)

        def mix(e=h, b=bh, off=0, f=kf, v=ka, k=2, s=None, fmt=_lib.RC_PCM_I16):
            return L.rc_engine_mix_frames(e, src, a.shape[0], fmt, b, off, f, v, k, s, C.byref(mixed))

        assert mix(b=None) == _lib.RC_EINVAL and mix(e=None) == _lib.RC_EINVAL
        assert mix(e=mono._h) == _lib.RC_EINVAL  # no send, 1 channel into 2
        assert mix(b=bus3._h) == _lib.RC_EINVAL
        assert mix(f=(C.c_uint64 * 2)(5, 5)) == _lib.RC_EINVAL and mix(f=(C.c_uint64 * 2)(5, 1)) == _lib.RC_EINVAL
        assert mix(v=(C.c_float * 2)(0.5, float("nan"))) == _lib.RC_EINVAL and mix(f=None) == _lib.RC_EINVAL
        assert mix(s=(C.c_float * 4)(1, 0, float("inf"), 1)) == _lib.RC_EINVAL
        assert mix(off=2 ** 62 + 1) == _lib.RC_EINVAL and mix(off=-2 ** 62 - 1) == _lib.RC_EINVAL
        assert mix(fmt=9) == _lib.RC_EINVAL
        many = np.arange(_lib.RC_MIX_MAX_KEYS + 1, dtype=np.uint64)
        amps = np.ones(many.size, np.float32)
        assert mix(f=many.ctypes.data_as(C.POINTER(C.c_uint64)), v=amps.ctypes.data_as(C.POINTER(C.c_float)), k=many.size) == _lib.RC_EINVAL
        eng.set_output_fade(n + 1000)  # a fade the layer's job does not hold: what rc_engine_stretch_frames rejects
        assert mix() == _lib.RC_EINVAL
        eng.set_output_fade()
        assert mixed.value == 99 and bus.layers == 5
        assert M.same(bus_rows(eng, bus), before)  # every refusal left the bus's bits as they were
        with pytest.raises(RocoderError):
            mono.mix_frames(a[:, :1], bus)
        # the master's refusals: nothing behind the out-pointers is written
        out = np.full(n * 2 * 4, 0xA5, np.uint8)
        got, peak = C.c_size_t(99), C.c_float(99)

        def master(e=h, b=bh, o=out.ctypes.data, cap=n, fmt=_lib.RC_PCM_I16, tp=0.0):
            return L.rc_engine_bus_frames(e, b, C.c_void_p(o) if o else None, cap, fmt, C.c_float(tp), C.byref(got), C.byref(peak), None, None)

        assert master(e=None) == _lib.RC_EINVAL and master(b=None) == _lib.RC_EINVAL and master(o=None) == _lib.RC_EINVAL
        assert master(b=bus3._h) == _lib.RC_EINVAL and master(e=mono._h) == _lib.RC_EINVAL
        assert master(fmt=0) == _lib.RC_EINVAL and master(fmt=6) == _lib.RC_EINVAL
        assert master(tp=-0.5) == _lib.RC_EINVAL and master(tp=float("inf")) == _lib.RC_EINVAL and master(tp=float("nan")) == _lib.RC_EINVAL
        assert master(cap=n - 1) == _lib.RC_ECAPACITY
        eng.set_output_fade(n + 1)
        assert master() == _lib.RC_EINVAL
        eng.set_output_fade()
        assert got.value == 99 and peak.value == 99 and (out == 0xA5).all()
        assert master() == _lib.RC_OK and got.value == n and peak.value > 0 and out[:n * 4].any()
        # clear: zeros, no layers; a bus of no frames
        bus.clear()
        assert bus.layers == 0 and not bus_rows(eng, bus).view(np.uint32).any()
        assert eng.mix_frames(a, empty) == 0 and empty.layers == 1
        e_out, e_stats = eng.bus_frames(empty, "i16")
        assert e_out.shape == (0, 2) and e_stats == {"peak": 0.0, "gain": 1.0, "clipped": 0}
        addr, stride = bus.device_rows()
        assert addr % 16 == 0 and stride % 4 == 0 and stride >= n


def test_with_a_host_frequency_kernel(layer):
    a, _ = layer
    with engine(kernel=lambda t, x: 0.5 * x, kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a).copy()
        with Bus(2, ref.shape[0]) as bus:
            assert eng.mix_frames(a, bus, keys=[(0, 0.25)]) == ref.shape[0]
            want, _ = M.mix(np.zeros(ref.T.shape, np.float32), np.ascontiguousarray(ref.T), 0, [(0, 0.25)])
            assert M.same(bus_rows(eng, bus), want)
